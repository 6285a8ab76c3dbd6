// Body of ln_modulate_kernel (LN_QUANT 0) and of ln_modulate_quant_kernel (LN_QUANT 1 and 2), elementwise.hip: one source for the
// arithmetic of all, included once per kernel form so that the plain kernel's text, and with it its code, is what it was before the
// quantising forms existed.  Expects the kernel's parameters and the template parameters T, NIT, TO in scope.
// LN_QUANT 1 (TO = bf16): `out` may be null; after the store step the row registers v hold the bf16-ROUNDED values, which
// apexmi_quant_rows_fp8's formula then turns into codes [row] and scales[row].
// LN_QUANT 2 (TO = bf16, C % 128 == 0): the rounded values leave as MXFP4 instead, apexmi_quant_blocks_mxfp4's formula per block of
// 32 columns = 4 adjacent lanes of one chunk step.  No row-wide maximum and no second pass; the two shuffles stand OUTSIDE the
// `c < nchunk` branch (nchunk % 16 == 0: a group of 4 lanes is live or dead as one, a dead lane brings 0).
    __shared__ float red[4];
    const int row = blockIdx.x;
    if (row < split) {  // rows [0, split) take the second modulation set (text stream of a joint buffer)
        scale = scale2;
        shift = shift2;
    }
    const int nchunk = C >> 3;
    const T* xp = x + (int64_t)row * ldx;
    float v[NIT][8];
    float sum = 0.0f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = it * 256 + threadIdx.x;
        if (c < nchunk) {
            load8<T>(xp + c * 8, v[it]);
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += v[it][j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[it][j] = 0.0f;
        }
    }
    float mean = 0.0f;
    if (!rms) mean = block_sum_256(sum, red) / (float)C;
    float sq = 0.0f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = it * 256 + threadIdx.x;
        if (c < nchunk) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[it][j] - mean;
                sq += d * d;
            }
        }
    }
    const float rstd = rsqrtf(block_sum_256(sq, red) / (float)C + eps);
#if LN_QUANT == 2
    TO* op = out == nullptr ? nullptr : out + (int64_t)row * ldo;
    uint8_t* qp = codes + (int64_t)row * ldq;
    uint8_t* sp = scales + (int64_t)row * lds;
#elif LN_QUANT
    TO* op = out == nullptr ? nullptr : out + (int64_t)row * ldo;
    float amax = 0.0f;
#else
    TO* op = out + (int64_t)row * ldo;
#endif
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = it * 256 + threadIdx.x;
#if LN_QUANT == 2
        float bmax = 0.0f;
#endif
        if (c < nchunk) {
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = (v[it][j] - mean) * rstd;
            if (gamma != nullptr) {
                float g[8];
                unpack8(*(const u32x4*)(gamma + c * 8), g);
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] *= g[j];
            }
            if (beta != nullptr) {
                float bt[8];
                unpack8(*(const u32x4*)(beta + c * 8), bt);
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] += bt[j];
            }
            if (scale != nullptr) {
                const f32x4 s0 = *(const f32x4*)(scale + c * 8);
                const f32x4 s1 = *(const f32x4*)(scale + c * 8 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] *= 1.0f + s0[j];
                    y[j + 4] *= 1.0f + s1[j];
                }
            }
            if (shift != nullptr) {
                const f32x4 s0 = *(const f32x4*)(shift + c * 8);
                const f32x4 s1 = *(const f32x4*)(shift + c * 8 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] += s0[j];
                    y[j + 4] += s1[j];
                }
            }
#if LN_QUANT == 2
            ln_quant_keep8(op == nullptr ? nullptr : op + c * 8, y, v[it], bmax);
#elif LN_QUANT
            ln_quant_keep8(op == nullptr ? nullptr : op + c * 8, y, v[it], amax);
#else
            store8<TO>(op + c * 8, y);
#endif
        }
#if LN_QUANT == 2
        const int sb = mx4_block_scale_byte(bmax);
        if (c < nchunk) mx4_store8(qp + c * 4, sp + (c >> 2), (c & 3) == 0, v[it], sb);
#endif
    }
#if LN_QUANT == 1
    const float qs = quant_row_scale(block_max_256(amax, red));
    if (threadIdx.x == 0) scales[row] = qs;
    uint8_t* qp = codes + (int64_t)row * ldq;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c = it * 256 + threadIdx.x;
        if (c < nchunk) quant_store8(qp + c * 8, v[it], qs);
    }
#endif
