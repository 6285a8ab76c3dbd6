// Body of ln_modulate_wave_kernel (LN_QUANT 0) and of ln_modulate_wave_quant_kernel (LN_QUANT 1 and 2), elementwise.hip: as
// ln_modulate_row.inc, for the wave-per-row family.  Expects the kernel's parameters and T, NCH, NR, TO in scope.  Every lane of a
// wave that reaches a row's store step is live (the row test is wave-uniform), so the block shuffles of LN_QUANT 2 are convergent.
    // NR rows per wave (`ln.wave` = NR): all NR rows' loads are issued before the first reduction, so a wave has NR x NCH
    // 16-byte loads in flight and the second row's statistics / stores overlap the first row's store drain.  Per row the
    // arithmetic is the same for every NR (bit-identical outputs).
    const int lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NR;
    if (row0 >= M) return;
    float v[NR][NCH][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int row = min(row0 + r, M - 1);
        const T* xp = x + (int64_t)row * ldx;
#pragma unroll
        for (int it = 0; it < NCH; ++it) load8<T>(xp + (it * 64 + lane) * 8, v[r][it]);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int row = row0 + r;
        if (row >= M) break;
        const float* sc = row < split ? scale2 : scale;
        const float* sh = row < split ? shift2 : shift;
        float sum = 0.0f;
#pragma unroll
        for (int it = 0; it < NCH; ++it)
#pragma unroll
            for (int j = 0; j < 8; ++j) sum += v[r][it][j];
        const float mean = rms ? 0.0f : wave_sum(sum) / (float)C;
        float sq = 0.0f;
#pragma unroll
        for (int it = 0; it < NCH; ++it)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[r][it][j] - mean;
                if constexpr (sizeof(T) == 4) sq = add_square_unfused(sq, d);
                else sq += d * d;
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
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
        for (int it = 0; it < NCH; ++it) {
            const int c = it * 64 + lane;
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = (v[r][it][j] - mean) * rstd;
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
            if (sc != nullptr) {
                const f32x4 s0 = *(const f32x4*)(sc + c * 8);
                const f32x4 s1 = *(const f32x4*)(sc + c * 8 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] *= 1.0f + s0[j];
                    y[j + 4] *= 1.0f + s1[j];
                }
            }
            if (sh != nullptr) {
                const f32x4 s0 = *(const f32x4*)(sh + c * 8);
                const f32x4 s1 = *(const f32x4*)(sh + c * 8 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    y[j] += s0[j];
                    y[j + 4] += s1[j];
                }
            }
#if LN_QUANT == 2
            float bmax = 0.0f;
            ln_quant_keep8(op == nullptr ? nullptr : op + c * 8, y, v[r][it], bmax);
            mx4_store8(qp + c * 4, sp + (c >> 2), (c & 3) == 0, v[r][it], mx4_block_scale_byte(bmax));
#elif LN_QUANT
            ln_quant_keep8(op == nullptr ? nullptr : op + c * 8, y, v[r][it], amax);
#else
            store8<TO>(op + c * 8, y);
#endif
        }
#if LN_QUANT == 1
        const float qs = quant_row_scale(wave_max(amax));
        if (lane == 0) scales[row] = qs;
        uint8_t* qp = codes + (int64_t)row * ldq;
#pragma unroll
        for (int it = 0; it < NCH; ++it) quant_store8(qp + (it * 64 + lane) * 8, v[r][it], qs);
#endif
    }
