// The grouped form of gemm_fp8_kernel and its fused q/k/v epilogue.  Included by gemm_fp8.hip inside its anonymous namespace, after
// gemm_fp8_kernel: it uses that file's tile constants (FBM, FBN, FBK, FOPB, UNIT_E8M0), i32x8 and lds_frag.
// ---- apexmi_gemm_fp8_grouped / apexmi_gemm_fp8_grouped_qkv -----------------------------------------------------------------------
// Up to 4 problems that share K in ONE launch of the tile above (the img + txt streams of a Flux double block, QKV + MLP-up of a
// single block): same 128 x 128 x 128 tile, staging, swizzle, one barrier per K-tile and epilogue arithmetic as gemm_fp8_kernel,
// which stays as it is.  The table travels by value in the kernel arguments.  xcd_remap runs over the launch's total tile count,
// the problem is found by the prefix sums of the tile counts (tile0), and inside a problem the band-of-8 order applies.  The
// epilogue (bias | gelu | gate_res) is chosen per problem: a block-uniform branch.
constexpr int FP8_MAX_GROUPS = 4;

struct Fp8Problem {
    const uint8_t* A;     // activation codes [M, K]
    const uint8_t* W;     // weight codes [N, K]
    const float* sa;      // [M]
    const bf16_t* sw;     // [N] or [1]
    const bf16_t* bias;   // [N] or null
    bf16_t* C;
    const float* gate;
    const bf16_t* R;
    int64_t lda, ldw, ldc, ldr;
    int M, N, sw_rows, epi;
    int tiles_m, tiles_n, tile0;
    // fused q/k/v preparation (apexmi_gemm_fp8_grouped_qkv): N = 3 H 128, rows [row0, row0 + M) of the joint sequence, nq / nk = the
    // per-head RMSNorm weights of this problem's stream (or null).  C is not written.
    int qkv, row0;
    const bf16_t* nq;
    const bf16_t* nk;
};
struct Fp8QkvShared {        // outputs of the fused preparation, shared by the problems of a launch
    bf16_t* qo;              // [H, S_out, 128]
    bf16_t* ko;              // [H, S_out, 128]
    bf16_t* vt;              // [H, 128, Skp]
    const float* rope;       // [2, S_out, 128] f32 (cos | sin), interleaved pairs
    int S_out, Skp, inner;   // inner = H * 128
    float eps;
};
struct Fp8Group {
    Fp8Problem p[FP8_MAX_GROUPS];
    int count, K, total;
    Fp8QkvShared qs;
    unsigned long long* clk;
};

// the epilogue of gemm_fp8_kernel (not LORA) on one problem of the table: out = epi(acc * sa[m] * sw[n] + bias[n])
template <int EPI>
APEXMI_DEVICE void fp8_group_epilogue(const f32x16 (&acc)[2][2], const Fp8Problem& G, int m0, int n0, int wr, int wc, int fr, int fh) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float sw[4][4], bs[4][4];
        f32x4 gt[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = min(n0 + 64 * wc + 32 * i + 8 * g + 4 * fh, G.N - 4);
            u32x2 s;
            if (G.sw_rows) {          // uniform condition
                s = *(const u32x2*)(G.sw + n);
            } else {
                const uint32_t one = G.sw[0];
                s = u32x2{one * 0x10001u, one * 0x10001u};
            }
            sw[g][0] = bf16_lo(s[0]), sw[g][1] = bf16_hi(s[0]), sw[g][2] = bf16_lo(s[1]), sw[g][3] = bf16_hi(s[1]);
            u32x2 b = {0u, 0u};
            if (G.bias != nullptr) b = *(const u32x2*)(G.bias + n);
            bs[g][0] = bf16_lo(b[0]), bs[g][1] = bf16_hi(b[0]), bs[g][2] = bf16_lo(b[1]), bs[g][3] = bf16_hi(b[1]);
            if (EPI == APEXMI_EPI_BIAS_GATE_RES) gt[g] = *(const f32x4*)(G.gate + n);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + 64 * wr + 32 * j + fr;
            const int mc = min(m, G.M - 1);
            const float sa = G.sa[mc];
            u32x2 rr[4];
            if (EPI == APEXMI_EPI_BIAS_GATE_RES) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = min(n0 + 64 * wc + 32 * i + 8 * g + 4 * fh, G.N - 4);
                    rr[g] = *(const u32x2*)(G.R + (int64_t)mc * G.ldr + n);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + 64 * wc + 32 * i + 8 * g + 4 * fh;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = acc[i][j][4 * g + e] * sa * sw[g][e] + bs[g][e];
                    if (EPI == APEXMI_EPI_BIAS_GELU) o[e] = gelu_tanh_f(o[e]);
                }
                if (EPI == APEXMI_EPI_BIAS_GATE_RES) {
                    o[0] = bf16_lo(rr[g][0]) + gt[g][0] * o[0];
                    o[1] = bf16_hi(rr[g][0]) + gt[g][1] * o[1];
                    o[2] = bf16_lo(rr[g][1]) + gt[g][2] * o[2];
                    o[3] = bf16_hi(rr[g][1]) + gt[g][3] * o[3];
                }
                if (m < G.M && n < G.N)
                    *(u32x2*)(G.C + (int64_t)m * G.ldc + n) = u32x2{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
            }
        }
    }
}

// Fused q/k/v preparation on a tile of a problem flagged `qkv` (N = 3 H 128: a 128-column tile is exactly one head of q, of k or
// of v, which = n0 / inner is block-uniform).  The tile y = bf16(acc * sa * sw + bias) — the value the two-pass path stores — goes
// into the staging LDS (free after the K-loop's last barrier) as [128 rows][128 bf16], row r rotated by rot(r) = (r >> 3) +
// 2 (r & 7) sixteen-byte chunks: the 16 consecutive rows of a store phase and the 8 position chunks of a transposed read each
// land on different chunks.
//   q / k: re-read in the layout of qk_norm_rope4_body (elementwise.hip): 16 lanes per row, 8 consecutive columns per lane, the
//          sequential sum of squares, the xor butterfly 8, 4, 2, 1, rsqrtf(sq / 128 + eps), x * r * w, the two fmaf forms of the
//          interleaved rotation and a 16-byte store into [H, S_out, 128] at row row0 + m: bit-identical to that pass.
//   v:     read transposed, 8 consecutive positions per lane, 16-byte stores into [H, 128, Skp]; a stream whose row0 | M is not
//          a multiple of 8 stores element-wise (a wave = 64 consecutive positions of one d-row).
// Rows >= M store nothing; columns >= S_out of V^T are not written.
APEXMI_DEVICE int fp8_qkv_rot(int r) { return (r >> 3) + 2 * (r & 7); }

APEXMI_DEVICE void fp8_qkv_epilogue(const f32x16 (&acc)[2][2], const Fp8Problem& G, const Fp8QkvShared& Q, int m0, int n0, int tid,
                                    uint8_t* lds) {
    bf16_t* tile = (bf16_t*)lds;
    const int lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1, fr = lane & 31, fh = lane >> 5;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float sw[4][4], bs[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n0 + 64 * wc + 32 * i + 8 * g + 4 * fh;          // N % 128 == 0: every column of the tile exists
            u32x2 s;
            if (G.sw_rows) {
                s = *(const u32x2*)(G.sw + n);
            } else {
                const uint32_t one = G.sw[0];
                s = u32x2{one * 0x10001u, one * 0x10001u};
            }
            sw[g][0] = bf16_lo(s[0]), sw[g][1] = bf16_hi(s[0]), sw[g][2] = bf16_lo(s[1]), sw[g][3] = bf16_hi(s[1]);
            u32x2 b = {0u, 0u};
            if (G.bias != nullptr) b = *(const u32x2*)(G.bias + n);
            bs[g][0] = bf16_lo(b[0]), bs[g][1] = bf16_hi(b[0]), bs[g][2] = bf16_lo(b[1]), bs[g][3] = bf16_hi(b[1]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 64 * wr + 32 * j + fr;
            const float sa = G.sa[min(m0 + r, G.M - 1)];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = 64 * wc + 32 * i + 8 * g + 4 * fh;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = acc[i][j][4 * g + e] * sa * sw[g][e] + bs[g][e];
                *(u32x2*)(tile + r * 128 + ((((c >> 3) + fp8_qkv_rot(r)) & 15) << 3) + (c & 4)) =
                    u32x2{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
            }
        }
    }
    __syncthreads();
    const int which = n0 / Q.inner;                    // 0 q, 1 k, 2 v: block-uniform
    const int h = (n0 - which * Q.inner) >> 7;
    if (which == 2) {
        bf16_t* vt = Q.vt + (int64_t)h * 128 * Q.Skp + G.row0 + m0;
        if (((G.row0 | G.M) & 7) != 0) {
            for (int i = 0; i < 64; ++i) {
                const int idx = i * 256 + tid;
                const int r = idx & 127, d = idx >> 7;
                const bf16_t e = tile[r * 128 + ((((d >> 3) + fp8_qkv_rot(r)) & 15) << 3) + (d & 7)];
                if (m0 + r < G.M) vt[(int64_t)d * Q.Skp + r] = e;
            }
            return;
        }
#pragma unroll 2
        for (int i = 0; i < 8; ++i) {
            const int idx = i * 256 + tid;
            const int sc = idx & 7, d = (idx >> 3) & 127, s8 = ((idx >> 10) * 8 + sc) * 8;     // 8 lanes = 8 position chunks of one d
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int r = s8 + j;
                const uint32_t e = tile[r * 128 + ((((d >> 3) + fp8_qkv_rot(r)) & 15) << 3) + (d & 7)];
                if (j & 1) w[j >> 1] |= e << 16;
                else w[j >> 1] = e;
            }
            if (m0 + s8 < G.M) *(u32x4*)(vt + (int64_t)d * Q.Skp + s8) = u32x4{w[0], w[1], w[2], w[3]};
        }
        return;
    }
    const bf16_t* nw = which ? G.nk : G.nq;
    bf16_t* dst = (which ? Q.ko : Q.qo) + (int64_t)h * Q.S_out * 128;
    const int l16 = tid & 15, d = l16 * 8;
    float wv[8];
    if (nw != nullptr) unpack8(*(const u32x4*)(nw + d), wv);
#pragma unroll 2
    for (int p = 0; p < 8; ++p) {
        const int r = p * 16 + (tid >> 4);
        const int srow = G.row0 + min(m0 + r, G.M - 1);
        const float* cp = Q.rope + (int64_t)srow * 128 + d;
        const float* sp = Q.rope + (int64_t)Q.S_out * 128 + (int64_t)srow * 128 + d;
        const f32x4 c0 = *(const f32x4*)cp, c1 = *(const f32x4*)(cp + 4);
        const f32x4 s0 = *(const f32x4*)sp, s1 = *(const f32x4*)(sp + 4);
        float cs[8], sn[8], x[8], y[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cs[j] = c0[j];
            cs[j + 4] = c1[j];
            sn[j] = s0[j];
            sn[j + 4] = s1[j];
        }
        unpack8(*(const u32x4*)(tile + r * 128 + (((l16 + fp8_qkv_rot(r)) & 15) << 3)), x);
        if (nw != nullptr) {
            float sq = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) sq += x[j] * x[j];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
            const float rn = rsqrtf(sq * (1.0f / 128) + Q.eps);
#pragma unroll
            for (int j = 0; j < 8; ++j) x[j] = x[j] * rn * wv[j];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            y[2 * q] = fmaf(x[2 * q], cs[2 * q], -(x[2 * q + 1] * sn[2 * q]));
            y[2 * q + 1] = fmaf(x[2 * q + 1], cs[2 * q + 1], x[2 * q] * sn[2 * q + 1]);
        }
        if (m0 + r < G.M) store8<bf16_t>(dst + (int64_t)srow * 128 + d, y);
    }
}

// the name contains "gemm_fp8_kernel": build.py's no-spill check covers this kernel too
__global__ __launch_bounds__(256, 2) void gemm_fp8_kernel_grouped(const Fp8Group G) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * FOPB];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    // tile id -> problem (prefix sums of the tile counts), then the band-of-8 order inside the problem
    int t = xcd_remap(blockIdx.x, G.total);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < FP8_MAX_GROUPS; ++i)
        if (i < G.count && t >= G.p[i].tile0) pi = i;
    const Fp8Problem P = G.p[pi];
    t -= P.tile0;
    const int band = 8 * P.tiles_n, first_m = (t / band) * 8;
    const int gsz = min(P.tiles_m - first_m, 8);
    const int m0 = (first_m + (t % band) % gsz) * FBM, n0 = ((t % band) / gsz) * FBN;

    const char* a_src[4];
    const char* w_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 32 * wid + 8 * i + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        a_src[i] = (const char*)(P.A + (int64_t)min(m0 + r, P.M - 1) * P.lda + c * 16);
        w_src[i] = (const char*)(P.W + (int64_t)min(n0 + r, P.N - 1) * P.ldw + c * 16);
    }
    auto stage = [&](int kt, int buf) {
        uint8_t* da = lds + buf * 2 * FOPB + (32 * wid) * FBK;     // wave-uniform; the hardware adds lane * 16
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            glds16(a_src[i] + (int64_t)kt * FBK, da + 8 * i * FBK);
            glds16(w_src[i] + (int64_t)kt * FBK, da + FOPB + 8 * i * FBK);
        }
    };

    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (G.clk != nullptr) {          // kernel-uniform
        clk_c0 = __builtin_readcyclecounter();
        clk_r0 = __builtin_amdgcn_s_memrealtime();
    }

    f32x16 acc[2][2];                 // [weight tile (output columns)][activation tile (output rows)]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nk = G.K / FBK;
    const int fr = lane & 31, fh = lane >> 5;
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const uint8_t* ta = lds + buf * 2 * FOPB;
        const uint8_t* tw = ta + FOPB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int piece = 4 * kk + 2 * fh;
            i32x8 fa[2], fw[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                fa[i] = lds_frag(ta, 64 * wr + 32 * i + fr, piece);
                fw[i] = lds_frag(tw, 64 * wc + 32 * i + fr, piece);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, UNIT_E8M0, 0,
                                                                               UNIT_E8M0);
        }
        __syncthreads();
    }

    if (G.clk != nullptr) {
        const unsigned long long c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            atomicAdd(G.clk, c1 - clk_c0);
            atomicAdd(G.clk + 1, r1 - clk_r0);
        }
    }

    if (P.qkv) fp8_qkv_epilogue(acc, P, G.qs, m0, n0, tid, lds);
    else if (P.epi == APEXMI_EPI_BIAS) fp8_group_epilogue<APEXMI_EPI_BIAS>(acc, P, m0, n0, wr, wc, fr, fh);
    else if (P.epi == APEXMI_EPI_BIAS_GELU) fp8_group_epilogue<APEXMI_EPI_BIAS_GELU>(acc, P, m0, n0, wr, wc, fr, fh);
    else fp8_group_epilogue<APEXMI_EPI_BIAS_GATE_RES>(acc, P, m0, n0, wr, wc, fr, fh);
}
