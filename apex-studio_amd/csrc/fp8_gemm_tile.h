// What the block-scaled-MFMA GEMMs share: the 128 x 128 output tile with 128-byte K-tiles, the operand record of ONE
// product, the f32 epilogue on the 32 x 32 result layout, and the grouped form's table entry with its fused q/k/v preparation.
// Included by gemm_fp8.hip (e4m3 x e4m3, every form) and gemm_mxfp4.hip (e2m1 x e2m1, single and grouped): the result layout of
// v_mfma_scale_f32_32x32x64_f8f6f4 does not depend on the operand format, so one epilogue serves both.  gemm_mxfp6.hip (e2m3 x e2m3)
// takes the tile order, the clock probe, the epilogue and the host side; its K-tile is 96 bytes a row, staged by its own code.
#pragma once
#include "common.h"
#include "fp8_quant.h"   // the MX output of the epilogue
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;

constexpr int FBM = 128, FBN = 128, FBK = 128;   // FBK in BYTES of a row: 128 e4m3 codes or 256 e2m1 codes
constexpr int FOPB = FBM * FBK;                  // bytes of one operand tile
constexpr int UNIT_E8M0 = 0x7f7f7f7f;            // 2^0 in every byte: the block scales are not used

// the operands of ONE product: what the staging, the K-loop and the epilogue read, in every form of the kernel
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
    int M, N, K, sw_rows;  // sw_rows: 1 = one scale per weight row, 0 = a single value
    int tiles_m, tiles_n;
    // MX forms (apexmi_gemm_fp8_mx, apexmi_gemm_fp8_grouped_mx; read by the MX instantiations only)
    const uint8_t* abs;   // e8m0 block scales of the activation [M, K / 32], or null = per-row scales `sa`
    uint8_t* Q;           // MX output codes [M, N], or null = the bf16 output C
    uint8_t* QS;          // MX output block scales [M, N / 32]
    int64_t ldabs, ldq, ldqs;
};

// ---- tile front end: what every form of both kernels does before and around its K-loop ----
// XCD-grouped tile order: each XCD takes a contiguous run of tile ids `t` (xcd_remap; of one problem); inside a run, bands of 8 tile
// rows are walked column by column, so a band shares its weight tiles.  ops.fp8_grouped_tiles restates this walk.
APEXMI_DEVICE void fp8_tile_origin(int t, int tiles_m, int tiles_n, int& m0, int& n0) {
    const int band = 8 * tiles_n, first_m = (t / band) * 8;
    const int gsz = min(tiles_m - first_m, 8);
    m0 = (first_m + (t % band) % gsz) * FBM, n0 = ((t % band) / gsz) * FBN;
}

// Staging layout: lds[buf][operand][row 0..127][128 bytes].  Wave w writes rows 32 w .. 32 w + 31 of both operand tiles, 8 whole
// rows per instruction (64 lanes x 16 bytes, lane-linear), and the XOR swizzle is on the SOURCE address: 16-byte piece c of row r
// holds the row's bytes 16 (c ^ ((r >> 1) & 7)) .., so the 16 lanes of one ds_read_b128 phase cover all 64 banks once.
// fp8_stage_src: what this lane copies in instruction i of a K-tile = its row (tile rows past `rows` clamp to the last one) and
// its swizzled piece of that row's first 128 bytes; `ld` in elements of T.
template <class T>
APEXMI_DEVICE const char* fp8_stage_src(const T* base, int64_t ld, int row0, int rows, int wid, int lane, int i) {
    const int r = 32 * wid + 8 * i + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    return (const char*)(base + (int64_t)min(row0 + r, rows - 1) * ld) + c * 16;
}
// the wave's destination of instruction 0 (wave-uniform; the hardware adds lane * 16); instruction i is 8 i rows further, the weight
// tile FOPB behind the activation tile
APEXMI_DEVICE uint8_t* fp8_stage_dst(uint8_t* lds, int buf, int wid) { return lds + buf * 2 * FOPB + (32 * wid) * FBK; }

// the eight source pointers of a K-loop over A [M, K] and W [N, K] (bytes); the call issues K-tile kt into lds[buf]
struct Fp8Stager {
    const char* a_src[4];
    const char* w_src[4];
    APEXMI_DEVICE Fp8Stager(const Fp8Problem& P, int m0, int n0, int wid, int lane) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a_src[i] = fp8_stage_src(P.A, P.lda, m0, P.M, wid, lane, i);
            w_src[i] = fp8_stage_src(P.W, P.ldw, n0, P.N, wid, lane, i);
        }
    }
    APEXMI_DEVICE void operator()(uint8_t* lds, int wid, int kt, int buf) const {
        uint8_t* da = fp8_stage_dst(lds, buf, wid);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            glds16(a_src[i] + (int64_t)kt * FBK, da + 8 * i * FBK);
            glds16(w_src[i] + (int64_t)kt * FBK, da + FOPB + 8 * i * FBK);
        }
    }
};

// the swizzled 16-byte piece `piece` of row `row` of a staged tile
APEXMI_DEVICE u32x4 lds_piece(const uint8_t* tile, int row, int piece) {
    return *(const u32x4*)(tile + row * FBK + ((piece ^ ((row >> 1) & 7)) << 4));
}

// the live clock probe (apexmi_clk_ptr; `clk` null = off, kernel-uniform): cycles and real time from start() to stop(), summed
// over the launch's workgroups
struct Fp8Clock {
    unsigned long long c0 = 0, r0 = 0;
    APEXMI_DEVICE void start(const unsigned long long* clk) {
        if (clk != nullptr) {
            c0 = __builtin_readcyclecounter();
            r0 = __builtin_amdgcn_s_memrealtime();
        }
    }
    APEXMI_DEVICE void stop(unsigned long long* clk, int tid) const {
        if (clk != nullptr) {
            const unsigned long long c1 = __builtin_readcyclecounter(), r1 = __builtin_amdgcn_s_memrealtime();
            if (tid == 0) {
                atomicAdd(clk, c1 - c0);
                atomicAdd(clk + 1, r1 - r0);
            }
        }
    }
};

// acc[weight tile (output columns)][activation tile (output rows)] = 0
APEXMI_DEVICE void fp8_zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// the weight scales / the bias of the 4 columns n .. n + 3 (n clamped by the caller; a null bias is 0)
APEXMI_DEVICE void fp8_unpack4(const u32x2 v, float (&f)[4]) { f[0] = bf16_lo(v[0]), f[1] = bf16_hi(v[0]), f[2] = bf16_lo(v[1]), f[3] = bf16_hi(v[1]); }

APEXMI_DEVICE void fp8_load_sw(const Fp8Problem& G, int n, float (&sw)[4]) {
    u32x2 s;
    if (G.sw_rows) {          // uniform condition
        s = *(const u32x2*)(G.sw + n);
    } else {
        const uint32_t one = G.sw[0];
        s = u32x2{one * 0x10001u, one * 0x10001u};
    }
    fp8_unpack4(s, sw);
}

APEXMI_DEVICE void fp8_load_bias(const Fp8Problem& G, int n, float (&bs)[4]) {
    u32x2 b = {0u, 0u};
    if (G.bias != nullptr) b = *(const u32x2*)(G.bias + n);
    fp8_unpack4(b, bs);
}

// ---- epilogue: out = epi(acc * sa[m] * sw[n] + bias[n]).  Loads go to clamped addresses; out-of-range lanes store nothing ----
// not SCALED (the LoRA form, and the fp4 kernel, whose block scales the MFMA applied): the scales are in acc already, out = epi(acc +
// bias[n]).  The problem travels BY VALUE: by reference the address arithmetic is redone at every store.
// MXIN (the MX instantiations): a problem with block-scaled activations (G.abs, block-uniform) uses sa = 1.  MXOUT (bias / gelu, N % 128 == 0): the value pack_bf16 would
// store is quantised per 32-column block instead — a lane holds 16 of the block's columns of its row in acc[i][j], lane l ^ 32 the
// other 16 — and leaves as 4 codes per register group plus one scale byte per block and row (the fh == 0 lane); C is not written.
// MXOUT is the FORMAT of that output: MXO_NONE, MXO_E4M3 (apexmi_quant_blocks_mxfp8's codes, a byte each; `true` of the e4m3
// callers) or MXO_E2M1 (apexmi_quant_blocks_mxfp4's, two to a byte: Q is [M, N / 2]).  A lane's four consecutive columns are two
// bytes of e2m1 codes; the lane pair swaps halves (one more exchange with l ^ 32) so that each lane stores two whole dwords — fh 0
// the row's bytes of register groups 0 and 1, fh 1 those of groups 2 and 3 — instead of four 2-byte pieces.
constexpr int MXO_NONE = 0, MXO_E4M3 = 1, MXO_E2M1 = 2;
template <int EPI, bool SCALED, bool MXIN = false, int MXOUT = MXO_NONE>
APEXMI_DEVICE void fp8_epilogue(const f32x16 (&acc)[2][2], const Fp8Problem G, int m0, int n0, int wr, int wc, int fr, int fh) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float sw[4][4], bs[4][4];
        f32x4 gt[4];
        if constexpr (SCALED) {
#pragma unroll
            for (int g = 0; g < 4; ++g) fp8_load_sw(G, min(n0 + 64 * wc + 32 * i + 8 * g + 4 * fh, G.N - 4), sw[g]);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = min(n0 + 64 * wc + 32 * i + 8 * g + 4 * fh, G.N - 4);
            fp8_load_bias(G, n, bs[g]);
            if (EPI == APEXMI_EPI_BIAS_GATE_RES) gt[g] = *(const f32x4*)(G.gate + n);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + 64 * wr + 32 * j + fr;
            const int mc = min(m, G.M - 1);
            float sa = 1.f;
            if constexpr (SCALED) {
                if constexpr (MXIN) sa = G.abs != nullptr ? 1.f : G.sa[mc];
                else sa = G.sa[mc];
            }
            u32x2 rr[4];
            [[maybe_unused]] float mxv[16];
            [[maybe_unused]] float mxm = 0.f;
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
                    if constexpr (SCALED) o[e] = acc[i][j][4 * g + e] * sa * sw[g][e] + bs[g][e];
                    else o[e] = acc[i][j][4 * g + e] + bs[g][e];
                    if (EPI == APEXMI_EPI_BIAS_GELU) o[e] = gelu_tanh_f(o[e]);
                }
                if (EPI == APEXMI_EPI_BIAS_GATE_RES) {
                    o[0] = bf16_lo(rr[g][0]) + gt[g][0] * o[0];
                    o[1] = bf16_hi(rr[g][0]) + gt[g][1] * o[1];
                    o[2] = bf16_lo(rr[g][1]) + gt[g][2] * o[2];
                    o[3] = bf16_hi(rr[g][1]) + gt[g][3] * o[3];
                }
                if constexpr (MXOUT != MXO_NONE) {
                    const uint32_t p0 = pack_bf16(o[0], o[1]), p1 = pack_bf16(o[2], o[3]);
                    mxv[4 * g] = bf16_lo(p0), mxv[4 * g + 1] = bf16_hi(p0), mxv[4 * g + 2] = bf16_lo(p1), mxv[4 * g + 3] = bf16_hi(p1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) mxm = fmaxf(mxm, fabsf(mxv[4 * g + e]));
                } else {
                    if (m < G.M && n < G.N)
                        *(u32x2*)(G.C + (int64_t)m * G.ldc + n) = u32x2{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
                }
            }
            if constexpr (MXOUT == MXO_E2M1) {
                mxm = fmaxf(mxm, __shfl_xor(mxm, 32, 64));       // every lane takes part: rows >= M compute on clamped loads
                const int sb = mx4_scale_byte(mxm);
                const float inv = mx_inv_scale(sb);
                const int nb = n0 + 64 * wc + 32 * i;           // N % 128 == 0: every column of the tile exists
                uint32_t h[4];                                  // group g: the codes of columns nb + 8 g + 4 fh .. + 3, 16 bits
#pragma unroll
                for (int g = 0; g < 4; ++g) h[g] = mx4_quant4f(mxv[4 * g], mxv[4 * g + 1], mxv[4 * g + 2], mxv[4 * g + 3], inv);
                const uint32_t w01 = h[0] | h[1] << 16, w23 = h[2] | h[3] << 16;
                const uint32_t got = (uint32_t)__shfl_xor((int)(fh ? w01 : w23), 32, 64);   // the partner's halves of MY two groups
                const uint32_t lo = fh ? got : w01, hi = fh ? w23 : got;                    // columns + 0..3 | columns + 4..7
                if (m < G.M) {
                    uint32_t* q = (uint32_t*)(G.Q + (int64_t)m * G.ldq + (nb >> 1) + 8 * fh);
                    q[0] = (lo & 0xffffu) | hi << 16;
                    q[1] = lo >> 16 | (hi & 0xffff0000u);
                    if (fh == 0) G.QS[(int64_t)m * G.ldqs + (nb >> 5)] = (uint8_t)sb;
                }
            } else if constexpr (MXOUT == MXO_E4M3) {
                mxm = fmaxf(mxm, __shfl_xor(mxm, 32, 64));       // every lane takes part: rows >= M compute on clamped loads
                const int sb = mx_scale_byte(mxm);
                const float inv = mx_inv_scale(sb);
                const int nb = n0 + 64 * wc + 32 * i;           // N % 128 == 0: every column of the tile exists
                if (m < G.M) {
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *(uint32_t*)(G.Q + (int64_t)m * G.ldq + nb + 8 * g + 4 * fh) =
                            mx_quant4f(mxv[4 * g], mxv[4 * g + 1], mxv[4 * g + 2], mxv[4 * g + 3], inv);
                    if (fh == 0) G.QS[(int64_t)m * G.ldqs + (nb >> 5)] = (uint8_t)sb;
                }
            }
        }
    }
}

// ---- the grouped form: what the table of either kernel holds per problem, and the fused q/k/v preparation ----
constexpr int FP8_MAX_GROUPS = 4;

// One problem of a grouped launch (Fp8Group in gemm_fp8.hip, Mxfp4Group in gemm_mxfp4.hip): up to 4 problems that share K in ONE
// launch (the img + txt streams of a Flux double block, QKV + MLP-up of a single block).  The table travels by value in the kernel
// arguments.  xcd_remap runs over the launch's total tile count, the problem is found by the prefix sums of the tile counts
// (tile0), and the epilogue (bias | gelu | gate_res) is chosen per problem: a block-uniform branch.
struct Fp8GroupProblem : Fp8Problem {
    int epi, tile0;
    // fused q/k/v preparation (apexmi_gemm_fp8_grouped_qkv, apexmi_gemm_mxfp4_grouped_qkv): N = 3 H 128, rows [row0, row0 + M) of the
    // joint sequence, nq / nk = the per-head RMSNorm weights of this problem's stream (or null).  C is not written.
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

// the table entry of this workgroup among `count` entries `p` (anything derived from Fp8GroupProblem) of a launch of `total` tiles;
// `t` = its tile id inside that problem
template <class Entry>
APEXMI_DEVICE Entry fp8_group_entry(const Entry (&p)[FP8_MAX_GROUPS], int count, int total, int& t, int& pi) {
    t = xcd_remap(blockIdx.x, total);
    pi = 0;
#pragma unroll
    for (int i = 1; i < FP8_MAX_GROUPS; ++i)
        if (i < count && t >= p[i].tile0) pi = i;
    const Entry P = p[pi];
    t -= P.tile0;
    return P;
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
// not SCALED (a problem of the grouped LoRA form that carried an adapter, and every problem of the fp4 kernel, whose block scales
// the MFMA applied): the scales (and the adapter term) are in acc already, y = bf16(acc + bias), and the staging LDS is free after
// the last barrier of the tail / the K-loop.
APEXMI_DEVICE int fp8_qkv_rot(int r) { return (r >> 3) + 2 * (r & 7); }

template <bool SCALED>
APEXMI_DEVICE void fp8_qkv_epilogue(const f32x16 (&acc)[2][2], const Fp8GroupProblem& G, const Fp8QkvShared& Q, int m0, int n0, int tid,
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
            if constexpr (SCALED) fp8_load_sw(G, n, sw[g]);
            fp8_load_bias(G, n, bs[g]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = 64 * wr + 32 * j + fr;
            float sa = 1.f;
            if constexpr (SCALED) sa = G.sa[min(m0 + r, G.M - 1)];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = 64 * wc + 32 * i + 8 * g + 4 * fh;
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (SCALED) o[e] = acc[i][j][4 * g + e] * sa * sw[g][e] + bs[g][e];
                    else o[e] = acc[i][j][4 * g + e] + bs[g][e];
                }
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

// ---- host side: the checks of ONE problem that do not depend on the operand format, and the launch by epilogue ----
// how the messages name a problem: `i` = its index in a grouped launch, or -1 for a single launch (every fragment empty)
struct Fp8Where {
    char of[32] = "", paren[32] = "", colon[32] = "", semi[32] = "";
    explicit Fp8Where(int i) {
        if (i < 0) return;
        snprintf(of, sizeof(of), " of problem %d", i);
        snprintf(paren, sizeof(paren), " (problem %d)", i);
        snprintf(colon, sizeof(colon), "problem %d: ", i);
        snprintf(semi, sizeof(semi), "; problem %d", i);
    }
};

// what differs between the formats, in the rules and in the wording of the messages (passed through as the entry points word them)
struct Fp8Format {
    int k_tile;              // codes of one K-tile (128 bytes of a row): K is a multiple of it
    const char* k_note;      // what follows "must be a multiple of <k_tile>"
    int codes_per_byte;      // 1 (e4m3) or 2 (e2m1): a code row is K / codes_per_byte bytes
    const char* ld_note;     // what follows "must keep rows 16-byte aligned"
    const char* ld_unit;     // the unit of the 2^22 bound
    bool scales_aligned;     // the alignment of the format's own scale operands
    const char* align_note;  // the parenthesis of the alignment message
    int code_bits = 0;       // 6 (e2m3): a code row is K * 6 / 8 bytes and codes_per_byte is not read; 0 = by codes_per_byte
};

// M, N, K, the epilogue, the leading dimensions, the alignment of A / W / C / bias / gate / R and the tile count (tile0 = the tiles
// of the problems before this one); then the operand record with sa / sw / the MX members left null
static int fp8_check_tile_problem(const char* who, const Fp8Where& at, const Fp8Format& f, int64_t tile0, const void* qa, int64_t lda,
                                  const void* qw, int64_t ldw, const void* bias, void* C, int64_t ldc, int M, int N, int K, int epilogue,
                                  const float* gate, const void* R, int64_t ldr, Fp8Problem* P) {
    APEXMI_REQUIRE(M >= 1, "%s: M=%d%s must be at least 1", who, M, at.of);
    APEXMI_REQUIRE(N >= 16 && N % 16 == 0, "%s: N=%d%s must be a multiple of 16", who, N, at.of);
    APEXMI_REQUIRE(K >= f.k_tile && K % f.k_tile == 0, "%s: K=%d must be a multiple of %d%s", who, K, f.k_tile, f.k_note);
    APEXMI_REQUIRE((epilogue & APEXMI_EPI_F32_IO) == 0 && epilogue != APEXMI_EPI_BIAS_F32,
                   "%s: f32 output (epilogue %d%s, the f32 residual stream) is not supported: the output is bf16", who, epilogue, at.of);
    APEXMI_REQUIRE(epilogue == APEXMI_EPI_BIAS || epilogue == APEXMI_EPI_BIAS_GELU || epilogue == APEXMI_EPI_BIAS_GATE_RES,
                   "%s: epilogue %d%s is not one of bias (0), tanh GELU (1), gate x y + residual (2)", who, epilogue, at.of);
    const int kb = f.code_bits ? K / 8 * f.code_bits : K / f.codes_per_byte;
    APEXMI_REQUIRE(lda % 16 == 0 && ldw % 16 == 0 && ldc % 4 == 0 && lda >= kb && ldw >= kb && ldc >= N,
                   "%s: leading dimensions must keep rows 16-byte aligned%s (%slda %lld, ldw %lld, ldc %lld)", who, f.ld_note, at.colon,
                   (long long)lda, (long long)ldw, (long long)ldc);
    APEXMI_REQUIRE(lda <= (1 << 22) && ldw <= (1 << 22), "%s: leading dimensions above 2^22 %s are not supported (%slda %lld, ldw %lld)",
                   who, f.ld_unit, at.colon, (long long)lda, (long long)ldw);
    APEXMI_REQUIRE(((uintptr_t)qa % 16) == 0 && ((uintptr_t)qw % 16) == 0 && ((uintptr_t)C % 8) == 0 && f.scales_aligned &&
                       ((uintptr_t)bias % 8) == 0,
                   "%s: operands must be 16-byte aligned (%s)", who, f.align_note);
    if (epilogue == APEXMI_EPI_BIAS_GATE_RES) {
        APEXMI_REQUIRE(gate && R, "%s: gate/residual epilogue needs gate and R%s", who, at.paren);
        APEXMI_REQUIRE(ldr % 4 == 0 && ldr >= N && ((uintptr_t)gate % 16) == 0 && ((uintptr_t)R % 8) == 0, "%s: gate/R alignment%s", who,
                       at.paren);
    }
    const int tm = (M + FBM - 1) / FBM, tn = (N + FBN - 1) / FBN;
    APEXMI_REQUIRE(tile0 + (int64_t)tm * tn < (1ll << 31), "%s: too many output tiles", who);
    *P = Fp8Problem{(const uint8_t*)qa, (const uint8_t*)qw, nullptr, nullptr, (const bf16_t*)bias, (bf16_t*)C, gate, (const bf16_t*)R,
                    lda, ldw, ldc, ldr, M, N, K, 0, tm, tn};
    return 0;
}

// the fused q/k/v operands of a grouped launch as the entry points take them (apexmi_gemm_fp8_grouped_qkv(_lora),
// apexmi_gemm_mxfp4_grouped_qkv), and their checks: the launch's shared part, then problem `i` if it is flagged
struct Fp8QkvArgs {
    const int* is_qkv;
    const void* const* norm_q;
    const void* const* norm_k;
    const int* row0;
    int H;
    float eps;
    const float* rope;
    void* q_out;
    void* k_out;
    void* vt_out;
    int S_out, Skp;
};

static int fp8_check_qkv_shared(const char* who, const Fp8QkvArgs& q, Fp8QkvShared* S) {
    APEXMI_REQUIRE(q.is_qkv && q.row0 && q.rope && q.q_out && q.k_out && q.vt_out && q.H > 0, "%s: null argument", who);
    APEXMI_REQUIRE(q.S_out > 0 && q.Skp >= q.S_out && q.Skp % 8 == 0, "%s: Skp=%d must be a multiple of 8 >= S_out=%d", who, q.Skp, q.S_out);
    APEXMI_REQUIRE(((uintptr_t)q.rope % 16) == 0 && ((uintptr_t)q.q_out % 16) == 0 && ((uintptr_t)q.k_out % 16) == 0 &&
                       ((uintptr_t)q.vt_out % 16) == 0,
                   "%s: rope / outputs must be 16-byte aligned", who);
    *S = Fp8QkvShared{(bf16_t*)q.q_out, (bf16_t*)q.k_out, (bf16_t*)q.vt_out, q.rope, q.S_out, q.Skp, q.H * 128, q.eps};
    return 0;
}

static int fp8_check_qkv_problem(const char* who, const Fp8QkvArgs& q, int i, Fp8GroupProblem* P) {
    APEXMI_REQUIRE(P->N == 3 * q.H * 128 && P->epi == APEXMI_EPI_BIAS,
                   "%s: a fused problem has N = 3 H 128 = %d (got %d) and the plain bias epilogue", who, 3 * q.H * 128, P->N);
    APEXMI_REQUIRE(q.row0[i] >= 0 && q.row0[i] + P->M <= q.S_out, "%s: rows [%d, %d) must lie inside S_out=%d", who, q.row0[i],
                   q.row0[i] + P->M, q.S_out);
    const void* nq = q.norm_q ? q.norm_q[i] : nullptr;
    const void* nk = q.norm_k ? q.norm_k[i] : nullptr;
    APEXMI_REQUIRE(((uintptr_t)nq % 16) == 0 && ((uintptr_t)nk % 16) == 0, "%s: norm weights must be 16-byte aligned", who);
    P->qkv = 1;
    P->row0 = q.row0[i];
    P->nq = (const bf16_t*)nq;
    P->nk = (const bf16_t*)nk;
    return 0;
}

// One launch of 256 threads per tile with the kernel chosen by the epilogue.  kernel_of(std::integral_constant<int, EPI>) returns
// the instantiation; dyn_lds > 0 = that much dynamic LDS, raised above the default limit once per device and instantiation.
template <class KernelOf, class Args>
static void launch_by_epilogue(int epilogue, KernelOf kernel_of, const Args& G, unsigned tiles, int dyn_lds, hipStream_t stream) {
    auto launch = [&](auto epi) {
        auto kernel = kernel_of(epi);
        if (dyn_lds > 0) {
            static uint64_t attr_set = 0;       // one per instantiation of this lambda = per kernel
            APEXMI_SET_ATTR_ONCE(attr_set, (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, dyn_lds));
        }
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), dyn_lds, stream, G);
    };
    switch (epilogue) {
        case APEXMI_EPI_BIAS: launch(std::integral_constant<int, APEXMI_EPI_BIAS>{}); break;
        case APEXMI_EPI_BIAS_GELU: launch(std::integral_constant<int, APEXMI_EPI_BIAS_GELU>{}); break;
        default: launch(std::integral_constant<int, APEXMI_EPI_BIAS_GATE_RES>{}); break;
    }
}

// ---- host side of the MX formats whose block scales ride in the MFMA (gemm_mxfp4.hip, gemm_mxfp6.hip): one problem record, one
// check; and the one body of the three MX block quantisers (apexmi_quant_blocks_mxfp8 / _mxfp4 / _mxfp6) ----
struct MxGemm : Fp8Problem {           // A / W: packed codes, lda / ldw in bytes; sa, sw, abs unused; Q / QS: the MX output (e2m1 only)
    const uint8_t* SA;                 // activation block scales [M, K / 32]
    const uint8_t* SW;                 // weight block scales [N, K / 32]
    int64_t ldsa, ldsw;
    unsigned long long* clk;
};

// the MX output of the _mx entry points (both members null = the bf16 output C): C may then be null and is not written
struct MxOut {
    void* Q;              // codes [M, N / 2]
    int64_t ldq;
    void* QS;             // scale bytes [M, N / 32]
    int64_t ldqs;
};

// ONE problem of any entry point: the null check, the MX output's rules (only a format whose kernel has that epilogue passes
// `mx`; e2m1 today, which the wording assumes), the format-independent checks (fp8_check_tile_problem with the rules of `f`, whose
// ld_note is a pattern for the bytes of a code row), then the scale-row rule; fills the Fp8Problem part of `P` and its SA / SW /
// ldsa / ldsw.  `i` = the problem's index in a grouped launch, which the messages name, or -1; tile0 = the tiles of the problems
// before it.
template <class Problem>
static int mx_check_problem(const char* who, int i, int64_t tile0, Fp8Format f, const void* qa, int64_t lda, const void* sa, int64_t ldsa,
                            const void* qw, int64_t ldw, const void* sw, int64_t ldsw, const void* bias, void* C, int64_t ldc, int M, int N,
                            int K, int epilogue, const float* gate, const void* R, int64_t ldr, Problem* P, const MxOut* mx = nullptr) {
    const Fp8Where at(i);
    const bool mxo = mx != nullptr && (mx->Q != nullptr || mx->QS != nullptr);
    APEXMI_REQUIRE(qa && sa && qw && sw && (C || mxo), "%s: null operand%s", who, at.paren);
    if (mxo) {
        APEXMI_REQUIRE(mx->Q && mx->QS, "%s: the MX output%s needs codes and block scales", who, at.of);
        APEXMI_REQUIRE(epilogue == APEXMI_EPI_BIAS || epilogue == APEXMI_EPI_BIAS_GELU,
                       "%s: the MX output%s exists for the bias (0) and tanh GELU (1) epilogues, not epilogue %d", who, at.of, epilogue);
        APEXMI_REQUIRE(N % 128 == 0, "%s: N=%d%s must be a multiple of 128 for the MX output", who, N, at.of);
        APEXMI_REQUIRE(mx->ldq >= N / 2 && mx->ldq % 4 == 0 && ((uintptr_t)mx->Q % 4) == 0 && mx->ldqs >= N / 32 && mx->ldqs % 4 == 0,
                       "%s: the MX output%s needs 4-byte aligned code rows at least N / 2 bytes wide and scale rows at least N / 32 "
                       "wide, a multiple of 4 (ldmc %lld, ldms %lld)", who, at.of, (long long)mx->ldq, (long long)mx->ldqs);
        if (C == nullptr) ldc = N;      // not written, not read
    }
    char ld_note[64];
    snprintf(ld_note, sizeof(ld_note), f.ld_note, f.code_bits ? K / 8 * f.code_bits : K / f.codes_per_byte);
    f.ld_note = ld_note;
    if (fp8_check_tile_problem(who, at, f, tile0, qa, lda, qw, ldw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, (Fp8Problem*)P)) return 1;
    APEXMI_REQUIRE(ldsa >= K / 32 && ldsw >= K / 32 && ldsa % 4 == 0 && ldsw % 4 == 0 && ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sw % 4) == 0,
                   "%s: the block scales%s must be 4-byte aligned rows of at least K / 32 = %d bytes (ldsa %lld, ldsw %lld)", who, at.of,
                   K / 32, (long long)ldsa, (long long)ldsw);
    P->SA = (const uint8_t*)sa, P->SW = (const uint8_t*)sw, P->ldsa = ldsa, P->ldsw = ldsw;
    if (mxo) P->Q = (uint8_t*)mx->Q, P->QS = (uint8_t*)mx->QS, P->ldq = mx->ldq, P->ldqs = mx->ldqs;
    return 0;
}

// what differs between the three MX block quantisers, in the rules and in the wording of the messages
struct MxQuantFormat {
    const char* who;         // the entry point's name without "apexmi_"
    int block_bytes;         // bytes of a block's 32 codes: 32 (e4m3), 16 (e2m1), 24 (e2m3); a code row is K / 32 of them
    int code_align;          // alignment of `codes` and of its rows, in bytes
    int k_mult;              // K is a multiple of it, and at least it
    const char* rows_rule;   // the rule of the rows, as its message words it
    const char* lds_name;    // how the messages name the leading dimension of the scales
};

// the body of apexmi_quant_blocks_mx*: `kernel` takes 16 elements per thread, (a, lda, M, K, codes, ldq, scales, lds)
template <class Kernel>
static int mx_quant_blocks(const MxQuantFormat& f, Kernel kernel, const void* a, int64_t lda, int M, int K, void* codes, int64_t ldq,
                           void* scales, int64_t lds_, hipStream_t stream) {
    APEXMI_REQUIRE(a && codes && scales, "%s: null operand", f.who);
    APEXMI_REQUIRE(M >= 1, "%s: M=%d must be at least 1", f.who, M);
    APEXMI_REQUIRE(K >= f.k_mult && K % f.k_mult == 0, "%s: K=%d must be a multiple of %d", f.who, K, f.k_mult);
    APEXMI_REQUIRE(lda >= K && ldq >= K / 32 * f.block_bytes && lda % 8 == 0 && ldq % f.code_align == 0 && ((uintptr_t)a % 16) == 0 &&
                       ((uintptr_t)codes % f.code_align) == 0,
                   "%s: %s (lda %lld, ldq %lld)", f.who, f.rows_rule, (long long)lda, (long long)ldq);
    APEXMI_REQUIRE(lds_ >= K / 32, "%s: rows of the block scales must be at least K / 32 = %d wide (%s %lld)", f.who, K / 32, f.lds_name,
                   (long long)lds_);
    ApexmiProfScope prof(5, stream, 0.0, (2.0 + (f.block_bytes + 1) / 32.0) * (double)M * K);     // bf16 in, codes and scale bytes out
    const int64_t threads = (int64_t)M * (K / 16);
    APEXMI_REQUIRE((threads + 255) / 256 < (1ll << 31), "%s: M=%d x K=%d is too large for one launch", f.who, M, K);
    hipLaunchKernelGGL(kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, (const bf16_t*)a, lda, M, K, (uint8_t*)codes,
                       ldq, (uint8_t*)scales, lds_);
    return apexmi_check_launch(f.who);
}

}  // namespace
