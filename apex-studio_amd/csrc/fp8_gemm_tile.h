// What the block-scaled-MFMA GEMMs share: the 128 x 128 output tile with 128-byte K-tiles, the operand record of ONE
// product and the f32 epilogue on the 32 x 32 result layout.  Included by gemm_fp8.hip (e4m3 x e4m3, every form) and gemm_mxfp4.hip
// (e2m1 x e2m1): the result layout of v_mfma_scale_f32_32x32x64_f8f6f4 does not depend on the operand format, so one epilogue
// serves both.
#pragma once
#include "common.h"
#include "fp8_quant.h"   // the MX output of the epilogue

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
template <int EPI, bool SCALED, bool MXIN = false, bool MXOUT = false>
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
                if constexpr (MXOUT) {
                    const uint32_t p0 = pack_bf16(o[0], o[1]), p1 = pack_bf16(o[2], o[3]);
                    mxv[4 * g] = bf16_lo(p0), mxv[4 * g + 1] = bf16_hi(p0), mxv[4 * g + 2] = bf16_lo(p1), mxv[4 * g + 3] = bf16_hi(p1);
#pragma unroll
                    for (int e = 0; e < 4; ++e) mxm = fmaxf(mxm, fabsf(mxv[4 * g + e]));
                } else {
                    if (m < G.M && n < G.N)
                        *(u32x2*)(G.C + (int64_t)m * G.ldc + n) = u32x2{pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
                }
            }
            if constexpr (MXOUT) {
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

}  // namespace
