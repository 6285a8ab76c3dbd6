// The 64-key tile step of the flash kernels that give a wave 32 query rows on v_mfma_f32_32x32x16: attn_fwd_d128_kernel
// (attention.hip), attn_masked_kernel (attention_masked.hip) and attn_dual_kernel (attention_dual.hip) are their own control flow
// around these pieces; the 8-wave c4 / mi16 / w64 kernels of attention.hip take the constants, perm32 and what fits their schedule.
// Device-only; E = element policy, D = head dim, NW = waves per workgroup, NDT = D / 32.  Everything works on arrays the caller owns.
//
// Layout.  Both products are swapped (S^T = K Q^T, O^T = V^T P^T) so lane l owns query row l & 31 (l31), its half hi = l >> 5:
//   K image   [64 rows][D / 8 chunks of 16 bytes], chunk ^= row & (D / 8 - 1), row i <- key (i & 32) + perm32(i & 31);
//   V^T image [D rows][8 chunks], chunk ^= (row >> 1) & 7;
// each image is D / 8 pieces of 1 KiB (one 16-byte global_load_lds per lane), piece i NW + wave belongs to wave `wave`.
// sacc[kt][r] is the score of key tile_key(kt, r, hi) of the tile, so registers 8 (kk & 1) .. + 7 of sacc[kk >> 1] are the 8
// CONSECUTIVE keys 16 kk + 8 hi .. + 7: P feeds the P V MFMA unshuffled and a V^T fragment is one ds_read_b128.
// oacc[dt][4 g + j] is O[query l31][d = 32 dt + 8 g + 4 hi + j].
//
// Rounding.  Online softmax in the base-2 domain with a DEFERRED rescale: the running maximum is raised (and O, l rescaled) only
// when some row's tile maximum exceeds it by more than DEFER, so p = 2^(s c - m) stays <= 2^DEFER and in steady state the rescale
// of O is skipped.  Every P of a tile is exponentiated after the decision that covers it.  The running maximum is kept an INTEGER
// (ceil): every rescale factor 2^(m_old - m_new) is then an exact power of two and bf16(2^k p) = 2^k bf16(p), so the rounding of P
// (and with it the result) does not depend on the key-tile order, the threshold or a key-range split:
//   O = sum_j bf16(2^(s_j c - M)) v_j / sum_j 2^(s_j c - M)   for ANY integer M, up to f32 summation order.
// That is what lets the CPU oracle reproduce the kernels' rounding points (oracle.layers.sdpa) without replaying their schedule,
// and what makes the three kernels agree bit for bit on an unmasked problem.
#pragma once
#include "common.h"

// unnamed: the kernels' mangled names (build.py NO_SPILL, the profiles) carry the namespace of the element policies
namespace {

constexpr int KV = 64;                          // keys per tile
constexpr float DEFER = 6.0f;                   // raise a running maximum only when a tile maximum exceeds it by more than 2^6
constexpr float SENTINEL = -1.0e30f;            // finite start of a running maximum; the plain kernels' excluded raw score
constexpr float LOG2E = 1.4426950408889634f;

typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;

struct ElemBf16 {
    using v8 = bf16x8;
    static APEXMI_DEVICE f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
    static APEXMI_DEVICE void cvt(v8& r, int j, float x) { r[j] = (__bf16)x; }
    static APEXMI_DEVICE uint32_t pack2(float a, float b) { return pack_bf16(a, b); }
};
struct ElemF16 {
    using v8 = f16x8;
    static APEXMI_DEVICE f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
    static APEXMI_DEVICE void cvt(v8& r, int j, float x) { r[j] = (_Float16)x; }
    static APEXMI_DEVICE uint32_t pack2(float a, float b) {
        f16x2 r;
        r[0] = (_Float16)a;
        r[1] = (_Float16)b;
        return __builtin_bit_cast(uint32_t, r);
    }
};

// row i of a 32-row K sub-tile holds key perm32(i): bits 2 and 3 swapped
APEXMI_DEVICE int perm32(int i) { return (i & ~0xC) | ((i & 4) << 1) | ((i & 8) >> 1); }

// key (within the tile) of score register r of sacc[kt]
APEXMI_DEVICE int tile_key(int kt, int r, int hi) {
    const int g = r >> 2;
    return kt * 32 + 16 * (g >> 1) + 8 * hi + 4 * (g & 1) + (r & 3);
}

template <int D, int NW>
constexpr int PIECES = (D / 8 + NW - 1) / NW;   // pieces per wave per image; piece i of a wave exists iff i NW + wave < D / 8

// staging sources of this lane's pieces: K = key k_key (within the tile), element k_c of its row; V^T = row v_row, element v_c
template <int D, int NW>
APEXMI_DEVICE void stage_sources(int wave, int lane, int (&k_key)[PIECES<D, NW>], int (&k_c)[PIECES<D, NW>],
                                 int (&v_row)[PIECES<D, NW>], int (&v_c)[PIECES<D, NW>]) {
    constexpr int CH = D / 8;
#pragma unroll
    for (int i = 0; i < PIECES<D, NW>; ++i) {
        const int p = (i * NW + wave) * 64 + lane;
        const int krow = (p / CH) & 63, kpc = p % CH;
        k_c[i] = (kpc ^ (krow & (CH - 1))) * 8;
        k_key[i] = (krow & 32) + perm32(krow & 31);
        const int vrow = (p >> 3) & (D - 1), vpc = p & 7;
        v_row[i] = vrow;
        v_c[i] = (vpc ^ ((vrow >> 1) & 7)) * 8;
    }
}

// fragment reads: byte offset of the lane's image row and the swizzle of its chunk index
template <int D>
APEXMI_DEVICE void fragment_offsets(int l31, int (&k_off)[2], int (&k_sw)[2], int (&v_off)[D / 32], int (&v_sw)[D / 32]) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int row = kt * 32 + l31;
        k_off[kt] = row * (D * 2);
        k_sw[kt] = row & (D / 8 - 1);
    }
#pragma unroll
    for (int dt = 0; dt < D / 32; ++dt) {
        const int row = dt * 32 + l31;
        v_off[dt] = row * 128;
        v_sw[dt] = (row >> 1) & 7;
    }
}

template <int N>
APEXMI_DEVICE void clear(f32x16 (&a)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) a[i][r] = 0.0f;
}

// S^T = K Q^T
template <typename E, int D>
APEXMI_DEVICE void scores(const char* Ks, const int (&k_off)[2], const int (&k_sw)[2], int hi, const typename E::v8 (&qf)[D / 16],
                          f32x16 (&sacc)[2]) {
    clear(sacc);
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        const int c = ks * 2 + hi;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const typename E::v8 kf = *(const typename E::v8*)(Ks + k_off[kt] + ((c ^ k_sw[kt]) << 4));
            sacc[kt] = E::mfma(kf, qf[ks], sacc[kt]);
        }
    }
}

// maximum of the lane's 32 scores (the row's other half is in lane l ^ 32: max_xor32)
APEXMI_DEVICE float tile_max(const f32x16 (&sacc)[2]) {
    float mx = sacc[0][0];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kt][r]);
    return mx;
}

// the deferred integer rescale (wave-uniform branch); mx = the row's tile maximum, -inf (nothing allowed) never raises
template <int NDT>
APEXMI_DEVICE void raise_max(float mx, float& m_run, float& l_run, f32x16 (&oacc)[NDT]) {
    if (__any(mx > m_run + DEFER)) {
        const float m_new = ceilf(fmaxf(m_run, mx));
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
    }
}

// sacc <- p; returns the lane's part of the row sum.  Fused: raw scores, p = 2^(s c - m) in one fma.
APEXMI_DEVICE float exp2_fused(f32x16 (&sacc)[2], float c, float m) {
    float psum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = fast_exp2(fmaf(sacc[kt][r], c, -m));
            sacc[kt][r] = p;
            psum += p;
        }
    return psum;
}
// Post-scaled: the scores already are s c (+ mask) or -inf, p = 2^(s - m)
APEXMI_DEVICE float exp2_scaled(f32x16 (&sacc)[2], float m) {
    float psum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = fast_exp2(sacc[kt][r] - m);
            sacc[kt][r] = p;
            psum += p;
        }
    return psum;
}

// P -> B-fragments: k-step kk takes registers 8 (kk & 1) .. + 7 of sacc[kk >> 1]
template <typename E>
APEXMI_DEVICE void p_fragments(const f32x16 (&sacc)[2], typename E::v8 (&pf)[4]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) E::cvt(pf[kk], j, sacc[kk >> 1][8 * (kk & 1) + j]);
}

// O^T += V^T P^T
template <typename E, int D>
APEXMI_DEVICE void accumulate(const char* Vs, const int (&v_off)[D / 32], const int (&v_sw)[D / 32], int hi,
                              const typename E::v8 (&pf)[4], f32x16 (&oacc)[D / 32]) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int c = kk * 2 + hi;
#pragma unroll
        for (int dt = 0; dt < D / 32; ++dt) {
            const typename E::v8 vf = *(const typename E::v8*)(Vs + v_off[dt] + ((c ^ v_sw[dt]) << 4));
            oacc[dt] = E::mfma(vf, pf[kk], oacc[dt]);
        }
    }
}

// normalise, round and store the lane's part of one output row (op = the row's address): d = 32 dt + 8 g + 4 hi + (0..3)
template <typename E, int NDT>
APEXMI_DEVICE void store_row(uint16_t* op, int hi, const f32x16 (&oacc)[NDT], float inv) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u32x2 o;
            o[0] = E::pack2(oacc[dt][4 * g + 0] * inv, oacc[dt][4 * g + 1] * inv);
            o[1] = E::pack2(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
            *(u32x2*)(op + dt * 32 + g * 8 + hi * 4) = o;
        }
}

}  // namespace
