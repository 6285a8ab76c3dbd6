// Variable-length attention forward over a PACKED batch: the contract of the reference's varlen backends ("sdpa_varlen",
// "flash_varlen": R/src/attention/functions.py:580-745, :932-1089) in one launch,
//   out[cu_q[i] + r] = softmax(scale q[cu_q[i] + r] K_i^T [causal]) V_i,   K_i / V_i = rows cu_k[i] .. cu_k[i + 1] - 1 of k / v,
// for n sequences packed along the token dimension: q [Tq, Hq, D], k / v [Tk, Hkv, D] read in place through element strides
// (token, head), grouped-query heads (query head h reads kv head h / (Hq / Hkv)), bf16 or f16, D = 64 or 128.  The two
// cu_seqlens arrays (int32, n + 1 entries, device memory) are read by the kernels only: the host sizes the launches from
// max_seqlen_q / max_seqlen_k and never synchronises.  causal is top-left aligned per sequence (local key j <= local query i).
// A sequence with queries and no keys stores zero rows (lse = -inf); rows at or past cu_q[n] are not written.
//
// One-pass flash kernel on the shared tile step (attn_tile.h), 4 waves x 32 rows = one 128-row query block of ONE sequence per
// workgroup, as attn_masked_kernel: blocks start at the sequence's first row and key tiles are 64 keys counted from the
// sequence's first key, so a sequence's rows see exactly the blocks, the tiles, the clamped rows and the per-wave rescale
// decisions of apexmi_attn_fwd_masked on that sequence alone, and come out bit-identical to it (out and lse).  No mask, no
// block map, no tile list: full tiles run the unmasked arithmetic, the key-tail tile and (causal) the tiles crossing the
// diagonal set the excluded scores to -inf per element, tiles above the diagonal are never visited.  The grid is
// n x Hq x ceil(max_seqlen_q / 128); a block at or past its sequence's length returns before any barrier or LDS-DMA.
//
// V^T staging.  The tile step reads V^T.  attn_varlen_vt_kernel writes sequence i into its own zero-padded SLOT of a
// [Hkv, D, pitch] array: columns align64(start_i) + 64 i .. + align64(len_i) - 1, pitch = align64(Tk) + 64 n.  Every slot begins
// on a 64-column boundary (the 16-byte LDS-DMA pieces), slot i + 1 begins at or after the end of slot i
// (align64(a) + align64(l) <= align64(a + l) + 64), the last ends inside the pitch, and the keys between len_i and
// align64(len_i) are zeros, so a probability of exactly 0 never meets uninitialised memory.
//
// Memory safety without a host check.  Both kernels clamp every sequence into its array, start = clamp(cu[i], 0, T),
// end = clamp(cu[i + 1], start, T), and its length to the max_seqlen they were launched for: a wrong cu_seqlens or a too-small
// max_seqlen truncates the result and never forms an address outside q / k / v / out / lse or the workspace.  Query rows past
// the end of a block's sequence are clamped to that sequence's LAST row and not stored.
#include "attn_host.h"
#include "attn_tile.h"

#include <cstdint>

namespace {

constexpr int VNW = 4;             // waves per workgroup
constexpr int VQB = VNW * 32;      // query rows per workgroup
constexpr float LN2 = 0.6931471805599453f;

struct VarlenArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* vt;
    uint16_t* o;
    float* lse;             // LSE kernels only: f32 [Hq, Tq] through element strides (head, token)
    const int* cu_q;
    const int* cu_k;
    int64_t q_st, q_sh, k_st, k_sh, o_st, o_sh, l_sh, l_st;   // element strides (token, head)
    int64_t pitch;          // columns of a V^T row
    int Tq, Tk, Hq, group, nqb, total, max_q, max_k, causal, neg;
    float c;                // |scale| * log2(e)
};

// sequence i of a packed array of T tokens, clamped into the array and to the launch's max_seqlen (wave-uniform)
APEXMI_DEVICE void seq_range(const int* cu, int i, int T, int max_len, int& start, int& len) {
    const int lo = __builtin_amdgcn_readfirstlane(cu[i]), hi = __builtin_amdgcn_readfirstlane(cu[i + 1]);
    start = min(max(lo, 0), T);
    len = min(min(max(hi, start), T) - start, max_len);
}

APEXMI_DEVICE int align64(int x) { return (x + 63) & ~63; }

// V rows of sequence z (strided, D contiguous) -> its slot of V^T [Hkv, D, pitch], keys >= len zero.  One workgroup per
// (64-key tile, kv head, sequence); tiles at or past the sequence's length exit (workgroup-uniform, before the barrier).
template <int D>
__global__ __launch_bounds__(256) void attn_varlen_vt_kernel(const uint16_t* __restrict__ v, int64_t st, int64_t sh,
                                                             const int* __restrict__ cu_k, int Tk, int max_k, int64_t pitch,
                                                             uint16_t* __restrict__ vt) {
    constexpr int LDW = D + 2;   // odd dword pitch: the column reads below spread over the banks
    __shared__ uint16_t tile[64 * LDW];
    const int tid = threadIdx.x;
    const int s0 = blockIdx.x * 64, h = blockIdx.y, z = blockIdx.z;
    int start, len;
    seq_range(cu_k, z, Tk, max_k, start, len);
    if (s0 >= len) return;
    const uint16_t* src = v + (int64_t)start * st + (int64_t)h * sh;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int idx = i * 256 + tid;
        const int r = idx / (D / 8), c = idx % (D / 8);
        u32x4 val = u32x4{0u, 0u, 0u, 0u};
        if (s0 + r < len) val = *(const u32x4*)(src + (int64_t)(s0 + r) * st + c * 8);
        uint32_t* dst = (uint32_t*)(tile + r * LDW + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = val[j];
    }
    __syncthreads();
    uint16_t* dstp = vt + (int64_t)h * D * pitch + align64(start) + 64 * z + s0;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int idx = i * 256 + tid;
        const int d = idx >> 3, sc = idx & 7;
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = (uint32_t)tile[(sc * 8 + 2 * j) * LDW + d] | ((uint32_t)tile[(sc * 8 + 2 * j + 1) * LDW + d] << 16);
        *(u32x4*)(dstp + (int64_t)d * pitch + sc * 8) = o;
    }
}

// LSE is a compile-time variant, as in attn_masked_kernel: the same loop, one logf and one f32 store per row more.
template <typename E, int D, bool LSE>
__global__ __launch_bounds__(VNW * 64, 2) void attn_varlen_kernel(const VarlenArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using v8 = typename E::v8;
    constexpr int K_TILE = KV * D * 2, V_TILE = D * KV * 2, STAGE = K_TILE + V_TILE;
    constexpr int NP = D / 8, LD = PIECES<D, VNW>, NDT = D / 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    // consecutive logical ids share a (sequence, head): its query blocks stay on one XCD
    const int s = xcd_remap(blockIdx.x, a.total);
    const int hb = s / a.nqb, qb = s % a.nqb;
    const int seq = hb / a.Hq, h = hb % a.Hq;
    const int hk = h / a.group;

    int q_start, Sq, k_start, Sk;
    seq_range(a.cu_q, seq, a.Tq, a.max_q, q_start, Sq);
    const int q0 = qb * VQB;
    if (q0 >= Sq) return;   // workgroup-uniform: an idle block, or an empty query sequence; nothing was issued yet
    seq_range(a.cu_k, seq, a.Tk, a.max_k, k_start, Sk);

    const uint16_t* Qp = a.q + (int64_t)q_start * a.q_st + (int64_t)h * a.q_sh;
    const uint16_t* Kp = a.k + (int64_t)k_start * a.k_st + (int64_t)hk * a.k_sh;
    const uint16_t* Vp = a.vt + (int64_t)hk * D * a.pitch + align64(k_start) + 64 * seq;

    const int qrow = q0 + wave * 32 + l31;      // local to the sequence, as every index below
    const int qrow_c = min(qrow, Sq - 1);       // never a row of the next sequence

    // key tiles 0 .. t_end - 1 of this sequence; causal blocks stop at the diagonal
    const int nt = (Sk + KV - 1) / KV;
    const int t_end = a.causal ? min(nt, min(q0 + VQB - 1, Sq - 1) / KV + 1) : nt;

    // Q fragments (B operand of S^T): lane supplies Q[qrow][16 ks + 8 hi .. +7]; a negative scale flips their signs (exact)
    v8 qf[D / 16];
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        u32x4 raw = *(const u32x4*)(Qp + (int64_t)qrow_c * a.q_st + ks * 16 + hi * 8);
        if (a.neg) raw ^= u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        qf[ks] = __builtin_bit_cast(v8, raw);
    }

    int k_key[LD], k_c[LD], v_row[LD], v_c[LD];
    stage_sources<D, VNW>(wave, lane, k_key, k_c, v_row, v_c);
    const uint16_t* v_src[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) v_src[i] = Vp + (int64_t)v_row[i] * a.pitch + v_c[i];
    auto stage = [&](int buf, int t) {   // only called with t < nt, so Sk >= 1
        char* base = smem + buf * STAGE + wave * 1024;
        const int kv0 = t * KV;
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * VNW + wave < NP) {   // wave-uniform
                const int key = min(kv0 + k_key[i], Sk - 1);
                glds16(Kp + (int64_t)key * a.k_st + k_c[i], base + i * (VNW * 1024));
            }
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * VNW + wave < NP) glds16(v_src[i] + kv0, base + K_TILE + i * (VNW * 1024));
    };

    int k_off[2], k_sw[2], v_off[NDT], v_sw[NDT];
    fragment_offsets<D>(l31, k_off, k_sw, v_off, v_sw);

    f32x16 oacc[NDT];
    clear(oacc);
    float m_run = SENTINEL;  // running maximum, base-2 domain, an integer
    float l_run = 0.0f;

    if (t_end > 0) stage(0, 0);
    for (int t = 0; t < t_end; ++t) {
        const int kv0 = t * KV;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile's LDS-DMA has landed (see attention.hip)
        __syncthreads();
        if (t + 1 < t_end) stage((t + 1) & 1, t + 1);
        const char* Ks = smem + (t & 1) * STAGE;

        f32x16 sacc[2];
        scores<E, D>(Ks, k_off, k_sw, hi, qf, sacc);

        // per-element path (workgroup-uniform): tiles crossing the causal diagonal, the key tail
        const bool elem = (a.causal && kv0 + KV - 1 > q0) || kv0 + KV > Sk;
        float mx;
        if (elem) {
            const int lim = a.causal ? min(Sk - 1, qrow) : Sk - 1;
            mx = -__builtin_inff();
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = fmaf(sacc[kt][r], a.c, 0.0f);
                    sacc[kt][r] = kv0 + tile_key(kt, r, hi) <= lim ? x : -__builtin_inff();
                    mx = fmaxf(mx, sacc[kt][r]);
                }
        } else {
            mx = tile_max(sacc) * a.c;
        }
        raise_max(max_xor32(mx), m_run, l_run, oacc);   // -inf (nothing allowed yet) never raises the sentinel
        l_run += elem ? exp2_scaled(sacc, m_run) : exp2_fused(sacc, a.c, m_run);

        v8 pf[4];
        p_fragments<E>(sacc, pf);
        accumulate<E, D>(Ks + K_TILE, v_off, v_sw, hi, pf, oacc);
    }

    // ---- epilogue: O[q][d] = O^T / l, 0 for a row without a key ----
    const float l_tot = sum_xor32(l_run);
    const float inv = l_tot > 0.0f ? 1.0f / l_tot : 0.0f;
    if (qrow < Sq) store_row<E>(a.o + (int64_t)(q_start + qrow) * a.o_st + (int64_t)h * a.o_sh, hi, oacc, inv);
    // ln sum_j exp(scale q k_j) = m ln 2 + ln l, -inf for a row without a key; the row's low-half lane stores it
    if constexpr (LSE) {
        if (hi == 0 && qrow < Sq)
            a.lse[(int64_t)h * a.l_sh + (int64_t)(q_start + qrow) * a.l_st] =
                l_tot > 0.0f ? fmaf(m_run, LN2, logf(l_tot)) : -__builtin_inff();
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int64_t vt_pitch(int Tk, int n) { return (((int64_t)Tk + KV - 1) / KV) * KV + (int64_t)KV * n; }

template <typename E, int D, bool LSE>
int launch_varlen(const VarlenArgs& a, hipStream_t stream) {
    constexpr int LDS = 2 * (2 * KV * D * 2);
    return launch_flash<attn_varlen_kernel<E, D, LSE>>(dim3(a.total), dim3(VNW * 64), LDS, LDS, stream, a, "attn_fwd_varlen");
}

template <typename E, int D>
int launch_varlen(const VarlenArgs& a, hipStream_t stream) {
    return a.lse ? launch_varlen<E, D, true>(a, stream) : launch_varlen<E, D, false>(a, stream);
}

}  // namespace

extern "C" size_t apexmi_attn_varlen_workspace_bytes(int Tk, int n, int Hkv, int D) {
    if (Tk <= 0 || n <= 0 || Hkv <= 0 || (D != 64 && D != 128)) return 0;
    return align256((size_t)Hkv * D * (size_t)vt_pitch(Tk, n) * 2);
}

extern "C" int apexmi_attn_fwd_varlen(const void* q, const void* k, const void* v, void* out, float* lse, const int* cu_seqlens_q,
                                      const int* cu_seqlens_k, int n, int Tq, int Tk, int Hq, int Hkv, int D, int max_seqlen_q,
                                      int max_seqlen_k, const int64_t q_strides[2], const int64_t k_strides[2],
                                      const int64_t v_strides[2], const int64_t o_strides[2], const int64_t lse_strides[2],
                                      int is_causal, float softmax_scale, int dtype, void* workspace, size_t workspace_bytes,
                                      apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "attn_fwd_varlen";
    if (int rc = require_operands(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides)) return rc;
    APEXMI_REQUIRE(cu_seqlens_q && cu_seqlens_k && ((uintptr_t)cu_seqlens_q % 4) == 0 && ((uintptr_t)cu_seqlens_k % 4) == 0,
                   "attn_fwd_varlen: null or misaligned cu_seqlens operand");
    if (int rc = require_lse(who, lse != nullptr, lse, lse_strides, "misaligned lse operand or null lse strides")) return rc;
    APEXMI_REQUIRE(n > 0 && Tq > 0 && Tk > 0 && Hq > 0 && Hkv > 0, "attn_fwd_varlen: empty problem (n=%d Tq=%d Tk=%d Hq=%d Hkv=%d)", n,
                   Tq, Tk, Hq, Hkv);
    APEXMI_REQUIRE(max_seqlen_q > 0 && max_seqlen_k > 0, "attn_fwd_varlen: max_seqlen_q=%d / max_seqlen_k=%d must be at least 1",
                   max_seqlen_q, max_seqlen_k);
    if (int rc = require_head_dim(who, D, D == 64 || D == 128, "64 or 128")) return rc;
    if (int rc = require_dtype(who, dtype)) return rc;
    if (int rc = require_head_ratio(who, Hq, Hkv)) return rc;
    // a sequence is never longer than its array: the clamped max_seqlen sizes the same launches
    const int max_q = max_seqlen_q < Tq ? max_seqlen_q : Tq, max_k = max_seqlen_k < Tk ? max_seqlen_k : Tk;
    const int nqb = (max_q + VQB - 1) / VQB;
    APEXMI_REQUIRE((int64_t)n * Hq * nqb < (1ll << 31) && n <= 65535 && Hkv <= 65535,
                   "attn_fwd_varlen: grid too large (n=%d sequences, Hq=%d, Hkv=%d, %d query blocks each)", n, Hq, Hkv, nqb);
    if (int rc = require_aligned(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides, 2)) return rc;
    if (int rc = require_workspace(who, workspace, workspace_bytes, apexmi_attn_varlen_workspace_bytes(Tk, n, Hkv, D), true)) return rc;

    VarlenArgs a{};
    a.q = (const uint16_t*)q, a.k = (const uint16_t*)k, a.vt = (const uint16_t*)workspace, a.o = (uint16_t*)out, a.lse = lse;
    a.cu_q = cu_seqlens_q, a.cu_k = cu_seqlens_k;
    a.q_st = q_strides[0], a.q_sh = q_strides[1], a.k_st = k_strides[0], a.k_sh = k_strides[1];
    a.o_st = o_strides[0], a.o_sh = o_strides[1];
    if (lse) a.l_sh = lse_strides[0], a.l_st = lse_strides[1];
    a.pitch = vt_pitch(Tk, n);
    a.Tq = Tq, a.Tk = Tk, a.Hq = Hq, a.group = Hq / Hkv, a.nqb = nqb, a.total = n * Hq * nqb;
    a.max_q = max_q, a.max_k = max_k;
    a.causal = is_causal ? 1 : 0;
    set_scale(a, softmax_scale);

    const dim3 vgrid((max_k + KV - 1) / KV, Hkv, n);
    if (D == 128)
        hipLaunchKernelGGL(attn_varlen_vt_kernel<128>, vgrid, dim3(256), 0, stream, (const uint16_t*)v, v_strides[0], v_strides[1],
                           cu_seqlens_k, Tk, max_k, a.pitch, (uint16_t*)workspace);
    else
        hipLaunchKernelGGL(attn_varlen_vt_kernel<64>, vgrid, dim3(256), 0, stream, (const uint16_t*)v, v_strides[0], v_strides[1],
                           cu_seqlens_k, Tk, max_k, a.pitch, (uint16_t*)workspace);
    if (int rc = apexmi_check_launch("attn_fwd_varlen (V^T)")) return rc;

    // the host does not know the lengths: the profile books the dense upper bound of the launch
    ApexmiProfScope prof(1, stream, 4.0 * Hq * (double)Tq * max_k * D, 0.0);
    if (dtype == APEXMI_BF16) return D == 128 ? launch_varlen<ElemBf16, 128>(a, stream) : launch_varlen<ElemBf16, 64>(a, stream);
    return D == 128 ? launch_varlen<ElemF16, 128>(a, stream) : launch_varlen<ElemF16, 64>(a, stream);
}
