// Wide-head attention forward: out = softmax(q k^T * scale [frame rule]) v for D = 256, 384 or 512, bf16 or f16, ONE launch over
// all (batch, head, 128-row query block) units and no O(Sq Sk) buffer.  It is the flash form of what attn_fwd_impl's materialised
// path (attention.hip) does with four launches per (batch, head) for the mid-block attention of the VAEs (Wan / QwenImage C = 384,
// Flux C = 512, HunyuanVideo-1.5 frame-causal).  Opt-in (ops.attention_wide, the VAEs' set_mid_attention("flash")): it keeps the
// ROUNDING CONTRACT of attn_tile.h — integer base-2 running maximum, deferred rescale, row sum over the unrounded p, p rounded to
// the storage type as the P V operand — which is oracle.layers.sdpa's bf16 policy and NOT the materialised path's (that one
// normalises before it rounds P), so the two paths differ in the last bits.
//
// One-pass online softmax on the shared tile step (attn_tile.h: tile_max / exp2_* / p_fragments; the two MFMA loops are
// this file's register-bounded forms of its scores / accumulate, same reads and MFMAs in the same order), 4 waves
// of 32 query rows, one workgroup per CU (__launch_bounds__(256, 1): 512 registers a lane).  Per lane: the Q fragments (D / 4
// registers) and the O accumulators (D / 2) stay in registers for the whole key loop.
//   * q, k and out are read / written in place through element strides (b, h, s); V^T [B, H, D, Skp] is staged in the workspace
//     by apexmi_v_transpose (128-column slices, keys >= Sk zero) and is the ONLY workspace: O(B H D Skp).
//   * LDS: ONE 64-key K image (128 D bytes) and ONE V^T image (128 D bytes), 64 / 96 / 128 KiB at D = 256 / 384 / 512 (two
//     double-buffered stages do not fit 160 KiB at D = 512).  The two are refilled alternately by global_load_lds: K of tile t + 1
//     is issued when every wave has finished Q K^T of tile t and lands under the softmax and P V of tile t; V^T of tile t is issued
//     when every wave has finished P V of tile t - 1 and lands under Q K^T of tile t.  Three barriers a tile.
//   * images: K [64 rows][D / 8 chunks of 16 bytes], chunk ^= row & 15, row i <- key (i & 32) + perm32(i & 31); V^T as in
//     attn_tile.h.  The K swizzle of attn_tile.h (row & (D / 8 - 1)) needs D / 8 to be a power of two, and 48 is not; a row is a
//     whole number of 256-byte bank rounds at every D here, so the low four chunk bits are all that decide the banks.
//   * frame rule (frame_tokens > 0, Sq == Sk, S % frame_tokens == 0): key j is allowed for query i iff j / ft <= i / ft.  Handled
//     as attn_masked_kernel handles `causal`: a workgroup's key tiles end at its last row's frame end, only the tiles that reach
//     past the FIRST row's frame end compare per element, excluded scores are -inf before the maximum.  Every row owns its whole
//     frame and tile 0 holds key 0, so the running maximum is finite after the first tile and no row is empty.  Query blocks run
//     last (longest) first.
//   * rows past Sq and keys past Sk use clamped indices (qrow_c, min(key, Sk - 1)): no out-of-range address is formed; the clamped
//     keys' scores are -inf (the key tail takes the per-element form), the clamped rows are not stored.
//   * MODE (apexmi_attn_fwd_wide_split) is a compile-time variant: the MODE 0 instantiations keep their device code.  MODE 1 and 2
//     take a grid of units x n (n = 1 .. 8 key splits): workgroup (unit, split) walks tiles [t_beg, t_lim) of the unit's own t_end
//     tiles, per = ceil(t_end / n), t_beg = min(split per, t_end), t_lim = min(t_beg + per, t_end), and every row stores its lse =
//     m ln 2 + ln l (-inf for l = 0).  MODE 1 (n == 1) stores `out` as MODE 0 does; MODE 2 (n > 1) stores the NORMALISED O in f32
//     as partial [split][b][q][h][d] instead (two epilogues in one kernel spill at D = 512), which attn_merge_f32 (attention_masked.hip, a plain second launch) combines: no workgroup
//     waits on, counts or signals another.  The units of one split are adjacent in launch order (split = id / units): an XCD's
//     neighbours walk the same key tiles of one (batch, head) and share them in its L2; under the frame rule each split's query
//     blocks still run longest first.  What "no row is empty" rules out above happens here: a workgroup whose range is empty
//     (fewer tiles than splits) stores lse = -inf and leaves its partial rows unwritten (weight 0 in the merge), and under the
//     frame rule a row may find every key of the range excluded beside live rows of its wave: its maximum stays SENTINEL
//     (wide_raise_max: m_new = SENTINEL, alpha = 2^0), every p is 2^(-inf) = 0, the partial is 0 and the lse -inf.
#include "attn_host.h"
#include "attn_tile.h"

#include <algorithm>
#include <cstdint>

namespace {

constexpr int WNW = 4;             // waves per workgroup
constexpr int WQB = WNW * 32;      // query rows per workgroup

struct WideArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* vt;
    uint16_t* o;
    int64_t q_sb, q_sh, q_ss, k_sb, k_sh, k_ss, o_sb, o_ss, o_sh;
    int H, Sq, Sk, Skp, nqb, total, neg, ft;
    float c;                // |scale| * log2(e)
};

// the SPLIT variant's own arguments behind the shared ones
struct WideSplitArgs : WideArgs {
    float* lse;             // n == 1: the caller's; n > 1: the workspace's [n, B, H, Sq]
    float* part;            // n > 1: f32 partials [n, B, Sq, H, D]
    int64_t l_sp, l_sb, l_sh, l_sq;   // lse element strides (split, b, h, q)
    int B, n;
};

constexpr float LN2 = 0.6931471805599453f;

// Staging sources of a lane.  Piece i (1 KiB) of wave `wave` is positions (4 i + wave) 64 + lane of an image, 16 bytes each.
// K image, CH = D / 8 chunks a row: PER = D / 128 pieces of a wave step through 16 rows (4 PER 64 positions = 16 CH), so piece
// j PER + r sits 16 j rows below piece r, with the same swizzle (row & 15) and its key 16 j higher (perm32 moves bits 2, 3 only):
// the lane keeps PER (key, element) pairs instead of D / 32.  V^T image: piece i is rows 32 i + 8 wave + lane / 8, and the swizzle
// ((row >> 1) & 7) does not depend on i: one byte offset (v_off in the kernel) and 32 i rows.
template <int D>
APEXMI_DEVICE void wide_stage_sources(int wave, int lane, int (&k_key)[D / 128], int (&k_c)[D / 128]) {
    constexpr int CH = D / 8;
#pragma unroll
    for (int r = 0; r < D / 128; ++r) {
        const int p = (r * WNW + wave) * 64 + lane;
        const int krow = p / CH, kpc = p % CH;       // krow < 16
        k_c[r] = (kpc ^ (krow & 15)) * 8;
        k_key[r] = perm32(krow);
    }
}

// Fragment reads.  attn_tile.h's scores / accumulate take one byte offset and one swizzle per image row (2 + D / 32 register
// pairs) and leave the order of their D / 8 ds_read_b128 to the compiler, which hoists them all: at D = 384 / 512 that spills
// (82 / 289 VGPRs).  The same reads and the same MFMAs in the same order, with the addresses folded and the reads bounded:
//   K   row r = 32 kt + l31, chunk c = 2 ks + hi:  r D 2 + ((c ^ (r & 15)) << 4) = (ka ^ 32 (ks & 7)) + 256 (ks >> 3) + 64 D kt
//       with ka = l31 D 2 | ((hi ^ (l31 & 15)) << 4)   (a row is a multiple of 256 bytes)
//   V^T row r = 32 dt + l31, chunk c = 2 kk + hi:  (va ^ 32 kk) + 4096 dt   with va = l31 128 | ((hi ^ ((l31 >> 1) & 7)) << 4)
// i.e. one v_xor and an immediate offset a read.  The reads run one group (2 or 4 fragments) ahead of the MFMAs that
// consume them, a sched_barrier after every group keeps the compiler from hoisting further.
template <typename E, int D>
APEXMI_DEVICE void wide_scores(const char* Ks, int ka, const typename E::v8 (&qf)[D / 16], f32x16 (&sacc)[2]) {
    using v8 = typename E::v8;
    constexpr int G = D == 512 ? 1 : 2, NG = D / 16 / G;   // k-steps per group (D = 512: Q alone is half the VGPRs)
    clear(sacc);
    v8 kf[2][2 * G];
    auto load = [&](v8 (&f)[2 * G], int g) {
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                const int ks = g * G + u;
                f[2 * u + kt] = *(const v8*)(Ks + (ka ^ (32 * (ks & 7))) + 256 * (ks >> 3) + 64 * D * kt);
            }
    };
    load(kf[0], 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) load(kf[(g + 1) & 1], g + 1);
#pragma unroll
        for (int u = 0; u < G; ++u)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) sacc[kt] = E::mfma(kf[g & 1][2 * u + kt], qf[g * G + u], sacc[kt]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <typename E, int D>
APEXMI_DEVICE void wide_accumulate(const char* Vs, int va, const typename E::v8 (&pf)[4], f32x16 (&oacc)[D / 32]) {
    using v8 = typename E::v8;
    constexpr int G = D == 512 ? 2 : 4, NDG = D / 32 / G, NG = 4 * NDG;   // d-tiles per group; group g = (kk = g / NDG, d-tiles G (g % NDG) ..)
    v8 vf[2][G];
    auto load = [&](v8 (&f)[G], int g) {
#pragma unroll
        for (int u = 0; u < G; ++u) f[u] = *(const v8*)(Vs + (va ^ (32 * (g / NDG))) + 4096 * ((g % NDG) * G + u));
    };
    load(vf[0], 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        if (g + 1 < NG) load(vf[(g + 1) & 1], g + 1);
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int dt = (g % NDG) * G + u;
            oacc[dt] = E::mfma(vf[g & 1][u], pf[g / NDG], oacc[dt]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// attn_tile.h's raise_max with the rescale of O done where O lives.  The 32 D / 64 accumulator registers only fit as AGPRs, and a
// plain `oacc *= alpha` makes the compiler keep O in VGPRs around the branch (a copy of all of it to and from the AGPRs every tile,
// and spills from D = 384 up).  The "a" constraints pin O to the AGPRs: read, multiply, write back, through one VGPR.  Every MFMA
// that wrote O has retired long before (the scores MFMAs issued after them have been read), and the next MFMA that reads O comes
// after the exponentials, so the statement needs no wait states around it.
template <int NDT>
APEXMI_DEVICE void wide_raise_max(float mx, float& m_run, float& l_run, f32x16 (&oacc)[NDT]) {
    if (__any(mx > m_run + DEFER)) {
        const float m_new = ceilf(fmaxf(m_run, mx));
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float x = oacc[dt][r], t;
                asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1"
                             : "+a"(x), "=&v"(t)
                             : "v"(alpha));
                oacc[dt][r] = x;
            }
    }
}

#define WIDE_BAR()                             \
    do {                                       \
        __builtin_amdgcn_sched_barrier(0);     \
        __builtin_amdgcn_s_barrier();          \
        __builtin_amdgcn_sched_barrier(0);     \
    } while (0)

template <int MODE>
struct WideArgsOf { using type = WideSplitArgs; };
template <>
struct WideArgsOf<0> { using type = WideArgs; };

// MODE 0: out;  1: out and lse (n == 1);  2: f32 partial and lse (n > 1)
template <typename E, int D, int MODE = 0>
__global__ __launch_bounds__(WNW * 64, 1) void attn_wide_kernel(const typename WideArgsOf<MODE>::type a) {
    constexpr bool SPLIT = MODE != 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using v8 = typename E::v8;
    constexpr int K_TILE = KV * D * 2;
    constexpr int LD = D / 32, PER = D / 128, NDT = D / 32;   // pieces per wave per image; LD = 4 PER
    static_assert(D % 128 == 0 && D >= 256 && D <= 512, "attn_wide_kernel: D = 256, 384 or 512");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // consecutive units of one (batch, head) stay on one XCD; under the frame rule its query blocks run longest first
    int s, split = 0;
    if constexpr (SPLIT) {   // the units of one split are adjacent
        s = xcd_remap(blockIdx.x, a.total * a.n);
        split = s / a.total;
        s -= split * a.total;
    } else {
        s = xcd_remap(blockIdx.x, a.total);
    }
    const int hb = s / a.nqb;
    const int qb = a.ft ? a.nqb - 1 - s % a.nqb : s % a.nqb;
    const int b = hb / a.H, h = hb % a.H;

    const uint16_t* Qp = a.q + (int64_t)b * a.q_sb + (int64_t)h * a.q_sh;
    const uint16_t* Kp = a.k + (int64_t)b * a.k_sb + (int64_t)h * a.k_sh;
    const uint16_t* Vp = a.vt + (int64_t)hb * D * a.Skp;

    const int q0 = qb * WQB;
    const int qrow_c = min(q0 + wave * 32 + (lane & 31), a.Sq - 1);

    // key range of the workgroup, first key position from which a tile compares per element, last allowed key of the lane's row
    int k_end = a.Sk, elem_from = a.Sk, lim = a.Sk - 1;
    if (a.ft) {
        k_end = (min(q0 + WQB - 1, a.Sq - 1) / a.ft + 1) * a.ft;   // <= S
        elem_from = (q0 / a.ft + 1) * a.ft;
        lim = (qrow_c / a.ft + 1) * a.ft - 1;
    }
    const int t_end = (k_end + KV - 1) / KV;   // >= 1
    int t_beg = 0, t_lim = t_end;              // the workgroup's tiles; SPLIT: its share of the unit's, possibly none
    if constexpr (SPLIT) {
        const int per = (t_end + a.n - 1) / a.n;
        t_beg = min(split * per, t_end);
        t_lim = min(t_beg + per, t_end);
    }

    // Q fragments (B operand of S^T): lane supplies Q[qrow][16 ks + 8 hi .. +7]; a negative scale flips their signs (exact)
    v8 qf[D / 16];
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        u32x4 raw = *(const u32x4*)(Qp + (int64_t)qrow_c * a.q_ss + ks * 16 + (lane >> 5) * 8);
        if (a.neg) raw ^= u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        qf[ks] = __builtin_bit_cast(v8, raw);
    }

    int k_key[PER], k_c[PER];
    wide_stage_sources<D>(wave, lane, k_key, k_c);
    // one uniform base and a 32-bit byte offset a piece (the entry point bounds both images below 4 GiB per (batch, head)): a
    // 64-bit address a piece is 2 D / 32 VGPRs the D = 512 instantiation does not have
    const uint32_t k_ss = (uint32_t)a.k_ss * 2, v_ss = (uint32_t)a.Skp * 2;
    char* const Ks = smem;
    char* const Vs = smem + K_TILE;
    // The lane number, made opaque once per tile and after the loop: what derives from it (hi, the LDS read addresses, the V^T
    // piece offset, the D / 4 addresses one xor / add away from those, and the row and output address of the epilogue) is then
    // recomputed where it is used, a few VALU operations a tile, instead of living in VGPRs across the loop; the D = 512
    // instantiation (Q alone is 128 VGPRs, the scores 32 more) has none to spare.
    int lane_o = lane;
    uint32_t v_off = 0;
    // D = 512 (64 chunks a row): a piece of K is one whole row, its key is wave-uniform and the lane is the chunk
    auto stage_k = [&](int kv0) {
        if constexpr (D == 512) {
#pragma unroll
            for (int i = 0; i < LD; ++i) {   // row 4 i + wave: perm32 moves bits 2, 3 only, so key and swizzle split into wave + constant
                const int key = min(kv0 + wave + ((4 * i) & 32) + perm32((4 * i) & 31), a.Sk - 1);
                glds16((const char*)Kp + ((uint32_t)key * k_ss + (uint32_t)((lane_o ^ wave ^ ((4 * i) & 15)) * 16)),
                       Ks + wave * 1024 + i * (WNW * 1024));
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < PER; ++r) {
                const int key = min(kv0 + k_key[r] + 16 * j, a.Sk - 1);
                glds16((const char*)Kp + ((uint32_t)key * k_ss + (uint32_t)k_c[r] * 2), Ks + wave * 1024 + (j * PER + r) * (WNW * 1024));
            }
    };
    auto stage_v = [&](int kv0) {   // V^T rows are Skp long, kv0 + 63 < Skp
#pragma unroll
        for (int i = 0; i < LD; ++i)
            glds16((const char*)Vp + (v_off + (uint32_t)(i * 32) * v_ss + (uint32_t)kv0 * 2), Vs + wave * 1024 + i * (WNW * 1024));
    };

    f32x16 oacc[NDT];
    clear(oacc);
    float m_run = SENTINEL;  // running maximum, base-2 domain, an integer
    float l_run = 0.0f;

    if (!SPLIT || t_beg < t_lim) stage_k(t_beg * KV);
    for (int t = t_beg; t < t_lim; ++t) {
        const int kv0 = t * KV;
        const bool more = t + 1 < t_lim;
        asm volatile("" : "+v"(lane_o));
        if constexpr (D != 512) {
#pragma unroll
            for (int r = 0; r < PER; ++r) asm volatile("" : "+v"(k_key[r]), "+v"(k_c[r]));
        }
        const int l31 = lane_o & 31, hi = lane_o >> 5;
        const int ka = l31 * (D * 2) | ((hi ^ (l31 & 15)) << 4);
        const int va = l31 * 128 | ((hi ^ ((l31 >> 1) & 7)) << 4);
        v_off = (uint32_t)(wave * 8 + (lane_o >> 3)) * v_ss + (uint32_t)(((lane_o & 7) ^ ((wave * 4 + (lane_o >> 4)) & 7)) * 16);
        // K of this tile has landed (this wave's pieces; the barrier makes it every wave's), and every wave is past P V of the
        // tile before: the V^T image is free.  hipcc does not add the vmcnt for LDS-DMA to a barrier (attention.hip).
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        WIDE_BAR();
        stage_v(kv0);

        f32x16 sacc[2];
        wide_scores<E, D>(Ks, ka, qf, sacc);

        // every wave has read its K fragments: the K image is free for the next tile
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        WIDE_BAR();
        if (more) stage_k(kv0 + KV);

        // per-element form (workgroup-uniform): the key tail and, under the frame rule, the tiles past the first row's frame end
        const bool elem = kv0 + KV > elem_from;
        float mx;
        if (elem) {
            mx = -__builtin_inff();
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = sacc[kt][r] * a.c;
                    sacc[kt][r] = kv0 + tile_key(kt, r, hi) <= lim ? x : -__builtin_inff();
                    mx = fmaxf(mx, sacc[kt][r]);
                }
        } else {
            mx = tile_max(sacc) * a.c;
        }
        wide_raise_max(max_xor32(mx), m_run, l_run, oacc);   // -inf (a later frame's tile) never raises
        l_run += elem ? exp2_scaled(sacc, m_run) : exp2_fused(sacc, a.c, m_run);

        v8 pf[4];
        p_fragments<E>(sacc, pf);

        // V^T of this tile has landed; the next tile's K pieces (issued after it) may still be on their way
        if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        WIDE_BAR();
        wide_accumulate<E, D>(Vs, va, pf, oacc);
    }

    // ---- epilogue: O[q][d] = O^T / l ----
    const float l_tot = sum_xor32(l_run);
    const float inv = l_tot > 0.0f ? 1.0f / l_tot : 0.0f;
    // attn_tile.h's store_row one d-tile at a time: left to itself the compiler reads all of O out of the AGPRs first
    asm volatile("" : "+v"(lane_o));
    const int qrow = q0 + wave * 32 + (lane_o & 31), hi = lane_o >> 5;
    if constexpr (SPLIT) {
        // ln sum_j exp(scale q k_j) over the workgroup's keys = m ln 2 + ln l, -inf for a row without one (attn_masked_kernel's
        // line); the row's low-half lane stores it
        if (hi == 0 && qrow < a.Sq)
            a.lse[(int64_t)split * a.l_sp + (int64_t)b * a.l_sb + (int64_t)h * a.l_sh + (int64_t)qrow * a.l_sq] =
                l_tot > 0.0f ? fmaf(m_run, LN2, logf(l_tot)) : -__builtin_inff();
        if constexpr (MODE == 2) {   // the normalised partial in f32; an empty range leaves its rows unwritten (weight 0 in the merge)
            if (qrow < a.Sq && t_beg < t_lim) {
                float* pp = a.part + ((((int64_t)split * a.B + b) * a.Sq + qrow) * a.H + h) * D;
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    // O stays in the AGPRs up to here: the 16-byte stores hold four times the bf16 epilogue's data in flight, and
                    // at D = 512 the compiler otherwise copies all of O out before the first store and spills
#pragma unroll
                    for (int r = 0; r < 16; ++r) asm volatile("" : "+a"(oacc[dt][r]));
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *(f32x4*)(pp + dt * 32 + g * 8 + hi * 4) = f32x4{oacc[dt][4 * g + 0] * inv, oacc[dt][4 * g + 1] * inv,
                                                                         oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv};
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            return;
        }
    }
    if (qrow < a.Sq) {
        uint16_t* op = a.o + (int64_t)b * a.o_sb + (int64_t)qrow * a.o_ss + (int64_t)h * a.o_sh;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 o;
                o[0] = E::pack2(oacc[dt][4 * g + 0] * inv, oacc[dt][4 * g + 1] * inv);
                o[1] = E::pack2(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
                *(u32x2*)(op + dt * 32 + g * 8 + hi * 4) = o;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <typename E, int D>
int launch_wide(const WideArgs& a, hipStream_t stream) {
    constexpr int LDS = 2 * KV * D * 2;
    return launch_flash<attn_wide_kernel<E, D>>(dim3(a.total), dim3(WNW * 64), LDS, LDS, stream, a, "attn_fwd_wide");
}

template <typename E, int D>
int launch_wide(const WideSplitArgs& a, hipStream_t stream) {
    constexpr int LDS = 2 * KV * D * 2;
    if (a.n == 1)
        return launch_flash<attn_wide_kernel<E, D, 1>>(dim3(a.total), dim3(WNW * 64), LDS, LDS, stream, a, "attn_fwd_wide_split (lse)");
    return launch_flash<attn_wide_kernel<E, D, 2>>(dim3(a.total * a.n), dim3(WNW * 64), LDS, LDS, stream, a, "attn_fwd_wide_split");
}

template <typename E, typename A>
int launch_wide_d(int D, const A& a, hipStream_t stream) {
    return D == 256 ? launch_wide<E, 256>(a, stream) : D == 384 ? launch_wide<E, 384>(a, stream) : launch_wide<E, 512>(a, stream);
}

bool wide_dim(int D) { return D == 256 || D == 384 || D == 512; }

constexpr int WIDE_SPLITS_MAX = 8;

// apexmi_attn_fwd_wide and apexmi_attn_fwd_wide_split: one argument check, one V^T pre-pass, two families of instantiations.
// key_splits and lse belong to the second entry point only (the first passes 1 and nullptr and launches what it always did).
int fwd_wide(const char* who, const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk, int D,
             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides,
             float softmax_scale, int dtype, int frame_tokens, float* lse, const int64_t* lse_strides, int key_splits,
             void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (int rc = require_operands(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides)) return rc;
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0, "%s: empty problem (B=%d H=%d Sq=%d Sk=%d)", who, B, H, Sq, Sk);
    if (int rc = require_head_dim(who, D, wide_dim(D), "256, 384 or 512; wider heads stay on apexmi_attn_fwd's materialised path"))
        return rc;
    if (int rc = require_dtype(who, dtype)) return rc;
    APEXMI_REQUIRE(frame_tokens >= 0, "%s: negative frame_tokens %d", who, frame_tokens);
    APEXMI_REQUIRE(frame_tokens == 0 || (Sq == Sk && Sq % frame_tokens == 0),
                   "%s: the frame rule needs Sq == Sk and a whole number of frames of %d tokens (Sq=%d Sk=%d)", who,
                   frame_tokens, Sq, Sk);
    const int64_t units = (int64_t)B * H * ((Sq + WQB - 1) / WQB);
    APEXMI_REQUIRE(units < (1ll << 31), "%s: too many query blocks", who);
    // the kernel addresses a (batch, head)'s K rows and V^T image with 32-bit byte offsets
    APEXMI_REQUIRE(k_strides[2] >= D, "%s: key row stride %lld below the head dim %d (rows must not overlap)", who,
                   (long long)k_strides[2], D);
    APEXMI_REQUIRE((int64_t)Sk * k_strides[2] < (1ll << 31) && (int64_t)D * (Sk + KV) < (1ll << 31),
                   "%s: the keys of one (batch, head) span 4 GiB or more (Sk=%d, row stride %lld)", who, Sk,
                   (long long)k_strides[2]);
    if (int rc = require_aligned(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides, 3)) return rc;
    APEXMI_REQUIRE(key_splits >= 0 && key_splits <= WIDE_SPLITS_MAX, "%s: key_splits=%d unsupported (0 = auto, 1 to %d)", who,
                   key_splits, WIDE_SPLITS_MAX);
    if (int rc = require_lse(who, lse != nullptr, lse, lse_strides, "lse without strides, or misaligned")) return rc;
    int n = key_splits;
    if (n == 0) {   // shape-only: the CU count of the current device and the pure rule
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 0;
        APEXMI_REQUIRE(cus > 0, "%s: key_splits = auto needs the device's compute-unit count, which the runtime did not give", who);
        n = apexmi_attn_wide_auto_splits((int)units, (Sk + KV - 1) / KV, cus);
    }
    APEXMI_REQUIRE(units * n < (1ll << 31), "%s: too many workgroups (%lld query blocks x %d key splits)", who, (long long)units, n);
    if (int rc = require_workspace(who, workspace, workspace_bytes, apexmi_attn_wide_split_workspace_bytes(B, H, Sq, Sk, D, n), true))
        return rc;

    WideSplitArgs a{};
    set_qko(a, q, k, out, q_strides, k_strides, o_strides);
    a.H = H, a.Sq = Sq, a.Sk = Sk, a.Skp = ((Sk + KV - 1) / KV) * KV;
    a.nqb = (Sq + WQB - 1) / WQB, a.total = B * H * a.nqb;
    set_scale(a, softmax_scale);
    a.ft = frame_tokens;
    a.B = B, a.n = n;

    // V^T [B, H, D, Skp]: the 128-wide transpose over the D / 128 column slices of a head (a pure 16-bit move: f16 too); heads
    // that follow each other at distance D in memory are slices of one launch
    uint16_t* vt = (uint16_t*)workspace;
    a.vt = vt;
    const bool heads_adjacent = H == 1 || v_strides[1] == D;
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < (heads_adjacent ? 1 : H); ++h)
            if (int rc = apexmi_v_transpose((const uint16_t*)v + b * v_strides[0] + h * v_strides[1], 128, v_strides[2], Sk,
                                            (heads_adjacent ? H : 1) * (D / 128), 128,
                                            vt + ((size_t)b * H + h) * D * a.Skp, a.Skp, 0, (apexmi_stream_t)stream))
                return rc;

    // under the frame rule frame f's queries see f + 1 frames of keys: half the square plus half the diagonal
    const double nf = frame_tokens ? (double)(Sq / frame_tokens) : 0.0;
    const double pairs = frame_tokens ? (double)frame_tokens * frame_tokens * nf * (nf + 1.0) * 0.5 : (double)Sq * Sk;
    const int64_t part_elems = (int64_t)n * B * Sq * H * D;
    {
        ApexmiProfScope prof(1, stream, 4.0 * B * H * pairs * D, 0.0);   // the attention launch: the useful flops, whatever n
        if (n == 1 && !lse) {   // the launch this entry point has always made
            const WideArgs& plain = a;
            return dtype == APEXMI_BF16 ? launch_wide_d<ElemBf16>(D, plain, stream) : launch_wide_d<ElemF16>(D, plain, stream);
        }
        if (n == 1) {
            a.lse = lse, a.l_sp = 0, a.l_sb = lse_strides[0], a.l_sh = lse_strides[1], a.l_sq = lse_strides[2];
            return dtype == APEXMI_BF16 ? launch_wide_d<ElemBf16>(D, a, stream) : launch_wide_d<ElemF16>(D, a, stream);
        }
        // n > 1: f32 partials [n, B, Sq, H, D] and their lses [n, B, H, Sq] behind V^T, then the merge launch
        a.part = (float*)((char*)workspace + apexmi_attn_wide_workspace_bytes(B, H, Sk, D));
        a.lse = a.part + part_elems;
        a.l_sp = (int64_t)B * H * Sq, a.l_sb = (int64_t)H * Sq, a.l_sh = Sq, a.l_sq = 1;
        if (int rc = dtype == APEXMI_BF16 ? launch_wide_d<ElemBf16>(D, a, stream) : launch_wide_d<ElemF16>(D, a, stream)) return rc;
    }
    return apexmi_attn_merge_f32(n, a.part, a.lse, out, lse, B, H, Sq, D, o_strides, lse_strides, dtype, stream);
}

}  // namespace

// V^T [B, H, D, Skp] (Skp = Sk rounded up to 64), rounded up to 256 bytes: linear in Sk, no term in Sq
extern "C" size_t apexmi_attn_wide_workspace_bytes(int B, int H, int Sk, int D) {
    if (B <= 0 || H <= 0 || Sk <= 0 || !wide_dim(D)) return 0;
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV;
    return ((size_t)B * H * D * skp * 2 + 255) & ~(size_t)255;
}

// V^T as above; key_splits > 1 adds the f32 partials [n, B, Sq, H, D] and their lses [n, B, H, Sq], no padding between them
extern "C" size_t apexmi_attn_wide_split_workspace_bytes(int B, int H, int Sq, int Sk, int D, int key_splits) {
    const size_t vt = apexmi_attn_wide_workspace_bytes(B, H, Sk, D);
    if (vt == 0 || Sq <= 0 || key_splits < 1 || key_splits > WIDE_SPLITS_MAX) return 0;
    if (key_splits == 1) return vt;
    return vt + (size_t)key_splits * B * Sq * H * ((size_t)D + 1) * 4;
}

// The split count of key_splits = 0.  One workgroup is one CU's whole register file, so `units` workgroups fill units / cus of the
// device: no split once the launch is more than half full (2 units > cus); otherwise as many splits as fill it (cus / units), at
// least 4 key tiles (256 keys) a split, at most 8 (the merge's limit).  Pure: no device, the same answer for the same numbers.
extern "C" int apexmi_attn_wide_auto_splits(int units, int key_tiles, int cus) {
    if (units <= 0 || key_tiles <= 0 || cus <= 0 || 2 * (int64_t)units > cus) return 1;
    const int n = std::min(std::min(WIDE_SPLITS_MAX, cus / units), key_tiles / 4);
    return std::max(n, 1);
}

extern "C" int apexmi_attn_fwd_wide(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk, int D,
                                    const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                                    const int64_t o_strides[3], float softmax_scale, int dtype, int frame_tokens,
                                    void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return fwd_wide("attn_fwd_wide", q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides, v_strides, o_strides, softmax_scale,
                    dtype, frame_tokens, nullptr, nullptr, 1, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int apexmi_attn_fwd_wide_split(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk,
                                          int D, const int64_t q_strides[3], const int64_t k_strides[3],
                                          const int64_t v_strides[3], const int64_t o_strides[3], float softmax_scale, int dtype,
                                          int frame_tokens, float* lse, const int64_t lse_strides[3], int key_splits,
                                          void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return fwd_wide("attn_fwd_wide_split", q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides, v_strides, o_strides,
                    softmax_scale, dtype, frame_tokens, lse, lse_strides, key_splits, workspace, workspace_bytes,
                    (hipStream_t)stream_);
}
