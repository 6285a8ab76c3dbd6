// Masked and causal attention forward: the whole contract of the reference's default "sdpa" backend
// (R/src/attention/functions.py:338-377, i.e. F.scaled_dot_product_attention without dropout):
//   out = softmax(q k^T * scale + mask) v,   mask broadcast to [B, Hq, Sq, Sk] (bool keep-mask or additive f32 / bf16 / f16),
//   optionally AND-ed with the top-left causal mask (key j <= query i), grouped-query heads (query head h reads kv head
//   h / (Hq / Hkv)), bf16 or f16, D = 64 or 128.  A query row without any allowed key yields zeros.
//
// One-pass flash kernel on the shared tile step (attn_tile.h: layout, rounding), 4 waves, bf16 or f16, D = 64 or 128, workgroups of
// one (batch, head) kept on one XCD.  Specific to this kernel:
//   * q and k are read in place through their strides (no packing); V^T [B, Hkv, D, Skp] is staged in the workspace.
//   * an additive mask can move a score by any amount and excluded scores are -inf, so a row whose keys are all excluded so far
//     never produces a NaN, and a row whose sum stays 0 stores zeros.  Consequence of the finite sentinel the running maximum
//     starts from: an allowed score below -1e30 (base-2 units) counts as excluded.
//   * per (query block, key tile) the kernel walks a list built at entry from the BLOCK MAP (attn_mask_map_kernel): SKIP tiles
//     are never loaded nor multiplied, DENSE tiles (all allowed, additive value 0) run exactly the unmasked arithmetic, only
//     PARTIAL tiles read the mask (4 runs of 8 keys per lane, issued ahead of the QK^T MFMAs).
//   * causal: the key-tile range of a workgroup is computed from its query block (tiles above the diagonal are never in the
//     list), only the tiles that cross the diagonal compare per element, and the query blocks of the whole launch run heaviest
//     first so the short ones fill the last round.
//
// COORDINATE WINDOW (attn_masked_kernel<.., WIN = true>, apexmi_attn_fwd_window / apexmi_attn_fwd_prepared_window): the mask is
// a rule instead of an array.  Every token carries three int16 coordinates (one 8-byte record {c0, c1, c2, 0}); key j is allowed
// for query i iff |cq[i][a] - ck[j][a]| <= r[a] on the three axes, one window for all batches and heads.  The block map of that
// rule is built ONCE per plan by attn_window_map_kernel from the two coordinate arrays (no Sq x Sk array exists anywhere); the
// kernel walks it exactly as it walks a mask's map, and a PARTIAL tile evaluates the rule in registers: the lane holds its query
// row's coordinates from entry, the tile's 64 key records arrive in LDS with the tile (one 8-byte load per key, wave 0, issued
// with the tile's staging and written before the barrier that publishes the tile).  Excluded scores become -inf through the
// same fmaf as a bool mask's, so the result equals apexmi_attn_fwd_masked on the equivalent dense bool mask bit for bit.
#include "attn_host.h"
#include "attn_tile.h"

#include <cstdint>

namespace {

constexpr int MNW = 4;             // waves per workgroup
constexpr int MQB = MNW * 32;      // query rows per workgroup (= rows of one block-map entry)
constexpr int MAP_SKIP = 0, MAP_DENSE = 1, MAP_PARTIAL = 2;
constexpr int MAX_TILES = 1 << 14;  // tile index + 2-bit code in the 16-bit LDS list entries
constexpr float LN2 = 0.6931471805599453f;

// mask element -> additive value in natural units (bool: 0 keep / -inf drop)
template <int MK>
APEXMI_DEVICE float mask_value(const void* m, int64_t off);
template <>
APEXMI_DEVICE float mask_value<APEXMI_MASK_BOOL>(const void* m, int64_t off) {
    return ((const uint8_t*)m)[off] ? 0.0f : -__builtin_inff();
}
template <>
APEXMI_DEVICE float mask_value<APEXMI_F32>(const void* m, int64_t off) { return ((const float*)m)[off]; }
template <>
APEXMI_DEVICE float mask_value<APEXMI_BF16>(const void* m, int64_t off) { return bf16_to_f32(((const uint16_t*)m)[off]); }
template <>
APEXMI_DEVICE float mask_value<APEXMI_F16>(const void* m, int64_t off) {
    return (float)__builtin_bit_cast(_Float16, ((const uint16_t*)m)[off]);
}

struct MaskedArgs {
    const uint16_t* q;
    const uint16_t* k;
    const uint16_t* vt;
    uint16_t* o;
    const void* mask;       // nullptr: no mask (every tile DENSE)
    const uint8_t* map;     // block map [Bm, Hm, nqb, nkt] (nullptr with mask == nullptr)
    int64_t q_sb, q_sh, q_ss, k_sb, k_sh, k_ss, o_sb, o_ss, o_sh;
    int64_t m_sb, m_sh, m_sq, m_sk;   // element strides of the mask broadcast to [B, Hq, Sq, Sk] (0 on broadcast dims)
    int Hq, group, Sq, Sk, Skp, nqb, nkt, total, mkind, causal, neg;
    float c;                // |scale| * log2(e)
    // coordinate window (WIN kernels only): packed records {c0, c1, c2, 0} as 4 x int16 per token, radii clamped to 65535
    const u32x2* wq;
    const u32x2* wk;
    int wr0, wr1, wr2;
    // log-sum-exp output (LSE kernels only): f32 [B, Hq, Sq] through element strides (b, h, q)
    float* lse;
    int64_t l_sb, l_sh, l_sq;
};

// coordinate a (0..2) of a packed record, sign-extended
APEXMI_DEVICE int wcoord0(u32x2 c) { return (int)(c[0] << 16) >> 16; }
APEXMI_DEVICE int wcoord1(u32x2 c) { return (int)c[0] >> 16; }
APEXMI_DEVICE int wcoord2(u32x2 c) { return (int)(c[1] << 16) >> 16; }

// Block map of a coordinate window, built once per plan: one WAVE per (128-row query block, 64-key tile), 4 tiles per workgroup.
// Lane l holds key l of the tile and query rows l and l + 64 of the block (indices clamped into the arrays: a clamped index
// repeats a row / key of the same block / tile, which changes neither a bounding box nor a classification).  The two bounding
// boxes settle most tiles: SKIP when on some axis the boxes are more than r apart, DENSE when on every axis the farthest pair
// of box corners is within r.  The undecided tiles take the exact pass: 128 steps, one query row against the 64 keys each.
// The codes equal what attn_mask_map_kernel gives for the dense bool mask of the same rule, ragged tails included.
__global__ __launch_bounds__(256) void attn_window_map_kernel(const u32x2* __restrict__ wq, const u32x2* __restrict__ wk, int r0,
                                                              int r1, int r2, int Sq, int Sk, int nkt,
                                                              uint8_t* __restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), qb = blockIdx.y;
    if (t >= nkt) return;   // wave-uniform; no barrier below
    const int q_lo = qb * MQB, q_n = min(Sq - q_lo, MQB);      // q_n >= 1
    const int k_lo = t * KV, k_n = min(Sk - k_lo, KV);        // k_n >= 1
    const u32x2 kc = wk[k_lo + min(lane, k_n - 1)];
    const u32x2 qa = wq[q_lo + min(lane, q_n - 1)], qc = wq[q_lo + min(lane + 64, q_n - 1)];
    const int k0 = wcoord0(kc), k1 = wcoord1(kc), k2 = wcoord2(kc);
    int lo[6], hi[6];   // 0..2: keys, 3..5: queries
    lo[0] = hi[0] = k0, lo[1] = hi[1] = k1, lo[2] = hi[2] = k2;
    lo[3] = min(wcoord0(qa), wcoord0(qc)), hi[3] = max(wcoord0(qa), wcoord0(qc));
    lo[4] = min(wcoord1(qa), wcoord1(qc)), hi[4] = max(wcoord1(qa), wcoord1(qc));
    lo[5] = min(wcoord2(qa), wcoord2(qc)), hi[5] = max(wcoord2(qa), wcoord2(qc));
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            lo[i] = min(lo[i], __shfl_xor(lo[i], m));
            hi[i] = max(hi[i], __shfl_xor(hi[i], m));
        }
    const int r[3] = {r0, r1, r2};
    bool apart = false, within = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        apart = apart || lo[a] - hi[3 + a] > r[a] || lo[3 + a] - hi[a] > r[a];
        within = within && hi[a] - lo[3 + a] <= r[a] && hi[3 + a] - lo[a] <= r[a];
    }
    int code = apart ? MAP_SKIP : within ? MAP_DENSE : -1;
    if (code < 0) {   // wave-uniform
        const uint64_t valid = k_n == 64 ? ~0ull : (1ull << k_n) - 1;
        bool any = false, dense = true;
        for (int i = 0; i < q_n; ++i) {
            const u32x2 q = wq[q_lo + i];   // one address for the wave
            const bool ok = (uint32_t)(wcoord0(q) - k0 + r0) <= 2u * (uint32_t)r0 && (uint32_t)(wcoord1(q) - k1 + r1) <= 2u * (uint32_t)r1 &&
                            (uint32_t)(wcoord2(q) - k2 + r2) <= 2u * (uint32_t)r2;
            const uint64_t bal = __ballot(ok) & valid;
            any = any || bal != 0;
            dense = dense && bal == valid;
        }
        code = !any ? MAP_SKIP : dense ? MAP_DENSE : MAP_PARTIAL;
    }
    if (lane == 0) map[(int64_t)qb * nkt + t] = (uint8_t)code;
}

// Block map pre-pass: one workgroup per (key tile, query block, own mask (batch, head)).  SKIP: no allowed element; DENSE:
// every element allowed with additive value 0; PARTIAL otherwise.  VEC (host: key stride 1, 16-byte aligned rows): whole tiles
// are read 16 bytes per lane; otherwise (and on the key tail) one element per lane, 64 lanes along the keys, 4 rows per step.
template <int MK, typename ET, bool VEC>
__global__ __launch_bounds__(256) void attn_mask_map_kernel(const void* __restrict__ mask, int64_t m_sb, int64_t m_sh,
                                                            int64_t m_sq, int64_t m_sk, int Hm, int Sq, int Sk, int nqb,
                                                            int nkt, uint8_t* __restrict__ map) {
    const int t = blockIdx.x, qb = blockIdx.y, z = blockIdx.z;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)(z / Hm) * m_sb + (int64_t)(z % Hm) * m_sh;
    int any = 0, dense = 1;
    if (VEC && (t + 1) * KV <= Sk) {
        constexpr int NE = 16 / sizeof(ET), LPR = KV / NE, RPS = 256 / LPR;   // elements per lane, lanes per row, rows per step
        const int key = t * KV + (tid % LPR) * NE;
        for (int r = qb * MQB + tid / LPR; r < min(Sq, (qb + 1) * MQB); r += RPS) {
            const u32x4 raw = *(const u32x4*)((const ET*)mask + base + (int64_t)r * m_sq + key);
            const ET* e = (const ET*)&raw;
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const float v = mask_value<MK>(e, j);
                const int ok = v != -__builtin_inff();
                any |= ok;
                dense &= ok && v == 0.0f;
            }
        }
    } else {
        const int key = t * KV + (tid & 63);
        if (key < Sk) {
            const int64_t kof = base + (int64_t)key * m_sk;
            for (int r = qb * MQB + (tid >> 6); r < min(Sq, (qb + 1) * MQB); r += 4) {
                const float v = mask_value<MK>(mask, kof + (int64_t)r * m_sq);
                const int ok = v != -__builtin_inff();
                any |= ok;
                dense &= ok && v == 0.0f;
            }
        }
    }
    any = __syncthreads_or(any);
    dense = __syncthreads_and(dense);
    if (tid == 0) map[((int64_t)z * nqb + qb) * nkt + t] = (uint8_t)(!any ? MAP_SKIP : dense ? MAP_DENSE : MAP_PARTIAL);
}

// V [B, Hkv, Sk, 64] (strided rows) -> V^T [B, Hkv, 64, Skp], keys >= Sk zero (the D = 128 case uses apexmi_v_transpose)
__global__ __launch_bounds__(256) void v_transpose64_kernel(const uint16_t* __restrict__ v, int64_t sb, int64_t sh, int64_t ss,
                                                            int Hkv, int Sk, int Skp, uint16_t* __restrict__ vt) {
    constexpr int LDW = 66;   // odd dword pitch: the column reads below spread over the banks
    __shared__ uint16_t tile[64 * LDW];
    const int tid = threadIdx.x;
    const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = i * 256 + tid;
        const int r = idx >> 3, c = idx & 7;
        u32x4 val = u32x4{0u, 0u, 0u, 0u};
        if (s0 + r < Sk) val = *(const u32x4*)(v + (int64_t)b * sb + (int64_t)h * sh + (int64_t)(s0 + r) * ss + c * 8);
        uint32_t* dst = (uint32_t*)(tile + r * LDW + c * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[j] = val[j];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = i * 256 + tid;
        const int d = idx >> 3, sc = idx & 7;
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[j] = (uint32_t)tile[(sc * 8 + 2 * j) * LDW + d] | ((uint32_t)tile[(sc * 8 + 2 * j + 1) * LDW + d] << 16);
        *(u32x4*)(vt + (((int64_t)b * Hkv + h) * 64 + d) * Skp + s0 + sc * 8) = o;
    }
}

// LSE (apexmi_attn_fwd_masked_lse) is a compile-time variant: the instantiations without it keep their registers (at D = 64
// the 186 VGPRs noted below), the ones with it run the same loop and add one logf and one f32 store per row to the epilogue.
template <typename E, int D, bool WIN, bool LSE = false>
__global__ __launch_bounds__(MNW * 64, 2) void attn_masked_kernel(const MaskedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using v8 = typename E::v8;
    constexpr int K_TILE = KV * D * 2, V_TILE = D * KV * 2, STAGE = K_TILE + V_TILE;
    constexpr int NP = D / 8, LD = PIECES<D, MNW>, NDT = D / 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    // causal: query blocks in decreasing order of work over the whole launch (block id = position in dispatch order); workgroup
    // b runs on XCD b % 8, so with B Hq a multiple of 8 every (batch, head) still stays on one XCD
    const int s = a.causal ? (int)blockIdx.x : xcd_remap(blockIdx.x, a.total);
    const int nhb = a.total / a.nqb;
    const int hb = a.causal ? s % nhb : s / a.nqb;
    const int qb = a.causal ? a.nqb - 1 - s / nhb : s % a.nqb;
    const int b = hb / a.Hq, h = hb % a.Hq;
    const int hk = h / a.group;

    const uint16_t* Qp = a.q + (int64_t)b * a.q_sb + (int64_t)h * a.q_sh;
    const uint16_t* Kp = a.k + (int64_t)b * a.k_sb + (int64_t)hk * a.k_sh;
    const uint16_t* Vp = a.vt + ((int64_t)b * (a.Hq / a.group) + hk) * D * a.Skp;

    const int q0 = qb * MQB;
    const int qrow = q0 + wave * 32 + l31;
    const int qrow_c = min(qrow, a.Sq - 1);

    // ---- tile list: the key tiles this workgroup visits, with their block-map code (wave 0 builds it, LDS) ----
    int* list_n = (int*)(smem + 2 * STAGE);
    uint16_t* list = (uint16_t*)(smem + 2 * STAGE + 16);
    const int nt = (a.Sk + KV - 1) / KV;
    const int t_end = a.causal ? min(nt, min(q0 + MQB - 1, a.Sq - 1) / KV + 1) : nt;
    if (wave == 0) {
        const uint8_t* mrow = nullptr;
        if (a.map) {
            const int mb = a.m_sb ? b : 0, mh = a.m_sh ? h : 0, Hm = a.m_sh ? a.Hq : 1;
            mrow = a.map + ((int64_t)(mb * Hm + mh) * a.nqb + qb) * a.nkt;
        }
        int n = 0;
        for (int t0 = 0; t0 < t_end; t0 += 64) {
            const int t = t0 + lane;
            const int code = t < t_end ? (mrow ? (int)mrow[t] : MAP_DENSE) : MAP_SKIP;
            const uint64_t bal = __ballot(code != MAP_SKIP);
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            if (code != MAP_SKIP) list[pos] = (uint16_t)(t | (code << 14));
            n += __builtin_popcountll(bal);
        }
        if (lane == 0) *list_n = n;
    }

    // Q fragments (B operand of S^T): lane supplies Q[qrow][16 ks + 8 hi .. +7]; a negative scale flips their signs (exact)
    // (kept in the kernel: behind a helper that fills qf this load costs the masked and dual kernels 18-35 VGPRs, and at D = 64
    // the third workgroup per CU that the parent's 186 VGPRs rule out)
    v8 qf[D / 16];
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        u32x4 raw = *(const u32x4*)(Qp + (int64_t)qrow_c * a.q_ss + ks * 16 + hi * 8);
        if (a.neg) raw ^= u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        qf[ks] = __builtin_bit_cast(v8, raw);
    }

    int k_key[LD], k_c[LD], v_row[LD], v_c[LD];
    stage_sources<D, MNW>(wave, lane, k_key, k_c, v_row, v_c);
    const uint16_t* v_src[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) v_src[i] = Vp + (int64_t)v_row[i] * a.Skp + v_c[i];
    auto stage = [&](int buf, int t) {
        char* base = smem + buf * STAGE + wave * 1024;
        const int kv0 = t * KV;
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * MNW + wave < NP) {   // wave-uniform
                const int key = min(kv0 + k_key[i], a.Sk - 1);
                glds16(Kp + (int64_t)key * a.k_ss + k_c[i], base + i * (MNW * 1024));
            }
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * MNW + wave < NP) glds16(v_src[i] + kv0, base + K_TILE + i * (MNW * 1024));
    };

    int k_off[2], k_sw[2], v_off[NDT], v_sw[NDT];
    fragment_offsets<D>(l31, k_off, k_sw, v_off, v_sw);
    const int64_t m_row = (int64_t)b * a.m_sb + (int64_t)h * a.m_sh + (int64_t)qrow_c * a.m_sq;

    // coordinate window: |cq - ck| <= r  <=>  (unsigned)(cq + r - ck) <= 2 r; the lane keeps cq + r of its query row.  The key
    // records of a PARTIAL tile live behind the tile list, one 512-byte image per LDS stage.
    int wqa0 = 0, wqa1 = 0, wqa2 = 0;
    u32x2 wk_next = u32x2{0u, 0u};
    u32x2* wk_lds = (u32x2*)(smem + 2 * STAGE + 16 + ((2 * a.nkt + 15) & ~15));
    if (WIN) {
        const u32x2 cq = a.wq[qrow_c];
        wqa0 = wcoord0(cq) + a.wr0, wqa1 = wcoord1(cq) + a.wr1, wqa2 = wcoord2(cq) + a.wr2;
    }
    const uint32_t w2r0 = 2u * (uint32_t)a.wr0, w2r1 = 2u * (uint32_t)a.wr1, w2r2 = 2u * (uint32_t)a.wr2;

    f32x16 oacc[NDT];
    clear(oacc);
    float m_run = SENTINEL;  // running maximum, base-2 domain, an integer
    float l_run = 0.0f;

    __syncthreads();
    const int n = *list_n;
    if (n > 0) {
        stage(0, list[0] & (MAX_TILES - 1));
        if (WIN && wave == 0 && (list[0] >> 14) == MAP_PARTIAL) wk_next = a.wk[min((list[0] & (MAX_TILES - 1)) * KV + lane, a.Sk - 1)];
    }
    for (int it = 0; it < n; ++it) {
        const int ent = list[it];
        const int t = ent & (MAX_TILES - 1), code = ent >> 14;
        const int kv0 = t * KV;
        // window: this tile's key records (loaded with its staging) into the image of its stage; the image was last read two
        // tiles ago, before the barrier every wave has passed since
        if (WIN && wave == 0 && code == MAP_PARTIAL) wk_lds[(it & 1) * KV + lane] = wk_next;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile's LDS-DMA has landed (see attention.hip)
        __syncthreads();

        // mask values of a PARTIAL tile, issued before the next tile's staging so waiting for them does not wait for it
        float mv[2][16];
        if (!WIN && code == MAP_PARTIAL) {
#define MASK_LOADS(MK)                                                                                          \
    _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) _Pragma("unroll") for (int r = 0; r < 16; ++r) {           \
        const int key = min(kv0 + tile_key(kt, r, hi), a.Sk - 1);                                               \
        mv[kt][r] = mask_value<MK>(a.mask, m_row + (int64_t)key * a.m_sk) * LOG2E;                              \
    }
            switch (a.mkind) {
                case APEXMI_MASK_BOOL: MASK_LOADS(APEXMI_MASK_BOOL); break;
                case APEXMI_F32: MASK_LOADS(APEXMI_F32); break;
                case APEXMI_BF16: MASK_LOADS(APEXMI_BF16); break;
                default: MASK_LOADS(APEXMI_F16); break;
            }
#undef MASK_LOADS
        }
        if (it + 1 < n) {
            stage((it + 1) & 1, list[it + 1] & (MAX_TILES - 1));
            if (WIN && wave == 0 && (list[it + 1] >> 14) == MAP_PARTIAL)
                wk_next = a.wk[min((list[it + 1] & (MAX_TILES - 1)) * KV + lane, a.Sk - 1)];
        }
        const char* Ks = smem + (it & 1) * STAGE;

        f32x16 sacc[2];
        scores<E, D>(Ks, k_off, k_sw, hi, qf, sacc);

        // per-element path (workgroup-uniform): PARTIAL tiles, tiles crossing the causal diagonal, the key tail
        const bool elem = code == MAP_PARTIAL || (a.causal && kv0 + KV - 1 > q0) || kv0 + KV > a.Sk;
        float mx;
        if (elem) {
            const bool part = code == MAP_PARTIAL;
            const int lim = a.causal ? min(a.Sk - 1, qrow) : a.Sk - 1;
            mx = -__builtin_inff();
            if (WIN && part) {   // the rule, evaluated on the tile's key records: 0 (keep) or -inf, as a bool mask's values
                const u32x2* kc = wk_lds + (it & 1) * KV;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const u32x2 c = kc[tile_key(kt, r, hi)];
                        const bool ok = (uint32_t)(wqa0 - wcoord0(c)) <= w2r0 && (uint32_t)(wqa1 - wcoord1(c)) <= w2r1 &&
                                        (uint32_t)(wqa2 - wcoord2(c)) <= w2r2;
                        mv[kt][r] = ok ? 0.0f : -__builtin_inff();
                    }
            }
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float x = fmaf(sacc[kt][r], a.c, part ? mv[kt][r] : 0.0f);
                    sacc[kt][r] = kv0 + tile_key(kt, r, hi) <= lim ? x : -__builtin_inff();
                    mx = fmaxf(mx, sacc[kt][r]);
                }
        } else {
            mx = tile_max(sacc) * a.c;
        }
        raise_max(max_xor32(mx), m_run, l_run, oacc);   // -inf (nothing allowed yet) never raises the sentinel
        // the two exponent forms of attn_tile.h (exp2_scaled / exp2_fused), written out: through the helpers this kernel's D = 64
        // tile loop is scheduled differently and measures 0.2-0.6 % slower (profiles/attn_tile_refactor.md)
        float psum = 0.0f;
        if (elem) {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = fast_exp2(sacc[kt][r] - m_run);
                    sacc[kt][r] = p;
                    psum += p;
                }
        } else {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float p = fast_exp2(fmaf(sacc[kt][r], a.c, -m_run));
                    sacc[kt][r] = p;
                    psum += p;
                }
        }
        l_run += psum;

        v8 pf[4];
        p_fragments<E>(sacc, pf);
        accumulate<E, D>(Ks + K_TILE, v_off, v_sw, hi, pf, oacc);
    }

    // ---- epilogue: O[q][d] = O^T / l, 0 for a row without an allowed key ----
    const float l_tot = sum_xor32(l_run);
    const float inv = l_tot > 0.0f ? 1.0f / l_tot : 0.0f;
    if (qrow < a.Sq) store_row<E>(a.o + (int64_t)b * a.o_sb + (int64_t)qrow * a.o_ss + (int64_t)h * a.o_sh, hi, oacc, inv);
    // ln sum_j exp(scale q k_j + mask_j) = m ln 2 + ln l from the row's (integer, base-2) maximum and its sum, -inf for a row
    // without an allowed key; the row's low-half lane stores it
    if constexpr (LSE) {
        if (hi == 0 && qrow < a.Sq)
            a.lse[(int64_t)b * a.l_sb + (int64_t)h * a.l_sh + (int64_t)qrow * a.l_sq] =
                l_tot > 0.0f ? fmaf(m_run, LN2, logf(l_tot)) : -__builtin_inff();
    }
}

// ---- merge of partial results over key chunks (apexmi_attn_merge) ----
// out = sum_p w_p o_p / sum_p w_p,  lse = m + ln sum_p w_p  with  m = max_p lse_p,  w_p = exp(lse_p - m)  (0 for lse_p = -inf, so
// a row whose partials are all -inf gives 0 and -inf and (-inf) - (-inf) is never formed).  One lane per 16 bytes of an output
// row: it reads its 8 elements of every partial once (all loads issued before the first use) and the row's N lse values (shared
// by the D / 8 lanes of the row through the cache), f32 arithmetic, one rounding at the store.  The lane reads what it
// overwrites before it writes, so `out` may be one of the partials.  The pointer tables travel in the kernel arguments.
constexpr int MERGE_MAX = 8;

struct MergeArgs {
    const uint16_t* o[MERGE_MAX];
    const float* l[MERGE_MAX];
    uint16_t* out;
    float* lse_out;          // nullptr: not wanted
    int64_t o_sb, o_ss, o_sh, l_sb, l_sh, l_sq;
    int64_t total;           // lanes: B Sq H (D / 8)
    int H, Sq, CH;           // CH = D / 8
};

template <typename E>
APEXMI_DEVICE void unpack8_as(const u32x4 v, float* f);
template <>
APEXMI_DEVICE void unpack8_as<ElemBf16>(const u32x4 v, float* f) { unpack8(v, f); }
template <>
APEXMI_DEVICE void unpack8_as<ElemF16>(const u32x4 v, float* f) {
    const f16x8 x = __builtin_bit_cast(f16x8, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)x[i];
}

template <typename E, int N>
__global__ __launch_bounds__(256) void attn_merge_kernel(const MergeArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total) return;
    const int c = (int)(t % a.CH);
    int64_t r = t / a.CH;
    const int h = (int)(r % a.H);
    r /= a.H;
    const int sq = (int)(r % a.Sq);
    const int64_t b = r / a.Sq;
    const int64_t oo = b * a.o_sb + (int64_t)sq * a.o_ss + (int64_t)h * a.o_sh + c * 8;
    const int64_t lo = b * a.l_sb + (int64_t)h * a.l_sh + (int64_t)sq * a.l_sq;
    float ls[N];
    u32x4 raw[N];
#pragma unroll
    for (int p = 0; p < N; ++p) {
        ls[p] = a.l[p][lo];
        raw[p] = *(const u32x4*)(a.o[p] + oo);
    }
    float m = ls[0];
#pragma unroll
    for (int p = 1; p < N; ++p) m = fmaxf(m, ls[p]);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float den = 0.0f;
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const float w = ls[p] == -__builtin_inff() ? 0.0f : expf(ls[p] - m);
        float f[8];
        unpack8_as<E>(raw[p], f);
        den += w;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += w > 0.0f ? w * f[i] : 0.0f;   // a partial of weight 0 contributes nothing, whatever it holds
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = den > 0.0f ? acc[i] / den : 0.0f;
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = E::pack2(acc[2 * i], acc[2 * i + 1]);
    *(u32x4*)(a.out + oo) = o;
    if (c == 0 && a.lse_out) a.lse_out[lo] = den > 0.0f ? m + logf(den) : -__builtin_inff();
}

template <typename E>
int launch_merge(int n, const MergeArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.total + 255) / 256)), block(256);
    switch (n) {
#define MERGE_CASE(N) \
    case N: hipLaunchKernelGGL((attn_merge_kernel<E, N>), grid, block, 0, stream, a); break;
        MERGE_CASE(1) MERGE_CASE(2) MERGE_CASE(3) MERGE_CASE(4) MERGE_CASE(5) MERGE_CASE(6) MERGE_CASE(7) MERGE_CASE(8)
#undef MERGE_CASE
    }
    return apexmi_check_launch("attn_merge");
}

// The same merge over the wide-head kernel's own partials (attention_wide.hip, key_splits > 1): N f32 partials [N, B, Sq, H, D]
// and lses [N, B, H, Sq] in one workspace, the result rounded once into the caller's strided out.  A partial of weight 0 (an
// empty key range, whose rows were never written) contributes nothing, whatever it holds.
struct MergeF32Args {
    const float* part;
    const float* lse;
    uint16_t* out;
    float* lse_out;          // nullptr: not wanted
    int64_t o_sb, o_ss, o_sh, l_sb, l_sh, l_sq;
    int64_t total;           // lanes: B Sq H (D / 8)
    int64_t p_stride, l_stride;   // elements between two partials: B Sq H D, B H Sq
    int H, Sq, CH;           // CH = D / 8
};

template <typename E, int N>
__global__ __launch_bounds__(256) void attn_merge_f32_kernel(const MergeF32Args a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.total) return;
    const int c = (int)(t % a.CH);
    int64_t r = t / a.CH;
    const int h = (int)(r % a.H);
    r /= a.H;
    const int sq = (int)(r % a.Sq);
    const int64_t b = r / a.Sq;
    const float* pp = a.part + t * 8;                                   // [B, Sq, H, D / 8] lanes of 8 elements
    const float* lp = a.lse + (b * a.H + h) * a.Sq + sq;
    float ls[N];
    f32x4 raw[N][2];
#pragma unroll
    for (int p = 0; p < N; ++p) {
        ls[p] = lp[p * a.l_stride];
        raw[p][0] = *(const f32x4*)(pp + p * a.p_stride);
        raw[p][1] = *(const f32x4*)(pp + p * a.p_stride + 4);
    }
    float m = ls[0];
#pragma unroll
    for (int p = 1; p < N; ++p) m = fmaxf(m, ls[p]);
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float den = 0.0f;
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const float w = ls[p] == -__builtin_inff() ? 0.0f : expf(ls[p] - m);
        den += w;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += w > 0.0f ? w * raw[p][i >> 2][i & 3] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = den > 0.0f ? acc[i] / den : 0.0f;
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = E::pack2(acc[2 * i], acc[2 * i + 1]);
    *(u32x4*)(a.out + b * a.o_sb + (int64_t)sq * a.o_ss + (int64_t)h * a.o_sh + c * 8) = o;
    if (c == 0 && a.lse_out)
        a.lse_out[b * a.l_sb + (int64_t)h * a.l_sh + (int64_t)sq * a.l_sq] = den > 0.0f ? m + logf(den) : -__builtin_inff();
}

template <typename E>
int launch_merge_f32(int n, const MergeF32Args& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.total + 255) / 256)), block(256);
    switch (n) {
#define MERGE_CASE(N) \
    case N: hipLaunchKernelGGL((attn_merge_f32_kernel<E, N>), grid, block, 0, stream, a); break;
        MERGE_CASE(2) MERGE_CASE(3) MERGE_CASE(4) MERGE_CASE(5) MERGE_CASE(6) MERGE_CASE(7) MERGE_CASE(8)
#undef MERGE_CASE
    }
    return apexmi_check_launch("attn_merge_f32");
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t vt_bytes(int B, int Hkv, int Sk, int D) {
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV;
    return align256((size_t)B * Hkv * D * skp * 2);
}

template <typename E, int D, bool WIN = false, bool LSE = false>
int launch_masked(const MaskedArgs& a, hipStream_t stream) {
    constexpr int STAGE = 2 * KV * D * 2;
    constexpr int WK = WIN ? 2 * KV * 8 : 0;   // the two key-record images of a window launch
    return launch_flash<attn_masked_kernel<E, D, WIN, LSE>>(dim3(a.total), dim3(MNW * 64), 2 * STAGE + 16 + 2 * MAX_TILES + WK,
                                                            2 * STAGE + 16 + ((2 * a.nkt + 15) & ~15) + WK, stream, a,
                                                            WIN ? "attn_fwd_window" : LSE ? "attn_fwd_masked_lse" : "attn_fwd_masked");
}

// V [B, Hkv, Sk, D] (strided rows) -> V^T [B, Hkv, D, Skp] zero padded
int transpose_v(const void* v, const int64_t v_strides[3], int B, int Hkv, int Sk, int Skp, int D, uint16_t* vt,
                apexmi_stream_t stream_) {
    if (D == 128) {
        for (int b = 0; b < B; ++b)
            if (int rc = apexmi_v_transpose((const uint16_t*)v + b * v_strides[0], v_strides[1], v_strides[2], Sk, Hkv, D,
                                            vt + (size_t)b * Hkv * D * Skp, Skp, 0, stream_))
                return rc;
        return 0;
    }
    hipLaunchKernelGGL(v_transpose64_kernel, dim3(Skp / 64, Hkv, B), dim3(256), 0, (hipStream_t)stream_, (const uint16_t*)v,
                       v_strides[0], v_strides[1], v_strides[2], Hkv, Sk, Skp, vt);
    return apexmi_check_launch("attn_fwd_masked (V^T)");
}

// the window operands of a launch: coordinates, radii (clamped: two int16 differ by at most 65535) and the plan's block map
int window_args(MaskedArgs& a, const void* q_coords, const void* k_coords, int r0, int r1, int r2, const void* map,
                const char* who) {
    APEXMI_REQUIRE(q_coords && k_coords && map, "%s: null window operand (coordinates / block map)", who);
    APEXMI_REQUIRE(((uintptr_t)q_coords % 8) == 0 && ((uintptr_t)k_coords % 8) == 0, "%s: coordinate records must be 8-byte aligned", who);
    APEXMI_REQUIRE(r0 >= 0 && r1 >= 0 && r2 >= 0, "%s: negative radius (%d, %d, %d)", who, r0, r1, r2);
    a.wq = (const u32x2*)q_coords, a.wk = (const u32x2*)k_coords;
    a.wr0 = r0 < 65535 ? r0 : 65535, a.wr1 = r1 < 65535 ? r1 : 65535, a.wr2 = r2 < 65535 ? r2 : 65535;
    a.map = (const uint8_t*)map;   // [nqb, nkt]: one window for every batch and head (mask strides stay 0)
    return 0;
}

// the shape fields of a launch (the prepared entry point has no grouped heads and takes Skp from its caller)
void set_shape(MaskedArgs& a, int B, int Hq, int group, int Sq, int Sk, int Skp) {
    a.Hq = Hq, a.group = group, a.Sq = Sq, a.Sk = Sk, a.Skp = Skp;
    a.nqb = (Sq + MQB - 1) / MQB, a.nkt = (Sk + KV - 1) / KV, a.total = B * Hq * a.nqb;
}

// the checks apexmi_attn_fwd_masked(_lse) and apexmi_attn_fwd_window make between their own: the problem, then the launch limits
int require_problem(const char* who, int B, int Hq, int Hkv, int Sq, int Sk, int D, int dtype) {
    APEXMI_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && Sq > 0 && Sk > 0, "%s: empty problem (B=%d Hq=%d Hkv=%d Sq=%d Sk=%d)", who,
                   B, Hq, Hkv, Sq, Sk);
    if (int rc = require_head_dim(who, D, D == 64 || D == 128, "64 or 128")) return rc;
    if (int rc = require_dtype(who, dtype)) return rc;
    return require_head_ratio(who, Hq, Hkv);
}

int require_launch_limits(const char* who, int B, int H, int Sq, int Sk) {
    APEXMI_REQUIRE((Sk + KV - 1) / KV <= MAX_TILES, "%s: Sk=%d above %d keys", who, Sk, MAX_TILES * KV);
    APEXMI_REQUIRE((int64_t)B * H * ((Sq + MQB - 1) / MQB) < (1ll << 31), "%s: too many query blocks", who);
    return 0;
}

template <int MK, typename ET>
void launch_map(const MaskedArgs& a, int Bm, int Hm, uint8_t* map, hipStream_t stream) {
    constexpr int64_t NE = 16 / sizeof(ET);
    const bool vec = a.m_sk == 1 && ((uintptr_t)a.mask % 16) == 0 && a.m_sb % NE == 0 && a.m_sh % NE == 0 && a.m_sq % NE == 0;
    auto kern = vec ? attn_mask_map_kernel<MK, ET, true> : attn_mask_map_kernel<MK, ET, false>;
    hipLaunchKernelGGL(kern, dim3(a.nkt, a.nqb, Bm * Hm), dim3(256), 0, stream, a.mask, a.m_sb, a.m_sh, a.m_sq, a.m_sk, Hm, a.Sq, a.Sk, a.nqb, a.nkt, map);
}

}  // namespace

extern "C" size_t apexmi_attn_masked_workspace_bytes(int B, int Hq, int Hkv, int Sq, int Sk, int D) {
    if (B <= 0 || Hq <= 0 || Hkv <= 0 || Sq <= 0 || Sk <= 0 || (D != 64 && D != 128)) return 0;
    const size_t nqb = (size_t)((Sq + MQB - 1) / MQB), nkt = (size_t)((Sk + KV - 1) / KV);
    return vt_bytes(B, Hkv, Sk, D) + align256((size_t)B * Hq * nqb * nkt);
}

// apexmi_attn_fwd_masked and apexmi_attn_fwd_masked_lse: one argument check, one set of pre-passes, two families of instantiations
static int fwd_masked(const char* who, bool want_lse, float* lse, const int64_t* lse_strides, const void* q, const void* k,
                      const void* v, void* out, int B, int Hq, int Hkv, int Sq, int Sk, int D,
                      const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                      const void* mask, int mask_dtype, const int64_t mask_strides[4], int is_causal, float softmax_scale, int dtype,
                      void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = require_operands(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides)) return rc;
    if (int rc = require_lse(who, want_lse, lse, lse_strides, "null or misaligned lse operand")) return rc;
    if (int rc = require_problem(who, B, Hq, Hkv, Sq, Sk, D, dtype)) return rc;
    APEXMI_REQUIRE(!mask || (mask_strides && (mask_dtype == APEXMI_MASK_BOOL || mask_dtype == APEXMI_F32 ||
                                              mask_dtype == APEXMI_BF16 || mask_dtype == APEXMI_F16)),
                   "%s: mask dtype code %d unsupported (bool, f32, bf16, f16)", who, mask_dtype);
    APEXMI_REQUIRE(!mask || mask_strides[3] == 0 || mask_strides[3] == 1,
                   "%s: mask key stride %lld must be 0 or 1", who, (long long)(mask ? mask_strides[3] : 0));
    if (int rc = require_launch_limits(who, B, Hq, Sq, Sk)) return rc;
    if (int rc = require_aligned(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides, 3)) return rc;
    // not required to be 16-byte aligned here, unlike the varlen and wide entry points
    if (int rc = require_workspace(who, workspace, workspace_bytes, apexmi_attn_masked_workspace_bytes(B, Hq, Hkv, Sq, Sk, D), false))
        return rc;

    MaskedArgs a{};
    set_qko(a, q, k, out, q_strides, k_strides, o_strides);
    set_shape(a, B, Hq, Hq / Hkv, Sq, Sk, ((Sk + KV - 1) / KV) * KV);
    a.causal = is_causal ? 1 : 0;
    set_scale(a, softmax_scale);
    if (want_lse) a.lse = lse, a.l_sb = lse_strides[0], a.l_sh = lse_strides[1], a.l_sq = lse_strides[2];

    // V^T [B, Hkv, D, Skp]
    uint16_t* vt = (uint16_t*)workspace;
    a.vt = vt;
    if (int rc = transpose_v(v, v_strides, B, Hkv, Sk, a.Skp, D, vt, stream_)) return rc;

    // block map of the mask over its own (batch, head) dims
    if (mask) {
        uint8_t* map = (uint8_t*)workspace + vt_bytes(B, Hkv, Sk, D);
        a.mask = mask, a.mkind = mask_dtype, a.map = map;
        a.m_sb = B > 1 ? mask_strides[0] : 0, a.m_sh = Hq > 1 ? mask_strides[1] : 0;
        a.m_sq = Sq > 1 ? mask_strides[2] : 0, a.m_sk = Sk > 1 ? mask_strides[3] : 0;
        const int Bm = a.m_sb ? B : 1, Hm = a.m_sh ? Hq : 1;
        APEXMI_REQUIRE((int64_t)Bm * Hm <= 65535 && a.nqb <= 65535, "%s: block map grid too large", who);
        switch (mask_dtype) {
            case APEXMI_MASK_BOOL: launch_map<APEXMI_MASK_BOOL, uint8_t>(a, Bm, Hm, map, stream); break;
            case APEXMI_F32: launch_map<APEXMI_F32, float>(a, Bm, Hm, map, stream); break;
            case APEXMI_BF16: launch_map<APEXMI_BF16, uint16_t>(a, Bm, Hm, map, stream); break;
            default: launch_map<APEXMI_F16, uint16_t>(a, Bm, Hm, map, stream); break;
        }
        if (int rc = apexmi_check_launch("attn_fwd_masked (block map)")) return rc;
    }

    ApexmiProfScope prof(1, stream, 4.0 * B * Hq * (double)Sq * Sk * D, 0.0);
    if (want_lse) {
        if (dtype == APEXMI_BF16)
            return D == 128 ? launch_masked<ElemBf16, 128, false, true>(a, stream) : launch_masked<ElemBf16, 64, false, true>(a, stream);
        return D == 128 ? launch_masked<ElemF16, 128, false, true>(a, stream) : launch_masked<ElemF16, 64, false, true>(a, stream);
    }
    if (dtype == APEXMI_BF16) return D == 128 ? launch_masked<ElemBf16, 128>(a, stream) : launch_masked<ElemBf16, 64>(a, stream);
    return D == 128 ? launch_masked<ElemF16, 128>(a, stream) : launch_masked<ElemF16, 64>(a, stream);
}

extern "C" int apexmi_attn_fwd_masked(const void* q, const void* k, const void* v, void* out, int B, int Hq, int Hkv, int Sq,
                                      int Sk, int D, const int64_t q_strides[3], const int64_t k_strides[3],
                                      const int64_t v_strides[3], const int64_t o_strides[3], const void* mask,
                                      int mask_dtype, const int64_t mask_strides[4], int is_causal, float softmax_scale,
                                      int dtype, void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return fwd_masked("attn_fwd_masked", false, nullptr, nullptr, q, k, v, out, B, Hq, Hkv, Sq, Sk, D, q_strides, k_strides, v_strides,
                      o_strides, mask, mask_dtype, mask_strides, is_causal, softmax_scale, dtype, workspace, workspace_bytes, stream_);
}

extern "C" int apexmi_attn_fwd_masked_lse(const void* q, const void* k, const void* v, void* out, float* lse, int B, int Hq,
                                          int Hkv, int Sq, int Sk, int D, const int64_t q_strides[3],
                                          const int64_t k_strides[3], const int64_t v_strides[3], const int64_t o_strides[3],
                                          const int64_t lse_strides[3], const void* mask, int mask_dtype,
                                          const int64_t mask_strides[4], int is_causal, float softmax_scale, int dtype,
                                          void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return fwd_masked("attn_fwd_masked_lse", true, lse, lse_strides, q, k, v, out, B, Hq, Hkv, Sq, Sk, D, q_strides, k_strides,
                      v_strides, o_strides, mask, mask_dtype, mask_strides, is_causal, softmax_scale, dtype, workspace,
                      workspace_bytes, stream_);
}

int apexmi_attn_merge_f32(int n, const float* parts, const float* lses, void* out, float* lse_out, int B, int H, int Sq, int D,
                          const int64_t* o_strides, const int64_t* lse_strides, int dtype, hipStream_t stream) {
    APEXMI_REQUIRE(n >= 2 && n <= MERGE_MAX, "attn_merge_f32: n=%d partials unsupported (2 to %d)", n, MERGE_MAX);
    APEXMI_REQUIRE(parts && lses && out && o_strides && (!lse_out || lse_strides), "attn_merge_f32: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && D > 0 && D % 8 == 0, "attn_merge_f32: bad problem (B=%d H=%d Sq=%d D=%d)", B, H, Sq, D);
    APEXMI_REQUIRE(dtype == APEXMI_BF16 || dtype == APEXMI_F16, "attn_merge_f32: dtype %d unsupported (bf16 or f16)", dtype);
    bool aligned = ((uintptr_t)out % 16) == 0 && ((uintptr_t)parts % 16) == 0 && ((uintptr_t)lses % 4) == 0 && ((uintptr_t)lse_out % 4) == 0;
    for (int i = 0; i < 3; ++i) aligned = aligned && o_strides[i] % 8 == 0;
    APEXMI_REQUIRE(aligned, "attn_merge_f32: out rows must be 16-byte aligned (strides multiples of 8 elements), lse 4-byte aligned");
    MergeF32Args a{};
    a.part = parts, a.lse = lses, a.out = (uint16_t*)out, a.lse_out = lse_out;
    a.o_sb = o_strides[0], a.o_ss = o_strides[1], a.o_sh = o_strides[2];
    if (lse_out) a.l_sb = lse_strides[0], a.l_sh = lse_strides[1], a.l_sq = lse_strides[2];
    a.H = H, a.Sq = Sq, a.CH = D / 8;
    a.total = (int64_t)B * Sq * H * a.CH;
    a.p_stride = (int64_t)B * Sq * H * D, a.l_stride = (int64_t)B * H * Sq;
    APEXMI_REQUIRE((a.total + 255) / 256 < (1ll << 31), "attn_merge_f32: too many rows");
    ApexmiProfScope prof(5, stream, 0.0, (double)a.total * 8 * (4.0 * n + 2.0));   // apexmi_attn_merge's class
    return dtype == APEXMI_BF16 ? launch_merge_f32<ElemBf16>(n, a, stream) : launch_merge_f32<ElemF16>(n, a, stream);
}

extern "C" int apexmi_attn_merge(int n, const void* const* outs, const float* const* lses, void* out, float* lse_out, int B, int H,
                                 int Sq, int D, const int64_t o_strides[3], const int64_t lse_strides[3], int dtype,
                                 apexmi_stream_t stream_) {
    APEXMI_REQUIRE(n >= 1 && n <= MERGE_MAX, "attn_merge: n=%d partials unsupported (1 to %d)", n, MERGE_MAX);
    APEXMI_REQUIRE(outs && lses && out && o_strides && lse_strides, "attn_merge: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && D > 0, "attn_merge: empty problem (B=%d H=%d Sq=%d D=%d)", B, H, Sq, D);
    APEXMI_REQUIRE(D % 8 == 0, "attn_merge: head dim %d must be a multiple of 8", D);
    APEXMI_REQUIRE(dtype == APEXMI_BF16 || dtype == APEXMI_F16, "attn_merge: dtype %d unsupported (bf16 or f16)", dtype);
    MergeArgs a{};
    bool aligned = ((uintptr_t)out % 16) == 0 && ((uintptr_t)lse_out % 4) == 0;
    for (int p = 0; p < n; ++p) {
        APEXMI_REQUIRE(outs[p] && lses[p], "attn_merge: null partial %d", p);
        // the row's D / 8 lanes all read lses[p]; the one that writes lse_out does not wait for the others
        APEXMI_REQUIRE(lses[p] != lse_out, "attn_merge: lse_out must not be lses[%d]", p);
        aligned = aligned && ((uintptr_t)outs[p] % 16) == 0 && ((uintptr_t)lses[p] % 4) == 0;
        a.o[p] = (const uint16_t*)outs[p], a.l[p] = lses[p];
    }
    for (int i = 0; i < 3; ++i) aligned = aligned && o_strides[i] % 8 == 0;
    APEXMI_REQUIRE(aligned, "attn_merge: out rows must be 16-byte aligned (strides multiples of 8 elements), lse 4-byte aligned");
    a.out = (uint16_t*)out, a.lse_out = lse_out;
    a.o_sb = o_strides[0], a.o_ss = o_strides[1], a.o_sh = o_strides[2];
    a.l_sb = lse_strides[0], a.l_sh = lse_strides[1], a.l_sq = lse_strides[2];
    a.H = H, a.Sq = Sq, a.CH = D / 8;
    a.total = (int64_t)B * Sq * H * a.CH;
    APEXMI_REQUIRE((a.total + 255) / 256 < (1ll << 31), "attn_merge: too many rows");
    hipStream_t stream = (hipStream_t)stream_;
    ApexmiProfScope prof(5, stream, 0.0, (double)a.total * 16.0 * (n + 1));
    return dtype == APEXMI_BF16 ? launch_merge<ElemBf16>(n, a, stream) : launch_merge<ElemF16>(n, a, stream);
}

// ---- coordinate window ------------------------------------------------------------------------------------------------------

extern "C" size_t apexmi_attn_window_map_bytes(int Sq, int Sk) {
    if (Sq <= 0 || Sk <= 0) return 0;
    return (size_t)((Sq + MQB - 1) / MQB) * (size_t)((Sk + KV - 1) / KV);
}

extern "C" int apexmi_attn_window_map(const void* q_coords, const void* k_coords, int Sq, int Sk, int r0, int r1, int r2,
                                      void* map, size_t map_bytes, apexmi_stream_t stream_) {
    APEXMI_REQUIRE(Sq > 0 && Sk > 0, "attn_window_map: empty problem (Sq=%d Sk=%d)", Sq, Sk);
    const int nqb = (Sq + MQB - 1) / MQB, nkt = (Sk + KV - 1) / KV;
    APEXMI_REQUIRE(nkt <= MAX_TILES, "attn_window_map: Sk=%d above %d keys", Sk, MAX_TILES * KV);
    APEXMI_REQUIRE(nqb <= 65535, "attn_window_map: Sq=%d above %d query rows", Sq, 65535 * MQB);
    APEXMI_REQUIRE(map && map_bytes >= apexmi_attn_window_map_bytes(Sq, Sk), "attn_window_map: map buffer too small (%zu < %zu)",
                   map_bytes, apexmi_attn_window_map_bytes(Sq, Sk));
    MaskedArgs a{};
    if (int rc = window_args(a, q_coords, k_coords, r0, r1, r2, map, "attn_window_map")) return rc;
    hipLaunchKernelGGL(attn_window_map_kernel, dim3((nkt + 3) / 4, nqb), dim3(256), 0, (hipStream_t)stream_, a.wq, a.wk, a.wr0,
                       a.wr1, a.wr2, Sq, Sk, nkt, (uint8_t*)map);
    return apexmi_check_launch("attn_window_map");
}

extern "C" int apexmi_attn_fwd_window(const void* q, const void* k, const void* v, void* out, int B, int Hq, int Hkv, int Sq,
                                      int Sk, int D, const int64_t q_strides[3], const int64_t k_strides[3],
                                      const int64_t v_strides[3], const int64_t o_strides[3], const void* q_coords,
                                      const void* k_coords, int r0, int r1, int r2, const void* map, float softmax_scale,
                                      int dtype, void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "attn_fwd_window";
    if (int rc = require_operands(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides)) return rc;
    if (int rc = require_problem(who, B, Hq, Hkv, Sq, Sk, D, dtype)) return rc;
    if (int rc = require_launch_limits(who, B, Hq, Sq, Sk)) return rc;
    if (int rc = require_aligned(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides, 3)) return rc;
    if (int rc = require_workspace(who, workspace, workspace_bytes, vt_bytes(B, Hkv, Sk, D), false)) return rc;

    MaskedArgs a{};
    if (int rc = window_args(a, q_coords, k_coords, r0, r1, r2, map, who)) return rc;
    set_qko(a, q, k, out, q_strides, k_strides, o_strides);
    set_shape(a, B, Hq, Hq / Hkv, Sq, Sk, ((Sk + KV - 1) / KV) * KV);
    set_scale(a, softmax_scale);
    uint16_t* vt = (uint16_t*)workspace;
    a.vt = vt;
    if (int rc = transpose_v(v, v_strides, B, Hkv, Sk, a.Skp, D, vt, stream_)) return rc;

    ApexmiProfScope prof(1, stream, 4.0 * B * Hq * (double)Sq * Sk * D, 0.0);
    if (dtype == APEXMI_BF16)
        return D == 128 ? launch_masked<ElemBf16, 128, true>(a, stream) : launch_masked<ElemBf16, 64, true>(a, stream);
    return D == 128 ? launch_masked<ElemF16, 128, true>(a, stream) : launch_masked<ElemF16, 64, true>(a, stream);
}

extern "C" int apexmi_attn_fwd_prepared_window(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq,
                                               int Sk, int Skp, const int64_t o_strides[3], const void* q_coords,
                                               const void* k_coords, int r0, int r1, int r2, const void* map,
                                               float softmax_scale, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    constexpr int D = 128;
    APEXMI_REQUIRE(q && k && vt && out && o_strides, "attn_fwd_prepared_window: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0, "attn_fwd_prepared_window: empty problem");
    APEXMI_REQUIRE(Skp % KV == 0 && Skp >= Sk, "attn_fwd_prepared_window: Skp=%d must be Sk=%d rounded up to 64", Skp, Sk);
    APEXMI_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)vt % 16) == 0 && ((uintptr_t)out % 8) == 0,
                   "attn_fwd_prepared_window: operands must be 16-byte aligned");
    APEXMI_REQUIRE(o_strides[0] % 4 == 0 && o_strides[1] % 4 == 0 && o_strides[2] % 4 == 0,
                   "attn_fwd_prepared_window: output strides must be multiples of 4 elements");
    if (int rc = require_launch_limits("attn_fwd_prepared_window", B, H, Sq, Sk)) return rc;

    MaskedArgs a{};
    if (int rc = window_args(a, q_coords, k_coords, r0, r1, r2, map, "attn_fwd_prepared_window")) return rc;
    const int64_t q_packed[3] = {(int64_t)H * Sq * D, (int64_t)Sq * D, D};
    const int64_t k_packed[3] = {(int64_t)H * Sk * D, (int64_t)Sk * D, D};
    set_qko(a, q, k, out, q_packed, k_packed, o_strides);
    a.vt = (const uint16_t*)vt;
    set_shape(a, B, H, 1, Sq, Sk, Skp);
    set_scale(a, softmax_scale);
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * Sk * D, 0.0);
    return launch_masked<ElemBf16, 128, true>(a, stream);
}
