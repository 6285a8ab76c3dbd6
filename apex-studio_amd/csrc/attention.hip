// Attention forward for the denoise path: softmax(q k^T * scale) v, no mask, non-causal.
// Replaces the callable behind attention_register.call (reference attention/functions.py:84,
// default "sdpa" :338-377) at the call sites flux/base/attention.py:89-94,
// wan/base/attention.py:397-399 and qwenimage/base/model.py:555-562.
//
// MFMA kernels (bf16, D = 128), per workgroup NW = 4..8 waves x 32 query rows, KV tile = 64 keys (169-238 VGPRs: two
// waves per SIMD, ONE workgroup per CU).  Launches that fill the chip use the 8-wave 4-cluster ping-pong kernel
// (attn_fwd_d128_c4_kernel, below); the plain loop (attn_fwd_d128_kernel) serves small launches and A/B.  The tile layout, the
// products and the rounding rule of the online softmax are attn_tile.h's.  V arrives pre-transposed ([B,H,128,Skp], produced by
// apexmi_qkv_prepare / apexmi_v_transpose), K and V^T tiles are staged by 16-byte global_load_lds into a double-buffered 64 KiB
// LDS image.  Workgroup ids are remapped so all query blocks of one (batch, head) run on one XCD and share its L2 copy of K / V^T.
#include "attn_host.h"
#include "attn_tile.h"

// Per-workgroup timeline of the shipped flash kernel (tools/attn_tile_trace.py): compiled in only with -DAPEXMI_ATTN_TRACE=1 into a side
// library; the host reads a device pointer from the environment variable APEXMI_ATTN_TRACE_PTR (hex) at every launch.  8 u64 per
// workgroup: {HW_ID, XCC_ID, t_entry, t_loop_begin, t_loop_end, t_stores_issued, t_stores_acknowledged, tile} (s_memrealtime, 10 ns).
#ifndef APEXMI_ATTN_TRACE
#define APEXMI_ATTN_TRACE 0
#endif
#if APEXMI_ATTN_TRACE
#include <stdlib.h>
__device__ unsigned long long* d_attn_trace = nullptr;
#endif
// workgroups of attn_fwd_d128_w64_kernel that re-ran their tiles with the running-maximum loop (attn_w64_kernel.h); read and
// cleared by apexmi_attn_w64_fallbacks
__device__ unsigned int d_attn_w64_fallbacks = 0;


#include <cstdint>

namespace {

constexpr int HD = 128;   // head dim
constexpr int K_TILE_BYTES = KV * HD * 2;   // 16 KiB
constexpr int V_TILE_BYTES = HD * KV * 2;   // 16 KiB
constexpr int ATT_STAGE = K_TILE_BYTES + V_TILE_BYTES;

// NW = waves per workgroup (4..8); every wave owns 32 query rows and reads the whole K / V^T tile, so 8 waves halve the LDS-DMA
// instructions each wave has to issue per tile.  Keys past Sk get SENTINEL on the raw score, 1 / l is unguarded, scale > 0.
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_d128_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ Vt,
    bf16_t* __restrict__ O, int H, int Sq, int Sk, int Skp, int nqb, int total, int64_t o_sb,
    int64_t o_ss, int64_t o_sh, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    const int s = xcd_remap(blockIdx.x, total);
    const int hb = s / nqb, qb = s % nqb;
    const int b = hb / H, h = hb % H;

    const bf16_t* Qp = Q + (int64_t)hb * Sq * HD;
    const bf16_t* Kp = K + (int64_t)hb * Sk * HD;
    const bf16_t* Vp = Vt + (int64_t)hb * HD * Skp;

    using E = ElemBf16;
    constexpr int QB = NW * 32, LD = PIECES<HD, NW>;
    const int qrow = qb * QB + wave * 32 + l31;
    const int qrow_c = min(qrow, Sq - 1);
    bf16x8 qf[8];   // B operand of S^T: lane supplies Q[qrow][16 ks + 8 hi .. +7]
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *(const bf16x8*)(Qp + (int64_t)qrow_c * HD + ks * 16 + hi * 8);

    int k_key[LD], k_c[LD], v_row[LD], v_c[LD];
    stage_sources<HD, NW>(wave, lane, k_key, k_c, v_row, v_c);
    const bf16_t* v_src[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) v_src[i] = Vp + (int64_t)v_row[i] * Skp + v_c[i];
    auto stage = [&](int buf, int t) {
        char* base = smem + buf * ATT_STAGE + wave * 1024;
        const int kv0 = t * KV;
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * NW + wave < 16) {  // wave-uniform
                const int key = min(kv0 + k_key[i], Sk - 1);
                glds16(Kp + (int64_t)key * HD + k_c[i], base + i * (NW * 1024));
            }
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * NW + wave < 16) glds16(v_src[i] + kv0, base + K_TILE_BYTES + i * (NW * 1024));
    };

    int k_off[2], k_sw[2], v_off[4], v_sw[4];
    fragment_offsets<HD>(l31, k_off, k_sw, v_off, v_sw);

    f32x16 oacc[4];
    clear(oacc);
    float m_run = SENTINEL;  // running max, already in the scaled (log2) domain
    float l_run = 0.0f;      // this lane's partial row sum (its 32 keys of every tile)

    const int nt = (Sk + KV - 1) / KV;
    stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        // Tile t's LDS-DMA must have landed before the barrier.  hipcc does NOT reliably add the
        // vmcnt(0) to __syncthreads() for LDS-DMA in this loop (observed in the .s: bare s_barrier;
        // symptom: rare run-to-run differences at the full Flux shape), so the wait is explicit.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t + 1 < nt) stage((t + 1) & 1, t + 1);
        const char* Ks = smem + (t & 1) * ATT_STAGE;

        f32x16 sacc[2];
        scores<E, HD>(Ks, k_off, k_sw, hi, qf, sacc);
        if (t == nt - 1 && (Sk & (KV - 1)) != 0) {   // keys past Sk (last tile only; wave-uniform branch)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (t * KV + tile_key(kt, r, hi) >= Sk) sacc[kt][r] = SENTINEL;
        }
        raise_max(max_xor32(tile_max(sacc)) * scale_log2e, m_run, l_run, oacc);     // always raises on the first tile
        l_run += exp2_fused(sacc, scale_log2e, m_run);

        bf16x8 pf[4];
        p_fragments<E>(sacc, pf);
        accumulate<E, HD>(Ks + K_TILE_BYTES, v_off, v_sw, hi, pf, oacc);
    }

    const float inv = 1.0f / sum_xor32(l_run);
    if (qrow < Sq) store_row<E>(O + (int64_t)b * o_sb + (int64_t)qrow * o_ss + (int64_t)h * o_sh, hi, oacc, inv);
}

// ---- 4-cluster ping-pong variant (8 waves) ---------------------------------------------------------------
// Tail mode (nsplit > 1): the launch covers the workgroups s_base .. of the (head, q-block) order that would otherwise
// form a nearly empty last round, each cut into nsplit key ranges; a workgroup writes its normalised partial output
// (bf16) and the log2-sum-exp of its rows, attn_combine_kernel merges them.
// Two LDS stages of the K / V^T tiles: tile t + 1 is staged during tile t (from C1, beside the K fragment reads) and waited for
// three clusters later.  Measured and not shipped: a third stage, the LDS-DMA issued from C2 or C3, and the row sums /
// bf16 pairs / exponentials moved into the gaps of C4's MFMAs.
template <int NW, int PRIO>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_d128_c4_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ Vt,
    bf16_t* __restrict__ O, int H, int Sq, int Sk_all, int Skp, int nqb, int total, int64_t o_sb,
    int64_t o_ss, int64_t o_sh, float scale_log2e, int s_base, int nsplit, float* __restrict__ opart,
    float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
#if APEXMI_ATTN_TRACE
    unsigned long long* const trace = d_attn_trace;
    unsigned long long tr_in = 0, tr_l0 = 0, tr_l1 = 0;
    if (trace) tr_in = __builtin_amdgcn_s_memrealtime();
#endif

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    int s, kv_begin = 0, Sk = Sk_all, part = 0;
    if (nsplit > 1) {   // block-uniform
        part = blockIdx.x;
        s = s_base + part / nsplit;
        const int per = (((Sk_all + KV - 1) / KV + nsplit - 1) / nsplit) * KV;   // keys per split, whole tiles
        kv_begin = (part % nsplit) * per;
        Sk = min(Sk_all - kv_begin, per);                                        // host guarantees kv_begin < Sk_all
    } else {
        s = xcd_remap(blockIdx.x, total);
    }
    const int hb = s / nqb, qb = s % nqb;
    const int b = hb / H, h = hb % H;

    const bf16_t* Qp = Q + (int64_t)hb * Sq * HD;
    const bf16_t* Kp = K + (int64_t)hb * Sk_all * HD + (int64_t)kv_begin * HD;
    const bf16_t* Vp = Vt + (int64_t)hb * HD * Skp + kv_begin;

    constexpr int QB = NW * 32;
    constexpr int LD = (16 + NW - 1) / NW;  // 1 KiB LDS-DMA pieces per wave per tile image (16 pieces each for K and V^T)
    const int qrow = qb * QB + wave * 32 + l31;
    const int qrow_c = min(qrow, Sq - 1);

    // Q fragments: B operand of S^T, lane supplies Q[qrow][16 ks + 8 hi .. +7]
    bf16x8 qf[8];
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
        qf[ks] = *(const bf16x8*)(Qp + (int64_t)qrow_c * HD + ks * 16 + hi * 8);

    // staging sources.  Piece p = i NW + wave (p < 16).  K image: [64 rows][16 chunks], chunk ^= row & 15,
    // row i <- key perm(i).  V^T image: [128 rows (d)][8 chunks], chunk ^= (row >> 1) & 7.
    int k_key[LD], k_c[LD];
    const char* v_src[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) {
        const int p = (i * NW + wave) * 64 + lane;
        {
            const int row = (p >> 4) & 63, pc = p & 15;
            k_c[i] = (pc ^ (row & 15)) * 8;
            k_key[i] = (row & 32) + perm32(row & 31);
        }
        {
            const int row = (p >> 3) & 127, pc = p & 7;
            const int c = pc ^ ((row >> 1) & 7);
            v_src[i] = (const char*)(Vp + (int64_t)row * Skp + c * 8);
        }
    }

    const int nt = (Sk + KV - 1) / KV;
    constexpr bool ALLP = (16 % NW) == 0;   // every wave owns LD whole pieces: no wave-uniform guard (and no branch) in the loop
    auto stage_piece = [&](int buf, int t, int j) {   // j < LD: K piece j; j >= LD: V^T piece j - LD
        char* base = smem + buf * ATT_STAGE + wave * 1024;
        const int kv0 = t * KV;
        if (j < LD) {
            const int i = j;
            if (ALLP || i * NW + wave < 16) {  // wave-uniform
                const int key = min(kv0 + k_key[i], Sk - 1);
                glds16(Kp + (int64_t)key * HD + k_c[i], base + i * (NW * 1024));
            }
        } else {
            const int i = j - LD;
            if (ALLP || i * NW + wave < 16) glds16(v_src[i] + (int64_t)kv0 * 2, base + K_TILE_BYTES + i * (NW * 1024));
        }
    };
    auto stage = [&](int buf, int t) {
#pragma unroll
        for (int j = 0; j < 2 * LD; ++j) stage_piece(buf, t, j);
    };
    // the loop's prefetch.  Stays a lambda: written straight in the loop, the compiler allocates all eight instantiations differently
    auto stage_next = [&](int t) {
        if (t + 1 < nt) stage((t + 1) & 1, t + 1);
    };

    // LDS read offsets
    int k_off[2], k_sw[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int row = kt * 32 + l31;
        k_off[kt] = row * 256;
        k_sw[kt] = row & 15;
    }
    int v_off[4], v_sw[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int row = dt * 32 + l31;
        v_off[dt] = row * 128;
        v_sw[dt] = (row >> 1) & 7;
    }

    f32x16 oacc[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.0f;
    float m_run = SENTINEL;  // running max, already in the scaled (log2) domain
    float l_run = 0.0f;      // this lane's partial row sum (its 32 keys of every tile)

    // ---- 4-cluster ping-pong (8 waves; wave w and w + 4 share a SIMD) -------------------------------------------
    // A tile is four clusters per wave, each closed by an s_barrier:
    //   C1 load K : 16 ds_read_b128 of the tile's K fragments into a 64-VGPR block; the LDS-DMA of tile t+1
    //   C2 K Q^T  : 16 MFMAs out of registers
    //   C3 load V : 16 ds_read_b128 of the V^T fragments into the SAME block, the softmax VALU beside them
    //   C4 P V    : 16 MFMAs out of registers
    // Waves 4..7 run one cluster behind waves 0..3, so on every SIMD one wave is in a matrix cluster while its partner
    // is in a load cluster: the fragment reads (-15 % when interleaved with the MFMAs they feed, profiles/
    // r01_attention_notes.md) and the softmax run in the partner's matrix time.
    const bool late = wave >= NW / 2;
    bf16x8 kv[16];
    f32x16 sacc[2];
    bf16x8 pf[4];
#define C4_BAR()                               \
    do {                                       \
        __builtin_amdgcn_sched_barrier(0);     \
        __builtin_amdgcn_s_barrier();          \
        __builtin_amdgcn_sched_barrier(0);     \
    } while (0)
#define C4_LGKM_BAR()                                            \
    do {                                                         \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
        C4_BAR();                                                \
    } while (0)
    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    C4_BAR();                  // tile 0 visible
    if (late) C4_BAR();        // second half runs one cluster behind
    if ((PRIO & 4) && late) __builtin_amdgcn_s_setprio(1);   // the younger half loses every age arbitration otherwise
#if APEXMI_ATTN_TRACE
    if (trace) tr_l0 = __builtin_amdgcn_s_memrealtime();
#endif
    for (int t = 0; t < nt; ++t) {
        const char* Ks = smem + (t & 1) * ATT_STAGE;
        const char* Vs = Ks + K_TILE_BYTES;
        // ---- C1: K fragments -> registers; LDS-DMA of the next tile (its stage was last read two clusters ago) ----
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
                kv[ks * 2 + kt] = *(const bf16x8*)(Ks + k_off[kt] + (((ks * 2 + hi) ^ k_sw[kt]) << 4));
        stage_next(t);
        C4_LGKM_BAR();
        // ---- C2: S^T = K Q^T ----
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) sacc[kt][r] = 0.0f;
        if (PRIO & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
                sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv[ks * 2 + kt], qf[ks], sacc[kt], 0, 0, 0);
        if (PRIO & 1) __builtin_amdgcn_s_setprio(0);
        C4_BAR();
        // ---- C3: V^T fragments -> the same registers, softmax beside the reads ----
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                kv[kk * 4 + dt] = *(const bf16x8*)(Vs + v_off[dt] + (((kk * 2 + hi) ^ v_sw[dt]) << 4));
        if (t == nt - 1 && (Sk & (KV - 1)) != 0) {   // mask keys past Sk (wave-uniform branch)
            const int kv0 = t * KV;
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int a = r >> 2, bb = r & 3;
                    const int key = kv0 + kt * 32 + 16 * (a >> 1) + 8 * hi + 4 * (a & 1) + bb;
                    if (key >= Sk) sacc[kt][r] = SENTINEL;
                }
        }
        {
            float mx = sacc[0][0];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sacc[kt][r]);
            mx = max_xor32(mx) * scale_log2e;
            if (__any(mx > m_run + DEFER)) {
                const float m_new = ceilf(fmaxf(m_run, mx));   // integer: attn_tile.h
                const float alpha = fast_exp2(m_run - m_new);
                m_run = m_new;
                l_run *= alpha;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            }
            if (PRIO & 2) {
                // packed f32 math: one v_pk_fma_f32 / v_pk_add_f32 per PAIR of scores (the accumulator registers of an
                // MFMA are consecutive, so the pairs are already aligned) — 32 fewer VALU issues per tile and wave
                const f32x2 c2 = {scale_log2e, scale_log2e}, nm2 = {-m_run, -m_run};
                f32x2 ps2 = {0.0f, 0.0f};
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; r += 2) {
                        f32x2 x = {sacc[kt][r], sacc[kt][r + 1]};
                        x = __builtin_elementwise_fma(x, c2, nm2);
                        x[0] = fast_exp2(x[0]);
                        x[1] = fast_exp2(x[1]);
                        sacc[kt][r] = x[0];
                        sacc[kt][r + 1] = x[1];
                        ps2 += x;
                    }
                l_run += ps2[0] + ps2[1];
            } else {
                float psum = 0.0f;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float pv = fast_exp2(fmaf(sacc[kt][r], scale_log2e, -m_run));
                        sacc[kt][r] = pv;
                        psum += pv;
                    }
                l_run += psum;
            }
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[kk][j] = (__bf16)sacc[kk >> 1][8 * (kk & 1) + j];
        }
        // this wave's LDS-DMA pieces of tile t+1 must have landed before the barrier that opens the first cluster
        // reading them: the early half's C1(t+1) follows ITS C4(t) and the late half's C3(t) in the same slot
        if (late) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        C4_LGKM_BAR();
        // ---- C4: O^T += V^T P^T ----
        if (PRIO & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kv[kk * 4 + dt], pf[kk], oacc[dt], 0, 0, 0);
        if (PRIO & 1) __builtin_amdgcn_s_setprio(0);
        if (!late) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        C4_BAR();
    }
    if (!late) C4_BAR();       // balance the barrier count of the two halves
#undef C4_BAR
#undef C4_LGKM_BAR
#if APEXMI_ATTN_TRACE
    if (trace) {
        __builtin_amdgcn_sched_barrier(0);
        tr_l1 = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_sched_barrier(0);
    }
#endif

    // ---- epilogue: O[q][d] = O^T / l ; lane holds d = 32 dt + 8 g + 4 hi + (0..3) ----
    const float l_tot = sum_xor32(l_run);
    const float inv = 1.0f / l_tot;
    if (nsplit > 1) {
        constexpr int QBR = NW * 32;
        const int rloc = wave * 32 + l31;
        // un-normalised f32 partial numerator + (integer max, partial sum): the merge applies exact power-of-two
        // weights, so a split launch rounds to bf16 once, exactly where the single launch does
        float* op = opart + ((int64_t)part * QBR + rloc) * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 o = {oacc[dt][4 * g + 0], oacc[dt][4 * g + 1], oacc[dt][4 * g + 2], oacc[dt][4 * g + 3]};
                *(f32x4*)(op + dt * 32 + g * 8 + hi * 4) = o;
            }
        if (hi == 0) {
            lse[((int64_t)part * QBR + rloc) * 2] = m_run;
            lse[((int64_t)part * QBR + rloc) * 2 + 1] = l_tot;
        }
        return;
    }
    if (qrow < Sq) {
        bf16_t* op = O + (int64_t)b * o_sb + (int64_t)qrow * o_ss + (int64_t)h * o_sh;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                u32x2 o;
                o[0] = pack_bf16(oacc[dt][4 * g + 0] * inv, oacc[dt][4 * g + 1] * inv);
                o[1] = pack_bf16(oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
                *(u32x2*)(op + dt * 32 + g * 8 + hi * 4) = o;
            }
    }
#if APEXMI_ATTN_TRACE
    if (trace) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long t_st = __builtin_amdgcn_s_memrealtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long t_ack = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            unsigned long long* o = trace + (size_t)blockIdx.x * 8;
            o[0] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
            o[1] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);
            o[2] = tr_in;
            o[3] = tr_l0;
            o[4] = tr_l1;
            o[5] = t_st;
            o[6] = t_ack;
            o[7] = (unsigned long long)s;
        }
    }
#endif
}


// ---- one wave per SIMD, 64 query rows per wave (`attn.w64`) ----------------------------------------------------
// What the cluster trace of the 4-cluster kernel said (profiles/r05_attn_cluster_trace*.log): with two
// waves per SIMD the softmax VALU of a load cluster gets almost no issue slots while the partner's MFMA cluster streams, every
// cluster hand-over costs a barrier, and a KV tile takes ~3800 cycles for 2048 cycles of MFMAs.  This kernel keeps the products, the
// LDS images and the fragment / score / P lane mapping of that kernel and changes the schedule: 4 waves, ONE per SIMD, each owning
// two 32-row query blocks (A, B) and the whole 512-register file; every K / V^T fragment read from LDS feeds TWO MFMAs; the softmax
// of a tile is split over the two 32-MFMA phases of the loop and issued in the wave's OWN MFMA gaps:
//   phase X(t): S(t+1) = K(t+1) Q^T  (32 MFMAs)  beside  exp2 / row-sum terms / bf16 pairs of tile t
//   phase Y(t): O^T += V^T(t) P(t)^T (32 MFMAs)  beside  row max / running-max decision / scaling of tile t+1
// One s_barrier per tile, LDS ring of four stages.  The running max is per ROW here (a row is raised when ITS tile max exceeds it
// by more than DEFER): with the integer max any choice gives the same result up to f32 summation order (attn_tile.h).
// The loop is ONE asm statement generated by tools/gen_attn_w64.py (register map, instruction placement, wait counts and the
// MFMA -> VALU hazards are the generator's): hipcc's allocator spilled 160-220 registers on every C++ form of it.

// Shipped (round 6): the loop WITHOUT a per-tile running maximum (attn_w64_first.inc: every row keeps the integer maximum of tile
// 0), checked at the end, with the running-maximum loop (attn_w64_body.inc) as the workgroup's fallback — attn_w64_kernel.h.
#define W64_NAME attn_fwd_d128_w64_kernel
#define W64_BODY "attn_w64_first.inc"
#define W64_FALLBACK "attn_w64_body.inc"
#include "attn_w64_kernel.h"
#undef W64_NAME
#undef W64_BODY
#undef W64_FALLBACK
// the running-maximum loop alone (round 5's kernel; attn.w64 = 8): the A/B arm and the reference the fallback is tested against
#define W64_NAME attn_fwd_d128_w64r_kernel
#define W64_BODY "attn_w64_body.inc"
#include "attn_w64_kernel.h"
#undef W64_NAME
#undef W64_BODY
// per-block key bands (apexmi_attn_fwd_prepared_band): the shipped pair of loops behind a shell that reads the
// workgroup's key range [lo, hi) from a plan and points the two descriptors, nt and rem at it (attn_w64_kernel.h, W64_BANDS)
#define W64_NAME attn_fwd_d128_w64_band_kernel
#define W64_BODY "attn_w64_first.inc"
#define W64_FALLBACK "attn_w64_body.inc"
#define W64_BANDS 1
#include "attn_w64_kernel.h"
#undef W64_NAME
#undef W64_BODY
#undef W64_FALLBACK
#undef W64_BANDS

// ---- the same kernel on v_mfma_f32_16x16x32_bf16 -----------------------------------------------
// The denoise step runs at the chip's power limit; at equal matrix-pipe occupancy the 16x16x32 form
// sustains ~13 % higher clocks than 32x32x16 (tools/ubench/mfma_power.hip), so it is the faster one.
// Layout: a wave owns 2 query tiles of 16; S^T tiles are 16 keys x 16 queries, lane (g = lane >> 4,
// c = lane & 15) holds S^T[key row 4 g + r][query c].  K rows are READ permuted — row 4 g + r of key
// tile 2 kk + t is key 32 kk + 8 g + 4 t + r — so the 8 scores a lane holds for PV step kk are the
// consecutive keys 32 kk + 8 g .. + 7: P feeds the PV MFMA unshuffled and a V^T fragment is one
// ds_read_b128.  K is staged in natural row order with chunk ^= ((row >> 3) & 3) << 2 | (row & 3)
// (bank-conflict-free for that read); V^T as before.  Row max / sum cross 4 lanes (c, c+16, c+32,
// c+48): one v_permlane16_swap + one v_permlane32_swap.
APEXMI_DEVICE float max_xor16(float x) {
    uint32_t u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
APEXMI_DEVICE float sum_xor16(float x) {
    uint32_t u = __float_as_uint(x);
    auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
APEXMI_DEVICE int kswz(int row) { return (((row >> 3) & 3) << 2) | (row & 3); }

template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_fwd_d128_mi16_kernel(
    const bf16_t* __restrict__ Q, const bf16_t* __restrict__ K, const bf16_t* __restrict__ Vt,
    bf16_t* __restrict__ O, int H, int Sq, int Sk, int Skp, int nqb, int total, int64_t o_sb,
    int64_t o_ss, int64_t o_sh, float scale_log2e) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((ext_vector_type(4))) float f4;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;

    const int s = xcd_remap(blockIdx.x, total);
    const int hb = s / nqb, qb = s % nqb;
    const int b = hb / H, h = hb % H;

    const bf16_t* Qp = Q + (int64_t)hb * Sq * HD;
    const bf16_t* Kp = K + (int64_t)hb * Sk * HD;
    const bf16_t* Vp = Vt + (int64_t)hb * HD * Skp;

    constexpr int QB = NW * 32;
    constexpr int LD = (16 + NW - 1) / NW;  // 1 KiB LDS-DMA pieces per wave per tile image
    int qrow[2];
    bf16x8 qf[2][4];  // B operand of S^T: lane supplies Q[query][32 ks + 8 g .. +7]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        qrow[qt] = qb * QB + wave * 32 + qt * 16 + l15;
        const int qc = min(qrow[qt], Sq - 1);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[qt][ks] = *(const bf16x8*)(Qp + (int64_t)qc * HD + ks * 32 + g4 * 8);
    }

    int k_key[LD], k_c[LD];
    const char* v_src[LD];
#pragma unroll
    for (int i = 0; i < LD; ++i) {
        const int p = (i * NW + wave) * 64 + lane;
        {
            const int row = (p >> 4) & 63, pc = p & 15;
            k_c[i] = (pc ^ kswz(row)) * 8;
            k_key[i] = row;
        }
        {
            const int row = (p >> 3) & 127, pc = p & 7;
            const int c = pc ^ ((row >> 1) & 7);
            v_src[i] = (const char*)(Vp + (int64_t)row * Skp + c * 8);
        }
    }
    auto stage = [&](int buf, int t) {
        char* base = smem + buf * ATT_STAGE + wave * 1024;
        const int kv0 = t * KV;
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * NW + wave < 16) {  // wave-uniform
                const int key = min(kv0 + k_key[i], Sk - 1);
                glds16(Kp + (int64_t)key * HD + k_c[i], base + i * (NW * 1024));
            }
#pragma unroll
        for (int i = 0; i < LD; ++i)
            if (i * NW + wave < 16) glds16(v_src[i] + (int64_t)kv0 * 2, base + K_TILE_BYTES + i * (NW * 1024));
    };

    // LDS read offsets.  K tile kt = 2 kk + t, lane row = 32 kk + 8 (c >> 2) + 4 t + (c & 3); its swizzle is c.
    int k_off[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) k_off[kt] = (32 * (kt >> 1) + 8 * (l15 >> 2) + 4 * (kt & 1) + (l15 & 3)) * 256;
    int k_ch[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) k_ch[ks] = ((4 * ks + g4) ^ l15) << 4;
    const int v_row = l15 * 128;
    int v_ch[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) v_ch[kk] = ((4 * kk + g4) ^ ((l15 >> 1) & 7)) << 4;

    f4 oacc[8][2];
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = f4{0.f, 0.f, 0.f, 0.f};
    float m_run[2] = {SENTINEL, SENTINEL};
    float l_run[2] = {0.0f, 0.0f};

    const int nt = (Sk + KV - 1) / KV;
    stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // LDS-DMA of tile t (see the 32x32 kernel)
        __syncthreads();
        if (t + 1 < nt) stage((t + 1) & 1, t + 1);
        const char* Ks = smem + (t & 1) * ATT_STAGE;
        const char* Vs = Ks + K_TILE_BYTES;

        f4 sacc[4][2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) sacc[kt][qt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                const bf16x8 kf = *(const bf16x8*)(Ks + k_off[kt] + k_ch[ks]);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
                    sacc[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[qt][ks], sacc[kt][qt], 0, 0, 0);
            }

        if (t == nt - 1 && (Sk & (KV - 1)) != 0) {  // mask keys past Sk (wave-uniform branch)
            const int kv0 = t * KV;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kv0 + 32 * (kt >> 1) + 8 * g4 + 4 * (kt & 1) + r;
                    if (key >= Sk) {
                        sacc[kt][0][r] = SENTINEL;
                        sacc[kt][1][r] = SENTINEL;
                    }
                }
        }

        float mx[2];
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float m = sacc[0][qt][0];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, sacc[kt][qt][r]);
            mx[qt] = max_xor32(max_xor16(m)) * scale_log2e;
        }
        if (__any(mx[0] > m_run[0] + DEFER || mx[1] > m_run[1] + DEFER)) {
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                const float m_new = ceilf(fmaxf(m_run[qt], mx[qt]));   // integer: attn_tile.h
                const float alpha = fast_exp2(m_run[qt] - m_new);
                m_run[qt] = m_new;
                l_run[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 8; ++dt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) oacc[dt][qt][r] *= alpha;
            }
        }
        bf16x8 pf[2][2];  // [query tile][PV step]: keys 32 kk + 8 g .. +7
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
            float psum = 0.0f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = fast_exp2(fmaf(sacc[kt][qt][r], scale_log2e, -m_run[qt]));
                    psum += pv;
                    pf[qt][kt >> 1][4 * (kt & 1) + r] = (__bf16)pv;
                }
            l_run[qt] += psum;
        }

#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const bf16x8 vf = *(const bf16x8*)(Vs + dt * 2048 + v_row + v_ch[kk]);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt)
                    oacc[dt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[qt][kk], oacc[dt][qt], 0, 0, 0);
            }
    }

    // ---- epilogue: lane holds O[query c][d = 16 dt + 4 g + (0..3)]; pairs of d-tiles are exchanged with
    // v_permlane16_swap into 8 consecutive d starting at 32 p + 16 (g & 1) + 8 (g >> 1) -> 16-byte stores
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const float inv = 1.0f / sum_xor32(sum_xor16(l_run[qt]));
        bf16_t* op = O + (int64_t)b * o_sb + (int64_t)min(qrow[qt], Sq - 1) * o_ss + (int64_t)h * o_sh;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            uint32_t x0 = pack_bf16(oacc[2 * p][qt][0] * inv, oacc[2 * p][qt][1] * inv);
            uint32_t x1 = pack_bf16(oacc[2 * p][qt][2] * inv, oacc[2 * p][qt][3] * inv);
            uint32_t y0 = pack_bf16(oacc[2 * p + 1][qt][0] * inv, oacc[2 * p + 1][qt][1] * inv);
            uint32_t y1 = pack_bf16(oacc[2 * p + 1][qt][2] * inv, oacc[2 * p + 1][qt][3] * inv);
            auto r0 = __builtin_amdgcn_permlane16_swap(x0, y0, false, false);
            auto r1 = __builtin_amdgcn_permlane16_swap(x1, y1, false, false);
            if (qrow[qt] < Sq) {
                const u32x4 o = {r0[0], r1[0], r0[1], r1[1]};
                *(u32x4*)(op + 32 * p + 16 * (g4 & 1) + 8 * (g4 >> 1)) = o;
            }
        }
    }
}

// ---- materialised attention for head dims the flash kernel does not cover (VAE mid blocks: one head of
// C = 384 / 512 over 1k-16k tokens).  scores (f32) = q k^T by the GEMM kernel's f32 epilogue, one row-softmax
// pass (f32 in, bf16 probabilities out, zero-padded to a multiple of 64 keys), out = P V by the GEMM kernel with
// V^T as its weight operand.  Same rounding points as the flash kernels: f32 scores, bf16 P, f32 accumulation.
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ x, int64_t ldx, int cols_all,
                                                           float scale_log2e, bf16_t* __restrict__ out, int64_t ldo,
                                                           int cols_pad, int causal_block) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xr = x + (int64_t)blockIdx.x * ldx;
    bf16_t* orow = out + (int64_t)blockIdx.x * ldo;
    // frame-causal mask (HunyuanVideo15AttnBlock.prepare_causal_attention_mask): row r sees the keys of frames <= its own,
    // i.e. columns < (r / block + 1) * block; masked probabilities are exact zeros, as exp(-inf) is
    const int cols = causal_block > 0 ? min(cols_all, ((int)blockIdx.x / causal_block + 1) * causal_block) : cols_all;
    constexpr int MAXCH = 16;  // register-resident up to 16 x 1024 columns; longer rows stream from L2
    f32x4 v[MAXCH];
    const bool fits = cols <= MAXCH * 1024;
    float mx = -1.0e30f;
    if (fits) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = (i * 256 + tid) * 4;
            v[i] = c < cols ? *(const f32x4*)(xr + c) : f32x4{-1.0e30f, -1.0e30f, -1.0e30f, -1.0e30f};
#pragma unroll
            for (int j = 1; j < 4; ++j) v[i][j] = c + j < cols ? v[i][j] : -1.0e30f;   // cols need not be a multiple of 4
            mx = fmaxf(mx, fmaxf(fmaxf(v[i][0], v[i][1]), fmaxf(v[i][2], v[i][3])));
        }
    } else {
        for (int c = tid * 4; c < cols; c += 1024) {
            f32x4 t = *(const f32x4*)(xr + c);
#pragma unroll
            for (int j = 1; j < 4; ++j) t[j] = c + j < cols ? t[j] : -1.0e30f;
            mx = fmaxf(mx, fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3])));
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * scale_log2e;
    float sum = 0.0f;
    if (fits) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[i][j] = fast_exp2(fmaf(v[i][j], scale_log2e, -mx));
                sum += v[i][j];
            }
        }
    } else {
        for (int c = tid * 4; c < cols; c += 1024) {
            const f32x4 t = *(const f32x4*)(xr + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) sum += c + j < cols ? fast_exp2(fmaf(t[j], scale_log2e, -mx)) : 0.0f;
        }
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float inv = 1.0f / (red[4] + red[5] + red[6] + red[7]);
    if (fits) {
#pragma unroll
        for (int i = 0; i < MAXCH; ++i) {
            const int c = (i * 256 + tid) * 4;
            if (c < cols_pad) {
                u32x2 o = {0u, 0u};
                if (c < cols) o = u32x2{pack_bf16(v[i][0] * inv, v[i][1] * inv), pack_bf16(v[i][2] * inv, v[i][3] * inv)};
                *(u32x2*)(orow + c) = o;
            }
        }
    } else {
        for (int c = tid * 4; c < cols_pad; c += 1024) {
            u32x2 o = {0u, 0u};
            if (c < cols) {
                const f32x4 t = *(const f32x4*)(xr + c);
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = c + j < cols ? fast_exp2(fmaf(t[j], scale_log2e, -mx)) * inv : 0.0f;
                o = u32x2{pack_bf16(e[0], e[1]), pack_bf16(e[2], e[3])};
            }
            *(u32x2*)(orow + c) = o;
        }
    }
}

// ---- row softmax with an additive bias and a key mask (text encoders: T5 / UMT5 relative-position bias shared by
// the batch, CLIP's causal mask).  Grid (Sq, heads); f32 scores [heads, Sq, ldx] in, bf16 probabilities
// [heads, Sq, ldo] out, zero beyond the kept keys.  p = softmax(x * scale + bias[head, row, :]) over the kept
// columns; masked keys get exact zeros, which is what the reference's finfo.min additive mask yields in f32.
__global__ __launch_bounds__(256) void softmax_bias_rows_kernel(const float* __restrict__ x, int64_t ldx, int Sq, int cols,
                                                                float scale_log2e, const float* __restrict__ bias,
                                                                int64_t bias_ld, const uint8_t* __restrict__ keep,
                                                                const int* __restrict__ seg, int causal,
                                                                bf16_t* __restrict__ out, int64_t ldo, int cols_pad) {
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.y * Sq + blockIdx.x;
    const float* xr = x + row * ldx;
    const float* br = bias ? bias + row * bias_ld : nullptr;
    bf16_t* orow = out + row * ldo;
    const int lim = causal ? min(cols, (int)blockIdx.x + 1) : cols;
    const int myseg = seg ? seg[blockIdx.x] : 0;   // block-diagonal attention: a query sees the keys of its own segment
    auto score = [&](int c) -> float {
        if (c >= lim || (keep && !keep[c]) || (seg && seg[c] != myseg)) return -1.0e30f;
        return fmaf(xr[c], scale_log2e, br ? br[c] * LOG2E : 0.0f);
    };
    float mx = -1.0e30f;
    for (int c = tid; c < lim; c += 256) mx = fmaxf(mx, score(c));
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.0f;
    for (int c = tid; c < lim; c += 256) {
        const float sc = score(c);
        sum += sc > -1.0e29f ? fast_exp2(sc - mx) : 0.0f;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float tot = red[4] + red[5] + red[6] + red[7];
    const float inv = tot > 0.0f ? 1.0f / tot : 0.0f;   // a row with no kept key (never produced by the encoders) -> zeros
    for (int c = tid; c < cols_pad; c += 256) {
        const float sc = score(c);
        orow[c] = f32_to_bf16(sc > -1.0e29f ? fast_exp2(sc - mx) * inv : 0.0f);
    }
}

// ---- f32-storage verification form of the text encoders' attention (apexmi_attn_fwd_bias_f32): one workgroup per (query row,
// head), float q / k / v / out, f32 arithmetic throughout (no bf16 probabilities), the same score / mask rules as
// softmax_bias_rows_kernel: p = softmax(q.k * scale + bias[h, row, :]) over the kept keys (key-padding mask, causal limit,
// segment ids), grouped-query key heads.  Scores of the row live in LDS (Sk floats).  Not a performance path.
__global__ __launch_bounds__(256) void attn_bias_rows_f32_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                 int64_t ldk, const float* __restrict__ v, int64_t ldv,
                                                                 float* __restrict__ out, int64_t ldo, int H, int Hkv, int Sq, int Sk,
                                                                 int D, float scale, const float* __restrict__ bias,
                                                                 const uint8_t* __restrict__ keep, const int* __restrict__ seg,
                                                                 int causal) {
    extern __shared__ __attribute__((aligned(16))) char smem_[];
    float* sc = (float*)smem_;                 // [Sk]
    float* qs = sc + Sk;                        // [D]
    __shared__ float red[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x, h = blockIdx.y, hk = h / (H / Hkv);
    for (int d = tid; d < D; d += 256) qs[d] = q[(int64_t)row * ldq + h * D + d];
    __syncthreads();
    const int lim = causal ? min(Sk, row + 1) : Sk;
    const int myseg = seg ? seg[row] : 0;
    const float* br = bias ? bias + ((int64_t)h * Sq + row) * Sk : nullptr;
    float mx = -1.0e30f;
    for (int c = tid; c < Sk; c += 256) {
        float s = -1.0e30f;
        if (c < lim && !(keep && !keep[c]) && !(seg && seg[c] != myseg)) {
            const float* kr = k + (int64_t)c * ldk + hk * D;
            float acc = 0.0f;
            for (int d = 0; d < D; ++d) acc = fmaf(qs[d], kr[d], acc);
            s = acc * scale + (br ? br[c] : 0.0f);
        }
        sc[c] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.0f;
    for (int c = tid; c < Sk; c += 256) {
        const float e = sc[c] > -1.0e29f ? expf(sc[c] - mx) : 0.0f;
        sc[c] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    const float tot = red[4] + red[5] + red[6] + red[7];
    const float inv = tot > 0.0f ? 1.0f / tot : 0.0f;
    for (int d = tid; d < D; d += 256) {
        float acc = 0.0f;
        for (int c = 0; c < Sk; ++c) acc = fmaf(sc[c], v[(int64_t)c * ldv + hk * D + d], acc);
        out[(int64_t)row * ldo + h * D + d] = acc * inv;
    }
}

// ---- generic fallback: any D <= 256, bf16 / f16 / f32, strided views; one workgroup per query row.
// Exists so the operator survives the reference's backend verification probe
// (B,H,S,D = 1,2,8,64 fp16; attention/functions.py:1999-2251) and odd head sizes (VAE C = 384 is
// handled by splitting is not needed: D <= 512 threads).  Not a performance path.
template <typename T>
APEXMI_DEVICE float ld_elem(const T* p);
template <>
APEXMI_DEVICE float ld_elem<uint16_t>(const uint16_t* p) { return bf16_to_f32(*p); }
template <>
APEXMI_DEVICE float ld_elem<_Float16>(const _Float16* p) { return (float)*p; }
template <>
APEXMI_DEVICE float ld_elem<float>(const float* p) { return *p; }
template <typename T>
APEXMI_DEVICE void st_elem(T* p, float v);
template <>
APEXMI_DEVICE void st_elem<uint16_t>(uint16_t* p, float v) { *p = f32_to_bf16(v); }
template <>
APEXMI_DEVICE void st_elem<_Float16>(_Float16* p, float v) { *p = (_Float16)v; }
template <>
APEXMI_DEVICE void st_elem<float>(float* p, float v) { *p = v; }

constexpr int GEN_THREADS = 512;

template <typename T>
__global__ __launch_bounds__(GEN_THREADS) void attn_fwd_generic_kernel(
    const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ V, T* __restrict__ O,
    int H, int Sq, int Sk, int D, int64_t q_sb, int64_t q_sh, int64_t q_ss, int64_t k_sb,
    int64_t k_sh, int64_t k_ss, int64_t v_sb, int64_t v_sh, int64_t v_ss, int64_t o_sb,
    int64_t o_ss, int64_t o_sh, float scale, int64_t v_sd) {
    __shared__ float qs[512];
    __shared__ float ps[GEN_THREADS];
    __shared__ float red[GEN_THREADS / 64];
    __shared__ float bc[2];
    const int tid = threadIdx.x;
    const int q = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const T* qp = Q + b * q_sb + h * q_sh + q * q_ss;
    for (int d = tid; d < D; d += GEN_THREADS) qs[d] = ld_elem<T>(qp + d) * scale;
    __syncthreads();
    float m_run = -1.0e30f, l_run = 0.0f, acc = 0.0f;
    for (int k0 = 0; k0 < Sk; k0 += GEN_THREADS) {
        const int key = k0 + tid;
        float sc = -1.0e30f;
        if (key < Sk) {
            const T* kp = K + b * k_sb + h * k_sh + key * k_ss;
            float a = 0.0f;
            for (int d = 0; d < D; ++d) a = fmaf(qs[d], ld_elem<T>(kp + d), a);
            sc = a;
        }
        float mx = wave_max(sc);
        if ((tid & 63) == 0) red[tid >> 6] = mx;
        __syncthreads();
        if (tid == 0) {
            float mm = red[0];
            for (int i = 1; i < GEN_THREADS / 64; ++i) mm = fmaxf(mm, red[i]);
            bc[0] = mm;
        }
        __syncthreads();
        const float m_new = fmaxf(m_run, bc[0]);
        const float alpha = __expf(m_run - m_new);
        const float p = (key < Sk) ? __expf(sc - m_new) : 0.0f;
        ps[tid] = p;
        float sm = wave_sum(p);
        __syncthreads();  // everyone has read bc[0]; ps complete after the next barrier
        if ((tid & 63) == 0) red[tid >> 6] = sm;
        __syncthreads();
        float tot = 0.0f;
        for (int i = 0; i < GEN_THREADS / 64; ++i) tot += red[i];
        l_run = l_run * alpha + tot;
        m_run = m_new;
        if (tid < D) {
            acc *= alpha;
            const int nk = min(GEN_THREADS, Sk - k0);
            const T* vp = V + b * v_sb + h * v_sh + (int64_t)k0 * v_ss + tid * v_sd;   // v_sd = 1, or Skp for a V^T operand
            for (int j = 0; j < nk; ++j) acc = fmaf(ps[j], ld_elem<T>(vp + (int64_t)j * v_ss), acc);
        }
        __syncthreads();
    }
    if (tid < D) st_elem<T>(O + b * o_sb + q * o_ss + h * o_sh + tid, acc / l_run);
}

template <typename T>
int launch_generic(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq,
                   int Sk, int D, const int64_t* qs, const int64_t* ks, const int64_t* vs,
                   const int64_t* os, float scale, hipStream_t stream, int64_t v_sd = 1) {
    hipLaunchKernelGGL(attn_fwd_generic_kernel<T>, dim3(Sq, H, B), dim3(GEN_THREADS), 0, stream,
                       (const T*)q, (const T*)k, (const T*)v, (T*)out, H, Sq, Sk, D, qs[0], qs[1],
                       qs[2], ks[0], ks[1], ks[2], vs[0], vs[1], vs[2], os[0], os[1], os[2], scale, v_sd);
    return apexmi_check_launch("attn_fwd_generic");
}

int g_attn_waves = 0;  // 0 auto, 4, 8 (apexmi_tune_set "attn.waves")
int g_attn_c4 = 3;  // apexmi_tune_set("attn.c4", v): 0 = plain loop; v >= 1: 8-wave launches use the 4-cluster ping-pong kernel
                    // (-3.4 % per attention launch in the Flux and HunyuanVideo steps) with the variant bits of (v - 1):
                    // 1 = s_setprio in the matrix clusters (neutral), 2 = packed-f32 softmax (shipped: +0.5..0.9 %,
                    // tools/attn_ab.py), 4 = static priority for waves 4..7 (-0.5 %)
int g_attn_mfma = 32;  // 32: 32x32x16 kernel (shipped: 3 % faster in the Flux step), 16: 16x16x32 kernel (apexmi_tune_set "attn.mfma")

// contiguity test for the MFMA path's packed [B,H,S,128] operands
bool packed_bhsd(const int64_t* st, int H, int S, int D) {
    return st[2] == D && st[1] == (int64_t)S * D && st[0] == (int64_t)H * S * D;
}



// workspace layout of the materialised path: [scores f32 Sq x Sk8][P bf16 Sq x Skp][V^T bf16 D x Skp][K bf16 Sk8 x D]
// (Sk8 = Sk rounded up to 8: the GEMM writes whole 8-column groups; the zero-padded K copy exists only when Sk8 != Sk)
bool use_materialised(int Sq, int Sk, int D, int dtype, const int64_t* qs, const int64_t* ks, const int64_t* vs,
                      const int64_t* os, int causal_block) {
    // D = 128 belongs to the flash kernels, except under the frame-causal mask (they carry no mask)
    return dtype == APEXMI_BF16 && (D != HD || causal_block > 0) && D % 128 == 0 && D <= 1024 &&
           ((int64_t)Sq * Sk >= 256 * 256 || causal_block > 0) && qs[2] % 8 == 0 && ks[2] % 8 == 0 && vs[2] % 8 == 0 &&
           os[1] % 8 == 0;
}
size_t materialised_bytes(int Sq, int Sk, int D) {
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV, sk8 = (size_t)((Sk + 7) / 8) * 8;
    return (size_t)Sq * sk8 * 4 + (size_t)Sq * skp * 2 + (size_t)D * skp * 2 + (sk8 != (size_t)Sk ? sk8 * D * 2 : 0);
}

}  // namespace

// out[row] = sum_i 2^(m_i - M) o_i / sum_i 2^(m_i - M) l_i, M = max_i m_i: merge of the tail launch's partial numerators
// o_i (f32), integer maxima m_i and partial sums l_i.  One wave per query row, 2 channels per lane.
__global__ __launch_bounds__(256) void attn_combine_kernel(const float* __restrict__ opart, const float* __restrict__ ml,
                                                           bf16_t* __restrict__ O, int nsplit, int qbr, int nqb, int H,
                                                           int Sq, int s_base, int ntail, int64_t o_sb, int64_t o_ss,
                                                           int64_t o_sh) {
    const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (gw >= (int64_t)ntail * qbr) return;
    const int j = (int)(gw / qbr), r = (int)(gw % qbr), lane = threadIdx.x & 63;
    const int s = s_base + j, hb = s / nqb, qb = s % nqb;
    const int qrow = qb * qbr + r;
    if (qrow >= Sq) return;
    float mx = -1.0e30f;
    for (int i = 0; i < nsplit; ++i) mx = fmaxf(mx, ml[(((int64_t)j * nsplit + i) * qbr + r) * 2]);
    float den = 0.0f, a0 = 0.0f, a1 = 0.0f;
    for (int i = 0; i < nsplit; ++i) {
        const int64_t p = ((int64_t)j * nsplit + i) * qbr + r;
        const float w = fast_exp2(ml[p * 2] - mx);          // exact power of two (integer maxima)
        const float2 v = *(const float2*)(opart + p * HD + lane * 2);
        den = fmaf(w, ml[p * 2 + 1], den);
        a0 = fmaf(w, v.x, a0);
        a1 = fmaf(w, v.y, a1);
    }
    const float inv = 1.0f / den;
    *(uint32_t*)(O + (int64_t)(hb / H) * o_sb + (int64_t)qrow * o_ss + (int64_t)(hb % H) * o_sh + lane * 2) =
        pack_bf16(a0 * inv, a1 * inv);
}

namespace {
int g_attn_split = 1;   // apexmi_tune_set("attn.split", 0/1)
int g_attn_w64 = 1;     // apexmi_tune_set("attn.w64", 0/1/8): main launch on attn_fwd_d128_w64_kernel (1, shipped), on its running-maximum form attn_fwd_d128_w64r_kernel (8), or on the 4-cluster kernel (0)
constexpr int ATT_NSPLIT = 4, ATT_NCU = 256;
// the tail of an 8-wave launch worth splitting: a last round with at most a quarter of the CUs busy after 1..8 full ones
// (measured with the limit raised to 3/4 of a round: the Flux launch, 256 + 176 workgroups, gets 13 % SLOWER, 0.281 vs
// 0.2485 ms — a 2/3-full last round already runs at the higher clock its idle CUs pay for)
int attn_tail(int total, int Sk) {
    const int tail = total % ATT_NCU, rounds = total / ATT_NCU;
    return (g_attn_split && tail > 0 && tail * 4 <= ATT_NCU && rounds >= 1 && rounds <= 8 && Sk >= ATT_NSPLIT * 8 * KV) ? tail : 0;
}
}  // namespace
void apexmi_set_attn_split(int v) { g_attn_split = v; }

extern "C" size_t apexmi_attn_prepared_workspace_bytes(int B, int H, int Sq, int Sk) {
    const int nqb = (Sq + 255) / 256;
    const int64_t total = (int64_t)nqb * H * B;
    if (total < 256 || g_attn_waves == 4 || (g_attn_waves != 0 && g_attn_waves != 8)) return 0;
    const int tail = attn_tail((int)total, Sk);
    return (size_t)tail * ATT_NSPLIT * 256 * (HD * 4 + 8);
}

static int attn_fwd_prepared_impl(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq, int Sk,
                                  int Skp, const int64_t o_strides[3], float softmax_scale, void* workspace,
                                  size_t workspace_bytes, apexmi_stream_t stream_);

extern "C" int apexmi_attn_fwd_prepared(const void* q, const void* k, const void* vt, void* out,
                                        int B, int H, int Sq, int Sk, int Skp,
                                        const int64_t o_strides[3], float softmax_scale,
                                        apexmi_stream_t stream_) {
    return attn_fwd_prepared_impl(q, k, vt, out, B, H, Sq, Sk, Skp, o_strides, softmax_scale, nullptr, 0, stream_);
}

extern "C" int apexmi_attn_fwd_prepared_ws(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq,
                                           int Sk, int Skp, const int64_t o_strides[3], float softmax_scale,
                                           void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return attn_fwd_prepared_impl(q, k, vt, out, B, H, Sq, Sk, Skp, o_strides, softmax_scale, workspace, workspace_bytes,
                                  stream_);
}

// the two kernel signatures of the dispatch: the plain / 16x16 / w64 kernels, and the 4-cluster kernel with its tail-split arguments
using AttnKernel = void (*)(const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, int, int, int, int, int64_t, int64_t,
                            int64_t, float);
using AttnSplitKernel = void (*)(const bf16_t*, const bf16_t*, const bf16_t*, bf16_t*, int, int, int, int, int, int, int64_t,
                                 int64_t, int64_t, float, int, int, float*, float*);

static int attn_fwd_prepared_impl(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq, int Sk,
                                  int Skp, const int64_t o_strides[3], float softmax_scale, void* workspace,
                                  size_t workspace_bytes, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && vt && out, "attn_fwd_prepared: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0, "attn_fwd_prepared: empty problem");
    APEXMI_REQUIRE(Skp % KV == 0 && Skp >= Sk, "attn_fwd_prepared: Skp=%d must be Sk=%d rounded up to 64", Skp, Sk);
    APEXMI_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)vt % 16) == 0 &&
                       ((uintptr_t)out % 16) == 0,
                   "attn_fwd_prepared: operands must be 16-byte aligned");
    APEXMI_REQUIRE(o_strides[0] % 8 == 0 && o_strides[1] % 8 == 0 && o_strides[2] % 8 == 0,
                   "attn_fwd_prepared: output strides must be multiples of 8 elements");
    const float c = softmax_scale * LOG2E;
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * Sk * HD,
                         2.0 * B * H * HD * (2.0 * Sq + 2.0 * Sk));
    // Workgroup height: NW waves x 32 query rows, two workgroups resident per CU (64 KiB LDS each).
    // 8-wave workgroups once there are enough of them to fill the chip, else 4.  (Measured and rejected:
    // the height in {4..8} that minimises rounds of 512 resident workgroups — Flux fits one round of 504
    // seven-wave workgroups — is 7 % SLOWER than 432 eight-wave ones: 14 waves per CU split 4/4/3/3 over
    // the SIMDs.  `attn.waves` still accepts 4..8.)
    int nw = g_attn_waves;
    // the w64 kernel (one 256-row workgroup per CU) beats 128-row 4-wave workgroups from 144 workgroups up although it leaves CUs
    // idle (24 x 1536, the 512^2 Flux geometry: 41 vs 52 us; 192: x1.30, 240: x1.21) and loses below (128: x0.96, 96: x0.89) —
    // tools/attn_small_ab.py, profiles/r05_attn_small_ab.log
    if (nw == 0) nw = (int64_t)((Sq + 255) / 256) * H * B >= (g_attn_w64 ? 140 : 256) ? 8 : 4;
    const int qbr = nw * 32;
    const int nqb = (Sq + qbr - 1) / qbr;
    const int total = nqb * H * B;
    const bool m16 = g_attn_mfma == 16;
    if (nw == 8 && !m16 && g_attn_c4) {
        // ---- shipped path: 4-cluster kernel; a nearly empty last round is cut into ATT_NSPLIT key ranges ----
        // bit 0: s_setprio around the matrix clusters; bit 1: packed-f32 softmax; bit 2: static priority for waves 4..7
        const int var = (g_attn_c4 - 1) & 7;
        static const AttnSplitKernel c4_tab[8] = {
            attn_fwd_d128_c4_kernel<8, 0>, attn_fwd_d128_c4_kernel<8, 1>, attn_fwd_d128_c4_kernel<8, 2>,
            attn_fwd_d128_c4_kernel<8, 3>, attn_fwd_d128_c4_kernel<8, 4>, attn_fwd_d128_c4_kernel<8, 5>,
            attn_fwd_d128_c4_kernel<8, 6>, attn_fwd_d128_c4_kernel<8, 7>};
        const AttnSplitKernel c4 = c4_tab[var];
        const int c4_lds = 2 * ATT_STAGE;
        static uint64_t c4_attr[8] = {};
        APEXMI_SET_ATTR_ONCE(c4_attr[var],
            (void)hipFuncSetAttribute((const void*)c4, hipFuncAttributeMaxDynamicSharedMemorySize, c4_lds));
        int tail = attn_tail(total, Sk);
        const size_t need = (size_t)tail * ATT_NSPLIT * 256 * (HD * 4 + 8);
        if (tail && (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 16) != 0)) tail = 0;
        const int main_wgs = total - tail;
#if APEXMI_ATTN_TRACE
        {
            const char* e = getenv("APEXMI_ATTN_TRACE_PTR");
            unsigned long long* p = e ? (unsigned long long*)strtoull(e, nullptr, 16) : nullptr;
            (void)hipMemcpyToSymbolAsync(HIP_SYMBOL(d_attn_trace), &p, sizeof(p), 0, hipMemcpyHostToDevice, stream);
        }
#endif
        if (g_attn_w64) {
            // ---- shipped main launch: one wave per SIMD, 64 query rows per wave (attn_fwd_d128_w64_kernel); the split tail
            // below stays on the 4-cluster kernel ----
            const AttnKernel w64 = g_attn_w64 == 8 ? attn_fwd_d128_w64r_kernel : attn_fwd_d128_w64_kernel;
            const int w64_lds = 4 * ATT_STAGE + 16;          // the rings + the fallback vote's word
            static uint64_t w64_attr[2] = {};
            APEXMI_SET_ATTR_ONCE(w64_attr[g_attn_w64 == 8],
                (void)hipFuncSetAttribute((const void*)w64, hipFuncAttributeMaxDynamicSharedMemorySize, w64_lds));
            hipLaunchKernelGGL(w64, dim3(main_wgs), dim3(256), w64_lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                               (const bf16_t*)vt, (bf16_t*)out, H, Sq, Sk, Skp, nqb, main_wgs, o_strides[0], o_strides[1],
                               o_strides[2], c);
            if (int rc = apexmi_check_launch("attn_fwd_d128_w64")) return rc;
        } else {
        hipLaunchKernelGGL(c4, dim3(main_wgs), dim3(512), c4_lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                           (const bf16_t*)vt, (bf16_t*)out, H, Sq, Sk, Skp, nqb, main_wgs, o_strides[0], o_strides[1],
                           o_strides[2], c, 0, 1, (float*)nullptr, (float*)nullptr);
        if (int rc = apexmi_check_launch("attn_fwd_d128")) return rc;
        }
        if (tail) {
            float* opart = (float*)workspace;
            float* lse = (float*)((char*)workspace + (size_t)tail * ATT_NSPLIT * 256 * HD * 4);
            hipLaunchKernelGGL(c4, dim3(tail * ATT_NSPLIT), dim3(512), c4_lds, stream, (const bf16_t*)q,
                               (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, H, Sq, Sk, Skp, nqb, total, o_strides[0],
                               o_strides[1], o_strides[2], c, main_wgs, ATT_NSPLIT, opart, lse);
            if (int rc = apexmi_check_launch("attn_fwd_d128 (tail)")) return rc;
            hipLaunchKernelGGL(attn_combine_kernel, dim3((tail * 256 + 3) / 4), dim3(256), 0, stream, opart, lse,
                               (bf16_t*)out, ATT_NSPLIT, 256, nqb, H, Sq, main_wgs, tail, o_strides[0], o_strides[1],
                               o_strides[2]);
            return apexmi_check_launch("attn_combine");
        }
        return 0;
    }
    AttnKernel kern = nullptr;
    switch (nw) {
        case 4: kern = m16 ? attn_fwd_d128_mi16_kernel<4> : attn_fwd_d128_kernel<4>; break;
        case 5: kern = m16 ? attn_fwd_d128_mi16_kernel<5> : attn_fwd_d128_kernel<5>; break;
        case 6: kern = m16 ? attn_fwd_d128_mi16_kernel<6> : attn_fwd_d128_kernel<6>; break;
        case 7: kern = m16 ? attn_fwd_d128_mi16_kernel<7> : attn_fwd_d128_kernel<7>; break;
        case 8: kern = m16 ? attn_fwd_d128_mi16_kernel<8> : attn_fwd_d128_kernel<8>; break;
        default: apexmi_set_error("attn_fwd_prepared: attn.waves=%d not in [4,8]", nw); return 1;
    }
    static uint64_t attr_done[2][9] = {};
    APEXMI_SET_ATTR_ONCE(attr_done[m16][nw],
        (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * ATT_STAGE));
    hipLaunchKernelGGL(kern, dim3(total), dim3(nw * 64), 2 * ATT_STAGE, stream, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)vt, (bf16_t*)out, H, Sq, Sk, Skp, nqb, total,
                       o_strides[0], o_strides[1], o_strides[2], c);
    return apexmi_check_launch("attn_fwd_d128");
}

// ---- per-block key bands on the w64 kernel --------------------------------------------------------------
// Always the band kernel, one 256-row workgroup per query block: no 4-wave form, no tail split.
extern "C" int apexmi_attn_fwd_prepared_band(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq,
                                             int Sk, int Skp, const int64_t o_strides[3], const void* bands, int Hb,
                                             float softmax_scale, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && vt && out && o_strides, "attn_fwd_prepared_band: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0, "attn_fwd_prepared_band: empty problem");
    APEXMI_REQUIRE(Skp % KV == 0 && Skp >= Sk, "attn_fwd_prepared_band: Skp=%d must be Sk=%d rounded up to 64", Skp, Sk);
    APEXMI_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)vt % 16) == 0 &&
                       ((uintptr_t)out % 16) == 0,
                   "attn_fwd_prepared_band: operands must be 16-byte aligned");
    APEXMI_REQUIRE(o_strides[0] % 8 == 0 && o_strides[1] % 8 == 0 && o_strides[2] % 8 == 0,
                   "attn_fwd_prepared_band: output strides must be multiples of 8 elements");
    // the descriptors hold byte ranges in 32 bits: 128 x Skp x 2 bytes of V^T
    APEXMI_REQUIRE(Sk <= (1 << 20) && Skp <= (1 << 20) + KV, "attn_fwd_prepared_band: Sk=%d above 1048576 keys", Sk);
    const int nqb = (Sq + 255) / 256;
    APEXMI_REQUIRE((int64_t)nqb * H * B < (int64_t)1 << 31, "attn_fwd_prepared_band: too many query blocks");
    APEXMI_REQUIRE(bands && ((uintptr_t)bands % 8) == 0, "attn_fwd_prepared_band: null or misaligned band plan (int32 pairs, 8-byte aligned)");
    APEXMI_REQUIRE(Hb == 1 || Hb == H, "attn_fwd_prepared_band: plan of %d heads for %d heads (1 or H)", Hb, H);
    const int total = nqb * H * B;
    // the work is not known on the host (the plan lives on the device): the profile counts the dense launch's
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * Sk * HD, 2.0 * B * H * HD * (2.0 * Sq + 2.0 * Sk));
    const int lds = 4 * ATT_STAGE + 16;              // the rings + the fallback vote's word
    static uint64_t attr_done = 0;
    APEXMI_SET_ATTR_ONCE(attr_done, (void)hipFuncSetAttribute((const void*)attn_fwd_d128_w64_band_kernel,
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(attn_fwd_d128_w64_band_kernel, dim3(total), dim3(256), lds, stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)vt, (bf16_t*)out, H, Sq, Sk, Skp, nqb, total, o_strides[0], o_strides[1], o_strides[2],
                       softmax_scale * LOG2E, (const int*)bands, Hb == 1 ? 0 : nqb);
    return apexmi_check_launch("attn_fwd_d128_w64_band");
}

extern "C" size_t apexmi_attn_band_workspace_bytes(int B, int H, int Sq, int Sk) {
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0) return 0;
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV;
    // V^T plus packed copies of q and k (used only when the caller's views are not packed)
    return (size_t)B * H * HD * skp * 2 + (size_t)B * H * ((size_t)Sq + Sk) * HD * 2;
}

int apexmi_pack_bhsd(const void* x, const int64_t* st, int B, int H, int S, int D, void* out, hipStream_t stream);

extern "C" int apexmi_attn_fwd_band(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk, int D,
                                    const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                                    const int64_t o_strides[3], const void* bands, int Hb, float softmax_scale, int dtype,
                                    void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "attn_fwd_band";
    if (int rc = require_operands(who, q, k, v, out, q_strides, k_strides, v_strides, o_strides)) return rc;
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0, "attn_fwd_band: empty problem (B=%d H=%d Sq=%d Sk=%d)", B, H, Sq, Sk);
    if (int rc = require_head_dim(who, D, D == HD, "128 only: the band kernel is the D = 128 flash kernel")) return rc;
    APEXMI_REQUIRE(dtype == APEXMI_BF16, "attn_fwd_band: dtype %d unsupported (bf16 only)", dtype);
    APEXMI_REQUIRE(q_strides[2] >= D && k_strides[2] >= D && v_strides[2] >= D,
                   "attn_fwd_band: row strides below the head dim %d (rows must not overlap)", D);
    if (int rc = require_workspace(who, workspace, workspace_bytes, apexmi_attn_band_workspace_bytes(B, H, Sq, Sk), true)) return rc;
    const int skp = ((Sk + KV - 1) / KV) * KV;
    char* ws = (char*)workspace;
    void* vt = ws;
    ws += (size_t)B * H * HD * skp * 2;
    const void* qp = q;
    const void* kp = k;
    // the other refusals (plan, output alignment, limits) are the prepared entry's: nothing is launched before they pass
    APEXMI_REQUIRE(bands && ((uintptr_t)bands % 8) == 0, "attn_fwd_band: null or misaligned band plan (int32 pairs, 8-byte aligned)");
    APEXMI_REQUIRE(Hb == 1 || Hb == H, "attn_fwd_band: plan of %d heads for %d heads (1 or H)", Hb, H);
    APEXMI_REQUIRE(((uintptr_t)out % 16) == 0 && o_strides[0] % 8 == 0 && o_strides[1] % 8 == 0 && o_strides[2] % 8 == 0,
                   "attn_fwd_band: out must be 16-byte aligned with strides multiples of 8 elements");
    APEXMI_REQUIRE(Sk <= (1 << 20), "attn_fwd_band: Sk=%d above 1048576 keys", Sk);
    APEXMI_REQUIRE((int64_t)((Sq + 255) / 256) * H * B < (int64_t)1 << 31, "attn_fwd_band: too many query blocks");
    if (!packed_bhsd(q_strides, H, Sq, D) || ((uintptr_t)q % 16) != 0) {
        if (int rc = apexmi_pack_bhsd(q, q_strides, B, H, Sq, D, ws, stream)) return rc;
        qp = ws;
    }
    ws += (size_t)B * H * Sq * HD * 2;
    if (!packed_bhsd(k_strides, H, Sk, D) || ((uintptr_t)k % 16) != 0) {
        if (int rc = apexmi_pack_bhsd(k, k_strides, B, H, Sk, D, ws, stream)) return rc;
        kp = ws;
    }
    for (int b = 0; b < B; ++b) {
        const bf16_t* vb = (const bf16_t*)v + b * v_strides[0];
        bf16_t* vtb = (bf16_t*)vt + (size_t)b * H * HD * skp;
        if (int rc = apexmi_v_transpose(vb, v_strides[1], v_strides[2], Sk, H, D, vtb, skp, 0, stream)) return rc;
    }
    return apexmi_attn_fwd_prepared_band(qp, kp, vt, out, B, H, Sq, Sk, skp, o_strides, bands, Hb, softmax_scale, stream_);
}

void apexmi_set_attn_waves(int v) { g_attn_waves = v; }
void apexmi_set_attn_mfma(int v) { g_attn_mfma = v; }
void apexmi_set_attn_c4(int v) { g_attn_c4 = v; }
void apexmi_set_attn_w64(int v) { g_attn_w64 = v; }

extern "C" int apexmi_attn_w64_fallbacks(uint64_t* count) {
    APEXMI_REQUIRE(count, "attn_w64_fallbacks: null count");
    unsigned int n = 0, zero = 0;
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpyFromSymbol(&n, HIP_SYMBOL(d_attn_w64_fallbacks), sizeof(n));
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(d_attn_w64_fallbacks), &zero, sizeof(zero));
    APEXMI_REQUIRE(e == hipSuccess, "attn_w64_fallbacks: %s", hipGetErrorString(e));
    *count = n;
    return 0;
}

extern "C" size_t apexmi_attn_workspace_bytes(int B, int H, int Sq, int Sk, int D, int dtype) {
    if (dtype == APEXMI_BF16 && D != HD && D % 128 == 0 && D <= 1024 && (int64_t)Sq * Sk >= 256 * 256)
        return materialised_bytes(Sq, Sk, D);   // one (batch, head) at a time on the stream
    if (dtype != APEXMI_BF16 || D != HD) return 0;
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV;
    // V^T plus packed copies of q and k (used only when the caller's views are not packed) plus the tail-split scratch
    return (size_t)B * H * HD * skp * 2 + (size_t)B * H * ((size_t)Sq + Sk) * HD * 2 +
           apexmi_attn_prepared_workspace_bytes(B, H, Sq, Sk);
}

int apexmi_pack_bhsd(const void* x, const int64_t* st, int B, int H, int S, int D, void* out,
                     hipStream_t stream);

// causal_block > 0: frame-causal mask with that many tokens per frame (materialised path only)
static int attn_fwd_impl(const void* q, const void* k, const void* v, void* out, int B, int H, int Sq, int Sk, int D,
                         const int64_t q_strides[3], const int64_t k_strides[3], const int64_t v_strides[3],
                         const int64_t o_strides[3], float softmax_scale, int dtype, void* workspace,
                         size_t workspace_bytes, int causal_block, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && v && out, "attn_fwd: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0 && D > 0, "attn_fwd: empty problem");
    if (dtype == APEXMI_BF16 && D == HD && causal_block == 0) {
        const size_t need = apexmi_attn_workspace_bytes(B, H, Sq, Sk, D, dtype);
        APEXMI_REQUIRE(workspace && workspace_bytes >= need,
                       "attn_fwd: workspace too small (%zu < %zu)", workspace_bytes, need);
        const int skp = ((Sk + KV - 1) / KV) * KV;
        char* ws = (char*)workspace;
        void* vt = ws;
        ws += (size_t)B * H * HD * skp * 2;
        const void* qp = q;
        const void* kp = k;
        if (!packed_bhsd(q_strides, H, Sq, D)) {
            if (int rc = apexmi_pack_bhsd(q, q_strides, B, H, Sq, D, ws, stream)) return rc;
            qp = ws;
        }
        ws += (size_t)B * H * Sq * HD * 2;
        if (!packed_bhsd(k_strides, H, Sk, D)) {
            if (int rc = apexmi_pack_bhsd(k, k_strides, B, H, Sk, D, ws, stream)) return rc;
            kp = ws;
        }
        for (int b = 0; b < B; ++b) {
            const bf16_t* vb = (const bf16_t*)v + b * v_strides[0];
            bf16_t* vtb = (bf16_t*)vt + (size_t)b * H * HD * skp;
            if (int rc = apexmi_v_transpose(vb, v_strides[1], v_strides[2], Sk, H, D, vtb, skp, 0, stream))
                return rc;
        }
        ws += (size_t)B * H * Sk * HD * 2;
        return apexmi_attn_fwd_prepared_ws(qp, kp, vt, out, B, H, Sq, Sk, skp, o_strides, softmax_scale, ws,
                                           apexmi_attn_prepared_workspace_bytes(B, H, Sq, Sk), stream);
    }
    if (use_materialised(Sq, Sk, D, dtype, q_strides, k_strides, v_strides, o_strides, causal_block) && workspace &&
        workspace_bytes >= materialised_bytes(Sq, Sk, D)) {
        const int skp = ((Sk + KV - 1) / KV) * KV, sk8 = (Sk + 7) / 8 * 8;
        float* sc = (float*)workspace;
        bf16_t* pb = (bf16_t*)((char*)workspace + (size_t)Sq * sk8 * 4);
        bf16_t* vt = pb + (size_t)Sq * skp;
        bf16_t* kpad = vt + (size_t)D * skp;
        const float c = softmax_scale * LOG2E;
        for (int b = 0; b < B; ++b)
            for (int h = 0; h < H; ++h) {
                const bf16_t* qp = (const bf16_t*)q + b * q_strides[0] + h * q_strides[1];
                const bf16_t* kp = (const bf16_t*)k + b * k_strides[0] + h * k_strides[1];
                const bf16_t* vp = (const bf16_t*)v + b * v_strides[0] + h * v_strides[1];
                bf16_t* op = (bf16_t*)out + b * o_strides[0] + h * o_strides[2];
                int64_t ldk = k_strides[2];
                if (sk8 != Sk) {   // the GEMM's weight operand needs whole groups of 8 rows: zero-padded copy of K
                    if (hipMemcpy2DAsync(kpad, (size_t)D * 2, kp, (size_t)ldk * 2, (size_t)D * 2, Sk, hipMemcpyDeviceToDevice,
                                         stream) != hipSuccess ||
                        hipMemsetAsync(kpad + (size_t)Sk * D, 0, (size_t)(sk8 - Sk) * D * 2, stream) != hipSuccess) {
                        apexmi_set_error("attn_fwd: padding K failed");
                        return 1;
                    }
                    kp = kpad;
                    ldk = D;
                }
                if (int rc = apexmi_gemm_bf16(qp, q_strides[2], kp, ldk, nullptr, sc, sk8, Sq, sk8, D,
                                              APEXMI_EPI_BIAS_F32, nullptr, nullptr, 0, stream_))
                    return rc;
                {
                    ApexmiProfScope prof(1, stream, 0.0, (double)Sq * Sk * 6.0);
                    hipLaunchKernelGGL(softmax_rows_kernel, dim3(Sq), dim3(256), 0, stream, sc, (int64_t)sk8, Sk, c, pb,
                                       (int64_t)skp, skp, causal_block);
                    if (int rc = apexmi_check_launch("softmax_rows")) return rc;
                }
                // V^T [D, skp]: the 128-wide transpose kernel over D / 128 column slices
                if (int rc = apexmi_v_transpose(vp, 128, v_strides[2], Sk, D / 128, 128, vt, skp, 0, stream_)) return rc;
                if (int rc = apexmi_gemm_bf16(pb, skp, vt, skp, nullptr, op, o_strides[1], Sq, D, skp, APEXMI_EPI_BIAS,
                                              nullptr, nullptr, 0, stream_))
                    return rc;
            }
        return 0;
    }
    APEXMI_REQUIRE(causal_block == 0, "attn_fwd_framecausal: operand strides must be multiples of 8 elements");
    APEXMI_REQUIRE(D <= GEN_THREADS, "attn_fwd: head dim %d > %d unsupported", D, GEN_THREADS);
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * Sk * D, 0.0);
    switch (dtype) {
        case APEXMI_BF16:
            return launch_generic<uint16_t>(q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides,
                                            v_strides, o_strides, softmax_scale, stream);
        case APEXMI_F16:
            return launch_generic<_Float16>(q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides,
                                            v_strides, o_strides, softmax_scale, stream);
        case APEXMI_F32:
            return launch_generic<float>(q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides,
                                         v_strides, o_strides, softmax_scale, stream);
        default:
            apexmi_set_error("attn_fwd: unknown dtype %d", dtype);
            return 1;
    }
}

extern "C" int apexmi_attn_fwd(const void* q, const void* k, const void* v, void* out, int B, int H,
                               int Sq, int Sk, int D, const int64_t q_strides[3],
                               const int64_t k_strides[3], const int64_t v_strides[3],
                               const int64_t o_strides[3], float softmax_scale, int dtype,
                               void* workspace, size_t workspace_bytes, apexmi_stream_t stream_) {
    return attn_fwd_impl(q, k, v, out, B, H, Sq, Sk, D, q_strides, k_strides, v_strides, o_strides, softmax_scale, dtype,
                         workspace, workspace_bytes, 0, stream_);
}

// f32-storage verification mode of apexmi_attn_fwd_prepared: q, k, vt, out are float in the prepared layouts.  Runs the
// one-workgroup-per-query-row kernel in f32 arithmetic (no bf16 rounding of the probabilities); V is read through V^T.
extern "C" int apexmi_attn_fwd_prepared_f32(const void* q, const void* k, const void* vt, void* out, int B, int H, int Sq,
                                            int Sk, int Skp, const int64_t o_strides[3], float softmax_scale,
                                            apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && vt && out, "attn_fwd_prepared_f32: null operand");
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk > 0 && Skp >= Sk, "attn_fwd_prepared_f32: bad problem");
    const int64_t qs[3] = {(int64_t)H * Sq * HD, (int64_t)Sq * HD, HD};
    const int64_t ks[3] = {(int64_t)H * Sk * HD, (int64_t)Sk * HD, HD};
    const int64_t vs[3] = {(int64_t)H * HD * Skp, (int64_t)HD * Skp, 1};
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * Sk * HD, 0.0);
    return launch_generic<float>(q, k, vt, out, B, H, Sq, Sk, HD, qs, ks, vs, o_strides, softmax_scale, stream, (int64_t)Skp);
}

extern "C" size_t apexmi_attn_framecausal_workspace_bytes(int S, int D) { return materialised_bytes(S, S, D); }

extern "C" int apexmi_attn_fwd_framecausal(const void* q, const void* k, const void* v, void* out, int B, int H,
                                           int S, int D, int block, const int64_t q_strides[3],
                                           const int64_t k_strides[3], const int64_t v_strides[3],
                                           const int64_t o_strides[3], float softmax_scale, void* workspace,
                                           size_t workspace_bytes, apexmi_stream_t stream_) {
    APEXMI_REQUIRE(block > 0 && S % block == 0, "attn_fwd_framecausal: S=%d is not a whole number of frames of %d tokens", S, block);
    APEXMI_REQUIRE(D % 128 == 0 && D <= 1024, "attn_fwd_framecausal: D=%d must be a multiple of 128 (<= 1024)", D);
    APEXMI_REQUIRE(workspace && workspace_bytes >= materialised_bytes(S, S, D), "attn_fwd_framecausal: workspace too small");
    return attn_fwd_impl(q, k, v, out, B, H, S, S, D, q_strides, k_strides, v_strides, o_strides, softmax_scale,
                         APEXMI_BF16, workspace, workspace_bytes, block, stream_);
}

// ---- attention with an additive bias / key mask / causal mask over packed projections (text encoders) ----------
namespace {
size_t attn_bias_bytes(int H, int Sq, int Sk, int D) {
    const size_t skp = (size_t)((Sk + KV - 1) / KV) * KV, sk8 = (size_t)((Sk + 7) / 8) * 8;
    return (size_t)H * Sq * sk8 * 4 + (size_t)H * Sq * skp * 2 + (size_t)H * D * skp * 2 +
           (sk8 != (size_t)Sk ? sk8 * (size_t)H * D * 2 : 0);
}
}  // namespace

extern "C" int apexmi_gemm_bf16_batched(const void* A, int64_t lda, int64_t stride_a, const void* W, int64_t ldw,
                                        int64_t stride_w, void* C, int64_t ldc, int64_t stride_c, int batch, int M,
                                        int N, int K, int epilogue, apexmi_stream_t stream);

extern "C" size_t apexmi_attn_bias_workspace_bytes(int H, int Sq, int Sk, int D) { return attn_bias_bytes(H, Sq, Sk, D); }

extern "C" int apexmi_attn_fwd_bias_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                                        int64_t ldo, int H, int Hkv, int Sq, int Sk, int D, float scale, const float* bias,
                                        const uint8_t* keep, const int* seg, int causal, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && v && out, "attn_fwd_bias_f32: null operand");
    APEXMI_REQUIRE(H > 0 && Hkv > 0 && H % Hkv == 0 && Sq > 0 && Sk > 0 && D > 0, "attn_fwd_bias_f32: bad shape");
    const size_t lds = (size_t)(Sk + D) * sizeof(float);
    APEXMI_REQUIRE(lds <= 64 * 1024, "attn_fwd_bias_f32: Sk=%d exceeds the verification kernel's LDS row (16 K keys)", Sk);
    hipLaunchKernelGGL(attn_bias_rows_f32_kernel, dim3(Sq, H), dim3(256), lds, stream, q, ldq, k, ldk, v, ldv, out, ldo, H, Hkv, Sq, Sk,
                       D, scale, bias, keep, seg, causal);
    return apexmi_check_launch("attn_fwd_bias_f32");
}

extern "C" int apexmi_attn_fwd_bias(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                                    void* out, int64_t ldo, int H, int Hkv, int Sq, int Sk, int D, float softmax_scale,
                                    const float* bias, const uint8_t* keep, const int* seg, int causal, void* workspace,
                                    size_t workspace_bytes, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k && v && out && workspace, "attn_fwd_bias: null operand");
    APEXMI_REQUIRE(H > 0 && Sq > 0 && Sk > 0, "attn_fwd_bias: empty problem");
    APEXMI_REQUIRE(Hkv > 0 && H % Hkv == 0, "attn_fwd_bias: %d query heads are not a multiple of %d key/value heads", H, Hkv);
    APEXMI_REQUIRE(D % 64 == 0 && (Hkv * D) % 128 == 0, "attn_fwd_bias: head dim %d must be a multiple of 64 and Hkv*D=%d of 128", D, Hkv * D);
    APEXMI_REQUIRE((!causal && !seg) || Sq == Sk, "attn_fwd_bias: the causal / segment masks need Sq == Sk");
    APEXMI_REQUIRE(workspace_bytes >= attn_bias_bytes(H, Sq, Sk, D), "attn_fwd_bias: workspace too small (%zu < %zu)",
                   workspace_bytes, attn_bias_bytes(H, Sq, Sk, D));
    const int skp = ((Sk + KV - 1) / KV) * KV, sk8 = (Sk + 7) / 8 * 8, rep = H / Hkv;
    float* sc = (float*)workspace;
    bf16_t* pb = (bf16_t*)((char*)workspace + (size_t)H * Sq * sk8 * 4);
    bf16_t* vt = pb + (size_t)H * Sq * skp;
    bf16_t* kpad = vt + (size_t)H * D * skp;
    const bf16_t* kp = (const bf16_t*)k;
    if (sk8 != Sk) {   // the GEMM's weight operand comes in whole groups of 8 rows
        if (hipMemcpy2DAsync(kpad, (size_t)Hkv * D * 2, k, (size_t)ldk * 2, (size_t)Hkv * D * 2, Sk,
                             hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipMemsetAsync(kpad + (size_t)Sk * Hkv * D, 0, (size_t)(sk8 - Sk) * Hkv * D * 2, stream) != hipSuccess) {
            apexmi_set_error("attn_fwd_bias: padding K failed");
            return 1;
        }
        kp = kpad;
        ldk = (int64_t)Hkv * D;
    }
    // scores[h] = q_h k_{h / rep}^T.  One batched launch over the heads that share a key head (stride 0 on K: grouped-
    // query attention without materialising the repeated keys); plain multi-head attention is a single launch.
    const int launches = rep == 1 ? 1 : Hkv, per = rep == 1 ? H : rep;
    for (int g = 0; g < launches; ++g)
        if (int rc = apexmi_gemm_bf16_batched((const bf16_t*)q + (int64_t)g * per * D, ldq, D, kp + (int64_t)g * D, ldk,
                                              rep == 1 ? D : 0, sc + (size_t)g * per * Sq * sk8, sk8, (int64_t)Sq * sk8, per,
                                              Sq, sk8, D, APEXMI_EPI_BIAS_F32, stream_))
            return rc;
    {
        ApexmiProfScope prof(1, stream, 0.0, (double)H * Sq * Sk * 10.0);
        hipLaunchKernelGGL(softmax_bias_rows_kernel, dim3(Sq, H), dim3(256), 0, stream, sc, (int64_t)sk8, Sq, Sk,
                           softmax_scale * LOG2E, bias, (int64_t)Sk, keep, seg, causal, pb, (int64_t)skp, skp);
        if (int rc = apexmi_check_launch("softmax_bias_rows")) return rc;
    }
    // V^T [Hkv*D, skp] by 128-column slices of V (independent of the head size), zero-padded key columns
    if (int rc = apexmi_v_transpose(v, 128, ldv, Sk, Hkv * D / 128, 128, vt, skp, 0, stream_)) return rc;
    for (int g = 0; g < launches; ++g)
        if (int rc = apexmi_gemm_bf16_batched(pb + (size_t)g * per * Sq * skp, skp, (int64_t)Sq * skp,
                                              vt + (size_t)g * D * skp, skp, rep == 1 ? (int64_t)D * skp : 0,
                                              (bf16_t*)out + (int64_t)g * per * D, ldo, D, per, Sq, D, skp, APEXMI_EPI_BIAS,
                                              stream_))
            return rc;
    return 0;
}
