// Two-context cross-attention forward: the image branch of Wan-2.1 I2V / FLF2V cross-attention (diffusers WanAttnProcessor with
// add_k_proj, which the reference's Wan base model mirrors: R/src/transformer/wan/base/model.py:207, 391-394).  The query attends
// the text keys and the image keys in two SEPARATE softmaxes; each branch result is a bf16 tensor and the two are added in bf16:
//   out = bf16( bf16(softmax(q k_t^T s) v_t) + bf16(softmax(q k_i^T s) v_i) )
//
// One-pass flash kernel on the shared tile step (attn_tile.h: layout, rounding), 4 waves, packed bf16 operands, D = 128, workgroups
// of one (batch, head) kept on one XCD.  The workgroup reads its query block ONCE and walks one list of tiles: the text tiles, then
// the image tiles (the staging of the first image tile overlaps the last text tile).  Each key set has its own online softmax with
// a RUNNING maximum (image keys are not near-uniform, so the w64 kernel's first-tile maximum does not apply).  At the seam the text
// branch is normalised and rounded to bf16 (kept packed, 32 VGPRs); at the end the image branch is normalised, rounded to bf16,
// the two are summed in f32 and stored as bf16 once.  The last tile of each set excludes the keys past its end (-inf after
// scaling); an empty image set (Sk_i = 0) stores the text branch alone.
#include "attn_tile.h"

#include <cstdint>

namespace {

constexpr int DNW = 4;             // waves per workgroup
constexpr int DQB = DNW * 32;      // query rows per workgroup
constexpr int DD = 128;            // head dim

struct DualArgs {
    const uint16_t* q;
    const uint16_t* k[2];
    const uint16_t* vt[2];
    uint16_t* o;
    int64_t o_sb, o_ss, o_sh;
    int H, Sq, nqb, total, neg;
    int Sk[2], Skp[2];
    float c;                // |scale| * log2(e)
};

__global__ __launch_bounds__(DNW * 64, 2) void attn_dual_kernel(const DualArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using E = ElemBf16;
    constexpr int K_TILE = KV * DD * 2, V_TILE = DD * KV * 2, STAGE = K_TILE + V_TILE;
    constexpr int LD = PIECES<DD, DNW>, NDT = DD / 32;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hi = lane >> 5;

    const int s = xcd_remap(blockIdx.x, a.total);
    const int hb = s / a.nqb, qb = s % a.nqb;
    const int b = hb / a.H, h = hb % a.H;

    const uint16_t* Qp = a.q + (int64_t)hb * a.Sq * DD;
    const uint16_t* Kp0 = a.k[0] + (int64_t)hb * a.Sk[0] * DD;
    const uint16_t* Kp1 = a.k[1] + (int64_t)hb * a.Sk[1] * DD;
    const uint16_t* Vp0 = a.vt[0] + (int64_t)hb * DD * a.Skp[0];
    const uint16_t* Vp1 = a.vt[1] + (int64_t)hb * DD * a.Skp[1];
    const int n0 = (a.Sk[0] + KV - 1) / KV;
    const int n = n0 + (a.Sk[1] + KV - 1) / KV;

    const int qrow = qb * DQB + wave * 32 + l31;
    const int qrow_c = min(qrow, a.Sq - 1);

    // Q fragments (B operand of S^T): lane supplies Q[qrow][16 ks + 8 hi .. +7]; a negative scale flips their signs (exact)
    // (kept in the kernel: behind a helper that fills qf the allocation moves, 255 -> 230 VGPRs; see attention_masked.hip)
    bf16x8 qf[DD / 16];
#pragma unroll
    for (int ks = 0; ks < DD / 16; ++ks) {
        u32x4 raw = *(const u32x4*)(Qp + (int64_t)qrow_c * DD + ks * 16 + hi * 8);
        if (a.neg) raw ^= u32x4{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u};
        qf[ks] = __builtin_bit_cast(bf16x8, raw);
    }

    int k_key[LD], k_c[LD], v_row[LD], v_c[LD];
    stage_sources<DD, DNW>(wave, lane, k_key, k_c, v_row, v_c);
    // tile `it` of the combined list: text tiles [0, n0), image tiles [n0, n)
    auto stage = [&](int buf, int it) {
        char* base = smem + buf * STAGE + wave * 1024;
        const bool img = it >= n0;
        const uint16_t* Kp = img ? Kp1 : Kp0;
        const uint16_t* Vp = img ? Vp1 : Vp0;
        const int sk = img ? a.Sk[1] : a.Sk[0], skp = img ? a.Skp[1] : a.Skp[0];
        const int kv0 = (img ? it - n0 : it) * KV;
#pragma unroll
        for (int i = 0; i < LD; ++i) {
            const int key = min(kv0 + k_key[i], sk - 1);
            glds16(Kp + (int64_t)key * DD + k_c[i], base + i * (DNW * 1024));
        }
#pragma unroll
        for (int i = 0; i < LD; ++i)
            glds16(Vp + (int64_t)v_row[i] * skp + kv0 + v_c[i], base + K_TILE + i * (DNW * 1024));
    };

    int k_off[2], k_sw[2], v_off[NDT], v_sw[NDT];
    fragment_offsets<DD>(l31, k_off, k_sw, v_off, v_sw);

    f32x16 oacc[NDT];
    clear(oacc);
    float m_run = SENTINEL;     // running maximum, base-2 domain, an integer
    float l_run = 0.0f;
    uint32_t txt[NDT][8];       // the text branch, normalised and rounded to bf16 (lane's d = 32 dt + 8 g + 4 hi + 0..3)

    auto finish = [&](uint32_t (&r)[NDT][8]) {
        const float inv = 1.0f / sum_xor32(l_run);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[dt][j] = pack_bf16(oacc[dt][2 * j] * inv, oacc[dt][2 * j + 1] * inv);
    };

    stage(0, 0);
    for (int it = 0; it < n; ++it) {
        const bool img = it >= n0;
        if (it == n0) {   // seam (workgroup-uniform): keep the text branch, start the image softmax
            finish(txt);
            clear(oacc);
            m_run = SENTINEL;
            l_run = 0.0f;
        }
        const int sk = img ? a.Sk[1] : a.Sk[0];
        const int kv0 = (img ? it - n0 : it) * KV;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the tile's LDS-DMA has landed (see attention.hip)
        __syncthreads();
        if (it + 1 < n) stage((it + 1) & 1, it + 1);
        const char* Ks = smem + (it & 1) * STAGE;

        f32x16 sacc[2];
        scores<E, DD>(Ks, k_off, k_sw, hi, qf, sacc);

        // the last tile of a set excludes the keys past its end (workgroup-uniform)
        const bool tail = kv0 + KV > sk;
        float mx;
        if (tail) {
            mx = -__builtin_inff();
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    sacc[kt][r] = kv0 + tile_key(kt, r, hi) < sk ? sacc[kt][r] * a.c : -__builtin_inff();
                    mx = fmaxf(mx, sacc[kt][r]);
                }
        } else {
            mx = tile_max(sacc) * a.c;
        }
        raise_max(max_xor32(mx), m_run, l_run, oacc);
        if (tail) l_run += exp2_scaled(sacc, m_run);
        else l_run += exp2_fused(sacc, a.c, m_run);

        E::v8 pf[4];
        p_fragments<E>(sacc, pf);
        accumulate<E, DD>(Ks + K_TILE, v_off, v_sw, hi, pf, oacc);
    }

    // ---- epilogue: bf16(text) + bf16(image) in f32, one bf16 store; the text branch alone when the image set is empty ----
    uint32_t res[NDT][8];
    if (n > n0) {
        uint32_t im[NDT][8];
        finish(im);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                res[dt][j] = pack_bf16(bf16_lo(txt[dt][j]) + bf16_lo(im[dt][j]), bf16_hi(txt[dt][j]) + bf16_hi(im[dt][j]));
    } else {
        finish(res);
    }
    if (qrow < a.Sq) {
        uint16_t* op = a.o + (int64_t)b * a.o_sb + (int64_t)qrow * a.o_ss + (int64_t)h * a.o_sh;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) *(u32x2*)(op + dt * 32 + g * 8 + hi * 4) = u32x2{res[dt][2 * g], res[dt][2 * g + 1]};
    }
}

}  // namespace

extern "C" int apexmi_attn_fwd_prepared_dual(const void* q, const void* k_t, const void* vt_t, int Sk_t, int Skp_t,
                                             const void* k_i, const void* vt_i, int Sk_i, int Skp_i, void* out, int B, int H,
                                             int Sq, const int64_t o_strides[3], float softmax_scale, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(q && k_t && vt_t && out && o_strides, "attn_fwd_prepared_dual: null operand");
    APEXMI_REQUIRE(Sk_i == 0 || (k_i && vt_i), "attn_fwd_prepared_dual: null image operand with Sk_i=%d", Sk_i);
    APEXMI_REQUIRE(B > 0 && H > 0 && Sq > 0 && Sk_t > 0 && Sk_i >= 0,
                   "attn_fwd_prepared_dual: empty problem (B=%d H=%d Sq=%d Sk_t=%d Sk_i=%d)", B, H, Sq, Sk_t, Sk_i);
    APEXMI_REQUIRE(Skp_t >= (Sk_t + KV - 1) / KV * KV && Skp_t % 8 == 0 &&
                       (Sk_i == 0 || (Skp_i >= (Sk_i + KV - 1) / KV * KV && Skp_i % 8 == 0)),
                   "attn_fwd_prepared_dual: V^T widths Skp_t=%d / Skp_i=%d must cover Sk rounded up to %d", Skp_t, Skp_i, KV);
    APEXMI_REQUIRE((int64_t)B * H * ((Sq + DQB - 1) / DQB) < (1ll << 31), "attn_fwd_prepared_dual: too many query blocks");
    bool aligned = ((uintptr_t)q % 16) == 0 && ((uintptr_t)k_t % 16) == 0 && ((uintptr_t)vt_t % 16) == 0 &&
                   ((uintptr_t)k_i % 16) == 0 && ((uintptr_t)vt_i % 16) == 0 && ((uintptr_t)out % 8) == 0;
    for (int i = 0; i < 3; ++i) aligned = aligned && o_strides[i] % 4 == 0;
    APEXMI_REQUIRE(aligned, "attn_fwd_prepared_dual: operands must be 16-byte aligned (out 8-byte, strides multiples of 4)");

    DualArgs a{};
    a.q = (const uint16_t*)q;
    a.k[0] = (const uint16_t*)k_t, a.vt[0] = (const uint16_t*)vt_t, a.Sk[0] = Sk_t, a.Skp[0] = Skp_t;
    a.k[1] = Sk_i ? (const uint16_t*)k_i : a.k[0], a.vt[1] = Sk_i ? (const uint16_t*)vt_i : a.vt[0];
    a.Sk[1] = Sk_i, a.Skp[1] = Sk_i ? Skp_i : Skp_t;
    a.o = (uint16_t*)out;
    a.o_sb = o_strides[0], a.o_ss = o_strides[1], a.o_sh = o_strides[2];
    a.H = H, a.Sq = Sq, a.nqb = (Sq + DQB - 1) / DQB, a.total = B * H * a.nqb;
    a.neg = softmax_scale < 0.0f;
    a.c = fabsf(softmax_scale) * LOG2E;

    constexpr int LDS = 2 * (KV * DD * 2 + DD * KV * 2);
    static uint64_t attr_done = 0;
    APEXMI_SET_ATTR_ONCE(attr_done, (void)hipFuncSetAttribute((const void*)attn_dual_kernel,
                                                              hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    ApexmiProfScope prof(1, stream, 4.0 * B * H * (double)Sq * ((double)Sk_t + Sk_i) * DD, 0.0);
    hipLaunchKernelGGL(attn_dual_kernel, dim3(a.total), dim3(DNW * 64), LDS, stream, a);
    return apexmi_check_launch("attn_fwd_prepared_dual");
}
