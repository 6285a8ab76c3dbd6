// Opt-in FP8 GEMM for resident fp8-scaled weights: a per-row e4m3 quantiser for the activations and a GEMM on
// the block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3 at twice the bf16 rate per clock) with UNIT block scales; the
// per-row activation scales and the per-row / single weight scales are applied in the f32 epilogue.  The run-time LoRA form
// (apexmi_gemm_fp8_lora) applies them to the accumulators instead and adds the adapter term t . B'^T by a bf16 MFMA tail; the grouped
// LoRA form (apexmi_gemm_fp8_grouped_lora, apexmi_gemm_fp8_grouped_qkv_lora) does so per problem of a grouped launch.
#include "common.h"
#include "fp8_quant.h"   // FP8_MAX, quant1, quant4, the MX block quantiser
#include "fp8_gemm_tile.h"   // the tile constants, Fp8Problem, fp8_epilogue (shared with gemm_mxfp4.hip)
#include <type_traits>

namespace {

// ---- apexmi_quant_rows_fp8 ----------------------------------------------------------------------------------------------------
// One wave per ROW PAIR (rows 2p, 2p + 1): the loads of both rows are in flight together.  Pass 1 reads the pair for its two
// absmax values (wave reduction), pass 2 reads it again — 2 x K x 2 bytes, served by the cache the first pass filled, so HBM is
// streamed once — and stores 16 codes (16 bytes) per lane and step.  K % 128 == 0: a step covers 64 lanes x 16 = 1024 elements,
// the last one may be partial in whole 16-element groups.
//   scale = absmax == 0 ? 1 : absmax / 448         (IEEE f32 division)
//   code  = e4m3fn_rne(min(max(x / scale, -448), 448))   (IEEE f32 division, round to nearest even, subnormals kept)
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const bf16_t* __restrict__ a, int64_t lda, int M, int K,
                                                             uint8_t* __restrict__ q, int64_t ldq, float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r0 = 2 * pair;
    if (r0 >= M) return;                                   // wave-uniform
    const int r1 = min(r0 + 1, M - 1);                     // odd M: the last pair reads its row twice and stores it once
    const bf16_t* p0 = a + (int64_t)r0 * lda;
    const bf16_t* p1 = a + (int64_t)r1 * lda;
    float m0 = 0.f, m1 = 0.f;
    for (int k = lane * 16; k < K; k += 1024) {
        const u32x4 x0 = *(const u32x4*)(p0 + k), x1 = *(const u32x4*)(p0 + k + 8);
        const u32x4 y0 = *(const u32x4*)(p1 + k), y1 = *(const u32x4*)(p1 + k + 8);
        m0 = fmaxf(m0, absmax16(x0, x1));
        m1 = fmaxf(m1, absmax16(y0, y1));
    }
    m0 = wave_max(m0);
    m1 = wave_max(m1);
    const float s0 = m0 == 0.f ? 1.0f : __fdiv_rn(m0, FP8_MAX);
    const float s1 = m1 == 0.f ? 1.0f : __fdiv_rn(m1, FP8_MAX);
    if (lane == 0) {
        scales[r0] = s0;
        if (r1 != r0) scales[r1] = s1;
    }
    uint8_t* q0 = q + (int64_t)r0 * ldq;
    uint8_t* q1 = q + (int64_t)r1 * ldq;
    for (int k = lane * 16; k < K; k += 1024) {
        const u32x4 x0 = *(const u32x4*)(p0 + k), x1 = *(const u32x4*)(p0 + k + 8);
        const u32x4 y0 = *(const u32x4*)(p1 + k), y1 = *(const u32x4*)(p1 + k + 8);
        *(u32x4*)(q0 + k) = u32x4{quant4(x0[0], x0[1], s0), quant4(x0[2], x0[3], s0), quant4(x1[0], x1[1], s0), quant4(x1[2], x1[3], s0)};
        if (r1 != r0)
            *(u32x4*)(q1 + k) = u32x4{quant4(y0[0], y0[1], s1), quant4(y0[2], y0[3], s1), quant4(y1[0], y1[1], s1), quant4(y1[2], y1[3], s1)};
    }
}

#include "quant_blocks_mxfp8.inc"   // apexmi_quant_blocks_mxfp8's streaming kernel

// ---- apexmi_gemm_fp8 ----------------------------------------------------------------------------------------------------------
// 128 x 128 output tile, K-tile of 128 codes, 256 threads = 2 x 2 waves of 64 x 64 (2 x 2 MFMA tiles of 32 x 32, 64 accumulator
// registers).  Both operands are K-contiguous bytes and staged by global_load_lds (16 bytes per lane) into ONE __shared__ array:
//   lds[buf][operand][row 0..127][128 bytes], 16 KB per operand and buffer, 64 KB in all (two workgroups per CU).
// A wave instruction writes 8 whole rows (64 lanes x 16 bytes = lane-linear); the XOR swizzle is on the SOURCE address:
//   16-byte piece c of row r holds the row's bytes 16 (c ^ ((r >> 1) & 7)) ..,
// so the 16 lanes of one ds_read_b128 phase (16 consecutive rows, one k position) cover all 64 banks once.
// One barrier per K-tile: tile t + 1 is requested into the other buffer before tile t is read; the barrier's vmcnt(0) retires it.
//
// Operand lane map of v_mfma_scale_f32_32x32x64_f8f6f4 with 8-bit formats, as verified by the exact integer tests
// (tests/test_gpu_gemm_fp8.py): lane l holds, in its 8 registers, the 32 codes k = 32 (l >> 5) + 0..31 of row (A) / column (B)
// l & 31, byte j of the 32 = k offset j.  The result layout is the 32 x 32 one of every gfx950 MFMA: column l & 31, rows
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  As in the bf16 kernels the WEIGHT tile is the A operand, so a lane holds 4 consecutive
// output columns of one output row per register group and stores them as 8 bytes.
// a single launch (apexmi_gemm_fp8)
struct Fp8Gemm : Fp8Problem {
    unsigned long long* clk;
};

// The MX forms of the single and the grouped launch: the same operands, chosen by type so that the kernel's unit-scale K-loop and
// epilogue compile from the code they always did.  Per problem: `abs` = the activation carries one e8m0 scale per 32 k (passed to
// the MFMA as the B-side block scale; the epilogue then uses sa = 1), `Q` = the output leaves as MX codes + block scales.
struct Fp8MxGemm : Fp8Gemm {};

// the run-time LoRA form (apexmi_gemm_fp8_lora): the adapter operands of the bf16 tail
struct Fp8LoraGemm : Fp8Gemm {
    const bf16_t* T;      // t = a A^T [M, Rp]
    const bf16_t* LB;     // B' [N, Rp]
    int64_t ldt, ldb;
    int Rp;               // padded rank, a multiple of 64
};

// The grouped form (apexmi_gemm_fp8_grouped, apexmi_gemm_fp8_grouped_qkv): a table of Fp8GroupProblem (fp8_gemm_tile.h)
struct Fp8Group {
    Fp8GroupProblem p[FP8_MAX_GROUPS];
    int count, total;
    Fp8QkvShared qs;
    unsigned long long* clk;
};
struct Fp8MxGroup : Fp8Group {};

// The grouped run-time LoRA form (apexmi_gemm_fp8_grouped_lora, apexmi_gemm_fp8_grouped_qkv_lora): one adapter entry per problem,
// by value like the table.  Rp == 0 = the problem has no adapter and is computed as the Fp8Group kernel computes it; Rp > 0 = the
// arithmetic of Fp8LoraGemm.  Both are block-uniform branches.
struct Fp8LoraEntry {
    const bf16_t* T;      // t = a A^T [M, Rp]
    const bf16_t* LB;     // B' [N, Rp]
    int64_t ldt, ldb;
    int Rp;               // padded rank, a multiple of 64, or 0
};
struct Fp8LoraGroup : Fp8Group {
    Fp8LoraEntry lora[FP8_MAX_GROUPS];
};

// The fragment of a BLOCK-SCALED k-step (the MX instantiations, problems with `abs`).  The instruction's two scale blocks are not
// the two lane halves: block 0 = registers 0..3 of BOTH halves, scaled by byte 0 (op-sel 0) of lane l & 31's scale register, block
// 1 = registers 4..7 of both halves, scaled by lane 32 + (l & 31)'s (measured with one-hot operands and a lane / byte code in the
// scale register; tests/test_gpu_gemm_fp8_mx.py pins it).  A dot product does not care where a k sits as long as both operands
// agree, so for these problems BOTH operands put the step's memory block b (32 codes) into scale block b: lane half h holds codes
// 16 h + 0..15 of block 0 in registers 0..3 and codes 16 h + 0..15 of block 1 in registers 4..7 = 16-byte pieces h and 2 + h.
APEXMI_DEVICE i32x8 lds_frag_blocks(const uint8_t* tile, int row, int piece0, int piece1) {
    const u32x4 lo = lds_piece(tile, row, piece0), hi = lds_piece(tile, row, piece1);
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// the fragment of a unit-scale k-step: the lane's 32 consecutive codes = pieces `piece` and `piece` + 1
APEXMI_DEVICE i32x8 lds_frag(const uint8_t* tile, int row, int piece) { return lds_frag_blocks(tile, row, piece, piece + 1); }

// a 16-byte piece of a staged tile as the operand of one v_mfma_f32_32x32x16_bf16 k-step: lane l holds the 8 bf16 k = 8 (l >> 5) + 0..7
// of row (A) / column (B) l & 31 (gemm.hip's fragment reads), so k-step ks of a 64-wide rank tile is piece 2 ks + (l >> 5)
APEXMI_DEVICE bf16x8 lds_frag16(const uint8_t* tile, int row, int piece) {
    return __builtin_bit_cast(bf16x8, lds_piece(tile, row, piece));
}

// this workgroup's tile id `t` inside its problem, and the problem (index `pi`): the launch itself, or the table entry found by the
// prefix sums
APEXMI_DEVICE const Fp8Gemm& fp8_problem(const Fp8Gemm& G, int& t, int& pi) {
    t = xcd_remap(blockIdx.x, G.tiles_m * G.tiles_n);
    pi = 0;
    return G;
}
APEXMI_DEVICE Fp8GroupProblem fp8_problem(const Fp8Group& G, int& t, int& pi) {
    return fp8_group_entry(G.p, G.count, G.total, t, pi);
}

// the adapter operands of this workgroup's problem: the launch's own (Fp8LoraGemm) or entry `pi` of the table (Fp8LoraGroup)
APEXMI_DEVICE const Fp8LoraGemm& fp8_lora_entry(const Fp8LoraGemm& G, int) { return G; }
APEXMI_DEVICE Fp8LoraEntry fp8_lora_entry(const Fp8LoraGroup& G, int pi) { return G.lora[pi]; }
APEXMI_DEVICE Fp8LoraEntry fp8_lora_entry(const Fp8Problem&, int) { return Fp8LoraEntry{}; }
APEXMI_DEVICE Fp8LoraEntry fp8_lora_entry(const Fp8Group&, int) { return Fp8LoraEntry{}; }

// LORA (G is an Fp8LoraGemm): after the fp8 K-loop the accumulators are scaled IN PLACE, acc = (acc * sa[m]) * sw[n], and a bf16 MFMA
// tail adds sum_r t[m, r] B'[n, r] into the same registers, rank ascending: both MFMA shapes write the same 32 x 32 layout.  A rank
// tile of 64 bf16 is 128 bytes per row — the geometry of a K-tile of codes — so t takes the activation half and B' the weight half
// of a buffer, staged and swizzled as they are; the first rank tile is requested during the last K-tile.
// The grouped LoRA form (G is an Fp8LoraGroup) does the same for the problems whose table entry has Rp > 0 and leaves the others to
// the SCALED epilogue, so those keep the bits of the plain grouped launch.
// ONE kernel for all forms, chosen by the argument type (Fp8Gemm, Fp8LoraGemm, Fp8Group, Fp8LoraGroup and the MX pair): build.py's
// no-spill check matches "gemm_fp8_kernel" and so covers every instantiation.
// EPI: APEXMI_EPI_BIAS, APEXMI_EPI_BIAS_GELU or APEXMI_EPI_BIAS_GATE_RES; the grouped form reads it from its problem instead
template <int EPI, class Args>
__global__ __launch_bounds__(256, 2) void gemm_fp8_kernel(const Args G) {
    constexpr bool LORA = std::is_same_v<Args, Fp8LoraGemm> || std::is_same_v<Args, Fp8LoraGroup>, GROUPED = std::is_base_of_v<Fp8Group, Args>;
    constexpr bool MX = std::is_same_v<Args, Fp8MxGemm> || std::is_same_v<Args, Fp8MxGroup>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[4 * FOPB];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    int t, pi, m0, n0;
    const auto& P = fp8_problem(G, t, pi);
    [[maybe_unused]] const auto& L = fp8_lora_entry(G, pi);     // LORA: the adapter operands; Rp == 0 (grouped) = none, block-uniform
    fp8_tile_origin(t, P.tiles_m, P.tiles_n, m0, n0);

    const Fp8Stager stage_codes(P, m0, n0, wid, lane);
    auto stage = [&](int kt, int buf) { stage_codes(lds, wid, kt, buf); };
    // LORA: rank tile rt of t (rows) and B' (columns), same rows, pieces and swizzle; the addresses are computed here, at the point of
    // use, so that no pointer is held across the K-loop
    auto stage_rank = [&](int rt, int buf) {
        if constexpr (LORA) {
            if (GROUPED && L.Rp == 0) return;
            uint8_t* da = fp8_stage_dst(lds, buf, wid);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                glds16(fp8_stage_src(L.T, L.ldt, m0, P.M, wid, lane, i) + rt * FBK, da + 8 * i * FBK);
                glds16(fp8_stage_src(L.LB, L.ldb, n0, P.N, wid, lane, i) + rt * FBK, da + FOPB + 8 * i * FBK);
            }
        }
    };

    Fp8Clock clock;
    clock.start(G.clk);

    f32x16 acc[2][2];                 // [weight tile (output columns)][activation tile (output rows)]
    fp8_zero_acc(acc);

    const int nk = P.K / FBK;
    const int fr = lane & 31, fh = lane >> 5;
    // MX: the lane's activation block scales.  Its row 64 wr + 32 j + fr of the tile has one e8m0 byte per 32 k = one dword per
    // K-tile; lane half fh supplies the scale of block 2 kk + fh of k-step kk (lds_frag_blocks).  A wave's 64 rows are 64 cache
    // lines, so the dwords are fetched FOUR K-tiles at a time (one 16-byte load per row where the rows are 16-byte aligned, else
    // and for the last part-filled group dword by dword), one group ahead, by plain global loads (a global-address-space pointer: a
    // flat load would count in lgkmcnt too and hold the K-tile's first LDS wait for HBM).  A problem without block scales
    // (block-uniform) passes 2^0, keeps sa[m] in the epilogue and reads its fragments as the unit-scale kernel does, so it leaves
    // that kernel's bits.
    typedef const __attribute__((address_space(1))) uint32_t* bs_ptr_t;
    typedef const __attribute__((address_space(1))) u32x4* bs_ptr4_t;
    [[maybe_unused]] bs_ptr_t bs_src[2];
    [[maybe_unused]] u32x4 bs_cur[2], bs_nxt[2];
    [[maybe_unused]] bool bs_wide = false;
    [[maybe_unused]] auto bs_load = [&](int t0, u32x4 (&g)[2]) {      // dwords t0 .. t0 + 3 (those below nk) of the lane's two rows
        const bool full = bs_wide && t0 + 4 <= nk;                     // block-uniform
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (full) {
                g[j] = *(bs_ptr4_t)(bs_src[j] + t0);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (t0 + q < nk) g[j][q] = bs_src[j][t0 + q];
            }
        }
    };
    if constexpr (MX) {
#pragma unroll
        for (int j = 0; j < 2; ++j) bs_cur[j] = bs_nxt[j] = u32x4{(uint32_t)UNIT_E8M0, (uint32_t)UNIT_E8M0, (uint32_t)UNIT_E8M0, (uint32_t)UNIT_E8M0};
        if (P.abs != nullptr) {
            bs_wide = ((uintptr_t)P.abs % 16) == 0 && (P.ldabs % 16) == 0;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bs_src[j] = (bs_ptr_t)(uintptr_t)(P.abs + (int64_t)min(m0 + 64 * wr + 32 * j + fr, P.M - 1) * P.ldabs);
            bs_load(0, bs_cur);
        }
    }
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        else stage_rank(0, buf ^ 1);
        [[maybe_unused]] uint32_t bs[2];
        if constexpr (MX) {
            if (P.abs != nullptr && (kt & 3) == 0 && kt + 4 < nk) bs_load(kt + 4, bs_nxt);
            const int q = kt & 3;                                       // uniform
#pragma unroll
            for (int j = 0; j < 2; ++j) bs[j] = q == 0 ? bs_cur[j][0] : q == 1 ? bs_cur[j][1] : q == 2 ? bs_cur[j][2] : bs_cur[j][3];
        }
        const uint8_t* ta = lds + buf * 2 * FOPB;
        const uint8_t* tw = ta + FOPB;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int piece = 4 * kk + 2 * fh;
            i32x8 fa[2], fw[2];
            if constexpr (MX) {
                const bool blk = P.abs != nullptr;
                const int p0 = blk ? 4 * kk + fh : piece, p1 = blk ? 4 * kk + 2 + fh : piece + 1;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = lds_frag_blocks(ta, 64 * wr + 32 * i + fr, p0, p1);
                    fw[i] = lds_frag_blocks(tw, 64 * wc + 32 * i + fr, p0, p1);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    fa[i] = lds_frag(ta, 64 * wr + 32 * i + fr, piece);
                    fw[i] = lds_frag(tw, 64 * wc + 32 * i + fr, piece);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (MX)       // the B-side scale: byte 0 (op-sel 0) of the lane's register = block 2 kk + fh
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, UNIT_E8M0, 0,
                                                                                   (int)(bs[j] >> (16 * kk + 8 * fh)));
                    else
                        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, UNIT_E8M0, 0,
                                                                                   UNIT_E8M0);
                }
        }
        if constexpr (MX) {
            if ((kt & 3) == 3) {
#pragma unroll
                for (int j = 0; j < 2; ++j) bs_cur[j] = bs_nxt[j];
            }
        }
        __syncthreads();
    }

    if constexpr (LORA) if (!GROUPED || L.Rp > 0) {     // a grouped problem without an adapter skips the tail: block-uniform
        float sa[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) sa[j] = P.sa[min(m0 + 64 * wr + 32 * j + fr, P.M - 1)];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float sw[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) fp8_load_sw(P, min(n0 + 64 * wc + 32 * i + 8 * g + 4 * fh, P.N - 4), sw[g]);
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = (acc[i][j][r] * sa[j]) * sw[r >> 2][r & 3];
        }
        const int nr = L.Rp / 64;
        for (int rt = 0; rt < nr; ++rt) {
            const int buf = (nk + rt) & 1;
            if (rt + 1 < nr) stage_rank(rt + 1, buf ^ 1);
            const uint8_t* tt = lds + buf * 2 * FOPB;
            const uint8_t* tb = tt + FOPB;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                bf16x8 ft[2], fb[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ft[i] = lds_frag16(tt, 64 * wr + 32 * i + fr, 2 * ks + fh);
                    fb[i] = lds_frag16(tb, 64 * wc + 32 * i + fr, 2 * ks + fh);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[i], ft[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
    }

    clock.stop(G.clk, tid);

    if constexpr (MX) {
        // block-uniform choices: bf16 or MX out; the epilogue of a grouped problem by its table entry
        int epi = EPI;
        if constexpr (GROUPED) epi = P.epi;
        const bool mxo = P.Q != nullptr;
        if (epi == APEXMI_EPI_BIAS_GATE_RES) fp8_epilogue<APEXMI_EPI_BIAS_GATE_RES, true, true>(acc, P, m0, n0, wr, wc, fr, fh);
        else if (epi == APEXMI_EPI_BIAS_GELU && mxo) fp8_epilogue<APEXMI_EPI_BIAS_GELU, true, true, true>(acc, P, m0, n0, wr, wc, fr, fh);
        else if (epi == APEXMI_EPI_BIAS_GELU) fp8_epilogue<APEXMI_EPI_BIAS_GELU, true, true>(acc, P, m0, n0, wr, wc, fr, fh);
        else if (mxo) fp8_epilogue<APEXMI_EPI_BIAS, true, true, true>(acc, P, m0, n0, wr, wc, fr, fh);
        else fp8_epilogue<APEXMI_EPI_BIAS, true, true>(acc, P, m0, n0, wr, wc, fr, fh);
    } else if constexpr (GROUPED) {
        auto group_epilogue = [&](auto scaled) {
            constexpr bool S = decltype(scaled)::value;
            if (P.qkv) fp8_qkv_epilogue<S>(acc, P, G.qs, m0, n0, tid, lds);
            else if (P.epi == APEXMI_EPI_BIAS) fp8_epilogue<APEXMI_EPI_BIAS, S>(acc, P, m0, n0, wr, wc, fr, fh);
            else if (P.epi == APEXMI_EPI_BIAS_GELU) fp8_epilogue<APEXMI_EPI_BIAS_GELU, S>(acc, P, m0, n0, wr, wc, fr, fh);
            else fp8_epilogue<APEXMI_EPI_BIAS_GATE_RES, S>(acc, P, m0, n0, wr, wc, fr, fh);
        };
        if constexpr (LORA) {
            if (L.Rp > 0) group_epilogue(std::false_type{});      // the scales and the adapter term are in acc
            else group_epilogue(std::true_type{});
        } else {
            group_epilogue(std::true_type{});
        }
    } else {
        fp8_epilogue<EPI, !LORA>(acc, P, m0, n0, wr, wc, fr, fh);
    }
}

}  // namespace

extern "C" int apexmi_quant_rows_fp8(const void* a, int64_t lda, int M, int K, void* codes, int64_t ldq, float* scales,
                                     apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(a && codes && scales, "quant_rows_fp8: null operand");
    APEXMI_REQUIRE(M >= 1, "quant_rows_fp8: M=%d must be at least 1", M);
    APEXMI_REQUIRE(K >= 128 && K % 128 == 0, "quant_rows_fp8: K=%d must be a multiple of 128", K);
    APEXMI_REQUIRE(lda >= K && ldq >= K && lda % 8 == 0 && ldq % 16 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)codes % 16) == 0,
                   "quant_rows_fp8: rows must be 16-byte aligned and at least K wide (lda %lld, ldq %lld)", (long long)lda,
                   (long long)ldq);
    ApexmiProfScope prof(5, stream, 0.0, 3.0 * (double)M * K);
    const int pairs = (M + 1) / 2;
    hipLaunchKernelGGL(quant_rows_fp8_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, stream, (const bf16_t*)a, lda, M, K,
                       (uint8_t*)codes, ldq, scales);
    return apexmi_check_launch("quant_rows_fp8");
}

extern "C" int apexmi_quant_blocks_mxfp8(const void* a, int64_t lda, int M, int K, void* codes, int64_t ldq, void* block_scales,
                                         int64_t ldbs, apexmi_stream_t stream_) {
    const MxQuantFormat e4m3{"quant_blocks_mxfp8", 32, 16, 128, "rows must be 16-byte aligned and at least K wide", "ldbs"};
    return mx_quant_blocks(e4m3, quant_blocks_mxfp8_kernel, a, lda, M, K, codes, ldq, block_scales, ldbs, (hipStream_t)stream_);
}

// the MX operands of one problem (apexmi_gemm_fp8_mx, apexmi_gemm_fp8_grouped_mx); null members = not used
struct Fp8MxOperands {
    const void* abs;      // activation block scales [M, K / 32] (then sa is null)
    int64_t ldabs;
    void* Q;              // MX output codes [M, N] (then C may be null)
    int64_t ldq;
    void* QS;             // MX output block scales [M, N / 32]
    int64_t ldqs;
};

// ONE problem of any entry point: every check, then its operand record.  `who` = the entry point's name; `i` = the problem's index
// in a grouped launch, which the messages name, or -1 for a single launch; tile0 = the tiles of the problems before it.  The e4m3
// rules stand here (weight format, scale kinds and counts, the MX operands), the rest in fp8_check_tile_problem.
static int fp8_check_problem(const char* who, int i, int64_t tile0, const void* qa, int64_t lda, const float* sa, const void* qw,
                             int64_t ldw, int w_format, const void* sw, int64_t sw_count, const void* bias, void* C, int64_t ldc, int M,
                             int N, int K, int epilogue, const float* gate, const void* R, int64_t ldr, Fp8Problem* P, const Fp8MxOperands* mx = nullptr) {
    const Fp8Where at(i);
    const char *of = at.of, *paren = at.paren;
    const bool blk = mx != nullptr && mx->abs != nullptr, mxo = mx != nullptr && (mx->Q != nullptr || mx->QS != nullptr);
    APEXMI_REQUIRE(qa && (sa || blk) && qw && sw && (C || mxo), "%s: null operand%s", who, paren);
    APEXMI_REQUIRE(!(sa && blk), "%s: row scales and block scales were both given%s: an activation carries one kind", who, paren);
    APEXMI_REQUIRE(w_format == 0, "%s: weight format %d%s is not e4m3fn (0): e5m2 weights take the bf16 path "
                                  "(apexmi_dequant_fp8_scaled + apexmi_gemm_bf16%s)", who, w_format, of, i >= 0 ? "_grouped" : "");
    APEXMI_REQUIRE(sw_count == 1 || sw_count == N, "%s: the weight scale%s has %lld values for N=%d rows", who, of, (long long)sw_count, N);
    char align_note[64];
    snprintf(align_note, sizeof(align_note), "scales and bias 8-byte%s", at.semi);
    const Fp8Format e4m3{128, "", 1, "", "elements", ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sw % (sw_count == 1 ? 2 : 8)) == 0, align_note};
    if (fp8_check_tile_problem(who, at, e4m3, tile0, qa, lda, qw, ldw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, P)) return 1;
    if (blk)
        APEXMI_REQUIRE(mx->ldabs >= K / 32 && mx->ldabs % 4 == 0 && ((uintptr_t)mx->abs % 4) == 0,
                       "%s: the block scales%s must be 4-byte aligned rows of at least K / 32 = %d bytes (ldabs %lld)", who, of, K / 32,
                       (long long)mx->ldabs);
    if (mxo) {
        APEXMI_REQUIRE(mx->Q && mx->QS, "%s: the MX output%s needs codes and block scales", who, of);
        APEXMI_REQUIRE(epilogue == APEXMI_EPI_BIAS || epilogue == APEXMI_EPI_BIAS_GELU,
                       "%s: the MX output%s exists for the bias (0) and tanh GELU (1) epilogues, not epilogue %d", who, of, epilogue);
        APEXMI_REQUIRE(N % 128 == 0, "%s: N=%d%s must be a multiple of 128 for the MX output", who, N, of);
        APEXMI_REQUIRE(mx->ldq >= N && mx->ldq % 4 == 0 && ((uintptr_t)mx->Q % 4) == 0 && mx->ldqs >= N / 32,
                       "%s: the MX output%s needs 4-byte aligned code rows at least N wide and scale rows at least N / 32 wide "
                       "(ldq %lld, ldqs %lld)", who, of, (long long)mx->ldq, (long long)mx->ldqs);
    }
    P->sa = sa, P->sw = (const bf16_t*)sw, P->sw_rows = sw_count == 1 ? 0 : 1;
    if (blk) P->abs = (const uint8_t*)mx->abs, P->ldabs = mx->ldabs;
    if (mxo) P->Q = (uint8_t*)mx->Q, P->QS = (uint8_t*)mx->QS, P->ldq = mx->ldq, P->ldqs = mx->ldqs;
    return 0;
}

// a single launch of the kernel form that takes `Args`, with its compile-time epilogue
template <class Args>
static void fp8_launch(int epilogue, const Args& G, hipStream_t stream) {
    launch_by_epilogue(epilogue, [](auto epi) { constexpr int EPI = decltype(epi)::value; return gemm_fp8_kernel<EPI, Args>; }, G,
                       (unsigned)(G.tiles_m * G.tiles_n), 0, stream);
}

// both single entry points: every check before any launch; lora = the adapter operands of apexmi_gemm_fp8_lora, or null for apexmi_gemm_fp8
struct Fp8LoraArgs {
    const void* t;
    int64_t ldt;
    const void* lb;
    int64_t ldb;
    int Rp;
};

// the adapter operands of one problem with Rp > 0 (`of` = " of problem i" in a grouped launch)
static int fp8_check_lora(const char* who, const char* of, const Fp8LoraArgs& lora) {
    const int Rp = lora.Rp;
    APEXMI_REQUIRE(Rp >= 64 && Rp % 64 == 0, "%s: the padded rank Rp=%d%s must be a multiple of 64 (set_lora pads to that)", who, Rp, of);
    APEXMI_REQUIRE(lora.t && lora.lb, "%s: null adapter operand%s (t %p, B' %p)", who, of, lora.t, lora.lb);
    APEXMI_REQUIRE(lora.ldt >= Rp && lora.ldb >= Rp, "%s: rows of t and B'%s must be at least Rp=%d wide (ldt %lld, ldb %lld)", who, of,
                   Rp, (long long)lora.ldt, (long long)lora.ldb);
    APEXMI_REQUIRE(lora.ldt % 8 == 0 && lora.ldb % 8 == 0 && ((uintptr_t)lora.t % 16) == 0 && ((uintptr_t)lora.lb % 16) == 0,
                   "%s: t and B'%s must be 16-byte aligned with leading dimensions that are multiples of 8 (ldt %lld, ldb %lld)", who, of,
                   (long long)lora.ldt, (long long)lora.ldb);
    APEXMI_REQUIRE(lora.ldt <= (1 << 22) && lora.ldb <= (1 << 22),
                   "%s: leading dimensions%s above 2^22 elements are not supported (ldt %lld, ldb %lld)", who, of, (long long)lora.ldt,
                   (long long)lora.ldb);
    return 0;
}

static int gemm_fp8_run(const void* qa, int64_t lda, const float* sa, const void* qw, int64_t ldw, int w_format, const void* sw,
                        int64_t sw_count, const void* bias, void* C, int64_t ldc, int M, int N, int K, int epilogue,
                        const float* gate, const void* R, int64_t ldr, const Fp8LoraArgs* lora, hipStream_t stream) {
    Fp8Gemm G{};
    if (fp8_check_problem("gemm_fp8", -1, 0, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &G))
        return 1;
    G.clk = apexmi_clk_ptr();
    if (lora != nullptr) {
        const int Rp = lora->Rp;
        if (fp8_check_lora("gemm_fp8_lora", "", *lora)) return 1;
        Fp8LoraGemm L{G, (const bf16_t*)lora->t, (const bf16_t*)lora->lb, lora->ldt, lora->ldb, Rp};
        ApexmiProfScope prof(0, stream, 2.0 * M * N * ((double)K + Rp),
                             (double)M * K + (double)N * K + 2.0 * ((double)M + N) * Rp + 2.0 * (double)M * N);
        fp8_launch(epilogue, L, stream);
        return apexmi_check_launch("gemm_fp8_lora");
    }
    ApexmiProfScope prof(0, stream, 2.0 * M * N * (double)K, (double)M * K + (double)N * K + 2.0 * (double)M * N);
    fp8_launch(epilogue, G, stream);
    return apexmi_check_launch("gemm_fp8");
}

extern "C" int apexmi_gemm_fp8(const void* qa, int64_t lda, const float* sa, const void* qw, int64_t ldw, int w_format,
                               const void* sw, int64_t sw_count, const void* bias, void* C, int64_t ldc, int M, int N, int K,
                               int epilogue, const float* gate, const void* R, int64_t ldr, apexmi_stream_t stream_) {
    return gemm_fp8_run(qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, nullptr,
                        (hipStream_t)stream_);
}

// replaces apexmi_gemm_fp8 + apexmi_quant_rows_fp8 around an activation that stays in fp8 between two GEMMs
extern "C" int apexmi_gemm_fp8_mx(const void* qa, int64_t lda, const float* sa, const void* abs, int64_t ldabs, const void* qw,
                                  int64_t ldw, int w_format, const void* sw, int64_t sw_count, const void* bias, void* C, int64_t ldc,
                                  void* mx_codes, int64_t ldmc, void* mx_scales, int64_t ldms, int M, int N, int K, int epilogue,
                                  const float* gate, const void* R, int64_t ldr, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const Fp8MxOperands mx{abs, ldabs, mx_codes, ldmc, mx_scales, ldms};
    Fp8MxGemm G{};
    if (fp8_check_problem("gemm_fp8_mx", -1, 0, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, C ? ldc : N, M, N, K, epilogue, gate, R,
                          ldr, &G, &mx))
        return 1;
    G.clk = apexmi_clk_ptr();
    const double out_bytes = mx_codes ? (1.0 + 1.0 / 32) * (double)M * N : 2.0 * (double)M * N;
    ApexmiProfScope prof(0, stream, 2.0 * M * N * (double)K, (abs ? 1.0 + 1.0 / 32 : 1.0) * (double)M * K + (double)N * K + out_bytes);
    fp8_launch(epilogue, G, stream);
    return apexmi_check_launch("gemm_fp8_mx");
}

extern "C" int apexmi_gemm_fp8_lora(const void* qa, int64_t lda, const float* sa, const void* qw, int64_t ldw, int w_format,
                                    const void* sw, int64_t sw_count, const void* bias, void* C, int64_t ldc, int M, int N, int K,
                                    int epilogue, const float* gate, const void* R, int64_t ldr, const void* t, int64_t ldt,
                                    const void* lb, int64_t ldb, int Rp, apexmi_stream_t stream_) {
    const Fp8LoraArgs lora{t, ldt, lb, ldb, Rp};
    return gemm_fp8_run(qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &lora,
                        (hipStream_t)stream_);
}

// every grouped entry point: fp8_check_problem per problem, before the launch; qkv = the fused q/k/v operands of
// apexmi_gemm_fp8_grouped_qkv(_lora) (Fp8QkvArgs, fp8_gemm_tile.h), or null; lora = the five adapter arrays of the _lora entry
// points, or null
struct Fp8LoraArrays {
    const void* const* t;
    const int64_t* ldt;
    const void* const* lb;
    const int64_t* ldb;
    const int* Rp;
};

static int gemm_fp8_grouped_run(int count, const void* const* qa, const int64_t* lda, const float* const* sa, const void* const* qw,
                                const int64_t* ldw, const int* w_format, const void* const* sw, const int64_t* sw_count,
                                const void* const* bias, void* const* C, const int64_t* ldc, const int* M, const int* N, int K,
                                const int* epilogue, const float* const* gate, const void* const* R, const int64_t* ldr,
                                const Fp8QkvArgs* qkv, hipStream_t stream, const Fp8MxOperands* mx = nullptr,
                                const Fp8LoraArrays* lora = nullptr) {
    APEXMI_REQUIRE(count >= 1 && count <= FP8_MAX_GROUPS, "gemm_fp8_grouped: count=%d not in [1,%d]", count, FP8_MAX_GROUPS);
    APEXMI_REQUIRE(qa && lda && sa && qw && ldw && w_format && sw && sw_count && C && ldc && M && N && epilogue,
                   "gemm_fp8_grouped: null argument array");
    APEXMI_REQUIRE(K >= 128 && K % 128 == 0, "gemm_fp8_grouped: K=%d must be a multiple of 128", K);
    Fp8Group G{};            // the table every form shares; copied into the derived struct that is launched
    Fp8LoraEntry entries[FP8_MAX_GROUPS] = {};
    G.count = count;
    const char* lwho = qkv ? "gemm_fp8_grouped_qkv_lora" : "gemm_fp8_grouped_lora";
    if (lora != nullptr) {
        APEXMI_REQUIRE(mx == nullptr, "%s: the MX forms are not combined with run-time LoRA", lwho);
        APEXMI_REQUIRE(lora->t && lora->ldt && lora->lb && lora->ldb && lora->Rp, "%s: null adapter argument array", lwho);
    }
    bool any_lora = false;
    G.clk = apexmi_clk_ptr();
    if (qkv != nullptr && fp8_check_qkv_shared("gemm_fp8_grouped_qkv", *qkv, &G.qs)) return 1;
    double flops = 0, bytes = 0;
    int64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        const bool fused = qkv != nullptr && qkv->is_qkv[i] != 0;
        Fp8GroupProblem& P = G.p[i];
        // a fused problem writes no C: its q_out stands in, N wide
        if (fp8_check_problem("gemm_fp8_grouped", i, tiles, qa[i], lda[i], sa[i], qw[i], ldw[i], w_format[i], sw[i], sw_count[i],
                              bias ? bias[i] : nullptr, fused ? qkv->q_out : C[i], fused || !C[i] ? N[i] : ldc[i], M[i], N[i], K,
                              epilogue[i], gate ? gate[i] : nullptr, R ? R[i] : nullptr, ldr ? ldr[i] : 0, &P, mx ? mx + i : nullptr))
            return 1;
        P.epi = epilogue[i];
        P.tile0 = (int)tiles;
        if (fused && fp8_check_qkv_problem("gemm_fp8_grouped_qkv", *qkv, i, &P)) return 1;
        tiles += (int64_t)P.tiles_m * P.tiles_n;
        flops += 2.0 * M[i] * N[i] * (double)K;
        bytes += (double)M[i] * K + (double)N[i] * K + 2.0 * (double)M[i] * N[i];
        if (lora != nullptr && lora->Rp[i] != 0) {          // Rp == 0: no adapter on this problem, t / B' may be null
            char of[32];
            snprintf(of, sizeof(of), " of problem %d", i);
            const Fp8LoraArgs la{lora->t[i], lora->ldt[i], lora->lb[i], lora->ldb[i], lora->Rp[i]};
            if (fp8_check_lora(lwho, of, la)) return 1;
            entries[i] = Fp8LoraEntry{(const bf16_t*)la.t, (const bf16_t*)la.lb, la.ldt, la.ldb, la.Rp};
            any_lora = true;
            flops += 2.0 * M[i] * N[i] * (double)la.Rp;
            bytes += 2.0 * ((double)M[i] + N[i]) * la.Rp;
        }
    }
    G.total = (int)tiles;
    if (lora != nullptr)
        APEXMI_REQUIRE(any_lora, "%s: no problem carries an adapter (every Rp is 0): use apexmi_gemm_fp8_grouped%s", lwho, qkv ? "_qkv" : "");
    ApexmiProfScope prof(0, stream, flops, bytes);
    if (lora != nullptr) {
        Fp8LoraGroup L{};
        (Fp8Group&)L = G;
        for (int i = 0; i < count; ++i) L.lora[i] = entries[i];
        hipLaunchKernelGGL((gemm_fp8_kernel<0, Fp8LoraGroup>), dim3((unsigned)tiles), dim3(256), 0, stream, L);
        return apexmi_check_launch(lwho);
    }
    if (mx != nullptr) {
        Fp8MxGroup X{};
        (Fp8Group&)X = G;
        hipLaunchKernelGGL((gemm_fp8_kernel<0, Fp8MxGroup>), dim3((unsigned)tiles), dim3(256), 0, stream, X);
        return apexmi_check_launch("gemm_fp8_grouped_mx");
    }
    hipLaunchKernelGGL((gemm_fp8_kernel<0, Fp8Group>), dim3((unsigned)tiles), dim3(256), 0, stream, G);
    return apexmi_check_launch(qkv ? "gemm_fp8_grouped_qkv" : "gemm_fp8_grouped");
}

extern "C" int apexmi_gemm_fp8_grouped(int count, const void* const* qa, const int64_t* lda, const float* const* sa,
                                       const void* const* qw, const int64_t* ldw, const int* w_format, const void* const* sw,
                                       const int64_t* sw_count, const void* const* bias, void* const* C, const int64_t* ldc,
                                       const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                       const void* const* R, const int64_t* ldr, apexmi_stream_t stream_) {
    return gemm_fp8_grouped_run(count, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr,
                                nullptr, (hipStream_t)stream_);
}

extern "C" int apexmi_gemm_fp8_grouped_qkv(int count, const void* const* qa, const int64_t* lda, const float* const* sa,
                                           const void* const* qw, const int64_t* ldw, const int* w_format, const void* const* sw,
                                           const int64_t* sw_count, const void* const* bias, void* const* C, const int64_t* ldc,
                                           const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                           const void* const* R, const int64_t* ldr, const int* is_qkv, const void* const* norm_q,
                                           const void* const* norm_k, const int* row0, int H, float eps, const float* rope,
                                           void* q_out, void* k_out, void* vt_out, int S_out, int Skp, apexmi_stream_t stream_) {
    const Fp8QkvArgs qkv{is_qkv, norm_q, norm_k, row0, H, eps, rope, q_out, k_out, vt_out, S_out, Skp};
    return gemm_fp8_grouped_run(count, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr,
                                &qkv, (hipStream_t)stream_);
}

// replaces apexmi_gemm_fp8_grouped + apexmi_quant_rows_fp8 per problem: per problem i, abs[i] (then sa[i] is null) = block-scaled
// activations, mx_codes[i] / mx_scales[i] (then C[i] may be null) = MX output; null entries = that problem as apexmi_gemm_fp8_grouped
extern "C" int apexmi_gemm_fp8_grouped_mx(int count, const void* const* qa, const int64_t* lda, const float* const* sa,
                                          const void* const* qw, const int64_t* ldw, const int* w_format, const void* const* sw,
                                          const int64_t* sw_count, const void* const* bias, void* const* C, const int64_t* ldc,
                                          const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                          const void* const* R, const int64_t* ldr, const void* const* abs, const int64_t* ldabs,
                                          void* const* mx_codes, const int64_t* ldmc, void* const* mx_scales, const int64_t* ldms,
                                          apexmi_stream_t stream_) {
    APEXMI_REQUIRE(count >= 1 && count <= FP8_MAX_GROUPS, "gemm_fp8_grouped_mx: count=%d not in [1,%d]", count, FP8_MAX_GROUPS);
    APEXMI_REQUIRE(abs && ldabs && mx_codes && ldmc && mx_scales && ldms, "gemm_fp8_grouped_mx: null argument array");
    Fp8MxOperands mx[FP8_MAX_GROUPS];
    for (int i = 0; i < count; ++i) mx[i] = Fp8MxOperands{abs[i], ldabs[i], mx_codes[i], ldmc[i], mx_scales[i], ldms[i]};
    return gemm_fp8_grouped_run(count, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, nullptr,
                                (hipStream_t)stream_, mx);
}

// apexmi_gemm_fp8_grouped with a run-time LoRA adapter per problem: t[i] [M_i, Rp_i], lb[i] = B' [N_i, Rp_i]; Rp[i] == 0 (t[i] / lb[i]
// may be null) = no adapter on problem i.  Every problem leaves the bits of its own single launch: apexmi_gemm_fp8_lora with an
// adapter, apexmi_gemm_fp8 without.
extern "C" int apexmi_gemm_fp8_grouped_lora(int count, const void* const* qa, const int64_t* lda, const float* const* sa,
                                            const void* const* qw, const int64_t* ldw, const int* w_format, const void* const* sw,
                                            const int64_t* sw_count, const void* const* bias, void* const* C, const int64_t* ldc,
                                            const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                            const void* const* R, const int64_t* ldr, const void* const* t, const int64_t* ldt,
                                            const void* const* lb, const int64_t* ldb, const int* Rp, apexmi_stream_t stream_) {
    const Fp8LoraArrays lora{t, ldt, lb, ldb, Rp};
    return gemm_fp8_grouped_run(count, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, nullptr,
                                (hipStream_t)stream_, nullptr, &lora);
}

// apexmi_gemm_fp8_grouped_qkv with the same five arrays: bit-identical to apexmi_gemm_fp8_grouped_lora + apexmi_qkv_prepare
extern "C" int apexmi_gemm_fp8_grouped_qkv_lora(int count, const void* const* qa, const int64_t* lda, const float* const* sa,
                                                const void* const* qw, const int64_t* ldw, const int* w_format, const void* const* sw,
                                                const int64_t* sw_count, const void* const* bias, void* const* C, const int64_t* ldc,
                                                const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                                const void* const* R, const int64_t* ldr, const int* is_qkv, const void* const* norm_q,
                                                const void* const* norm_k, const int* row0, int H, float eps, const float* rope,
                                                void* q_out, void* k_out, void* vt_out, int S_out, int Skp, const void* const* t,
                                                const int64_t* ldt, const void* const* lb, const int64_t* ldb, const int* Rp,
                                                apexmi_stream_t stream_) {
    const Fp8QkvArgs qkv{is_qkv, norm_q, norm_k, row0, H, eps, rope, q_out, k_out, vt_out, S_out, Skp};
    const Fp8LoraArrays lora{t, ldt, lb, ldb, Rp};
    return gemm_fp8_grouped_run(count, qa, lda, sa, qw, ldw, w_format, sw, sw_count, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &qkv,
                                (hipStream_t)stream_, nullptr, &lora);
}
