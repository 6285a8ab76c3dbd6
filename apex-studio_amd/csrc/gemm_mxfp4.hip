// Opt-in MXFP4 compute: an MX block quantiser to OCP e2m1 codes with one e8m0 scale byte per 32 consecutive k, and a
// GEMM of two such operands on v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 4 (e2m1 x e2m1: half the cycles of the e4m3 form,
// 4x bf16 per clock), BOTH block scales applied by the instruction.  Nothing is multiplied after the K-loop: the epilogue is the
// unscaled one of fp8_gemm_tile.h.
#include "common.h"
#include "fp8_quant.h"        // mx4_scale_byte, mx4_quant8, mx_inv_scale
#include "fp8_gemm_tile.h"    // the 128 x 128 tile, Fp8Problem, fp8_epilogue

namespace {

// ---- apexmi_quant_blocks_mxfp4 ------------------------------------------------------------------------------------------------
// One pass, as quant_blocks_mxfp8_kernel: a lane holds 16 elements (32 bytes in, 8 bytes out), lanes l and l ^ 1 share a block of
// 32, the even lane stores the scale byte.  K % 32 == 0: a row is a whole number of lane pairs and a pair never straddles two rows.
// Threads past the last row read the last row again and store nothing.
__global__ __launch_bounds__(256) void quant_blocks_mxfp4_kernel(const bf16_t* __restrict__ a, int64_t lda, int M, int K,
                                                                 uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ bs,
                                                                 int64_t ldbs) {
    const int gpr = K >> 4;                                 // 16-element groups per row
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / gpr;
    const int k = (int)(gid - row * gpr) << 4;
    const bool live = row < M;
    const bf16_t* p = a + (live ? row : (int64_t)M - 1) * lda + k;
    const u32x4 x0 = *(const u32x4*)p, x1 = *(const u32x4*)(p + 8);
    float m = absmax16(x0, x1);
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    const int sb = mx4_scale_byte(m);
    const float inv = mx_inv_scale(sb);
    if (!live) return;
    *(u32x2*)(q + row * ldq + (k >> 1)) = u32x2{mx4_quant8(x0, inv), mx4_quant8(x1, inv)};
    if ((k & 16) == 0) bs[row * ldbs + (k >> 5)] = (uint8_t)sb;
}

// ---- apexmi_gemm_mxfp4 --------------------------------------------------------------------------------------------------------
// gemm_fp8_kernel's structure (gemm_fp8.hip): 128 x 128 output tile, 256 threads = 2 x 2 waves of 64 x 64, K-tiles of 128 BYTES per
// row = 256 codes, both operand tiles staged by global_load_lds (16 bytes per lane) with the XOR swizzle on the source address, two
// buffers, one barrier per K-tile, the XCD tile order with bands of 8 tile rows, clamped edge rows.
//
// A K-tile is four k-steps of 64 codes.  Operand lane map of the instruction with 4-bit formats (4 registers per lane), pinned by
// the one-hot probes of tests/test_gpu_mxfp4.py: lane l holds the 32 codes k = 32 (l >> 5) + 0..31 of row (A) / column (B) l & 31 =
// ONE 16-byte piece of the staged row, piece 2 ks + (l >> 5) of k-step ks; the order of the nibbles inside the piece is the same
// for both operands and so does not matter to a dot product.  A lane's 32 codes are exactly one MX block, and the instruction
// scales them by byte 0 (op-sel 0) of THAT lane's scale register, on either side.
//
// Scale bytes: a K-tile needs 8 per row and operand.  They are staged through LDS with the tile — one 4-byte global_load_lds per
// thread and operand (thread t: row t >> 1, dword t & 1), 2 KB per buffer behind the 64 KB of codes (dynamic LDS, 68 KB: two
// workgroups per CU fit the 160 KB) — and read back as one ds_read_b64 per row and K-tile.  The alternative, plain global loads
// some K-tiles ahead as the MX-input form of gemm_fp8_kernel does, puts 64 cache lines per wave instruction on the vector-memory
// path next to the staging loads; staging keeps every scale access of the K-loop on LDS.  The two were not compared by measurement.
constexpr int X4_SCB = FBM * 8;                              // scale bytes of one operand tile: 128 rows x 8 blocks
constexpr int X4_LDS = 4 * FOPB + 4 * X4_SCB;                // codes [buf][operand] + scales [buf][operand]

// The grouped form (apexmi_gemm_mxfp4_grouped, apexmi_gemm_mxfp4_grouped_qkv): the table entry of the fp8 kernel's grouped form
// (Fp8GroupProblem, fp8_gemm_tile.h) plus the problem's own block scales; the table travels by value, as Fp8Group does.
struct Mxfp4GroupProblem : Fp8GroupProblem {
    const uint8_t* SA;
    const uint8_t* SW;
    int64_t ldsa, ldsw;
};
struct Mxfp4Group {
    Mxfp4GroupProblem p[FP8_MAX_GROUPS];
    int count, total;
    Fp8QkvShared qs;
    unsigned long long* clk;
};

// this workgroup's tile id `t` inside its problem, and the problem: the launch itself, or the table entry found by the prefix sums
APEXMI_DEVICE const MxGemm& mxfp4_problem(const MxGemm& G, int& t) {
    t = xcd_remap(blockIdx.x, G.tiles_m * G.tiles_n);
    return G;
}
APEXMI_DEVICE Mxfp4GroupProblem mxfp4_problem(const Mxfp4Group& G, int& t) {
    int pi;
    return fp8_group_entry(G.p, G.count, G.total, t, pi);
}

// ONE kernel for both forms, chosen by the argument type (MxGemm, Mxfp4Group), as gemm_fp8_kernel: build.py's no-spill check
// matches "gemm_mxfp4_kernel" and so covers every instantiation.
// EPI: APEXMI_EPI_BIAS, APEXMI_EPI_BIAS_GELU or APEXMI_EPI_BIAS_GATE_RES; the grouped form reads it from its problem instead
// MXO (apexmi_gemm_mxfp4_mx, apexmi_gemm_mxfp4_grouped(_qkv)_mx): the output leaves as MXFP4 codes and scale bytes (Q / QS, the
// MXO_E2M1 epilogue of fp8_gemm_tile.h; bias and gelu) — the single form always, a problem of the grouped form where its Q is set
// (block-uniform).  Instantiations of their own: the launches without MX output run the kernels they ran before MXO existed.
template <int EPI, class Args, bool MXO = false>
__global__ __launch_bounds__(256, 2) void gemm_mxfp4_kernel(const Args A) {
    constexpr bool GROUPED = std::is_same_v<Args, Mxfp4Group>;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    int t, m0, n0;
    const auto& G = mxfp4_problem(A, t);         // everything per problem (row clamps, scale rows, nk) is read from it
    fp8_tile_origin(t, G.tiles_m, G.tiles_n, m0, n0);

    // staging: the codes as in gemm_fp8_kernel; thread t adds one scale dword per operand
    const Fp8Stager stage_codes(G, m0, n0, wid, lane);
    const char* sa_src = (const char*)(G.SA + (int64_t)min(m0 + (tid >> 1), G.M - 1) * G.ldsa + (tid & 1) * 4);
    const char* sw_src = (const char*)(G.SW + (int64_t)min(n0 + (tid >> 1), G.N - 1) * G.ldsw + (tid & 1) * 4);
    auto stage = [&](int kt, int buf) {
        stage_codes(lds, wid, kt, buf);
        uint8_t* ds = lds + 4 * FOPB + buf * 2 * X4_SCB + wid * 256;   // wave-uniform; the hardware adds lane * 4
        glds4(sa_src + kt * 8, ds);
        glds4(sw_src + kt * 8, ds + X4_SCB);
    };

    Fp8Clock clock;
    clock.start(A.clk);

    f32x16 acc[2][2];                 // [weight tile (output columns)][activation tile (output rows)]
    fp8_zero_acc(acc);

    const int nk = G.K / (2 * FBK);
    const int fr = lane & 31, fh = lane >> 5;
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const uint8_t* ta = lds + buf * 2 * FOPB;
        const uint8_t* tw = ta + FOPB;
        const uint8_t* sa = lds + 4 * FOPB + buf * 2 * X4_SCB;
        const uint8_t* sw = sa + X4_SCB;
        // the 8 scale bytes of the lane's rows; lane half fh takes the odd blocks: byte 2 ks + fh of the 8 is byte 0 after the shift
        u32x2 xa[2], xw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xa[i] = *(const u32x2*)(sa + (64 * wr + 32 * i + fr) * 8);
            xw[i] = *(const u32x2*)(sw + (64 * wc + 32 * i + fr) * 8);
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int piece = 2 * ks + fh;
            const int shift = 16 * (ks & 1) + 8 * fh;
            i32x8 fa[2], fw[2];
            int ea[2], ew[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const u32x4 pa = lds_piece(ta, 64 * wr + 32 * i + fr, piece), pw = lds_piece(tw, 64 * wc + 32 * i + fr, piece);
                fa[i] = i32x8{(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], 0, 0, 0, 0};
                fw[i] = i32x8{(int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3], 0, 0, 0, 0};
                ea[i] = (int)(xa[i][ks >> 1] >> shift);
                ew[i] = (int)(xw[i][ks >> 1] >> shift);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 4, 4, 0, ew[i], 0, ea[j]);
        }
        __syncthreads();
    }

    clock.stop(A.clk, tid);
    if constexpr (GROUPED) {
        // block-uniform: the epilogue by the table entry.  The fused q/k/v preparation lays its bf16 tile over the first 32 KB of
        // the code buffers (buffer 0, both operands), which nothing reads after the K-loop's last barrier.
        if (G.qkv) fp8_qkv_epilogue<false>(acc, G, A.qs, m0, n0, tid, lds);
        else if (MXO && G.Q != nullptr && G.epi == APEXMI_EPI_BIAS_GELU)
            fp8_epilogue<APEXMI_EPI_BIAS_GELU, false, false, MXO_E2M1>(acc, G, m0, n0, wr, wc, fr, fh);
        else if (MXO && G.Q != nullptr) fp8_epilogue<APEXMI_EPI_BIAS, false, false, MXO_E2M1>(acc, G, m0, n0, wr, wc, fr, fh);
        else if (G.epi == APEXMI_EPI_BIAS) fp8_epilogue<APEXMI_EPI_BIAS, false>(acc, G, m0, n0, wr, wc, fr, fh);
        else if (G.epi == APEXMI_EPI_BIAS_GELU) fp8_epilogue<APEXMI_EPI_BIAS_GELU, false>(acc, G, m0, n0, wr, wc, fr, fh);
        else fp8_epilogue<APEXMI_EPI_BIAS_GATE_RES, false>(acc, G, m0, n0, wr, wc, fr, fh);
    } else if constexpr (MXO) {
        fp8_epilogue<EPI, false, false, MXO_E2M1>(acc, G, m0, n0, wr, wc, fr, fh);
    } else {
        fp8_epilogue<EPI, false>(acc, G, m0, n0, wr, wc, fr, fh);
    }
}

}  // namespace

extern "C" int apexmi_quant_blocks_mxfp4(const void* a, int64_t lda, int M, int K, void* codes, int64_t ldq, void* scales, int64_t lds_,
                                         apexmi_stream_t stream_) {
    const MxQuantFormat e2m1{"quant_blocks_mxfp4", 16, 16, 32,
                             "rows must be 16-byte aligned, a at least K and the codes at least K / 2 bytes wide", "lds"};
    return mx_quant_blocks(e2m1, quant_blocks_mxfp4_kernel, a, lda, M, K, codes, ldq, scales, lds_, (hipStream_t)stream_);
}

// the e2m1 rules and wording of mx_check_problem (fp8_gemm_tile.h)
constexpr Fp8Format X4_FORMAT{256, " (a K-tile is 128 bytes of e2m1 codes)", 2, ", code rows at least K / 2 = %d bytes", "bytes", true,
                              "output and bias 8-byte"};

extern "C" int apexmi_gemm_mxfp4(const void* qa, int64_t lda, const void* sa, int64_t ldsa, const void* qw, int64_t ldw, const void* sw,
                                 int64_t ldsw, const void* bias, void* C, int64_t ldc, int M, int N, int K, int epilogue,
                                 const float* gate, const void* R, int64_t ldr, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "gemm_mxfp4";
    MxGemm G{};
    if (mx_check_problem(who, -1, 0, X4_FORMAT, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &G)) return 1;
    G.clk = apexmi_clk_ptr();
    ApexmiProfScope prof(0, stream, 2.0 * M * N * (double)K, (0.5 + 1.0 / 32) * ((double)M + N) * K + 2.0 * (double)M * N);
    // 68 KB of dynamic LDS is above the default limit
    launch_by_epilogue(epilogue, [](auto epi) { return gemm_mxfp4_kernel<decltype(epi)::value, MxGemm>; }, G,
                       (unsigned)(G.tiles_m * G.tiles_n), X4_LDS, stream);
    return apexmi_check_launch(who);
}

// apexmi_gemm_mxfp4 whose output leaves as MXFP4 (include/apexmi.h): the bf16 launch followed by apexmi_quant_blocks_mxfp4 on its
// output, bit for bit, as one launch that writes no C.  Null mx_codes and mx_scales = apexmi_gemm_mxfp4 itself.
extern "C" int apexmi_gemm_mxfp4_mx(const void* qa, int64_t lda, const void* sa, int64_t ldsa, const void* qw, int64_t ldw, const void* sw,
                                    int64_t ldsw, const void* bias, void* C, int64_t ldc, void* mx_codes, int64_t ldmc, void* mx_scales,
                                    int64_t ldms, int M, int N, int K, int epilogue, const float* gate, const void* R, int64_t ldr,
                                    apexmi_stream_t stream_) {
    if (!mx_codes && !mx_scales)
        return apexmi_gemm_mxfp4(qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, stream_);
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "gemm_mxfp4_mx";
    const MxOut mx{mx_codes, ldmc, mx_scales, ldms};
    MxGemm G{};
    if (mx_check_problem(who, -1, 0, X4_FORMAT, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &G, &mx)) return 1;
    G.clk = apexmi_clk_ptr();
    ApexmiProfScope prof(0, stream, 2.0 * M * N * (double)K, (0.5 + 1.0 / 32) * (((double)M + N) * K + (double)M * N));
    // the check left bias or gelu: the gate_res case of the switch names the bias kernel and is never taken
    launch_by_epilogue(epilogue, [](auto epi) {
        constexpr int EPI = decltype(epi)::value == APEXMI_EPI_BIAS_GELU ? APEXMI_EPI_BIAS_GELU : APEXMI_EPI_BIAS;
        return gemm_mxfp4_kernel<EPI, MxGemm, true>;
    }, G, (unsigned)(G.tiles_m * G.tiles_n), X4_LDS, stream);
    return apexmi_check_launch(who);
}

// the MX outputs of a grouped launch as the _mx entry points take them: entry i both null = problem i writes its bf16 C
struct Mxfp4MxArrays {
    void* const* codes;
    const int64_t* ldmc;
    void* const* scales;
    const int64_t* ldms;
};

// every grouped entry point: every check of every problem before the launch; qkv = the fused q/k/v operands of
// apexmi_gemm_mxfp4_grouped_qkv(_mx), or null; mxa = the MX outputs of the _mx entry points, or null
static int gemm_mxfp4_grouped_run(const char* who, int count, const void* const* qa, const int64_t* lda, const void* const* sa,
                                  const int64_t* ldsa, const void* const* qw, const int64_t* ldw, const void* const* sw,
                                  const int64_t* ldsw, const void* const* bias, void* const* C, const int64_t* ldc, const int* M,
                                  const int* N, int K, const int* epilogue, const float* const* gate, const void* const* R,
                                  const int64_t* ldr, const Fp8QkvArgs* qkv, hipStream_t stream, const Mxfp4MxArrays* mxa = nullptr) {
    APEXMI_REQUIRE(count >= 1 && count <= FP8_MAX_GROUPS, "%s: count=%d not in [1,%d]", who, count, FP8_MAX_GROUPS);
    APEXMI_REQUIRE(qa && lda && sa && ldsa && qw && ldw && sw && ldsw && C && ldc && M && N && epilogue, "%s: null argument array", who);
    APEXMI_REQUIRE(K >= 256 && K % 256 == 0, "%s: K=%d must be a multiple of 256 (a K-tile is 128 bytes of e2m1 codes; the problems share K)",
                   who, K);
    APEXMI_REQUIRE(!mxa || (mxa->codes && mxa->ldmc && mxa->scales && mxa->ldms), "%s: null argument array", who);
    Mxfp4Group G{};
    G.count = count;
    G.clk = apexmi_clk_ptr();
    if (qkv != nullptr && fp8_check_qkv_shared(who, *qkv, &G.qs)) return 1;
    double flops = 0, bytes = 0;
    int64_t tiles = 0;
    bool any_mx = false;
    for (int i = 0; i < count; ++i) {
        const bool fused = qkv != nullptr && qkv->is_qkv[i] != 0;
        const MxOut mx = mxa ? MxOut{mxa->codes[i], mxa->ldmc[i], mxa->scales[i], mxa->ldms[i]} : MxOut{};
        const bool mxo = mx.Q != nullptr || mx.QS != nullptr;
        APEXMI_REQUIRE(!(fused && mxo), "%s: a fused q/k/v problem (problem %d) writes q / k / V^T and takes no MX output", who, i);
        any_mx |= mxo;
        Mxfp4GroupProblem& P = G.p[i];
        // a fused problem writes no C: its q_out stands in, N wide
        if (mx_check_problem(who, i, tiles, X4_FORMAT, qa[i], lda[i], sa[i], ldsa[i], qw[i], ldw[i], sw[i], ldsw[i], bias ? bias[i] : nullptr,
                                fused ? qkv->q_out : C[i], fused ? N[i] : ldc[i], M[i], N[i], K, epilogue[i], gate ? gate[i] : nullptr,
                                R ? R[i] : nullptr, ldr ? ldr[i] : 0, &P, &mx))
            return 1;
        P.epi = epilogue[i];
        P.tile0 = (int)tiles;
        if (fused && fp8_check_qkv_problem(who, *qkv, i, &P)) return 1;
        tiles += (int64_t)P.tiles_m * P.tiles_n;
        flops += 2.0 * M[i] * N[i] * (double)K;
        bytes += (0.5 + 1.0 / 32) * ((double)M[i] + N[i]) * K + (mxo ? 0.5 + 1.0 / 32 : 2.0) * (double)M[i] * N[i];
    }
    G.total = (int)tiles;
    ApexmiProfScope prof(0, stream, flops, bytes);
    // 68 KB of dynamic LDS is above the default limit.  The table entries carry the epilogues: the launch names none, and one without
    // an MX output runs the kernel it always ran.
    if (any_mx)
        launch_by_epilogue(APEXMI_EPI_BIAS, [](auto) { return gemm_mxfp4_kernel<0, Mxfp4Group, true>; }, G, (unsigned)tiles, X4_LDS, stream);
    else
        launch_by_epilogue(APEXMI_EPI_BIAS, [](auto) { return gemm_mxfp4_kernel<0, Mxfp4Group>; }, G, (unsigned)tiles, X4_LDS, stream);
    return apexmi_check_launch(who);
}

// the grouped launches of the Flux blocks (apexmi_gemm_bf16_grouped) on MXFP4 operands: problem i = apexmi_gemm_mxfp4 of
// (qa[i], sa[i]) x (qw[i], sw[i]), bit for bit
extern "C" int apexmi_gemm_mxfp4_grouped(int count, const void* const* qa, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                                         const void* const* qw, const int64_t* ldw, const void* const* sw, const int64_t* ldsw,
                                         const void* const* bias, void* const* C, const int64_t* ldc, const int* M, const int* N, int K,
                                         const int* epilogue, const float* const* gate, const void* const* R, const int64_t* ldr,
                                         apexmi_stream_t stream_) {
    return gemm_mxfp4_grouped_run("gemm_mxfp4_grouped", count, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue, gate,
                                  R, ldr, nullptr, (hipStream_t)stream_);
}

// apexmi_gemm_mxfp4_grouped with apexmi_qkv_prepare fused into the epilogue of the problems flagged in is_qkv: bit-identical to the
// two launches on the same codes; C[i] of a fused problem may be null and is not written
extern "C" int apexmi_gemm_mxfp4_grouped_qkv(int count, const void* const* qa, const int64_t* lda, const void* const* sa,
                                             const int64_t* ldsa, const void* const* qw, const int64_t* ldw, const void* const* sw,
                                             const int64_t* ldsw, const void* const* bias, void* const* C, const int64_t* ldc,
                                             const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                             const void* const* R, const int64_t* ldr, const int* is_qkv, const void* const* norm_q,
                                             const void* const* norm_k, const int* row0, int H, float eps, const float* rope,
                                             void* q_out, void* k_out, void* vt_out, int S_out, int Skp, apexmi_stream_t stream_) {
    const Fp8QkvArgs qkv{is_qkv, norm_q, norm_k, row0, H, eps, rope, q_out, k_out, vt_out, S_out, Skp};
    return gemm_mxfp4_grouped_run("gemm_mxfp4_grouped_qkv", count, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue,
                                  gate, R, ldr, &qkv, (hipStream_t)stream_);
}

// apexmi_gemm_mxfp4_grouped where problem i with mx_codes[i] set leaves as MXFP4 (include/apexmi.h): that problem is
// apexmi_gemm_mxfp4_mx, the others apexmi_gemm_mxfp4, bit for bit, in one launch
extern "C" int apexmi_gemm_mxfp4_grouped_mx(int count, const void* const* qa, const int64_t* lda, const void* const* sa, const int64_t* ldsa,
                                            const void* const* qw, const int64_t* ldw, const void* const* sw, const int64_t* ldsw,
                                            const void* const* bias, void* const* C, const int64_t* ldc, void* const* mx_codes,
                                            const int64_t* ldmc, void* const* mx_scales, const int64_t* ldms, const int* M, const int* N,
                                            int K, const int* epilogue, const float* const* gate, const void* const* R,
                                            const int64_t* ldr, apexmi_stream_t stream_) {
    const Mxfp4MxArrays mxa{mx_codes, ldmc, mx_scales, ldms};
    return gemm_mxfp4_grouped_run("gemm_mxfp4_grouped_mx", count, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue,
                                  gate, R, ldr, nullptr, (hipStream_t)stream_, &mxa);
}

// apexmi_gemm_mxfp4_grouped_qkv with the MX outputs of apexmi_gemm_mxfp4_grouped_mx on the problems that are NOT fused q/k/v
extern "C" int apexmi_gemm_mxfp4_grouped_qkv_mx(int count, const void* const* qa, const int64_t* lda, const void* const* sa,
                                                const int64_t* ldsa, const void* const* qw, const int64_t* ldw, const void* const* sw,
                                                const int64_t* ldsw, const void* const* bias, void* const* C, const int64_t* ldc,
                                                void* const* mx_codes, const int64_t* ldmc, void* const* mx_scales, const int64_t* ldms,
                                                const int* M, const int* N, int K, const int* epilogue, const float* const* gate,
                                                const void* const* R, const int64_t* ldr, const int* is_qkv, const void* const* norm_q,
                                                const void* const* norm_k, const int* row0, int H, float eps, const float* rope,
                                                void* q_out, void* k_out, void* vt_out, int S_out, int Skp, apexmi_stream_t stream_) {
    const Fp8QkvArgs qkv{is_qkv, norm_q, norm_k, row0, H, eps, rope, q_out, k_out, vt_out, S_out, Skp};
    const Mxfp4MxArrays mxa{mx_codes, ldmc, mx_scales, ldms};
    return gemm_mxfp4_grouped_run("gemm_mxfp4_grouped_qkv_mx", count, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue,
                                  gate, R, ldr, &qkv, (hipStream_t)stream_, &mxa);
}
