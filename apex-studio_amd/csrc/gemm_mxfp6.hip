// Opt-in MXFP6 compute: an MX block quantiser to OCP e2m3 codes, 32 codes packed into 24 bytes, with one e8m0 scale
// byte per 32 consecutive k, and a GEMM of two such operands on v_mfma_scale_f32_32x32x64_f8f6f4 with cbsz = blgp = 2 (e2m3 x e2m3:
// the passes of the e2m1 form, 4x bf16 per clock, with the three mantissa bits of e4m3), BOTH block scales applied by the
// instruction.  Nothing is multiplied after the K-loop: the epilogue is the unscaled one of fp8_gemm_tile.h.
#include "common.h"
#include "fp8_quant.h"        // mx6_scale_byte, mx6_quant16, mx_inv_scale
#include "fp8_gemm_tile.h"    // the 128 x 128 tile order, MxGemm, fp8_epilogue, the host-side checks and launch

namespace {

// ---- apexmi_quant_blocks_mxfp6 ------------------------------------------------------------------------------------------------
// One pass, as quant_blocks_mxfp4_kernel: a lane holds 16 elements (32 bytes in, 12 bytes out = codes 0..15 or 16..31 of the
// block's 24 bytes), lanes l and l ^ 1 share a block of 32, the even lane stores the scale byte.  K % 32 == 0: a row is a whole
// number of lane pairs and a pair never straddles two rows.  Threads past the last row read the last row again and store nothing.
__global__ __launch_bounds__(256) void quant_blocks_mxfp6_kernel(const bf16_t* __restrict__ a, int64_t lda, int M, int K,
                                                                 uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ bs,
                                                                 int64_t ldbs) {
    const int gpr = K >> 4;                                 // 16-element groups per row
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = gid / gpr;
    const int g = (int)(gid - row * gpr);
    const int k = g << 4;
    const bool live = row < M;
    const bf16_t* p = a + (live ? row : (int64_t)M - 1) * lda + k;
    const u32x4 x0 = *(const u32x4*)p, x1 = *(const u32x4*)(p + 8);
    float m = absmax16(x0, x1);
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    const int sb = mx6_scale_byte(m);
    const float inv = mx_inv_scale(sb);
    if (!live) return;
    uint32_t c[3];
    mx6_quant16(x0, x1, inv, c);
    uint32_t* dst = (uint32_t*)(q + row * ldq + g * 12);    // 4-byte aligned: rows are 8-byte aligned
    dst[0] = c[0], dst[1] = c[1], dst[2] = c[2];
    if ((k & 16) == 0) bs[row * ldbs + (k >> 5)] = (uint8_t)sb;
}

// ---- apexmi_gemm_mxfp6 --------------------------------------------------------------------------------------------------------
// gemm_mxfp4_kernel's structure (gemm_mxfp4.hip): 128 x 128 output tile, 256 threads = 2 x 2 waves of 64 x 64, both operand tiles
// staged by global_load_lds (16 bytes per lane), two buffers, one barrier per K-tile, the XCD tile order with bands of 8 tile rows,
// clamped edge rows.  What differs is the row of a K-tile: 128 codes = 4 blocks = 96 BYTES = six 16-byte pieces (a 256-code K-tile
// would be 192 bytes a row, 96 KB for two buffers: one workgroup per CU).  An operand tile is 128 x 96 = 12 KB = 768 pieces, three
// global_load_lds per thread; the four scale bytes of a row and K-tile are ONE 4-byte global_load_lds per thread (waves 0, 1: the
// 128 activation rows, waves 2, 3: the 128 weight rows).  A buffer is 2 x 12 KB + 2 x 512 B = 25 600 B, two are 51 200 B: two
// workgroups per CU.
//
// Staging layout: lds[buf] = [A codes][W codes][A scales][W scales]; a code tile is row-major, 96 bytes a row.  global_load_lds
// writes wave-uniform base + lane x 16, so LDS piece P = 192 wave + 64 i + lane (i = 0..2) of a tile is row P / 6, slot P % 6, and
// the swizzle is on the SOURCE address: slot c of row r holds the row's piece c ^ ((r >> 3) & 1).
//
// Bank arithmetic (64 banks x 4 bytes = sixteen 16-byte columns).  ds_read_b128 serves 16 lanes a cycle, the lane groups {0-3,
// 12-15, 20-27} and {4-11, 16-19, 28-31} of each half wave; all lanes of a group read the same piece c of their own row r = the
// lane's number in the half wave.  Unswizzled the 16-byte column is (6 r + c) mod 16, and 6 r mod 16 = 0, 6, 12, 2, 8, 14, 4, 10
// repeats every 8 rows: only the eight even columns, each hit twice.  In both groups the rows that collide are 8 or 24 apart (0-3
// with 24-27, 12-15 with 20-23; 4-7 with 28-31, 8-11 with 16-19), so bit 3 of the row differs between them: moving the rows with
// that bit set to the piece's neighbour column c ^ 1 puts them on the odd columns, and every group covers all sixteen once.  A
// rotation (c + 1) mod 6 does the same; the XOR with 1 is the cheaper form and stays inside six pieces, which an XOR with a wider
// row term would not.  The 8-byte half of a fragment is read by ds_read_b64, 32 lanes a cycle, all of them the same half of the
// same piece: 32 rows on the 16 eight-byte columns of that parity, a 2-way conflict that no placement of 16-byte pieces removes
// (4 LDS cycles, what a second ds_read_b128 would cost).  With both k-steps unrolled hipcc merges the low-half read of k-step 0 and
// the high-half read of k-step 1 of the same piece into one conflict-free ds_read_b128: 12 per wave and K-tile, no ds_read_b64.
//
// A K-tile is two k-steps of 64 codes.  Operand lane map of the instruction with 6-bit formats (6 registers per lane, the low 192
// bits), pinned by the one-hot probe of tests/test_gpu_mxfp6.py: lane l holds 32 codes of row (A) / column (B) l & 31, lane half
// l >> 5 the second 32 of the k-step's 64; code j of the 32 is bits 6 j .. 6 j + 5 of the registers read as one little-endian
// integer = the 24 bytes of one MX block as the quantiser packs them.  WHICH two blocks form a k-step is free as long as both
// operands agree (a dot product): k-step ks takes block ks for lane half 0 and block ks + 2 for lane half 1, i.e. block ks + 2 fh,
// so that all lanes of an instruction have the same alignment — blocks 0 and 2 (bytes 0, 48 of the row) are a whole piece and the
// low half of the next, blocks 1 and 3 (bytes 24, 72) the high half of a piece and the whole next: one ds_read_b128 and one
// ds_read_b64 per fragment, no select and no shuffle in the K-loop.  The instruction scales a lane's 32 codes by byte 0 (op-sel 0)
// of THAT lane's scale register, on either side.
constexpr int X6_KT = 128;                                   // codes of a K-tile
constexpr int X6_ROW = X6_KT * 6 / 8;                        // bytes of a row of a K-tile
constexpr int X6_OPB = FBM * X6_ROW;                         // bytes of one operand tile
constexpr int X6_SCB = FBM * 4;                              // scale bytes of one operand tile: 128 rows x 4 blocks
constexpr int X6_BUF = 2 * X6_OPB + 2 * X6_SCB;              // one buffer
constexpr int X6_LDS = 2 * X6_BUF;
static_assert(FBM == FBN && X6_OPB == 3 * 256 * 16 && X6_BUF % 16 == 0, "three 16-byte pieces per thread and operand tile");

// this workgroup's tile id `t` inside its problem, and the problem: the launch itself (a grouped table would be another overload)
APEXMI_DEVICE const MxGemm& mxfp6_problem(const MxGemm& G, int& t) {
    t = xcd_remap(blockIdx.x, G.tiles_m * G.tiles_n);
    return G;
}

// what this lane copies in instruction i of a K-tile: LDS piece 192 wid + 64 i + lane = its row (tile rows past `rows` clamp to
// the last one) and the swizzled piece of that row's first 96 bytes; `ld` in bytes
APEXMI_DEVICE const char* mxfp6_stage_src(const uint8_t* base, int64_t ld, int row0, int rows, int wid, int lane, int i) {
    const int p = 192 * wid + 64 * i + lane;
    const int r = p / 6, c = p - 6 * r;
    return (const char*)(base + (int64_t)min(row0 + r, rows - 1) * ld) + ((c ^ ((r >> 3) & 1)) << 4);
}

// the address of piece `piece` of row `row` of a staged tile
APEXMI_DEVICE const uint8_t* mxfp6_piece(const uint8_t* tile, int row, int piece) {
    return tile + row * X6_ROW + ((piece ^ ((row >> 3) & 1)) << 4);
}

// EPI: APEXMI_EPI_BIAS, APEXMI_EPI_BIAS_GELU or APEXMI_EPI_BIAS_GATE_RES.  Templated on the argument type as gemm_mxfp4_kernel is:
// build.py's no-spill check matches "gemm_mxfp6_kernel" and so covers every instantiation.
template <int EPI, class Args>
__global__ __launch_bounds__(256, 2) void gemm_mxfp6_kernel(const Args A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;

    int t, m0, n0;
    const auto& G = mxfp6_problem(A, t);
    fp8_tile_origin(t, G.tiles_m, G.tiles_n, m0, n0);

    const char* a_src[3];
    const char* w_src[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a_src[i] = mxfp6_stage_src(G.A, G.lda, m0, G.M, wid, lane, i);
        w_src[i] = mxfp6_stage_src(G.W, G.ldw, n0, G.N, wid, lane, i);
    }
    // the scale dword of this thread: waves 0, 1 take the activation rows 64 (wid & 1) + lane, waves 2, 3 the weight rows (wave-uniform)
    const int sr = 64 * (wid & 1) + lane;
    const char* s_src = wid < 2 ? (const char*)(G.SA + (int64_t)min(m0 + sr, G.M - 1) * G.ldsa)
                                : (const char*)(G.SW + (int64_t)min(n0 + sr, G.N - 1) * G.ldsw);
    auto stage = [&](int kt, int buf) {
        uint8_t* d = lds + buf * X6_BUF;
        uint8_t* dc = d + wid * 192 * 16;                   // wave-uniform; the hardware adds lane * 16
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            glds16(a_src[i] + (int64_t)kt * X6_ROW, dc + i * 1024);
            glds16(w_src[i] + (int64_t)kt * X6_ROW, dc + X6_OPB + i * 1024);
        }
        glds4(s_src + kt * 4, d + 2 * X6_OPB + wid * 256);  // [A scales 512][W scales 512]; the hardware adds lane * 4
    };

    Fp8Clock clock;
    clock.start(A.clk);

    f32x16 acc[2][2];                 // [weight tile (output columns)][activation tile (output rows)]
    fp8_zero_acc(acc);

    const int nk = G.K / X6_KT;
    const int fr = lane & 31, fh = lane >> 5;
    stage(0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) stage(kt + 1, buf ^ 1);
        const uint8_t* ta = lds + buf * X6_BUF;
        const uint8_t* tw = ta + X6_OPB;
        const uint8_t* sa = ta + 2 * X6_OPB;
        const uint8_t* sw = sa + X6_SCB;
        // the 4 scale bytes of the lane's rows; block ks + 2 fh of the 4 is byte 0 after the shift
        uint32_t xa[2], xw[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            xa[i] = *(const uint32_t*)(sa + (64 * wr + 32 * i + fr) * 4);
            xw[i] = *(const uint32_t*)(sw + (64 * wc + 32 * i + fr) * 4);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            // block ks + 2 fh = bytes 48 fh + 24 ks of the row: pieces 3 fh, 3 fh + 1 (low half) or 3 fh + 1 (high half), 3 fh + 2
            const int whole = 3 * fh + 2 * ks, half = 3 * fh + 1;
            const int shift = 16 * fh + 8 * ks;
            i32x8 fa[2], fw[2];
            int ea[2], ew[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ra = 64 * wr + 32 * i + fr, rw = 64 * wc + 32 * i + fr;
                const u32x4 pa = *(const u32x4*)mxfp6_piece(ta, ra, whole), pw = *(const u32x4*)mxfp6_piece(tw, rw, whole);
                const u32x2 ha = *(const u32x2*)(mxfp6_piece(ta, ra, half) + 8 * ks);
                const u32x2 hw = *(const u32x2*)(mxfp6_piece(tw, rw, half) + 8 * ks);
                if (ks == 0) {
                    fa[i] = i32x8{(int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], (int)ha[0], (int)ha[1], 0, 0};
                    fw[i] = i32x8{(int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3], (int)hw[0], (int)hw[1], 0, 0};
                } else {
                    fa[i] = i32x8{(int)ha[0], (int)ha[1], (int)pa[0], (int)pa[1], (int)pa[2], (int)pa[3], 0, 0};
                    fw[i] = i32x8{(int)hw[0], (int)hw[1], (int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3], 0, 0};
                }
                ea[i] = (int)(xa[i] >> shift);
                ew[i] = (int)(xw[i] >> shift);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fw[i], fa[j], acc[i][j], 2, 2, 0, ew[i], 0, ea[j]);
        }
        __syncthreads();
    }

    clock.stop(A.clk, tid);
    fp8_epilogue<EPI, false>(acc, G, m0, n0, wr, wc, fr, fh);
}

}  // namespace

extern "C" int apexmi_quant_blocks_mxfp6(const void* a, int64_t lda, int M, int K, void* codes, int64_t ldq, void* scales, int64_t lds_,
                                         apexmi_stream_t stream_) {
    const MxQuantFormat e2m3{"quant_blocks_mxfp6", 24, 8, 32,
                             "rows of a must be 16-byte and code rows 8-byte aligned, a at least K and the codes at least 3 K / 4 bytes wide",
                             "lds"};
    return mx_quant_blocks(e2m3, quant_blocks_mxfp6_kernel, a, lda, M, K, codes, ldq, scales, lds_, (hipStream_t)stream_);
}

// the e2m3 rules and wording of mx_check_problem (fp8_gemm_tile.h)
constexpr Fp8Format X6_FORMAT{X6_KT, " (a K-tile is 96 bytes of e2m3 codes)", 1, ", code rows at least 3 K / 4 = %d bytes", "bytes", true,
                              "output and bias 8-byte", 6};

extern "C" int apexmi_gemm_mxfp6(const void* qa, int64_t lda, const void* sa, int64_t ldsa, const void* qw, int64_t ldw, const void* sw,
                                 int64_t ldsw, const void* bias, void* C, int64_t ldc, int M, int N, int K, int epilogue,
                                 const float* gate, const void* R, int64_t ldr, apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char* who = "gemm_mxfp6";
    MxGemm G{};
    if (mx_check_problem(who, -1, 0, X6_FORMAT, qa, lda, sa, ldsa, qw, ldw, sw, ldsw, bias, C, ldc, M, N, K, epilogue, gate, R, ldr, &G)) return 1;
    G.clk = apexmi_clk_ptr();
    ApexmiProfScope prof(0, stream, 2.0 * M * N * (double)K, (0.75 + 1.0 / 32) * ((double)M + N) * K + 2.0 * (double)M * N);
    launch_by_epilogue(epilogue, [](auto epi) { return gemm_mxfp6_kernel<decltype(epi)::value, MxGemm>; }, G,
                       (unsigned)(G.tiles_m * G.tiles_n), X6_LDS, stream);
    return apexmi_check_launch(who);
}
