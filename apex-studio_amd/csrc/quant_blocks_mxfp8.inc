// The streaming kernel of apexmi_quant_blocks_mxfp8 (DESIGN.md §3.6), included by gemm_fp8.hip inside its anonymous namespace, after
// fp8_quant.h (absmax16, the MX block quantiser).  It is a file of its own because gemm_fp8.hip's `__global__` list is pinned to gemm_fp8_kernel and
// quant_rows_fp8_kernel (tests/test_gemm_fp8_lora_host.py): that pin guarantees that every GEMM form — LoRA, grouped, fused q/k/v,
// MX — is an instantiation of the ONE kernel the build's no-spill list names, never a second GEMM kernel beside it.  This kernel
// is a streaming pass with no MFMA, so the guarantee does not concern it; the build digest covers `.inc` files.
// ---- apexmi_quant_blocks_mxfp8 ------------------------------------------------------------------------------------------------
// MX block quantiser (fp8_quant.h): one e8m0 scale byte per 32 consecutive columns instead of one f32 scale per row, so ONE pass:
// a lane holds 16 elements (32 bytes in, 16 bytes out), lanes l and l ^ 1 share a block, the even lane stores the scale byte.
// K % 128 == 0: a row is a whole number of lane pairs, and a pair never straddles two rows.  Threads past the last row read the
// last row again and store nothing.
__global__ __launch_bounds__(256) void quant_blocks_mxfp8_kernel(const bf16_t* __restrict__ a, int64_t lda, int M, int K,
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
    const int sb = mx_scale_byte(m);
    const float inv = mx_inv_scale(sb);
    if (!live) return;
    *(u32x4*)(q + row * ldq + k) = u32x4{mx_quant4(x0[0], x0[1], inv), mx_quant4(x0[2], x0[3], inv), mx_quant4(x1[0], x1[1], inv),
                                         mx_quant4(x1[2], x1[3], inv)};
    if ((k & 16) == 0) bs[row * ldbs + (k >> 5)] = (uint8_t)sb;
}
