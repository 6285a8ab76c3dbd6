// GGUF block formats -> bf16 (the reference's `load_gguf` / `GGMLLinear`, R/src/quantize/load.py:364,
// ggml_layer.py:220, dequantise with torch ops per forward).  One streaming kernel per block type.
//
// NUMERICAL CONTRACT.  An element is ggml's `dequantize_row_*` formula in IEEE float32 with every multiply / add / subtract
// rounded separately (`__fmul_rn` / `__fadd_rn` / `__fsub_rn`: never contracted into an FMA), then rounded once to bf16
// (nearest-even).  f16 block scales widen to f32 by bits.  The output is a pure function of the block bytes: tests compare with
// torch.equal against the numpy restatement in gguf_file.py.
//
// SHAPE.  The blocks of an [rows, K] weight are one contiguous byte stream (blocks run along K, rows follow each other), so the
// matrix is cut into flat tiles of 2048 elements = 64 blocks of 32 or 8 blocks of 256.  A workgroup of 256 lanes copies its tile's
// bytes (1.1 - 2.2 KB) into LDS with 16-byte loads from the enclosing ALIGNED window — the 18 / 22 / 34 / 210-byte blocks start at
// any even address, so no lane ever issues a misaligned vector load; the first / last window of the whole buffer is read byte-wise
// where it sticks out — then every lane owns 8 consecutive elements of one block: it picks the block's scale fields and its 4 - 8
// payload bytes out of LDS, unpacks in registers and writes one 16-byte bf16x8.  K is a multiple of 32, so a lane's 8 elements
// never straddle a row and the row stride `ldo` only enters the store address.
#include "common.h"

namespace {

enum : int { GGML_F32 = 0, GGML_F16 = 1, GGML_Q4_0 = 2, GGML_Q4_1 = 3, GGML_Q5_0 = 6, GGML_Q5_1 = 7, GGML_Q8_0 = 8,
             GGML_Q4_K = 12, GGML_Q5_K = 13, GGML_Q6_K = 14, GGML_BF16 = 30 };

constexpr int TILE = 2048;                     // elements per workgroup: 256 lanes x 8
constexpr int LDS_BYTES = 64 * 34 + 16 + 16;   // largest tile (Q8_0) + the alignment window + the tail dwords lds_u64 may touch

// IEEE half -> float by bits (exact, subnormals included; independent of the denormal mode of the conversion instruction)
APEXMI_DEVICE float f16_bits_to_f32(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    if (e == 0u) return __uint_as_float(sign | __float_as_uint((float)m * 5.9604644775390625e-08f));   // m * 2^-24
    if (e == 31u) return __uint_as_float(sign | 0x7F800000u | (m << 13));
    return __uint_as_float(sign | ((e + 112u) << 23) | (m << 13));
}

// bytes at ANY offset of the LDS tile, assembled from aligned dwords (v_alignbyte_b32)
APEXMI_DEVICE uint32_t lds_u32(const uint32_t* lds, int off) {
    const uint32_t* w = lds + (off >> 2);
    return __builtin_amdgcn_alignbyte(w[1], w[0], (uint32_t)(off & 3));
}
APEXMI_DEVICE void lds_u64(const uint32_t* lds, int off, uint32_t& lo, uint32_t& hi) {
    const uint32_t* w = lds + (off >> 2);
    const uint32_t a = w[0], b = w[1], c = w[2], s = (uint32_t)(off & 3);
    lo = __builtin_amdgcn_alignbyte(b, a, s);
    hi = __builtin_amdgcn_alignbyte(c, b, s);
}
APEXMI_DEVICE uint32_t lds_u16(const uint32_t* lds, int off) { return lds_u32(lds, off) & 0xFFFFu; }
APEXMI_DEVICE uint32_t lds_u8(const uint32_t* lds, int off) { return (lds[off >> 2] >> (8 * (off & 3))) & 0xFFu; }
APEXMI_DEVICE uint32_t byte_of(uint32_t lo, uint32_t hi, int i) { return ((i < 4 ? lo : hi) >> (8 * (i & 3))) & 0xFFu; }

// ggml's get_scale_min_k4: the 6-bit scale / min of sub-block j (0..7) out of the 12 packed bytes at `s`
APEXMI_DEVICE void scale_min_k4(const uint32_t* lds, int s, int j, float& sc, float& mn) {
    if (j < 4) {
        sc = (float)(lds_u8(lds, s + j) & 63u);
        mn = (float)(lds_u8(lds, s + j + 4) & 63u);
    } else {
        const uint32_t a = lds_u8(lds, s + j + 4), lo = lds_u8(lds, s + j - 4), hi = lds_u8(lds, s + j);
        sc = (float)((a & 15u) | ((lo >> 6) << 4));
        mn = (float)((a >> 4) | ((hi >> 6) << 4));
    }
}

template <int TYPE>
struct Fmt;
template <> struct Fmt<GGML_Q4_0> { static constexpr int BLK = 32, BYTES = 18; };
template <> struct Fmt<GGML_Q4_1> { static constexpr int BLK = 32, BYTES = 20; };
template <> struct Fmt<GGML_Q5_0> { static constexpr int BLK = 32, BYTES = 22; };
template <> struct Fmt<GGML_Q5_1> { static constexpr int BLK = 32, BYTES = 24; };
template <> struct Fmt<GGML_Q8_0> { static constexpr int BLK = 32, BYTES = 34; };
template <> struct Fmt<GGML_Q4_K> { static constexpr int BLK = 256, BYTES = 144; };
template <> struct Fmt<GGML_Q5_K> { static constexpr int BLK = 256, BYTES = 176; };
template <> struct Fmt<GGML_Q6_K> { static constexpr int BLK = 256, BYTES = 210; };

// elements e0 .. e0 + 7 (e0 a multiple of 8) of the block that starts at byte `b` of the LDS tile
template <int TYPE>
APEXMI_DEVICE void unpack_block8(const uint32_t* lds, int b, int e0, float* y) {
    uint32_t lo, hi;
    if constexpr (TYPE == GGML_Q4_0 || TYPE == GGML_Q4_1) {
        // {f16 d; [f16 m;] u8 qs[16]}: y[j] = low nibble of qs[j], y[j + 16] = high nibble
        constexpr int QS = TYPE == GGML_Q4_0 ? 2 : 4;
        const float d = f16_bits_to_f32(lds_u16(lds, b));
        const float m = TYPE == GGML_Q4_1 ? f16_bits_to_f32(lds_u16(lds, b + 2)) : 0.f;
        lds_u64(lds, b + QS + (e0 & 15), lo, hi);
        const int sh = (e0 >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = (int)((byte_of(lo, hi, i) >> sh) & 15u);
            y[i] = TYPE == GGML_Q4_0 ? __fmul_rn((float)(q - 8), d) : __fadd_rn(__fmul_rn((float)q, d), m);
        }
    } else if constexpr (TYPE == GGML_Q5_0 || TYPE == GGML_Q5_1) {
        // {f16 d; [f16 m;] u32 qh; u8 qs[16]}: bit e of qh is the fifth bit of element e
        constexpr int QH = TYPE == GGML_Q5_0 ? 2 : 4;
        const float d = f16_bits_to_f32(lds_u16(lds, b));
        const float m = TYPE == GGML_Q5_1 ? f16_bits_to_f32(lds_u16(lds, b + 2)) : 0.f;
        const uint32_t qh = lds_u32(lds, b + QH) >> e0;
        lds_u64(lds, b + QH + 4 + (e0 & 15), lo, hi);
        const int sh = (e0 >> 4) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = (int)(((byte_of(lo, hi, i) >> sh) & 15u) | (((qh >> i) & 1u) << 4));
            y[i] = TYPE == GGML_Q5_0 ? __fmul_rn((float)(q - 16), d) : __fadd_rn(__fmul_rn((float)q, d), m);
        }
    } else if constexpr (TYPE == GGML_Q8_0) {
        const float d = f16_bits_to_f32(lds_u16(lds, b));
        lds_u64(lds, b + 2 + e0, lo, hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) y[i] = __fmul_rn((float)(int)(int8_t)byte_of(lo, hi, i), d);
    } else if constexpr (TYPE == GGML_Q4_K || TYPE == GGML_Q5_K) {
        // {f16 d; f16 dmin; u8 scales[12]; [u8 qh[32];] u8 qs[128]}: 4 groups of 64 = 32 low nibbles then 32 high nibbles
        constexpr int QS = TYPE == GGML_Q4_K ? 16 : 48;
        const float d = f16_bits_to_f32(lds_u16(lds, b)), dmin = f16_bits_to_f32(lds_u16(lds, b + 2));
        const int g = e0 >> 6, half = (e0 >> 5) & 1, l0 = e0 & 31, j = 2 * g + half;
        float sc, mn;
        scale_min_k4(lds, b + 4, j, sc, mn);
        const float d1 = __fmul_rn(d, sc), n1 = __fmul_rn(dmin, mn);
        lds_u64(lds, b + QS + 32 * g + l0, lo, hi);
        uint32_t hlo = 0u, hhi = 0u;
        if constexpr (TYPE == GGML_Q5_K) lds_u64(lds, b + 16 + l0, hlo, hhi);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t q = (byte_of(lo, hi, i) >> (4 * half)) & 15u;
            if constexpr (TYPE == GGML_Q5_K) q += ((byte_of(hlo, hhi, i) >> j) & 1u) << 4;
            y[i] = __fsub_rn(__fmul_rn(d1, (float)q), n1);
        }
    } else {
        // Q6_K {u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d}: two halves of 128 = 4 quarters of 32, one i8 scale per 16
        static_assert(TYPE == GGML_Q6_K, "unknown block type");
        const float d = f16_bits_to_f32(lds_u16(lds, b + 208));
        const int h = e0 >> 7, quarter = (e0 >> 5) & 3, l0 = e0 & 31;
        const float sc = (float)(int)(int8_t)lds_u8(lds, b + 192 + 8 * h + (l0 >> 4) + 2 * quarter);
        const float ds = __fmul_rn(d, sc);
        lds_u64(lds, b + 64 * h + l0 + 32 * (quarter & 1), lo, hi);
        uint32_t hlo, hhi;
        lds_u64(lds, b + 128 + 32 * h + l0, hlo, hhi);
        const int sh = (quarter >> 1) * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int q = (int)(((byte_of(lo, hi, i) >> sh) & 15u) | (((byte_of(hlo, hhi, i) >> (2 * quarter)) & 3u) << 4));
            y[i] = __fmul_rn(ds, (float)(q - 32));
        }
    }
}

template <int TYPE>
__global__ __launch_bounds__(256) void dequant_gguf_kernel(const uint8_t* __restrict__ blocks, int64_t total_bytes, int64_t total,
                                                           uint32_t K, bf16_t* __restrict__ out, int64_t ldo) {
    constexpr int BLK = Fmt<TYPE>::BLK, BYTES = Fmt<TYPE>::BYTES, TILE_BYTES = TILE / BLK * BYTES;
    static_assert(TILE_BYTES + 32 <= LDS_BYTES, "tile does not fit the LDS window");
    __shared__ __attribute__((aligned(16))) uint32_t lds[LDS_BYTES / 4];
    const int t = threadIdx.x;
    const int64_t tb0 = (int64_t)blockIdx.x * TILE_BYTES;                      // first byte of this tile in the block stream
    const int64_t tb1 = tb0 + TILE_BYTES < total_bytes ? tb0 + TILE_BYTES : total_bytes;
    const uintptr_t g0 = (uintptr_t)blocks + (uintptr_t)tb0;
    const int mis = (int)(g0 & 15);
    const uint8_t* ga = (const uint8_t*)(g0 - mis);                            // the aligned window starts here ...
    const int nchunk = (mis + (int)(tb1 - tb0) + 15) >> 4;                     // ... and has this many 16-byte pieces (<= 138)
    const uint8_t* lo_ok = blocks;
    const uint8_t* hi_ok = blocks + total_bytes;
    if (t < nchunk) {
        const uint8_t* p = ga + 16 * t;
        u32x4 v;
        if (p >= lo_ok && p + 16 <= hi_ok) {
            v = *(const u32x4*)p;
        } else {                                                               // window sticks out of the buffer: valid bytes only
            v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (p + i >= lo_ok && p + i < hi_ok) v[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
        }
        *(u32x4*)(lds + 4 * t) = v;
    }
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * TILE + t * 8;                      // flat element index of this lane's 8
    if (e >= total) return;
    const int64_t r0 = ((int64_t)blockIdx.x * TILE) / K;                       // uniform: row of the tile's first element
    const uint32_t rem = (uint32_t)((int64_t)blockIdx.x * TILE - r0 * K) + (uint32_t)t * 8;   // < K + TILE
    const uint32_t dr = rem / K, c = rem - dr * K;
    float y[8];
    const int te = t * 8;
    unpack_block8<TYPE>(lds, mis + (te / BLK) * BYTES, te % BLK, y);
    *(u32x4*)(out + (r0 + dr) * ldo + c) = pack8(y);
}

// F32 / F16 / BF16 "blocks" of one element: a plain conversion, 8 elements per lane (ragged tail and unaligned shapes per element)
template <int TYPE>
APEXMI_DEVICE float plain_elem(const uint8_t* src, int64_t i) {
    if constexpr (TYPE == GGML_F32) return ((const float*)src)[i];
    if constexpr (TYPE == GGML_F16) return f16_bits_to_f32(((const uint16_t*)src)[i]);
    return bf16_to_f32(((const bf16_t*)src)[i]);
}
template <int TYPE>
__global__ __launch_bounds__(256) void dequant_plain_kernel(const uint8_t* __restrict__ src, int64_t rows, int64_t K,
                                                            bf16_t* __restrict__ out, int64_t ldo, int vec) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        const int64_t nch = K >> 3;
        if (idx >= rows * nch) return;
        const int64_t r = idx / nch, c = (idx - r * nch) * 8;
        float y[8];
        if constexpr (TYPE == GGML_F32) {
            load8<float>((const float*)src + r * K + c, y);
        } else if constexpr (TYPE == GGML_F16) {
            const u32x4 v = *(const u32x4*)((const uint16_t*)src + r * K + c);
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = f16_bits_to_f32((v[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
        } else {
            *(u32x4*)(out + r * ldo + c) = *(const u32x4*)((const bf16_t*)src + r * K + c);
            return;
        }
        *(u32x4*)(out + r * ldo + c) = pack8(y);
    } else {
        if (idx >= rows * K) return;
        const int64_t r = idx / K, c = idx - r * K;
        out[r * ldo + c] = f32_to_bf16(plain_elem<TYPE>(src, r * K + c));
    }
}

template <int TYPE>
void launch_quant(const void* blocks, int64_t rows, int64_t K, void* out, int64_t ldo, hipStream_t stream) {
    const int64_t total = rows * K, total_bytes = total / Fmt<TYPE>::BLK * Fmt<TYPE>::BYTES;
    hipLaunchKernelGGL(dequant_gguf_kernel<TYPE>, dim3((unsigned)((total + TILE - 1) / TILE)), dim3(256), 0, stream,
                       (const uint8_t*)blocks, total_bytes, total, (uint32_t)K, (bf16_t*)out, ldo);
}
template <int TYPE>
void launch_plain(const void* src, int64_t rows, int64_t K, void* out, int64_t ldo, hipStream_t stream) {
    const int esz = TYPE == GGML_F32 ? 4 : 2;
    const int vec = (K % 8 == 0 && ldo % 8 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)out % 16 == 0 && (K * esz) % 16 == 0) ? 1 : 0;
    const int64_t n = vec ? rows * (K / 8) : rows * K;
    hipLaunchKernelGGL(dequant_plain_kernel<TYPE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const uint8_t*)src,
                       rows, K, (bf16_t*)out, ldo, vec);
}

}  // namespace

extern "C" int apexmi_dequant_gguf(const void* blocks, int ggml_type, int64_t rows, int64_t K, void* out, int64_t ldo,
                                   apexmi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    APEXMI_REQUIRE(blocks && out && rows > 0 && K > 0, "dequant_gguf: bad arguments");
    int blk = 0, bytes = 0;
    switch (ggml_type) {
        case GGML_F32: blk = 1, bytes = 4; break;
        case GGML_F16: case GGML_BF16: blk = 1, bytes = 2; break;
        case GGML_Q4_0: blk = 32, bytes = 18; break;
        case GGML_Q4_1: blk = 32, bytes = 20; break;
        case GGML_Q5_0: blk = 32, bytes = 22; break;
        case GGML_Q5_1: blk = 32, bytes = 24; break;
        case GGML_Q8_0: blk = 32, bytes = 34; break;
        case GGML_Q4_K: blk = 256, bytes = 144; break;
        case GGML_Q5_K: blk = 256, bytes = 176; break;
        case GGML_Q6_K: blk = 256, bytes = 210; break;
        default:
            APEXMI_REQUIRE(false, "dequant_gguf: ggml type %d is not supported (F32, F16, BF16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, "
                                  "Q5_K, Q6_K are)", ggml_type);
    }
    APEXMI_REQUIRE(K % blk == 0, "dequant_gguf: K=%lld is not a multiple of the block length %d of ggml type %d", (long long)K, blk,
                   ggml_type);
    APEXMI_REQUIRE(ldo >= K, "dequant_gguf: output row stride ldo=%lld is smaller than K=%lld", (long long)ldo, (long long)K);
    APEXMI_REQUIRE((uintptr_t)blocks % (blk == 1 ? bytes : 1) == 0, "dequant_gguf: misaligned source pointer");
    if (blk > 1)
        APEXMI_REQUIRE((uintptr_t)out % 16 == 0 && ldo % 8 == 0,
                       "dequant_gguf: misaligned output (needs a 16-byte aligned pointer and ldo %% 8 == 0, got ldo=%lld)", (long long)ldo);
    else
        APEXMI_REQUIRE((uintptr_t)out % 2 == 0, "dequant_gguf: misaligned output pointer");
    APEXMI_REQUIRE(rows <= (1LL << 40) / K && (rows * K + TILE - 1) / TILE < (1LL << 31) && K < (1LL << 31) - TILE,
                   "dequant_gguf: tensor too large");
    ApexmiProfScope prof(5, stream, 0.0, (double)rows * K * bytes / blk + 2.0 * rows * K);
    switch (ggml_type) {
        case GGML_F32: launch_plain<GGML_F32>(blocks, rows, K, out, ldo, stream); break;
        case GGML_F16: launch_plain<GGML_F16>(blocks, rows, K, out, ldo, stream); break;
        case GGML_BF16: launch_plain<GGML_BF16>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q4_0: launch_quant<GGML_Q4_0>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q4_1: launch_quant<GGML_Q4_1>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q5_0: launch_quant<GGML_Q5_0>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q5_1: launch_quant<GGML_Q5_1>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q8_0: launch_quant<GGML_Q8_0>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q4_K: launch_quant<GGML_Q4_K>(blocks, rows, K, out, ldo, stream); break;
        case GGML_Q5_K: launch_quant<GGML_Q5_K>(blocks, rows, K, out, ldo, stream); break;
        default: launch_quant<GGML_Q6_K>(blocks, rows, K, out, ldo, stream); break;
    }
    return apexmi_check_launch("dequant_gguf");
}
