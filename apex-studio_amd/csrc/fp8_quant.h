// Per-row e4m3 activation quantiser arithmetic, shared by apexmi_quant_rows_fp8 (gemm_fp8.hip) and the norm
// that quantises its own output (apexmi_ln_modulate_quant_fp8, elementwise.hip): both must produce the same codes from the same
// bf16 values, so the formula has one source.
#pragma once
#include "common.h"

namespace {

constexpr float FP8_MAX = 448.0f;        // largest finite e4m3fn value

// max |x| over 16 bf16 values (8 dwords): what one lane of every quantiser here holds per step
APEXMI_DEVICE float absmax16(const u32x4 a, const u32x4 b) {
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m = fmaxf(m, fmaxf(fabsf(bf16_lo(a[i])), fabsf(bf16_hi(a[i]))));
        m = fmaxf(m, fmaxf(fabsf(bf16_lo(b[i])), fabsf(bf16_hi(b[i]))));
    }
    return m;
}

APEXMI_DEVICE float quant1(float x, float scale) {
    const float y = __fdiv_rn(x, scale);
    return fminf(fmaxf(y, -FP8_MAX), FP8_MAX);
}

// 4 bf16 (2 dwords) -> 4 e4m3fn codes in one dword (v_cvt_pk_fp8_f32: OCP e4m3fn on gfx950, round to nearest even)
APEXMI_DEVICE uint32_t quant4(uint32_t lo, uint32_t hi, float scale) {
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(quant1(bf16_lo(lo), scale), quant1(bf16_hi(lo), scale), r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(quant1(bf16_lo(hi), scale), quant1(bf16_hi(hi), scale), r, true);
    return (uint32_t)r;
}

// ---- MX block quantiser (apexmi_quant_blocks_mxfp8 and the MX output of apexmi_gemm_fp8_mx, gemm_fp8.hip) -----------------------
// A block = 32 consecutive bf16 values of one row, aligned to 32 columns.  amax = max |x| with unbiased f32 exponent E and mantissa
// man:  e = clamp(E - 8 + (man > 0x600000), -126, 127)  (448 = 1.75 x 2^8: the smallest 2^e with amax / 2^e <= 448; 0 for a zero
// block), the scale byte is e + 127 (e8m0; 127 for a zero block, never 255), code = e4m3fn_rne(clamp(x * 2^-e, -448, 448)).  The
// factor 2^-e is built from exponent bits: bf16 inputs give e <= 120, so 127 - e is a normal exponent field.
APEXMI_DEVICE int mx_scale_byte(float amax) {
    const uint32_t b = __float_as_uint(amax) & 0x7fffffffu;
    if (b == 0u) return 127;
    const int e = (int)(b >> 23) - 127 - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);
    return min(max(e, -126), 127) + 127;
}

APEXMI_DEVICE float mx_inv_scale(int scale_byte) { return __uint_as_float((uint32_t)(254 - scale_byte) << 23); }

APEXMI_DEVICE float mx_quant1(float x, float inv) { return fminf(fmaxf(x * inv, -FP8_MAX), FP8_MAX); }

// 4 f32 values (bf16-exact) -> 4 codes in one dword
APEXMI_DEVICE uint32_t mx_quant4f(float a, float b, float c, float d, float inv) {
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(mx_quant1(a, inv), mx_quant1(b, inv), r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(mx_quant1(c, inv), mx_quant1(d, inv), r, true);
    return (uint32_t)r;
}

APEXMI_DEVICE uint32_t mx_quant4(uint32_t lo, uint32_t hi, float inv) {
    return mx_quant4f(bf16_lo(lo), bf16_hi(lo), bf16_lo(hi), bf16_hi(hi), inv);
}

// ---- MXFP4 block quantiser (apexmi_quant_blocks_mxfp4, gemm_mxfp4.hip) -----------------------------------------------------------
// The same block of 32 bf16 values and the same e8m0 scale byte, for OCP e2m1 codes: bit 3 = sign, the low three bits index the
// magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6.  e = clamp(E - 2 + (man > 0x400000), -126, 127)  (6 = 1.5 x 2^2: the smallest 2^e with
// amax / 2^e <= 6; 0 for a zero block), scale byte = e + 127, code = e2m1_rne(clamp(x * 2^-e, -6, 6)): round to nearest, ties to the
// even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4).  The sign bit of x is KEPT, also where the
// magnitude rounds to zero (-0.1 -> code 8 = -0).  The rounding is done in VALU arithmetic, not by v_cvt_scalef32_pk_fp4_f32:
// that instruction's tie rule, saturation and sign of zero have not been checked against this definition, and the quantiser is a
// streaming pass with VALU time to spare.  bf16 inputs give e <= 126, so 2^-e (mx_inv_scale) is a normal float.
APEXMI_DEVICE int mx4_scale_byte(float amax) {
    const uint32_t b = __float_as_uint(amax) & 0x7fffffffu;
    if (b == 0u) return 127;
    const int e = (int)(b >> 23) - 127 - 2 + ((b & 0x7fffffu) > 0x400000u ? 1 : 0);
    return min(max(e, -126), 127) + 127;
}

// one value -> its e2m1 code (4 bits).  y = min(|x| 2^-e, 6) is exact (a power-of-two factor).  y >= 1: the code is the float's
// exponent and top mantissa bit after rounding the other 22 mantissa bits to nearest even (1.0 = exponent field 127 -> code 2);
// y < 1: the grid is 0, 0.5, 1 and y + 2^22 rounds to nearest-even halves, its two lowest mantissa bits are the code.
APEXMI_DEVICE uint32_t mx4_code(float x, float inv) {
    const float y = fminf(fabsf(x) * inv, 6.0f);
    const uint32_t b = __float_as_uint(y);
    const uint32_t normal = ((b + 0x1fffffu + ((b >> 22) & 1u)) >> 22) - 252u;
    const uint32_t sub = __float_as_uint(y + 4194304.0f) & 3u;
    return (y < 1.0f ? sub : normal) | ((__float_as_uint(x) >> 28) & 8u);
}

// 8 bf16 (4 dwords) -> 8 codes in one dword: byte j holds code[2 j] | code[2 j + 1] << 4 (torch's float4_e2m1fn_x2 packing)
APEXMI_DEVICE uint32_t mx4_quant8(const u32x4 v, float inv) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) r |= (mx4_code(bf16_lo(v[i]), inv) | (mx4_code(bf16_hi(v[i]), inv) << 4)) << (8 * i);
    return r;
}

// 4 / 8 f32 values (bf16-exact) -> their codes, packed as mx4_quant8 packs them: the norm that quantises its own output
// (apexmi_ln_modulate_quant_mxfp4) and the MX output of apexmi_gemm_mxfp4_mx hold the rounded values unpacked
APEXMI_DEVICE uint32_t mx4_quant4f(float a, float b, float c, float d, float inv) {
    return mx4_code(a, inv) | mx4_code(b, inv) << 4 | mx4_code(c, inv) << 8 | mx4_code(d, inv) << 12;
}

APEXMI_DEVICE uint32_t mx4_quant8f(const float* f, float inv) {
    return mx4_quant4f(f[0], f[1], f[2], f[3], inv) | mx4_quant4f(f[4], f[5], f[6], f[7], inv) << 16;
}

// ---- MXFP6 block quantiser (apexmi_quant_blocks_mxfp6, gemm_mxfp6.hip) -----------------------------------------------------------
// The same block of 32 bf16 values and the same e8m0 scale byte, for OCP e2m3 codes: sign << 5 | exp << 3 | man, bias 1; exp = 0 is
// man / 8, otherwise (1 + man / 8) 2^(exp - 1): 0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5.  e = clamp(E - 2 + (man >
// 0x700000), -126, 127)  (7.5 = 1.875 x 2^2: the smallest 2^e with amax / 2^e <= 7.5; 0 for a zero block), scale byte = e + 127,
// code = e2m3_rne(clamp(x * 2^-e, -7.5, 7.5)): round to nearest, ties to the even code; the sign bit of x is KEPT, also on a zero
// magnitude.  VALU arithmetic as mx4_code, not v_cvt_scalef32_pk32_fp6_bf16: that instruction's tie rule, saturation and sign of
// zero have not been checked against this definition.
APEXMI_DEVICE int mx6_scale_byte(float amax) {
    const uint32_t b = __float_as_uint(amax) & 0x7fffffffu;
    if (b == 0u) return 127;
    const int e = (int)(b >> 23) - 127 - 2 + ((b & 0x7fffffu) > 0x700000u ? 1 : 0);
    return min(max(e, -126), 127) + 127;
}

// one value -> its e2m3 code (6 bits).  y = min(|x| 2^-e, 7.5) is exact.  y >= 1: the low five code bits are the float's exponent
// and top three mantissa bits after rounding the other 20 to nearest even (1.0 = exponent field 127 -> exp 1, man 0 = 8; a carry
// out of the mantissa moves into the exponent, as it must); y < 1: the grid is k / 8, and y + 2^20 (ulp 2^-3) rounds to nearest-even
// eighths, its four lowest mantissa bits are the code (8 / 8 = code 8 = 1.0).
APEXMI_DEVICE uint32_t mx6_code(float x, float inv) {
    const float y = fminf(fabsf(x) * inv, 7.5f);
    const uint32_t b = __float_as_uint(y);
    const uint32_t normal = ((b + 0x7ffffu + ((b >> 20) & 1u)) >> 20) - 1008u;
    const uint32_t sub = __float_as_uint(y + 1048576.0f) & 15u;
    return (y < 1.0f ? sub : normal) | ((__float_as_uint(x) >> 26) & 32u);
}

// 16 bf16 (8 dwords) -> 16 codes in three dwords: code j in bits 6 j .. 6 j + 5 of the 96-bit little-endian integer, half of a
// block's 24 bytes
APEXMI_DEVICE void mx6_quant16(const u32x4 v0, const u32x4 v1, float inv, uint32_t (&out)[3]) {
    uint32_t c[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = mx6_code(bf16_lo(v0[i]), inv), c[2 * i + 1] = mx6_code(bf16_hi(v0[i]), inv);
        c[8 + 2 * i] = mx6_code(bf16_lo(v1[i]), inv), c[9 + 2 * i] = mx6_code(bf16_hi(v1[i]), inv);
    }
    out[0] = c[0] | c[1] << 6 | c[2] << 12 | c[3] << 18 | c[4] << 24 | c[5] << 30;
    out[1] = c[5] >> 2 | c[6] << 4 | c[7] << 10 | c[8] << 16 | c[9] << 22 | c[10] << 28;
    out[2] = c[10] >> 4 | c[11] << 2 | c[12] << 8 | c[13] << 14 | c[14] << 20 | c[15] << 26;
}

}  // namespace
