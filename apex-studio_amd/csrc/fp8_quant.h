// Per-row e4m3 activation quantiser arithmetic, shared by apexmi_quant_rows_fp8 (gemm_fp8.hip) and the norm
// that quantises its own output (apexmi_ln_modulate_quant_fp8, elementwise.hip): both must produce the same codes from the same
// bf16 values, so the formula has one source.
#pragma once
#include "common.h"

namespace {

constexpr float FP8_MAX = 448.0f;        // largest finite e4m3fn value

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

}  // namespace
