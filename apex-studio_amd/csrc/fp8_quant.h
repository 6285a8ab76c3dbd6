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

}  // namespace
