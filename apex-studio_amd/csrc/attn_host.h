// Host-side front end of the one-launch flash entry points (attention_masked.hip, attention_varlen.hip, attention_wide.hip): the
// operand checks they share, the fill of the argument fields they share and the one launch sequence.  Host code only; nothing
// here reaches a kernel.
//
// A check takes the entry point's message prefix `who`, sets the error and returns 1 when it refuses (APEXMI_REQUIRE), 0 otherwise,
// so an entry point lists its checks in ITS order, `if (int rc = require_x(who, ...)) return rc;`, and a call with two faults
// reports the one that entry point has always reported.  The message texts are part of the contract
// (tests/test_attention_refusals_host.py holds every one of them); where entry points word the same refusal differently, the
// caller passes its wording.
#pragma once
#include "attn_tile.h"

#include <cmath>
#include <cstdint>

namespace {

// q / k / v / out and their stride arrays
inline int require_operands(const char* who, const void* q, const void* k, const void* v, const void* out, const int64_t* q_strides,
                            const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides) {
    APEXMI_REQUIRE(q && k && v && out && q_strides && k_strides && v_strides && o_strides, "%s: null operand", who);
    return 0;
}

// in-place reads take 16 bytes of a row at a time, the epilogue stores 8: nstrides = 3 (b, h, s) or 2 (packed: token, head)
inline int require_aligned(const char* who, const void* q, const void* k, const void* v, const void* out, const int64_t* q_strides,
                           const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, int nstrides) {
    bool aligned = ((uintptr_t)q % 16) == 0 && ((uintptr_t)k % 16) == 0 && ((uintptr_t)v % 16) == 0 && ((uintptr_t)out % 8) == 0;
    for (int i = 0; i < nstrides; ++i)
        aligned = aligned && q_strides[i] % 8 == 0 && k_strides[i] % 8 == 0 && v_strides[i] % 8 == 0 && o_strides[i] % 4 == 0;
    APEXMI_REQUIRE(aligned, "%s: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)", who);
    return 0;
}

inline int require_dtype(const char* who, int dtype) {
    APEXMI_REQUIRE(dtype == APEXMI_BF16 || dtype == APEXMI_F16, "%s: dtype %d unsupported (bf16 or f16)", who, dtype);
    return 0;
}

// `supported`: D is one of the kernel's head dims, `dims` names them in the message
inline int require_head_dim(const char* who, int D, bool supported, const char* dims) {
    APEXMI_REQUIRE(supported, "%s: head dim %d unsupported (%s)", who, D, dims);
    return 0;
}

inline int require_head_ratio(const char* who, int Hq, int Hkv) {
    APEXMI_REQUIRE(Hq % Hkv == 0, "%s: head ratio Hq=%d / Hkv=%d is not whole", who, Hq, Hkv);
    return 0;
}

// the optional lse output: f32 through its own strides.  `wanted` is the entry point's own rule (a separate entry point, or a
// non-null pointer), `wording` its own text.
inline int require_lse(const char* who, bool wanted, const float* lse, const int64_t* lse_strides, const char* wording) {
    APEXMI_REQUIRE(!wanted || (lse && lse_strides && ((uintptr_t)lse % 4) == 0), "%s: %s", who, wording);
    return 0;
}

// aligned16: the entry points that refuse a workspace off a 16-byte boundary say so in the message
inline int require_workspace(const char* who, const void* workspace, size_t workspace_bytes, size_t need, bool aligned16) {
    if (aligned16)
        APEXMI_REQUIRE(workspace && ((uintptr_t)workspace % 16) == 0 && workspace_bytes >= need,
                       "%s: workspace too small or misaligned (%zu < %zu)", who, workspace_bytes, need);
    else
        APEXMI_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    return 0;
}

// q / k / out and their element strides (b, h, s; out: b, s, h) of an args struct with the 4-D field names
template <typename A>
void set_qko(A& a, const void* q, const void* k, void* out, const int64_t* q_strides, const int64_t* k_strides,
             const int64_t* o_strides) {
    a.q = (const uint16_t*)q, a.k = (const uint16_t*)k, a.o = (uint16_t*)out;
    a.q_sb = q_strides[0], a.q_sh = q_strides[1], a.q_ss = q_strides[2];
    a.k_sb = k_strides[0], a.k_sh = k_strides[1], a.k_ss = k_strides[2];
    a.o_sb = o_strides[0], a.o_ss = o_strides[1], a.o_sh = o_strides[2];
}

// the kernels multiply by |scale| log2(e) and flip the sign of q for a negative scale
template <typename A>
void set_scale(A& a, float softmax_scale) {
    a.neg = softmax_scale < 0.0f;
    a.c = fabsf(softmax_scale) * LOG2E;
}

// Raise the kernel's dynamic-LDS limit to lds_attr once per device (one flag per kernel instantiation), launch it with `lds`
// bytes, and report a launch error under `what`.
template <auto Kernel, typename A>
int launch_flash(dim3 grid, dim3 block, int lds_attr, int lds, hipStream_t stream, const A& args, const char* what) {
    static uint64_t attr_done = 0;
    APEXMI_SET_ATTR_ONCE(attr_done,
                         (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr));
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args);
    return apexmi_check_launch(what);
}

}  // namespace
