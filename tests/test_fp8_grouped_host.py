"""Host-side checks of the grouped fp8 GEMM: the pure routing predicate `ops.fp8_grouped_route`, the tile ->
problem lookup of the grouped `gemm_fp8_kernel` (`fp8_problem`) restated in Python (`ops.fp8_grouped_tiles`) against a brute-force cover, and the two
exported names in the header and in `lib.SIGNATURES`.  No GPU."""
import os

import pytest
import torch

F8 = torch.float8_e4m3fn
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _weight(N, K, compute="fp8", dtype=F8):
    ops = _ops()
    w = ops.Fp8Weight(torch.zeros(N, K).to(dtype), torch.ones(N))
    w.compute = compute
    return w


def _problem(M=200, N=144, K=256, out_dtype=torch.bfloat16, **kw):
    return torch.zeros(M, K, dtype=torch.bfloat16), _weight(N, K, **kw), torch.zeros(M, N, dtype=out_dtype)


def _route(problems, epilogues="bias"):
    a, w, o = zip(*problems)
    return _ops().fp8_grouped_route(list(a), list(w), list(o), epilogues)


def test_route_is_true_only_when_every_problem_routes():
    ops = _ops()
    good = [_problem(200), _problem(72)]
    assert _route(good) and _route(good, ["bias", "gelu"]) and _route(good, ["gate_res", "gate_res"])
    assert _route([_problem(4608, 9216, 3072), _problem(4608, 12288, 3072)], ["bias", "gelu"])
    assert ops.fp8_grouped_route([p[0] for p in good], [p[1] for p in good]), "out_list is optional"
    for p in good:
        assert ops.fp8_compute_route(*p)
    assert not _route([good[0], _problem(72, compute="bf16")]), "one bf16-compute record"
    assert not _route([_problem(72, compute="bf16"), good[0]])
    assert not _route([good[0], _problem(72, out_dtype=torch.float32)]), "a float out (the f32 residual stream)"
    assert not _route([_problem(200, K=192), _problem(72, K=192)]), "K % 128 != 0"
    lora = _problem(72)
    lora[1].lora_A, lora[1].lora_B = torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(144, 64, dtype=torch.bfloat16)
    assert not _route([good[0], lora]), "a record with LoRA factors"
    assert not _route([good[0], _problem(72, dtype=torch.float8_e5m2)]), "an e5m2 record"
    assert not _route([good[0], _problem(72, N=152)]), "N % 16 != 0"
    assert not _route([good[0], _problem(72, K=384)]), "the problems share K"
    assert not _route(good, ["bias", "silu"]), "an epilogue the fp8 kernel does not have"
    assert not _route([_problem(8)] * 5), "at most 4 problems"
    assert not ops.fp8_grouped_route([], [])
    plain = (good[1][0], torch.zeros(144, 256, dtype=torch.bfloat16), good[1][2])
    assert not _route([good[0], plain]), "a bf16 weight"


@pytest.mark.parametrize("shapes", [[(200, 144), (72, 144)], [(1160, 768), (1160, 1024)], [(1, 16)]],
                         ids=["ragged", "past-one-band", "one-tile"])
def test_every_tile_of_every_problem_runs_exactly_once(shapes):
    """(200, 144) + (72, 144): ragged M, N % 128 != 0.  (1160, 768) + (1160, 1024): 1160 = 9 x 128 + 8 rows, nine full tile rows
    and one of 8 rows, so each problem spans a band boundary of 8 tile rows and ends in a part-filled band."""
    ops = _ops()
    cover = sorted((p, tm, tn) for p, (M, N) in enumerate(shapes) for tm in range(-(-M // 128)) for tn in range(-(-N // 128)))
    got = ops.fp8_grouped_tiles(shapes)
    assert len(got) == len(cover) and sorted(got) == cover
    if shapes[0][0] == 1160:
        assert len(cover) == 10 * 6 + 10 * 8 and {tm for _, tm, _ in got} == set(range(10))


def test_exported_names_in_the_header_and_the_signatures():
    from apex_studio_amd import lib
    header = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    for name, nargs in (("apexmi_gemm_fp8_grouped", 20), ("apexmi_gemm_fp8_grouped_qkv", 32)):
        assert f"int {name}(" in header
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs


def test_both_entry_forms_word_a_refusal_the_same_and_the_grouped_one_names_the_problem():
    """One validation routine serves the single and the grouped entry points: the same wrong argument is refused with the same
    sentence, the grouped form adding which problem.  Dummy (never dereferenced) pointers; every call is refused before a launch."""
    import ctypes as C
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000

    def single(M=1, N=16, K=128, fmt=0, epi=lib.EPI_BIAS, nsw=1, lda=128):
        assert L.apexmi_gemm_fp8(P, lda, P, P, K, fmt, P, nsw, None, P, N, M, N, K, epi, None, None, 0, None) != 0
        return L.apexmi_last_error().decode()

    def grouped(M=1, N=16, K=128, fmt=0, epi=lib.EPI_BIAS, nsw=1, lda=128):
        """two problems, the second one wrong"""
        VP, I64, INT = C.c_void_p * 2, C.c_int64 * 2, C.c_int * 2
        rc = L.apexmi_gemm_fp8_grouped(2, VP(P, P), I64(K, lda), VP(P, P), VP(P, P), I64(K, K), INT(0, fmt), VP(P, P), I64(1, nsw),
                                       VP(None, None), VP(P, P), I64(16, N), INT(1, M), INT(16, N), K, INT(lib.EPI_BIAS, epi),
                                       VP(None, None), VP(None, None), I64(0, 0), None)
        assert rc != 0
        return L.apexmi_last_error().decode()

    assert single(M=0) == "gemm_fp8: M=0 must be at least 1"
    assert grouped(M=0) == "gemm_fp8_grouped: M=0 of problem 1 must be at least 1"
    assert single(N=24) == "gemm_fp8: N=24 must be a multiple of 16"
    assert grouped(N=24) == "gemm_fp8_grouped: N=24 of problem 1 must be a multiple of 16"
    assert single(fmt=1) == ("gemm_fp8: weight format 1 is not e4m3fn (0): e5m2 weights take the bf16 path "
                             "(apexmi_dequant_fp8_scaled + apexmi_gemm_bf16)")
    assert grouped(fmt=1) == ("gemm_fp8_grouped: weight format 1 of problem 1 is not e4m3fn (0): e5m2 weights take the bf16 path "
                              "(apexmi_dequant_fp8_scaled + apexmi_gemm_bf16_grouped)")
    assert single(epi=lib.EPI_BIAS_F32) == (f"gemm_fp8: f32 output (epilogue {lib.EPI_BIAS_F32}, the f32 residual stream) is not "
                                            "supported: the output is bf16")
    assert grouped(epi=lib.EPI_BIAS_F32) == (f"gemm_fp8_grouped: f32 output (epilogue {lib.EPI_BIAS_F32} of problem 1, the f32 residual "
                                             "stream) is not supported: the output is bf16")
    assert single(nsw=3) == "gemm_fp8: the weight scale has 3 values for N=16 rows"
    assert grouped(nsw=3) == "gemm_fp8_grouped: the weight scale of problem 1 has 3 values for N=16 rows"
    assert single(lda=136) == "gemm_fp8: leading dimensions must keep rows 16-byte aligned (lda 136, ldw 128, ldc 16)"
    assert grouped(lda=136) == "gemm_fp8_grouped: leading dimensions must keep rows 16-byte aligned (problem 1: lda 136, ldw 128, ldc 16)"
    assert single(K=100) == "gemm_fp8: K=100 must be a multiple of 128"
    assert grouped(K=100) == "gemm_fp8_grouped: K=100 must be a multiple of 128"


def test_preflight_refuses_a_fused_tensor_with_one_scale():
    """What a BFL-format fp8 file gives after key conversion: q / k / v rows of one tensor and a single scale between them"""
    from apex_studio_amd import lib
    from apex_studio_amd.flux import FluxTransformer2DModel as F
    base = "transformer_blocks.0.attn."
    ok = [f"{base}{n}.{s}" for n in ("to_q", "to_k", "to_v", "to_out.0") for s in ("weight", "scale_weight")]
    F._fp8_preflight(ok)
    with pytest.raises(lib.ApexMIError, match="BFL-format"):
        F._fp8_preflight([k for k in ok if k not in (f"{base}to_k.scale_weight", f"{base}to_v.scale_weight")])
    with pytest.raises(NotImplementedError, match="no fp8-scaled block Linear"):
        F._fp8_preflight(["blocks.0.attn1.to_q.weight", "blocks.0.attn1.to_q.scale_weight", f"{base}to_q.weight"])
