"""The one route rule and the one grouped-list rule behind the opt-in low-precision GEMM routes (ops._block_gemm_route,
ops._grouped_problems), driven over a table and compared with a plain restatement written here; and that the public predicates
built on the rule — ops.fp8_compute_route, the problem rule of ops.fp8_lora_route, ops.mxfp4_route and ops.mxfp6_route — differ from
each other in exactly two places, three ways: the K multiple and the row-stride bound are (128, 2^22) for fp8, (256, none) for fp4
and (128, none) for fp6.  No GPU: meta tensors."""
import itertools

import torch

BF, F8 = torch.bfloat16, torch.float8_e4m3fn
BOUND = 1 << 22
EPIS = ("bias", "gelu", "gate_res")

A_DTYPES = (BF, torch.float32, torch.float16)
OUT_DTYPES = (None, BF, torch.float32)
KS = (64, 128, 192, 256, 384, 512)           # below 128; 128 and 384: multiples of 128 only; 256 and 512: of both; 192: of neither
NS = (32, 24)
EPILOGUES = ("bias", "gelu", "gate_res", "silu", "gelu_erf")
# name -> (shape, strides) of `a` for a given K
LAYOUTS = {
    "dense": lambda K: ((4, K), (K, 1)),
    "padded rows": lambda K: ((4, K), (K + 8, 1)),
    "rows off 16 bytes": lambda K: ((4, K), (K + 4, 1)),
    "stride at the bound": lambda K: ((2, K), (BOUND, 1)),
    "stride past the bound": lambda K: ((2, K), (BOUND + 8, 1)),
    "column major": lambda K: ((4, K), (1, 4)),
    "three dims": lambda K: ((1, 4, K), (4 * K, K, 1)),
    "one dim": lambda K: ((K,), (1,)),
    "no rows": lambda K: ((0, K), (K, 1)),
}


def _meta(shape, strides, dtype):
    return torch.empty_strided(shape, strides, dtype=dtype, device="meta")


def _want(a, w_shape, out, epilogue, k_mult, bound):
    """the rule, restated"""
    if a.dtype != BF:
        return False
    if out is not None and out.dtype != BF:
        return False
    if a.dim() != 2:
        return False
    if a.stride(1) != 1:
        return False
    if epilogue not in EPIS:
        return False
    M, K = a.shape
    N, Kw = w_shape
    if M < 1 or K != Kw or K % k_mult != 0 or N % 16 != 0:
        return False
    if a.stride(0) % 8 != 0:
        return False
    return bound is None or a.stride(0) <= bound


def _table():
    """(label, a, w_shape, out, epilogue): the full product of the factors, plus a K mismatch per K"""
    for dt, odt, K, N, epi, (lname, lay) in itertools.product(A_DTYPES, OUT_DTYPES, KS, NS, EPILOGUES, LAYOUTS.items()):
        a = _meta(*lay(K), dt)
        out = None if odt is None else _meta((a.shape[0] if a.dim() == 2 else 4, N), (N, 1), odt)
        yield f"a {dt} out {odt} K={K} N={N} {epi} {lname}", a, (N, K), out, epi
    for K in KS:
        yield f"K={K} against a record of K={K + 128}", _meta((4, K), (K, 1), BF), (32, K + 128), None, "bias"


def test_the_rule_against_its_restatement():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    seen = {True: 0, False: 0}
    for k_mult, bound in ((128, BOUND), (256, None), (256, BOUND), (128, None)):
        for label, a, w_shape, out, epi in _table():
            want = _want(a, w_shape, out, epi, k_mult, bound)
            assert ops._block_gemm_route(a, w_shape, out, epi, k_mult, bound) is want, (label, k_mult, bound)
            seen[want] += 1
    assert seen[True] > 100 and seen[False] > 100, seen


def _records(N, K):
    """an e4m3 record without factors, one with factors, and an fp4 and an fp6 record beside a bf16 weight, all [N, K] and switched on"""
    from apex_studio_amd import ops
    plain = ops.Fp8Weight(torch.zeros(N, K).to(F8), torch.ones(N))
    plain.compute = "fp8"
    lora = ops.Fp8Weight(torch.zeros(N, K).to(F8), torch.ones(N))
    lora.compute = lora.lora_compute = "fp8"
    lora.parts = [("lin", 0, N)]
    lora.set_lora([("lin", torch.zeros(4, K), torch.zeros(N, 4), 1.0)])
    fp4 = ops.Mxfp4Weight(torch.zeros(N, K // 2, dtype=torch.uint8), torch.full((N, K // 32), 127, dtype=torch.uint8))
    fp6 = ops.Mxfp6Weight(torch.zeros(N, K // 4 * 3, dtype=torch.uint8), torch.full((N, K // 32), 127, dtype=torch.uint8))
    return plain, lora, fp4, fp6


def test_the_three_public_predicates_differ_only_in_k_multiple_and_stride_bound():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    recs = {}
    differ = {"k": 0, "stride": 0, "6 from 8": 0, "6 from 4": 0}
    for label, a, (N, Kw), out, epi in _table():
        if (N, Kw) not in recs:
            recs[(N, Kw)] = _records(N, Kw)
        plain, lora, fp4, fp6 = recs[(N, Kw)]
        r8 = ops.fp8_compute_route(a, plain, out, epi)
        rl = ops._fp8_lora_problem_route(a, lora, out, epi)
        r4 = ops.mxfp4_route(a, fp4, out, epi)
        r6 = ops.mxfp6_route(a, fp6, out, epi)
        # each is its record test plus the one rule with its own two constants
        assert r8 is _want(a, (N, Kw), out, epi, 128, BOUND), label
        assert rl is r8, label
        assert r4 is _want(a, (N, Kw), out, epi, 256, None), label
        assert r6 is _want(a, (N, Kw), out, epi, 128, None), label
        if r8 != r4:
            k_only_128 = Kw % 128 == 0 and Kw % 256 != 0
            past = a.dim() == 2 and a.stride(0) > BOUND
            assert (r8 and k_only_128 and not past) or (r4 and past and not k_only_128), label
            differ["k" if r8 else "stride"] += 1
        # fp6 shares its K multiple with fp8 and its missing bound with fp4: it parts from fp8 only past the bound, and from fp4
        # only at a K that is a multiple of 128 alone
        if r6 != r8:
            assert r6 and a.dim() == 2 and a.stride(0) > BOUND, label
            differ["6 from 8"] += 1
        if r6 != r4:
            assert r6 and Kw % 128 == 0 and Kw % 256 != 0, label
            differ["6 from 4"] += 1
    assert all(n > 0 for n in differ.values()), differ
    # the record tests themselves: a record of the wrong kind, or switched off, never routes
    a = _meta((4, 256), (256, 1), BF)
    plain, lora, fp4, fp6 = _records(32, 256)
    assert ops.fp8_compute_route(a, plain) and ops._fp8_lora_problem_route(a, lora, None, "bias") and ops.mxfp4_route(a, fp4)
    assert ops.mxfp6_route(a, fp6)
    assert not ops.fp8_compute_route(a, lora) and not ops._fp8_lora_problem_route(a, plain, None, "bias")
    assert not ops.fp8_compute_route(a, fp4) and not ops.mxfp4_route(a, plain)
    assert not ops.mxfp6_route(a, fp4) and not ops.mxfp4_route(a, fp6) and not ops.mxfp6_route(a, plain) and not ops.fp8_compute_route(a, fp6)
    w = torch.empty(32, 256, dtype=BF, device="meta")
    w._fp6, w._fp4 = fp4, fp6                      # each record in the other format's slot
    assert not ops.mxfp6_route(a, w) and not ops.mxfp4_route(a, w)
    w._fp6, w._fp4 = fp6, fp4
    assert ops.mxfp6_route(a, w) and ops.mxfp4_route(a, w)
    plain.compute, lora.lora_compute, fp4.compute, fp6.compute = "bf16", "bf16", "bf16", "bf16"
    assert not ops.fp8_compute_route(a, plain) and not ops._fp8_lora_problem_route(a, lora, None, "bias") and not ops.mxfp4_route(a, fp4)
    assert not ops.mxfp6_route(a, fp6) and not ops.mxfp6_route(a, w) and not ops.mxfp4_route(a, w)


def _want_problems(a_list, w_list, out_list, epilogues):
    """the grouped-list rule, restated: None, or the problems"""
    n = len(a_list)
    if n < 1 or n > 4:
        return None
    if len(w_list) != n:
        return None
    epis = [epilogues for _ in range(n)] if isinstance(epilogues, str) else list(epilogues)
    outs = [None for _ in range(n)] if out_list is None else list(out_list)
    if len(epis) != n or len(outs) != n:
        return None
    if any(a.shape[-1] != a_list[0].shape[-1] for a in a_list):
        return None
    return [(a_list[i], w_list[i], outs[i], epis[i]) for i in range(n)]


def test_the_grouped_list_rule_and_both_grouped_predicates():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    plain, lora, _, _ = _records(32, 256)
    a = _meta((4, 256), (256, 1), BF)
    other_k = _meta((4, 128), (128, 1), BF)
    o = _meta((4, 32), (32, 1), BF)
    cases = []
    for n in (0, 1, 4, 5):
        for nw in {n, max(n - 1, 0), n + 1}:
            for epis in ("bias", ["gelu"] * n, ["bias"] * (n + 1), ["bias"] * max(n - 1, 0)):
                for outs in (None, [o] * n, [None] * n, [o] * (n + 1)):
                    cases.append(([a] * n, [plain] * nw, outs, epis))
    cases.append(([a, other_k], [plain, plain], None, "bias"))                     # K is not shared
    cases.append(([a, a, other_k, a], [plain] * 4, None, "bias"))
    cases.append(([a, a], [lora, plain], [o, None], ["bias", "gate_res"]))
    some = {True: 0, False: 0}
    for a_list, w_list, outs, epis in cases:
        want = _want_problems(a_list, w_list, outs, epis)
        got = ops._grouped_problems(a_list, w_list, outs, epis)
        assert (got is None) == (want is None), (len(a_list), len(w_list), outs, epis)
        some[want is not None] += 1
        if want is None:
            assert not ops.fp8_grouped_route(a_list, w_list, outs, epis) and not ops.fp8_grouped_lora_route(a_list, w_list, outs, epis)
            continue
        assert len(got) == len(want) and all(all(x is y for x, y in zip(g, w)) for g, w in zip(got, want))
        assert ops.fp8_grouped_route(a_list, w_list, outs, epis) is all(ops.fp8_compute_route(*p) for p in want)
        with_factors = [p for p in want if p[1].lora_A is not None]
        want_lora = bool(with_factors) and all(
            ops._fp8_lora_problem_route(p[0], p[1], p[2], p[3]) if p[1].lora_A is not None else ops.fp8_compute_route(*p) for p in want)
        assert ops.fp8_grouped_lora_route(a_list, w_list, outs, epis) is want_lora
    assert some[True] > 5 and some[False] > 20, some
    assert ops.fp8_grouped_lora_route([a, a], [lora, plain], [o, None], ["bias", "gelu"])
    assert ops.fp8_grouped_route([a] * 4, [plain] * 4) and not ops.fp8_grouped_route([a] * 5, [plain] * 5)
