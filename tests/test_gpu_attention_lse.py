"""The log-sum-exp output of the masked flash kernel and the merge over key chunks, on the GPU: exact counting
and membership probes (tests/attention_probes.py), random inputs against the float64 yardsticks of tests/attention_lse_ref.py
(proved on the CPU by tests/test_attention_lse_host.py), the merge kernel alone, and the plumbing.  Shapes: B 2, Hq 4, Hkv 2,
Sq 200 (a tail in the 128-row block), Sk 333 (a tail in the 64-key tile), D 64 and 128."""
import functools
import math

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import ops
from tests import attention_probes as P
from tests.attention_lse_ref import attention_ref, merge_ref
from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16 = torch.bfloat16, torch.float16
B, HQ, HKV, SQ, SK = 2, 4, 2, 200, 333
CUTS = ((0, 70), (70, 71), (71, 333))      # a one-key chunk, and cuts off the 64-key grid
COUNT_BAR = 1e-5                           # a handful of f32 roundings on values <= ln 1024; one key more or less moves >= 1 / 1024
LSE_CEILING = 4e-3                         # every probability carries at most one 2^-9 rounding: the sum is off by < 2^-8 relative


def _dev(t, layout="bhsd"):
    if t is None:
        return None
    if layout == "bshd":
        return t.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    return t.to(DEV)


def _check_lse_shape(lse, Bn, H, Sq):
    assert lse.shape == (Bn, H, Sq) and lse.dtype == torch.float32 and lse.is_contiguous()


def _count_check(name, lse, n):
    """lse against ln n for a probe whose probabilities are all exactly 1; -inf exactly where no key is allowed"""
    lse = lse.double().cpu()
    assert not torch.isnan(lse).any()
    dead = n == 0
    assert torch.equal(lse[dead], torch.full_like(lse[dead], float("-inf"))), f"{name}: a row without keys is not -inf"
    err = (lse[~dead] - torch.log(n[~dead])).abs().max().item() if bool((~dead).any()) else 0.0
    measured(f"lse count {name}", err, COUNT_BAR)


# ------------------------------------------------------------------------------------------------------ 1. counting probe
def _count_cases():
    c = {n: v for n, v in P.masked_cases().items() if v["mask"] is not None and v["mask"].dtype == torch.bool}
    for D, dtype, tag in ((128, BF, "bf16 D128"), (64, F16, "f16 D64")):
        c[f"causal gqa 4/2 {SQ}x{SK} {tag}"] = dict(B=B, Hq=HQ, Hkv=HKV, Sq=SQ, Sk=SK, D=D, dtype=dtype, mask=None, causal=True,
                                                    gqa=True, layout="bhsd")
        c[f"causal gqa 4/2 {SK}x{SQ} {tag}"] = dict(B=B, Hq=HQ, Hkv=HKV, Sq=SK, Sk=SQ, D=D, dtype=dtype, mask=None, causal=True,
                                                    gqa=True, layout="bhsd")
    return c


@pytest.mark.parametrize("name", list(_count_cases()))
def test_lse_counts_the_allowed_keys(name):
    c = _count_cases()[name]
    g = torch.Generator().manual_seed(1)
    q = _dev(torch.zeros(c["B"], c["Hq"], c["Sq"], c["D"], dtype=c["dtype"]), c["layout"])
    k = _dev(torch.randn(c["B"], c["Hkv"], c["Sk"], c["D"], generator=g).to(c["dtype"]), c["layout"])
    v = _dev(P.case_values(c), c["layout"])
    mask = _dev(c["mask"])
    kw = dict(is_causal=c["causal"], enable_gqa=c["gqa"])
    out, lse = ops.attention_masked(q, k, v, mask, return_lse=True, **kw)
    plain = ops.attention_masked(q, k, v, mask, **kw)
    torch.cuda.synchronize()
    _check_lse_shape(lse, c["B"], c["Hq"], c["Sq"])
    assert torch.equal(out, plain)
    _count_check(name, lse, P.case_weights(c).sum(-1))


# ------------------------------------------------------------------------------------------------------- 2. random inputs
MASK_KINDS = ("none", "bool", "additive f32", "causal")
FORMATS = ((BF, 128), (F16, 64), (BF, 64), (F16, 128))


@functools.lru_cache(maxsize=None)
def _random_case(dtype, D, kind):
    """q, k, v rounded to dtype, the mask, the rule's weights and the float64 reference of the rounded inputs (computed once)"""
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, HQ, SQ, D, generator=g).to(dtype)
    k = torch.randn(B, HKV, SK, D, generator=g).to(dtype)
    v = torch.randn(B, HKV, SK, D, generator=g).to(dtype)
    mask, causal = None, False
    if kind == "bool":
        mask = P._rand_bool((B, 1, SQ, SK), 12, 0.5)
        mask[:, :, [0, 127, 128, 199]] = False
    elif kind == "additive f32":
        mask = P._additive((1, HQ, SQ, SK), 13, torch.float32, dead_rows=(3, 128))
    elif kind == "causal":
        causal = True
    scale = 2.0 / math.sqrt(D)
    w = P.weights_of(mask, B, HQ, SQ, SK, causal)
    ref_o, ref_l = attention_ref(q, k, v, w, scale)
    smax = ((q.double() @ k.double().repeat_interleave(HQ // HKV, 1).transpose(2, 3)) * scale).abs().max().item()
    assert smax <= 16.0, smax
    return q, k, v, mask, causal, scale, w, ref_o, ref_l


# worst |lse - ref| over the live rows, per format: the bar is twice the worst value measured on the MI355X over the mask kinds, the
# single call and the chunked run.  The row sum is kept in f32 from unrounded probabilities, so the error is one to three f32 ulps of
# an lse of up to 10.4 (ulp 4.8e-7 below 8, 9.5e-7 above), far under the ceiling; a lost key, a wrong ln 2 digit or a rounded sum lands well above the bars.
LSE_BARS = {(BF, 128): 2.9e-6,     # measured 1.41e-6 (chunked, no mask); single call 1.28e-6 (bool)
            (F16, 64): 3.0e-6,     # measured 1.48e-6 (additive f32); chunked 1.33e-6
            (BF, 64): 2.4e-6,      # measured 1.18e-6 (bool)
            (F16, 128): 2.7e-6}    # measured 1.35e-6 (bool, additive f32)


def _lse_error(lse, ref_l):
    lse = lse.double().cpu()
    dead = torch.isinf(ref_l)
    assert not torch.isnan(lse).any()
    assert torch.equal(lse[dead], torch.full_like(lse[dead], float("-inf")))
    return (lse[~dead] - ref_l[~dead]).abs().max().item()


def _rel(out, ref):
    return float((out.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("dtype,D", FORMATS)
def test_lse_random_inputs(dtype, D, kind):
    q, k, v, mask, causal, scale, w, ref_o, ref_l = _random_case(dtype, D, kind)
    args = (_dev(q), _dev(k), _dev(v), _dev(mask))
    kw = dict(is_causal=causal, softmax_scale=scale, enable_gqa=True)
    out, lse = ops.attention_masked(*args, return_lse=True, **kw)
    plain = ops.attention_masked(*args, **kw)
    torch.cuda.synchronize()
    _check_lse_shape(lse, B, HQ, SQ)
    assert torch.equal(out, plain)
    err = _lse_error(lse, ref_l)
    name = f"lse random {'bf16' if dtype == BF else 'f16'} D{D} {kind}"
    print(f"{name}: worst |lse - ref| = {err:.3e}")
    assert err <= LSE_CEILING, (name, err)
    measured(name, err, LSE_BARS[(dtype, D)])


# ------------------------------------------------------------------------------------------- 3. merge through the probes
def _chunk_mask():
    """bool [B, 1, Sq, Sk]: rows without any key, and rows whose keys all sit in the first, the one-key or the last chunk"""
    m = P._rand_bool((B, 1, SQ, SK), 21, 0.5)
    m[:, :, [0, 127, 128, 199]] = False
    for r in (5, 64, 131):
        m[:, :, r, 70:] = False
    for r in (6, 129, 198):
        m[:, :, r] = False
        m[:, :, r, 70] = True
    for r in (7, 63, 130):
        m[:, :, r, :71] = False
    return m


def _chunked(q, k, v, mask, **kw):
    ks, vs = [k[:, :, a:b] for a, b in CUTS], [v[:, :, a:b] for a, b in CUTS]
    masks = None if mask is None else [mask[..., a:b] for a, b in CUTS]
    return ops.attention_chunked(q, ks, vs, masks, **kw)


@pytest.mark.parametrize("dtype,D", [(BF, 128), (F16, 64)])
def test_chunked_membership(dtype, D):
    mask = _chunk_mask()
    w = P.weights_of(mask, B, HQ, SQ, SK)
    n = w.sum(-1)
    per_chunk = torch.stack([w[..., a:b].sum(-1) for a, b in CUTS])
    assert bool((n == 0).any()) and all(bool(((per_chunk[i] == n) & (n > 0)).any()) for i in range(3))
    v = P.code_values(B, HKV, SK, D, dtype)
    g = torch.Generator().manual_seed(2)
    q = torch.zeros(B, HQ, SQ, D, dtype=dtype)
    k = torch.randn(B, HKV, SK, D, generator=g).to(dtype)
    out, lse = _chunked(_dev(q), _dev(k), _dev(v), _dev(mask), enable_gqa=True)
    torch.cuda.synchronize()
    assert out.shape == (B, HQ, SQ, D) and out.dtype == dtype
    _check_lse_shape(lse, B, HQ, SQ)
    assert not torch.isnan(out.float()).any()
    tag = f"chunked {'bf16' if dtype == BF else 'f16'} D{D}"
    ratio, zeros = P.membership_check(out.cpu(), P.membership_expected(w, v), dtype)
    assert zeros, f"{tag}: a non-zero where the expectation is an exact zero"
    measured(f"probe A {tag}", ratio, 1.0)
    assert P.membership_ok(out.cpu(), P.membership_expected(w, v), dtype)
    _count_check(tag, lse, n)


# ----------------------------------------------------------------------------------------- 4. merge on random inputs
@pytest.mark.parametrize("kind", ["none", "bool"])
@pytest.mark.parametrize("dtype,D", [(BF, 128), (F16, 64)])
def test_chunked_random_inputs(dtype, D, kind):
    q, k, v, mask, causal, scale, w, ref_o, ref_l = _random_case(dtype, D, kind)
    dq, dk, dv, dm = _dev(q), _dev(k), _dev(v), _dev(mask)
    single, single_lse = ops.attention_masked(dq, dk, dv, dm, softmax_scale=scale, enable_gqa=True, return_lse=True)
    out, lse = _chunked(dq, dk, dv, dm, softmax_scale=scale, enable_gqa=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    dead = torch.isinf(ref_l)
    assert torch.equal(out.cpu()[dead], torch.zeros_like(out.cpu()[dead]))
    name = f"chunked random {'bf16' if dtype == BF else 'f16'} D{D} {kind}"
    e_single, e_chunked = _rel(single, ref_o), _rel(out, ref_o)
    print(f"{name}: rel-L2 single {e_single:.3e}, chunked {e_chunked:.3e}, ratio {e_chunked / e_single:.3f}")
    measured(name, e_chunked, 1.5 * e_single)       # every partial out adds one rounding of the store dtype
    err = _lse_error(lse, ref_l)
    print(f"{name}: worst |lse - ref| = {err:.3e}")
    assert err <= LSE_CEILING
    measured(name + " lse", err, LSE_BARS[(dtype, D)])


# ------------------------------------------------------------------------------------------------ 5. the merge kernel alone
def _partials(n, dtype, D, seed):
    """n synthetic partials [2, 3, 77, D] (views of [B, Sq, H, D] buffers) and their lse, spread over +-80 with a few -inf, one
    row of them all -inf.  The partials of one output element share their sign: the f32 arithmetic is exact to ~n 2^-24 of
    sum_p w_p |o_p|, which is |ref| only without cancellation, and the bar below leaves room for the one rounding of the store."""
    Bn, H, Sq = 2, 3, 77
    g = torch.Generator().manual_seed(seed)
    sign = torch.where(torch.rand(Bn, Sq, H, D, generator=g) < 0.5, -1.0, 1.0)
    outs = [(torch.randn(Bn, Sq, H, D, generator=g).abs() * sign).to(dtype) for _ in range(n)]
    lses = [(torch.rand(Bn, H, Sq, generator=g) * 160.0 - 80.0) for _ in range(n)]
    for p, l in enumerate(lses):
        l[torch.rand(Bn, H, Sq, generator=g) < 0.1] = float("-inf")
        l[1, 2, 5 + p % 3] = float("-inf")
        l[0, 1, 7] = float("-inf")                                          # in every partial: a row without any key
    if n > 1:
        lses[1][0, 0, :8] = lses[0][0, 0, :8] + torch.linspace(-1, 1, 8)    # close weights too
    return [o.permute(0, 2, 1, 3) for o in outs], lses


@pytest.mark.parametrize("aliased", [False, True])
@pytest.mark.parametrize("n,dtype,D", [(1, BF, 64), (3, BF, 128), (8, BF, 64), (1, F16, 128), (3, F16, 40), (8, F16, 128)])
def test_merge_kernel_alone(n, dtype, D, aliased):
    outs, lses = _partials(n, dtype, D, 100 + n)
    ref_o, ref_l = merge_ref(outs, lses)
    d_outs, d_lses = [_dev(o, "bshd") for o in outs], [l.to(DEV) for l in lses]
    if n > 1:
        d_outs[1].masked_fill_((d_lses[1] == float("-inf"))[..., None], float("nan"))      # weight 0: whatever it holds
    out, lse = ops.attention_merge(d_outs, d_lses, out=d_outs[0] if aliased else None)
    torch.cuda.synchronize()
    assert (out.data_ptr() == d_outs[0].data_ptr()) == aliased
    assert out.shape == ref_o.shape and out.dtype == dtype and out.permute(0, 2, 1, 3).is_contiguous()
    _check_lse_shape(lse, *ref_l.shape)
    o, l = out.double().cpu(), lse.double().cpu()
    assert torch.isfinite(o).all() and not torch.isnan(l).any()
    dead = torch.isinf(ref_l)
    assert bool(dead.any()) and torch.equal(l[dead], ref_l[dead]) and torch.equal(o[dead], torch.zeros_like(o[dead]))
    assert bool(((o - ref_o).abs() <= P.U[dtype] * ref_o.abs() + 1e-30).all()), ((o - ref_o).abs() / ref_o.abs().clamp_min(1e-30)).max()
    assert bool(((l - ref_l)[~dead].abs() <= 1e-5 * ref_l[~dead].abs().clamp_min(1.0)).all())


# --------------------------------------------------------------------------------------------------------------- 6. plumbing
def test_backend_keyword_returns_the_same_pair():
    q, k, v, mask, causal, scale, *_ = _random_case(BF, 128, "bool")
    args = (_dev(q), _dev(k), _dev(v))
    a = ab.hip_mfma_sdpa(*args, attn_mask=_dev(mask), softmax_scale=scale, enable_gqa=True, return_lse=True)
    b = ops.attention_masked(*args, _dev(mask), softmax_scale=scale, enable_gqa=True, return_lse=True)
    plain = ab.hip_mfma_sdpa(*args, attn_mask=_dev(mask), softmax_scale=scale, enable_gqa=True)
    torch.cuda.synchronize()
    assert isinstance(a, tuple) and len(a) == 2 and torch.is_tensor(plain)
    assert torch.equal(a[0], b[0]) and torch.equal(a[0], plain)
    assert torch.equal(a[1], b[1]) and bool(torch.isinf(a[1]).any())


def test_permuted_bshd_views():
    q, k, v, mask, causal, scale, w, ref_o, ref_l = _random_case(F16, 64, "causal")
    kw = dict(is_causal=True, softmax_scale=scale, enable_gqa=True)
    a = ops.attention_masked(_dev(q, "bshd"), _dev(k, "bshd"), _dev(v, "bshd"), None, return_lse=True, **kw)
    b = ops.attention_masked(_dev(q), _dev(k), _dev(v), None, return_lse=True, **kw)
    c, c_lse = _chunked(_dev(q, "bshd"), _dev(k, "bshd"), _dev(v, "bshd"), _dev(P.causal_rule(SQ, SK)), softmax_scale=scale,
                        enable_gqa=True)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _check_lse_shape(a[1], B, HQ, SQ)
    assert _lse_error(a[1], ref_l) <= LSE_CEILING and _lse_error(c_lse, ref_l) <= LSE_CEILING
    assert _rel(c, ref_o) <= 1.5 * _rel(a[0], ref_o)


def test_no_host_sync():
    q, k, v, mask, causal, scale, *_ = _random_case(BF, 128, "bool")
    q, k, v, mask = _dev(q), _dev(k), _dev(v), _dev(mask)

    def run():
        a = ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, softmax_scale=scale, enable_gqa=True, return_lse=True)
        b = _chunked(q, k, v, mask, softmax_scale=scale, enable_gqa=True)
        c = ops.attention_merge([a[0], b[0]], [a[1], b[1]])
        return a, b, c

    run()                                          # workspace allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b, c = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(c[0].float()).all() and not torch.isnan(c[1]).any()
