"""Probe C, "graded weights", on the GPU: +-1 operands whose scores are exact integers, a float64 reference from the definition and
the derived bars (m u + e_s) |ref| and e_l of tests/attention_weight_probes.py, which also says which entry gets m = 2 and which 3;
tests/test_attention_weight_probes_host.py proves that the verdicts reject single wrong decisions.  Every case reports its worst
elementwise ratio to the bar through measured(name, ratio, 1.0): the bar is the derivation's, not a measurement
(profiles/attn_weight_probes_measured.jsonl holds the MI355X values)."""
import functools

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from tests import attention_probes as P
from tests import attention_weight_probes as W
from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16 = torch.bfloat16, torch.float16
PAD = 512.0      # planted in the V^T columns past Sk of the prepared layouts: a padded key let through is visibly wrong


def _dev(t, layout="bhsd"):
    if layout == "bshd":
        return t.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    return t.to(DEV)


def _verdict(name, tag, out, lse=None, merged=None):
    """out [B, Hq, Sq, D] (and lse [B, Hq, Sq]) of problem `name` against its float64 reference"""
    p = W.problems()[name]
    ref, ref_lse = W.reference(name)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype == p["dtype"]
    ratio, zeros = W.out_ratio(out.cpu(), ref, W.out_bar(p, merged=merged))
    print(f"probe C {tag}: worst |out - ref| / bar = {ratio:.3f}")
    assert zeros, f"{tag}: a non-zero where the reference is an exact zero"
    if lse is not None:
        assert tuple(lse.shape) == tuple(ref_lse.shape) and lse.dtype == torch.float32
        lr = W.lse_ratio(lse.cpu(), ref_lse, W.lse_bar(p, merged))
        print(f"probe C lse {tag}: worst |lse - ref| / e_l = {lr:.3f}")
    measured(f"probe C {tag}", ratio, 1.0)
    if lse is not None:
        measured(f"probe C lse {tag}", lr, 1.0)


def _sentinel(*shape, dtype=BF):
    return torch.full(shape, W.SENTINEL, dtype=dtype, device=DEV)


def _prepared(k, v, pad=PAD):
    """k [B,H,Sk,128] contiguous and V^T [B,H,128,Skp] with `pad` in the columns past Sk"""
    B, H, Sk, D = v.shape
    vt = torch.full((B, H, D, (Sk + 63) // 64 * 64), pad, dtype=v.dtype)
    vt[..., :Sk] = v.transpose(2, 3)
    return k.contiguous().to(DEV), vt.to(DEV)


def _scale_kw(p, key="softmax_scale"):
    return {} if p["scale"] is None else {key: p["scale"]}


# --------------------------------------------------------------------------------- ops.attention / ops.attention_prepared (no mask)
def _plain(name, tag, prepared=False):
    p = W.problems()[name]
    q, k, v = W.inputs(name)
    if prepared:
        out = _sentinel(p["B"], p["Sq"], p["Hq"], 128)
        kd, vt = _prepared(k, v)
        ops.attention_prepared(q.to(DEV), kd, vt, out, p["Sk"], **_scale_kw(p, "scale"))
        out = out.permute(0, 2, 1, 3)
    else:
        out = ops.attention(q.to(DEV), k.to(DEV), v.to(DEV), **_scale_kw(p))
    _verdict(name, ("attention_prepared " if prepared else "attention ") + tag, out)


def _shape_name(s):
    return "plain " + "x".join(map(str, s))


@pytest.mark.parametrize("name", [_shape_name(s) for s in P.UNMASKED_SHAPES["default"]] +
                         ["plain 1x3x129x65 scale 0.125", "plain 2x2x333x1000 scale 0.125", "staged 1x2x200x333"])
def test_attention_default_launch(name):
    _plain(name, name)
    _plain(name, name, prepared=True)


@pytest.mark.parametrize("mfma", [16, 32])
@pytest.mark.parametrize("waves", [4, 5, 6, 7, 8])
def test_attention_workgroup_sizes(waves, mfma):
    lib.tune_set("attn.waves", waves)
    lib.tune_set("attn.mfma", mfma)
    try:
        _plain(_shape_name(W.RAGGED), f"waves={waves} mfma={mfma} {_shape_name(W.RAGGED)}")
        _plain(_shape_name(W.RAGGED), f"waves={waves} mfma={mfma} {_shape_name(W.RAGGED)}", prepared=True)
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.mfma", 32)


@pytest.mark.parametrize("c4", [1, 3, 4, 8])
def test_attention_four_cluster_variants(c4):
    lib.tune_set("attn.waves", 8)
    lib.tune_set("attn.c4", c4)
    lib.tune_set("attn.w64", 0)
    try:
        a, b = P.UNMASKED_SHAPES["c4"]
        _plain(_shape_name(a), f"c4={c4} {_shape_name(a)}")
        _plain(_shape_name(b), f"c4={c4} {_shape_name(b)}", prepared=True)
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.c4", 3)
        lib.tune_set("attn.w64", 1)


@pytest.mark.parametrize("w64", [1, 8])
def test_attention_w64_forced(w64):
    """w64 = 1 is the shipped first-tile-maximum loop: the exponents of a row spread over less than 40 binades (host condition),
    so no workgroup may take the running-maximum pass; w64 = 8 is the running-maximum form itself"""
    lib.tune_set("attn.waves", 8)
    lib.tune_set("attn.w64", w64)
    try:
        lib.attn_w64_fallbacks()
        a, b = P.UNMASKED_SHAPES["w64"]
        _plain(_shape_name(a), f"w64={w64} {_shape_name(a)}")
        _plain(_shape_name(b), f"w64={w64} {_shape_name(b)}", prepared=True)
        if w64 == 1:
            assert lib.attn_w64_fallbacks() == 0
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.w64", 1)


def test_attention_tail_split():
    a, b = P.UNMASKED_SHAPES["tail"]
    for B, H, Sq, Sk in (a, b):
        assert lib.load().apexmi_attn_prepared_workspace_bytes(B, H, Sq, Sk) > 0           # the split is taken
    _plain(_shape_name(a), "tail split " + _shape_name(a))
    _plain(_shape_name(b), "tail split " + _shape_name(b), prepared=True)


@pytest.mark.parametrize("dtype", [BF, F16])
@pytest.mark.parametrize("D", [40, 64, 192, 320])
def test_attention_other_head_dims(D, dtype):
    name = f"head dim {D} {'bf16' if dtype == BF else 'f16'} 1x2x129x200"
    _plain(name, name)


# ------------------------------------------------------------------------------------- ops.attention_masked / hip_mfma_sdpa
MASKED = [n for n, p in W.problems().items() if n.startswith("masked ")]


@pytest.mark.parametrize("n,name", list(enumerate(MASKED)))
def test_masked_with_lse(n, name):
    p = W.problems()[name]
    layout = P.masked_cases()[p["case"]]["layout"] if "case" in p else "bhsd"
    gqa = P.masked_cases()[p["case"]]["gqa"] if "case" in p else False
    q, k, v = (_dev(t, layout) for t in W.inputs(name))
    mask = None if p["mask"] is None else p["mask"].to(DEV)
    kw = dict(is_causal=p["causal"], enable_gqa=gqa, return_lse=True, **_scale_kw(p))
    if n % 2:       # the backend entry forwards to the same operator: alternate the two over the cases
        out, lse = ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, **kw)
    else:
        out, lse = ops.attention_masked(q, k, v, mask, **kw)
    _verdict(name, name, out, lse)


# ---------------------------------------------------------------------------------------------------------- coordinate windows
@functools.lru_cache(maxsize=None)
def _window_plan(case):
    cq, ck, radius, _ = P.window_case(case)
    return ops.window_plan(cq.to(DEV), None if ck is None else ck.to(DEV), radius=radius)


@pytest.mark.parametrize("name", [n for n in W.problems() if n.startswith("window ")])
def test_window(name):
    p = W.problems()[name]
    q, k, v = W.inputs(name)
    out = ops.attention_window(q.to(DEV), k.to(DEV), v.to(DEV), _window_plan(p["window"]))
    _verdict(name, name, out)


@pytest.mark.parametrize("name", [n for n in W.problems() if n.startswith("prepared window ")])
def test_prepared_window(name):
    p = W.problems()[name]
    q, k, v = W.inputs(name)
    kd, vt = _prepared(k, v)
    out = _sentinel(p["B"], p["Sq"], p["Hq"], 128)
    ops.attention_prepared_window(q.to(DEV), kd, vt, out, p["Sk"], _window_plan(p["window"]))
    _verdict(name, name, out.permute(0, 2, 1, 3))


# ------------------------------------------------------------------------------------------------------------- per-block key bands
@pytest.mark.parametrize("plan", list(W.BAND_PLANS))
def test_band(plan):
    name = "band " + plan
    p = W.problems()[name]
    lo, hi, Sq, Sk = W.BAND_PLANS[plan]
    bp = ops.band_plan(lo, hi, Sq, Sk, DEV)
    assert torch.equal(bp.dense_mask()[0], p["mask"])
    q, k, v = W.inputs(name)
    _verdict(name, "attention_band " + plan, ops.attention_band(q.to(DEV), k.to(DEV), v.to(DEV), bp))
    kd, vt = _prepared(k, v)
    out = _sentinel(p["B"], Sq, p["Hq"], 128)
    ops.attention_prepared_band(q.to(DEV), kd, vt, out, Sk, bp)
    _verdict(name, "attention_prepared_band " + plan, out.permute(0, 2, 1, 3))


# --------------------------------------------------------------------- the materialised entries: m = 3 (bf16(p / l) is stored)
@pytest.mark.parametrize("D,frames,per", P.FRAMECAUSAL_CASES)
def test_attention_framecausal(D, frames, per):
    name = f"framecausal D{D} {frames}x{per}"
    q, k, v = W.inputs(name)
    _verdict(name, "attention_" + name, ops.attention_framecausal(q.to(DEV), k.to(DEV), v.to(DEV), per))


@pytest.mark.parametrize("case", list(P.bias_cases()))
def test_attention_bias(case):
    name = "bias " + case
    p, c = W.problems()[name], P.bias_cases()[case]
    H, S, D = c["H"], c["S"], c["D"]
    q, k, v = W.inputs(name)
    rows = lambda t: t[0].permute(1, 0, 2).reshape(S, -1).contiguous().to(DEV)   # noqa: E731  [1, H, S, D] -> [S, H * D]
    bias = None if p["bias_values"] is None else p["bias_values"].contiguous().to(DEV)
    out = _sentinel(S, H * D)
    ops.attention_bias(rows(q), rows(k), rows(v), H, p["scale"], bias=bias, keep=None if c["keep"] is None else c["keep"].to(DEV),
                       seg=None if c["seg"] is None else c["seg"].to(DEV), causal=c["causal"], out=out, kv_heads=c["Hkv"])
    _verdict(name, "attention_" + name, out.reshape(S, H, D).permute(1, 0, 2)[None])


# ----------------------------------------------------------------------------------------------- ops.attention_prepared_dual
@pytest.mark.parametrize("Sk_i", P.DUAL_SK_I)
def test_dual(Sk_i):
    """out = bf16(bf16(o_t) + bf16(o_i)): |out - (r_t + r_i)| <= ((2 u + e_s)(1 + u) + u)(r_t + r_i), e_s of the longer key set"""
    tname = f"dual text Sk={P.DUAL_SK_T}"
    p = W.problems()[tname]
    q, k_t, v_t = W.inputs(tname)
    ref = W.reference(tname)[0]
    kd_t, vt_t = _prepared(k_t, v_t)
    kd_i = vt_i = None
    if Sk_i:
        qi, k_i, v_i = W.inputs(f"dual image Sk={Sk_i}")
        assert torch.equal(q, qi)
        ref = ref + W.reference(f"dual image Sk={Sk_i}")[0]
        kd_i, vt_i = _prepared(k_i, v_i)
    out = _sentinel(p["B"], p["Sq"], p["Hq"], 128)
    ops.attention_prepared_dual(q.to(DEV), kd_t, vt_t, P.DUAL_SK_T, kd_i, vt_i, Sk_i, out)
    torch.cuda.synchronize()
    u = W.U[BF]
    ratio, zeros = W.out_ratio(out.permute(0, 2, 1, 3).cpu(), ref, (2 * u + W.e_s(p)) * (1 + u) + u)
    assert zeros
    measured(f"probe C dual Sk_t={P.DUAL_SK_T} Sk_i={Sk_i}", ratio, 1.0)


# ------------------------------------------------------------------------------------------------------------ ops.attention_wide
WIDE = [n for n in W.problems() if n.startswith("wide ")]


@pytest.mark.parametrize("name", WIDE)
def test_wide(name):
    q, k, v = (t.to(DEV) for t in W.inputs(name))
    plain = ops.attention_wide(q, k, v)
    out, lse = ops.attention_wide(q, k, v, return_lse=True)
    _verdict(name, name, out, lse, merged=False)
    assert torch.equal(out, plain)


@pytest.mark.parametrize("splits", [2, 3])
@pytest.mark.parametrize("name", WIDE)
def test_wide_key_splits(name, splits):
    """f32 partials merged in a second launch: m = 2, + 2 e_l for the merge weights, 2 e_l for the merged lse"""
    q, k, v = (t.to(DEV) for t in W.inputs(name))
    out, lse = ops.attention_wide(q, k, v, key_splits=splits, return_lse=True)
    _verdict(name, f"{name} key_splits={splits}", out, lse, merged=True)


# ---------------------------------------------------------------------------------------------------------- ops.attention_varlen
@pytest.mark.parametrize("name", [n for n in W.problems() if n.startswith("varlen ")])
def test_varlen(name):
    """three packed sequences of (65, 200, 1) queries over (1, 65, 200) keys, grouped-query heads 4 / 2: the rule is the
    block-diagonal mask over the packed rows"""
    ql, kl = W.VARLEN_LENS
    q, k, v = (t[0].permute(1, 0, 2).contiguous().to(DEV) for t in W.inputs(name))              # packed [T, H, D]
    cu = lambda lens: torch.tensor([0] + list(lens), dtype=torch.int32).cumsum(0).to(torch.int32).to(DEV)   # noqa: E731
    out, lse = ops.attention_varlen(q, k, v, cu(ql), cu(kl), max(ql), max(kl), enable_gqa=True, return_lse=True)
    _verdict(name, name, out.permute(1, 0, 2)[None], lse[None])


# ------------------------------------------------------------------------------- ops.attention_chunked / ops.attention_merge
def _chunks(name):
    p = W.problems()[name]
    q, k, v = (t.to(DEV) for t in W.inputs(name))
    mask = None if p["mask"] is None else p["mask"].to(DEV)
    ks, vs = [k[:, :, a:b] for a, b in W.CUTS], [v[:, :, a:b] for a, b in W.CUTS]
    masks = None if mask is None else [mask[..., a:b] for a, b in W.CUTS]
    return q, ks, vs, masks


@pytest.mark.parametrize("name", [n for n in W.problems() if n.startswith("chunked ")])
def test_chunked(name):
    """every partial is a stored result, the merge rounds once more: m = 3, + 2 e_l for the merge weights"""
    q, ks, vs, masks = _chunks(name)
    out, lse = ops.attention_chunked(q, ks, vs, masks, enable_gqa=True)
    _verdict(name, "attention_" + name, out, lse)


@pytest.mark.parametrize("name", ["chunked bool bf16 D128", "chunked f16 D64"])
def test_merge_of_the_partials(name):
    p = W.problems()[name]
    q, ks, vs, masks = _chunks(name)
    parts = [ops.attention_masked(q, k, v, None if masks is None else m, enable_gqa=True, return_lse=True)
             for k, v, m in zip(ks, vs, masks or [None] * len(ks))]
    buf = _sentinel(p["B"], p["Sq"], p["Hq"], p["D"], dtype=p["dtype"]).permute(0, 2, 1, 3)
    out, lse = ops.attention_merge([o for o, _ in parts], [l for _, l in parts], out=buf)
    assert out.data_ptr() == buf.data_ptr()
    _verdict(name, "attention_merge " + name, out, lse)

# Worst ratio to the bar on the MI355X (each bar is 1.0; every case: profiles/attn_weight_probes_measured.jsonl).  Output: 0.41 ..
# 0.93 over the 242 records, 0.00 where a row has one key (prepared window self (3,7,11) 0.93, attention_masked bf16 up to 0.90,
# f16 up to 0.89, ops.attention other head dims 0.41 .. 0.49, attention_bias 0.49 .. 0.57 and attention_framecausal 0.53 .. 0.60
# of their 3 u bar, dual 0.51 .. 0.74, wide 0.58 .. 0.81, varlen 0.81 / 0.88, chunked and merge 0.62 .. 0.76).  LSE: at most 0.05
# of e_l (wide staged D512).
