"""Exact per-row probes of the attention kernels on the GPU (tests/attention_probes.py has the inputs, the closed-form expectations
and the derived bars; tests/test_attention_probes_host.py proves that they reject single wrong decisions).  Every case reports its
worst elementwise |out - ref| / bound through measured(name, ratio, 1.0): the bar is the derivation's, not a measurement."""
import functools

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from tests import attention_probes as P
from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, F16 = torch.bfloat16, torch.float16
PAD = 512.0      # planted in the V^T columns past Sk of the prepared layouts: a padded key let through is visibly wrong


def _dev(t, layout="bhsd"):
    """[B, H, S, D] on the device; "bshd": a permuted view of [B, S, H, D] storage"""
    if layout == "bshd":
        return t.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    return t.to(DEV)


def _rand_k(B, H, S, D, dtype, seed=0):
    return torch.randn(B, H, S, D, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _membership(name, out, ref, dtype):
    ratio, zeros = P.membership_check(out.cpu(), ref, dtype)
    assert zeros, f"{name}: a non-zero where the expectation is an exact zero"
    measured(f"probe A {name}", ratio, 1.0)


def _selection(name, out, s):
    measured(f"probe B {name}", P.selection_ratio(out.cpu(), s["expect"], s["bound"]), 1.0)


def _prepared(k, v, pad=PAD):
    """k [B,H,Sk,128] contiguous and V^T [B,H,128,Skp] with `pad` in the columns past Sk"""
    B, H, Sk, D = v.shape
    vt = torch.full((B, H, D, (Sk + 63) // 64 * 64), pad, dtype=v.dtype)
    vt[..., :Sk] = v.transpose(2, 3)
    return k.contiguous().to(DEV), vt.to(DEV)


# ------------------------------------------------------------------------------------- ops.attention_masked / hip_mfma_sdpa
def _run_masked(c, q, k, v, n, scale=None):
    mask = None if c["mask"] is None else c["mask"].to(DEV)
    q, k, v = (_dev(t, c["layout"]) for t in (q, k, v))
    if n % 2:       # the backend entry forwards to the same operator: alternate the two over the cases
        out = ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, is_causal=c["causal"], softmax_scale=scale, enable_gqa=c["gqa"])
    else:
        out = ops.attention_masked(q, k, v, mask, is_causal=c["causal"], softmax_scale=scale, enable_gqa=c["gqa"])
    torch.cuda.synchronize()
    assert out.shape == (c["B"], c["Hq"], c["Sq"], c["D"]) and out.dtype == c["dtype"]
    return out


@pytest.mark.parametrize("n,name", list(enumerate(P.masked_cases())))
def test_masked_membership(n, name):
    c = P.masked_cases()[name]
    v = P.case_values(c)
    q = torch.zeros(c["B"], c["Hq"], c["Sq"], c["D"], dtype=c["dtype"])
    out = _run_masked(c, q, _rand_k(c["B"], c["Hkv"], c["Sk"], c["D"], c["dtype"], n), v, n)
    _membership("masked " + name, out, P.membership_expected(P.case_weights(c), v), c["dtype"])


@pytest.mark.parametrize("kind", [torch.bool, torch.float32, BF])
def test_masked_vector_and_element_map_passes_agree(kind):
    """One rule in two layouts, 333 x 333 (a ragged last key tile), with DENSE, SKIP and PARTIAL tiles.  The block-map pre-pass
    reads whole tiles 16 bytes per lane only when the key stride is 1, the mask pointer is 16-byte aligned and the row stride is a
    whole number of 16-byte groups (the host condition of launch_map, restated below): rows of 336 elements at offset 0 take that
    vector pass (and its element path on the key tail), rows of 339 elements at offset 3 the element pass.  Both exact, same bits."""
    rule, buf, wide = P.aligned_and_sliced_mask(333, 333, kind)
    aligned, sliced = buf.to(DEV)[:, :333], wide.to(DEV)[:, 3:336]
    per16 = 16 // rule.element_size()
    assert aligned.stride(1) == 1 and aligned.data_ptr() % 16 == 0 and aligned.stride(0) % per16 == 0          # vector pass
    assert sliced.stride(1) == 1 and (sliced.data_ptr() % 16 != 0 or sliced.stride(0) % per16 != 0)            # element pass
    assert sliced.stride(0) % 2 == 1 and torch.equal(aligned, sliced)
    v = P.code_values(1, 2, 333, 128, BF)
    q, k = torch.zeros(1, 2, 333, 128, dtype=BF).to(DEV), _rand_k(1, 2, 333, 128, BF).to(DEV)
    ref = P.membership_expected(P.weights_of(rule, 1, 2, 333, 333), v)
    a = ops.attention_masked(q, k, v.to(DEV), aligned)
    b = ops.attention_masked(q, k, v.to(DEV), sliced)
    tag = {torch.bool: "bool", torch.float32: "additive f32", BF: "additive bf16"}[kind]
    _membership(f"masked {tag} rows of 336 (vector map pass)", a, ref, BF)
    _membership(f"masked {tag} rows of 339 at offset 3 (element map pass)", b, ref, BF)
    assert torch.equal(a, b)


@pytest.mark.parametrize("n,name", list(enumerate(P.selection_cases())))
def test_masked_selection(n, name):
    c, neg = P.selection_cases()[name]
    s = P.selection_inputs(P.case_allowed(c), c["Hkv"], c["D"], c["dtype"], seed=3, neg=neg)
    out = _run_masked(c, s["q"], s["k"], s["v"], n, scale=-1.0 if neg else 1.0)
    _selection("masked " + name, out, s)


# ---------------------------------------------------------------------------------------------------------- coordinate windows
@functools.lru_cache(maxsize=None)
def _plan(name):
    cq, ck, radius, _ = P.window_case(name)
    return ops.window_plan(cq.to(DEV), None if ck is None else ck.to(DEV), radius=radius)


@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
@pytest.mark.parametrize("D,dtype", [(128, BF), (64, F16)])
def test_window_membership_and_selection_from_the_coordinate_rule(name, D, dtype):
    """the first witness of the window kernel that is independent of the masked kernel for every (row, key) decision"""
    allowed = P.window_case(name)[3]
    Sq, Sk = allowed.shape
    B, H = 2, 2
    tag = f"window {name} {'bf16' if dtype == BF else 'f16'} D{D}"
    assert torch.equal(_plan(name).block_map.cpu(), P.block_map(allowed))
    v = P.code_values(B, H, Sk, D, dtype)
    out = ops.attention_window(torch.zeros(B, H, Sq, D, dtype=dtype, device=DEV), _rand_k(B, H, Sk, D, dtype).to(DEV), v.to(DEV),
                               _plan(name))
    _membership(tag, out, P.membership_expected(P.weights_of(allowed, B, H, Sq, Sk), v), dtype)
    s = P.window_selection(name, D, dtype)
    out = ops.attention_window(s["q"].to(DEV), s["k"].to(DEV), s["v"].to(DEV), _plan(name), softmax_scale=1.0)
    _selection(tag, out, s)


@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
def test_prepared_window_membership_and_selection(name):
    allowed = P.window_case(name)[3]
    Sq, Sk = allowed.shape
    B, H = 1, 3
    tag = f"prepared window {name}"
    v = P.code_values(B, H, Sk, 128, BF)
    k, vt = _prepared(_rand_k(B, H, Sk, 128, BF), v)
    out = torch.empty(B, Sq, H, 128, dtype=BF, device=DEV)
    ops.attention_prepared_window(torch.zeros(B, H, Sq, 128, dtype=BF, device=DEV), k, vt, out, Sk, _plan(name))
    _membership(tag, out.permute(0, 2, 1, 3), P.membership_expected(P.weights_of(allowed, B, H, Sq, Sk), v), BF)
    s = P.window_selection(name, 128, BF, prepared=True)
    k, vt = _prepared(s["k"], s["v"])
    ops.attention_prepared_window(s["q"].to(DEV), k, vt, out, Sk, _plan(name), scale=1.0)
    _selection(tag, out.permute(0, 2, 1, 3), s)


# --------------------------------------------------------------------------------- ops.attention / ops.attention_prepared (no mask)
def _unmasked_probes(tag, B, H, Sq, Sk, levels=2, prepared=False):
    """probe A (the mean over exactly Sk keys: the key tail and the padding of V^T) and probe B through one launch variant"""
    v = P.code_values(B, H, Sk, 128, BF, levels)
    ref = P.membership_expected(torch.ones(B, H, 1, Sk, dtype=torch.float64), v).expand(B, H, Sq, 128)
    s = P.unmasked_selection(B, H, Sq, Sk)          # targets in the first tile and in the last: the rescale runs for some rows only
    if prepared:
        out = torch.empty(B, Sq, H, 128, dtype=BF, device=DEV)
        k, vt = _prepared(_rand_k(B, H, Sk, 128, BF), v)
        ops.attention_prepared(torch.zeros(B, H, Sq, 128, dtype=BF, device=DEV), k, vt, out, Sk)
        a = out.permute(0, 2, 1, 3).clone()
        k, vt = _prepared(s["k"], s["v"])
        ops.attention_prepared(s["q"].to(DEV), k, vt, out, Sk, scale=1.0)
        b = out.permute(0, 2, 1, 3)
    else:
        a = ops.attention(torch.zeros(B, H, Sq, 128, dtype=BF, device=DEV), _rand_k(B, H, Sk, 128, BF).to(DEV), v.to(DEV))
        b = ops.attention(s["q"].to(DEV), s["k"].to(DEV), s["v"].to(DEV), softmax_scale=1.0)
    torch.cuda.synchronize()
    _membership(tag, a, ref, BF)
    _selection(tag, b, s)


@pytest.mark.parametrize("B,H,Sq,Sk", P.UNMASKED_SHAPES["default"])
def test_attention_default_launch(B, H, Sq, Sk):
    _unmasked_probes(f"attention default {B}x{H}x{Sq}x{Sk}", B, H, Sq, Sk)
    _unmasked_probes(f"attention_prepared default {B}x{H}x{Sq}x{Sk}", B, H, Sq, Sk, prepared=True)


@pytest.mark.parametrize("c4", [1, 3, 4, 8])
def test_attention_four_cluster_variants(c4):
    lib.tune_set("attn.waves", 8)
    lib.tune_set("attn.c4", c4)
    lib.tune_set("attn.w64", 0)
    try:
        a, b = P.UNMASKED_SHAPES["c4"]
        _unmasked_probes(f"attention c4={c4} {'x'.join(map(str, a))}", *a)
        _unmasked_probes(f"attention_prepared c4={c4} {'x'.join(map(str, b))}", *b, prepared=True)
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.c4", 3)
        lib.tune_set("attn.w64", 1)


@pytest.mark.parametrize("w64", [1, 8])
def test_attention_w64_forced(w64):
    """the main launch, forced at H = 3, S = 2048 (three-level codes above 1024 keys).  w64 = 1 is the shipped first-tile-maximum
    loop: the 46-binade target stays under its 2^60 threshold, so no workgroup may take the running-maximum pass (the counter
    proves that the shipped loop is what ran).  w64 = 8 is the running-maximum form itself, which has no fallback to count."""
    lib.tune_set("attn.waves", 8)
    lib.tune_set("attn.w64", w64)
    try:
        lib.attn_w64_fallbacks()
        a, b = P.UNMASKED_SHAPES["w64"]
        _unmasked_probes(f"attention w64={w64} {'x'.join(map(str, a))}", *a, levels=3)
        _unmasked_probes(f"attention_prepared w64={w64} {'x'.join(map(str, b))}", *b, levels=3, prepared=True)
        if w64 == 1:
            assert lib.attn_w64_fallbacks() == 0
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.w64", 1)


def test_attention_tail_split():
    """the smallest self-attention launch whose last round is split into key ranges (the default, attn.split = 1): 33 heads x 8
    query blocks = 256 + 8 workgroups.  Both entries hand the split's scratch to the launch, so its size being non-zero is the
    split being taken."""
    a, b = P.UNMASKED_SHAPES["tail"]
    for B, H, Sq, Sk in (a, b):
        assert 0 < ((Sq + 255) // 256 * H * B) % 256 <= 64
        assert lib.load().apexmi_attn_prepared_workspace_bytes(B, H, Sq, Sk) > 0
    _unmasked_probes(f"attention tail split {'x'.join(map(str, a))}", *a, levels=3)
    _unmasked_probes(f"attention_prepared tail split {'x'.join(map(str, b))}", *b, levels=3, prepared=True)


# ----------------------------------------------------------------------------------------------- ops.attention_prepared_dual
@pytest.mark.parametrize("Sk_i", P.DUAL_SK_I)
def test_dual_selection(Sk_i):
    """two key sets, one softmax each, one shared q (P.dual_selection): out = bf16(bf16(V_t[pi_t]) + bf16(V_i[pi_i]))"""
    t, i, q, expect, bound = P.dual_selection(Sk_i)
    B, H, Sq, _ = q.shape
    k_t, vt_t = _prepared(t["k"], t["v"])
    k_i, vt_i = _prepared(i["k"], i["v"]) if i else (None, None)
    out = torch.empty(B, Sq, H, 128, dtype=BF, device=DEV)
    ops.attention_prepared_dual(q.to(DEV), k_t, vt_t, P.DUAL_SK_T, k_i, vt_i, Sk_i, out, scale=1.0)
    torch.cuda.synchronize()
    measured(f"probe B dual Sk_t={P.DUAL_SK_T} Sk_i={Sk_i}", P.selection_ratio(out.permute(0, 2, 1, 3).cpu(), expect, bound), 1.0)


# ----------------------------------------------------------------------- one tile step (csrc/attn_tile.h) behind three kernels
@pytest.mark.parametrize("Sk", [64, 192, 65, 200])
def test_plain_masked_and_dual_kernels_agree_bit_for_bit(Sk):
    """Without a mask and with a positive scale the 4-wave plain kernel, the masked kernel and the dual kernel with an empty image
    set run the same arithmetic in the same order: the same MFMA and summation order, and the multiply by c > 0 commutes exactly
    with the row maximum.  On a ragged last tile (Sk = 65, 200) the plain kernel's finite sentinel and the others' -inf both give
    p = 0 and leave the row maximum alone.  Sq = 160 is one full and one ragged query block."""
    B, H, Sq, D = 1, 2, 160, 128
    g = torch.Generator().manual_seed(Sk)
    q, k, v = (torch.randn(B, H, S, D, generator=g).to(BF) for S in (Sq, Sk, Sk))
    qd, (kd, vt) = q.to(DEV), _prepared(k, v)
    plain, dual = (torch.empty(B, Sq, H, D, dtype=BF, device=DEV) for _ in range(2))
    lib.tune_set("attn.waves", 4)
    try:
        ops.attention_prepared(qd, kd, vt, plain, Sk)
        torch.cuda.synchronize()
    finally:
        lib.tune_set("attn.waves", 0)
    masked = ops.attention_masked(qd, kd, v.to(DEV))
    ops.attention_prepared_dual(qd, kd, vt, Sk, None, None, 0, dual)
    torch.cuda.synchronize()
    plain, dual = plain.permute(0, 2, 1, 3), dual.permute(0, 2, 1, 3)
    assert torch.isfinite(plain.float()).all() and plain.float().abs().max() > 0
    assert torch.equal(plain, masked), "plain (attn.waves = 4) vs masked without a mask"
    assert torch.equal(masked, dual), "masked without a mask vs dual with Sk_i = 0"
    assert torch.equal(plain, dual), "plain (attn.waves = 4) vs dual with Sk_i = 0"


# ------------------------------------------------------------------------- ops.attention_bias / ops.attention_framecausal: probe A
# These two materialise P: the row softmax stores bf16(p / l), the NORMALISED probability, so P = bf16(1 / n) is rounded (<= u),
# a rounding the flash kernels' derivation (P exactly 1) does not have; the store adds its own u.  The worst case is 2 u (1 + u / 2),
# a hair over the bar, but both roundings would have to be extreme at once: measured 0.44 .. 0.75 (attention_bias) and 0.00 .. 0.82
# (attention_framecausal) of the 2 u bar on the MI355X, so the derived bar stands.
@pytest.mark.parametrize("name", list(P.bias_cases()))
def test_attention_bias_membership(name):
    c = P.bias_cases()[name]
    H, Hkv, S, D = c["H"], c["Hkv"], c["S"], c["D"]
    v = P.code_values(1, Hkv, S, D, BF)
    k = _rand_k(1, Hkv, S, D, BF)
    rows = lambda t: t[0].permute(1, 0, 2).reshape(S, -1).contiguous().to(DEV)   # noqa: E731  [1, H, S, D] -> [S, H * D]
    out = ops.attention_bias(torch.zeros(S, H * D, dtype=BF, device=DEV), rows(k), rows(v), H, D ** -0.5,
                             keep=None if c["keep"] is None else c["keep"].to(DEV),
                             seg=None if c["seg"] is None else c["seg"].to(DEV), causal=c["causal"], kv_heads=Hkv)
    torch.cuda.synchronize()
    out = out.reshape(S, H, D).permute(1, 0, 2)[None]
    _membership("attention_bias " + name, out, P.membership_expected(P.weights_of(c["allowed"], 1, H, S, S), v), BF)


@pytest.mark.parametrize("D,frames,per", P.FRAMECAUSAL_CASES)
def test_attention_framecausal_membership(D, frames, per):
    S = frames * per
    v = P.code_values(1, 1, S, D, BF)
    out = ops.attention_framecausal(torch.zeros(1, 1, S, D, dtype=BF, device=DEV), _rand_k(1, 1, S, D, BF).to(DEV), v.to(DEV), per)
    torch.cuda.synchronize()
    ref = P.membership_expected(P.weights_of(P.framecausal_allowed(frames, per), 1, 1, S, S), v)
    _membership(f"attention_framecausal D{D} {frames}x{per}", out, ref, BF)

# Worst |out - ref| / bound of every case on the MI355X (probe, case, ratio; each bar is 1.0):
#   A masked causal 1x1 bf16 D128 0.00; A masked bool [Sq,Sk] 1x1 f16 D64 0.00; A masked causal & bool 1x1 bf16 D128 0.00; A
#   masked causal 63x64 f16 D64 0.46; A masked bool [Sq,Sk] 63x64 bf16 D128 0.45; A masked causal & bool 63x64 f16 D64 0.46; A
#   masked causal 64x63 bf16 D128 0.48; A masked bool [Sq,Sk] 64x63 f16 D64 0.46; A masked causal & bool 64x63 bf16 D128 0.45; A
#   masked causal 65x127 f16 D64 0.46; A masked bool [Sq,Sk] 65x127 bf16 D128 0.48; A masked causal & bool 65x127 f16 D64 0.43; A
#   masked causal 127x65 bf16 D128 0.48; A masked bool [Sq,Sk] 127x65 f16 D64 0.42; A masked causal & bool 127x65 bf16 D128 0.48;
#   A masked causal 128x129 f16 D64 0.46; A masked bool [Sq,Sk] 128x129 bf16 D128 0.45; A masked causal & bool 128x129 f16 D64
#   0.47; A masked causal 129x128 bf16 D128 0.48; A masked bool [Sq,Sk] 129x128 f16 D64 0.46; A masked causal & bool 129x128 bf16
#   D128 0.48; A masked causal 333x333 f16 D64 0.48; A masked bool [Sq,Sk] 333x333 bf16 D128 0.47; A masked causal & bool 333x333
#   f16 D64 0.48; A masked causal 64x333 bf16 D128 0.48; A masked bool [Sq,Sk] 64x333 f16 D64 0.45; A masked causal & bool 64x333
#   bf16 D128 0.44; A masked causal 333x63 f16 D64 0.46; A masked bool [Sq,Sk] 333x63 bf16 D128 0.45; A masked causal & bool
#   333x63 f16 D64 0.46; A masked no mask 129x65 bf16 D128 0.32; A masked bool [B,1,1,Sk] 127x333 bf16 D128 0.45; A masked bool
#   [B,H,Sq,Sk] 129x127 bf16 D128 0.48; A masked bool [Sq,1] over keys 333x129 bf16 D128 0.33; A masked band 449x449 bf16 D128
#   0.48; A masked additive f32 129x333 bf16 D128 0.67; A masked additive q dtype 333x129 bf16 D128 0.71; A masked additive &
#   causal 128x128 bf16 D128 0.71; A masked gqa 4/2 causal & bool 129x333 bf16 D128 0.48; A masked gqa Hkv=1 bool 65x129 bf16 D128
#   0.44; A masked bshd views causal & bool 333x333 bf16 D128 0.48; A masked no mask 129x65 f16 D64 0.25; A masked bool [B,1,1,Sk]
#   127x333 f16 D64 0.35; A masked bool [B,H,Sq,Sk] 129x127 f16 D64 0.46; A masked bool [Sq,1] over keys 333x129 f16 D64 0.41; A
#   masked band 449x449 f16 D64 0.47; A masked additive f32 129x333 f16 D64 0.62; A masked additive q dtype 333x129 f16 D64 0.67;
#   A masked additive & causal 128x128 f16 D64 0.65; A masked gqa 4/2 causal & bool 129x333 f16 D64 0.46; A masked gqa Hkv=1 bool
#   65x129 f16 D64 0.46; A masked bshd views causal & bool 333x333 f16 D64 0.48; A masked bool rows of 336 (vector map pass) 0.48;
#   A masked bool rows of 339 at offset 3 (element map pass) 0.48; A masked additive f32 rows of 336 (vector map pass) 0.68; A
#   masked additive f32 rows of 339 at offset 3 (element map pass) 0.68; A masked additive bf16 rows of 336 (vector map pass)
#   0.68; A masked additive bf16 rows of 339 at offset 3 (element map pass) 0.68; B masked causal 333x333 f16 D64 0.00; B masked
#   causal 129x128 bf16 D128 0.65; B masked causal 128x129 f16 D64 0.00; B masked causal 333x63 f16 D64 0.00; B masked causal
#   64x333 bf16 D128 0.65; B masked causal & bool 333x333 f16 D64 0.00; B masked causal & bool 129x128 bf16 D128 0.65; B masked
#   bool [Sq,Sk] 333x333 bf16 D128 0.65; B masked bool [Sq,Sk] 64x63 f16 D64 0.00; B masked band 449x449 bf16 D128 0.65; B masked
#   band 449x449 f16 D64 0.00; B masked bool [B,1,1,Sk] 127x333 bf16 D128 0.65; B masked additive q dtype 333x129 f16 D64 0.52; B
#   masked gqa 4/2 causal & bool 129x333 bf16 D128 0.65; B masked gqa Hkv=1 bool 65x129 f16 D64 0.00; B masked bshd views causal &
#   bool 333x333 bf16 D128 0.65; B masked causal 1x1 bf16 D128 0.65; B masked no mask 129x65 bf16 D128 0.65; B masked no mask
#   129x65 f16 D64 0.00; B masked negative scale causal & bool 129x128 bf16 D128 0.65; B masked negative scale band 449x449 f16
#   D64 0.00; B masked negative scale gqa 4/2 causal & bool 129x333 bf16 D128 0.65; A window self (6,10,12) r(1,9,11) bf16 D128
#   0.44; B window self (6,10,12) r(1,9,11) bf16 D128 0.65; A window self (5,9,13) r(1,8,12) ragged bf16 D128 0.37; B window self
#   (5,9,13) r(1,8,12) ragged bf16 D128 0.65; A window self (3,7,11) r(0,2,3) ragged bf16 D128 0.44; B window self (3,7,11)
#   r(0,2,3) ragged bf16 D128 0.65; A window cross (5,9,13)->(6,10,12) r(1,4,6) + a row without keys bf16 D128 0.45; B window
#   cross (5,9,13)->(6,10,12) r(1,4,6) + a row without keys bf16 D128 0.65; A window self (6,10,12) r(1,9,11) f16 D64 0.41; B
#   window self (6,10,12) r(1,9,11) f16 D64 0.00; A window self (5,9,13) r(1,8,12) ragged f16 D64 0.25; B window self (5,9,13)
#   r(1,8,12) ragged f16 D64 0.00; A window self (3,7,11) r(0,2,3) ragged f16 D64 0.41; B window self (3,7,11) r(0,2,3) ragged f16
#   D64 0.00; A window cross (5,9,13)->(6,10,12) r(1,4,6) + a row without keys f16 D64 0.45; B window cross (5,9,13)->(6,10,12)
#   r(1,4,6) + a row without keys f16 D64 0.00; A prepared window self (6,10,12) r(1,9,11) 0.44; B prepared window self (6,10,12)
#   r(1,9,11) 0.65; A prepared window self (5,9,13) r(1,8,12) ragged 0.37; B prepared window self (5,9,13) r(1,8,12) ragged 0.65;
#   A prepared window self (3,7,11) r(0,2,3) ragged 0.44; B prepared window self (3,7,11) r(0,2,3) ragged 0.65; A prepared window
#   cross (5,9,13)->(6,10,12) r(1,4,6) + a row without keys 0.45; B prepared window cross (5,9,13)->(6,10,12) r(1,4,6) + a row
#   without keys 0.65; A attention default 2x2x333x1000 0.40; B attention default 2x2x333x1000 0.65; A attention_prepared default
#   2x2x333x1000 0.40; B attention_prepared default 2x2x333x1000 0.65; A attention default 1x3x129x65 0.32; B attention default
#   1x3x129x65 0.65; A attention_prepared default 1x3x129x65 0.32; B attention_prepared default 1x3x129x65 0.65; A attention
#   default 2x4x1x1 0.00; B attention default 2x4x1x1 0.65; A attention_prepared default 2x4x1x1 0.00; B attention_prepared
#   default 2x4x1x1 0.65; A attention default 1x2x700x63 0.36; B attention default 1x2x700x63 0.65; A attention_prepared default
#   1x2x700x63 0.36; B attention_prepared default 1x2x700x63 0.65; A attention c4=1 2x2x700x333 0.41; B attention c4=1 2x2x700x333
#   0.65; A attention_prepared c4=1 1x2x260x1000 0.40; B attention_prepared c4=1 1x2x260x1000 0.65; A attention c4=3 2x2x700x333
#   0.41; B attention c4=3 2x2x700x333 0.65; A attention_prepared c4=3 1x2x260x1000 0.40; B attention_prepared c4=3 1x2x260x1000
#   0.65; A attention c4=4 2x2x700x333 0.41; B attention c4=4 2x2x700x333 0.65; A attention_prepared c4=4 1x2x260x1000 0.40; B
#   attention_prepared c4=4 1x2x260x1000 0.65; A attention c4=8 2x2x700x333 0.41; B attention c4=8 2x2x700x333 0.65; A
#   attention_prepared c4=8 1x2x260x1000 0.40; B attention_prepared c4=8 1x2x260x1000 0.65; A attention w64=1 1x3x2048x2048 0.25;
#   B attention w64=1 1x3x2048x2048 0.65; A attention_prepared w64=1 1x3x513x2085 0.42; B attention_prepared w64=1 1x3x513x2085
#   0.65; A attention w64=8 1x3x2048x2048 0.25; B attention w64=8 1x3x2048x2048 0.65; A attention_prepared w64=8 1x3x513x2085
#   0.42; B attention_prepared w64=8 1x3x513x2085 0.65; A attention tail split 1x33x2048x2048 0.29; B attention tail split
#   1x33x2048x2048 0.65; A attention_prepared tail split 1x33x2048x2085 0.45; B attention_prepared tail split 1x33x2048x2085 0.65;
#   B dual Sk_t=512 Sk_i=0 0.65; B dual Sk_t=512 Sk_i=1 0.56; B dual Sk_t=512 Sk_i=63 0.56; B dual Sk_t=512 Sk_i=257 0.56; A
#   attention_bias keep holes 0.56; A attention_bias causal keep 0.70; A attention_bias causal gqa 4/2 0.75; A attention_bias seg
#   keep D128 0.44; A attention_bias seg causal gqa 4/1 D128 0.71; A attention_framecausal D128 3x80 0.82; A attention_framecausal
#   D256 5x35 0.40; A attention_framecausal D128 1x64 0.00
