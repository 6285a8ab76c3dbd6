"""Key splits and the log-sum-exp of ops.attention_wide (attn_wide_kernel's MODE 1 / 2 and the f32 partial merge, DESIGN.md
§3.4.3) on the GPU: the exact probes of tests/attention_probes.py under every (case, split count, head size), the lse as a key
count and against the float64 yardstick of tests/attention_lse_ref.py, bit-identity of everything that must not move, split
against unsplit like for like, attention_chunked at a wide head, and the VAEs' set_mid_attention(mode, key_splits).
QB = 128 query rows a workgroup, 64 keys a tile; the shapes are the smallest that put the split arithmetic at risk:
  plain 1021    16 tiles with a key tail, two query blocks of which one has a single row
  plain 7       one tile: every split but the first is empty
  frames 48x5   frame ends inside tiles
  frames 160x3  block 0 has 3 tiles and block 3 has 8; in block 1 rows 128-159 see nothing in tiles 3-4 while rows 160-255 do:
                dead partial rows beside live ones in one wave
Measured on the MI355X (profiles/attn_wide_split_measured.jsonl): lse as a key count 2.7e-8 ... 4.5e-7 (bar 1e-5); lse on seeded
inputs 3.3e-7 ... 8.76e-7 (worst: plain 1021, D 512, n = 2; f16 7.1e-7; through attention_chunked 7.5e-7); like-for-like rel-L2 of
the split runs 3.6e-5 ... 1.339e-4 (worst: plain 1021, D 512, n = 8, where the unsplit launch has 6.7e-5; (2, 1, 1024, 1000, 384)
1.13e-4 / 1.09e-4 at n = 2 / 8 against 1.164e-4 unsplit); chunked / single rel-L2 against float64 2.884e-3 / 2.365e-3 (1.22)."""
import functools
import math

import pytest
import torch

from oracle import layers as OL
from tests import attention_probes as AP
from tests.attention_lse_ref import attention_ref, lse_ref
from tests.conftest import measured
from tests.golden.seeded import seeded, vae_synthetic_state_dict
from tests.test_attention_wide_host import frame_allowed

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F16 = torch.bfloat16, torch.float16
# (name, Sq, Sk, frame_tokens)
CASES = (("plain 1021", 129, 1021, 0), ("plain 7", 33, 7, 0), ("frames 48x5", 240, 240, 48), ("frames 160x3", 480, 480, 160))
IDS = [c[0] for c in CASES]
SPLITS = (2, 3, 8)
# (D, n) of the probes: every split count at D = 384 and 512, D = 256 once
DN = [(D, n) for D in (384, 512) for n in SPLITS] + [(256, 3)]
COUNT_BAR = 1e-5      # tests/test_gpu_attention_lse.py's: a handful of f32 roundings on values <= ln 1024; one key more or less
#                       moves ln(count) by about 1 / count >= 1 / 1021 here
# |lse - float64 reference| on seeded inputs: twice the worst value measured on the MI355X over (case, D, n), under a ceiling of a
# tenth of what one lost key among 1021 equal ones moves
LSE_CEILING = 1e-4
LSE_BAR = 1.8e-6      # measured 8.76e-7 (plain 1021, D 512, n = 2); one to three f32 ulps of an lse of up to 7
# like-for-like rel-L2 against oracle.layers.sdpa's bf16 policy, split runs: twice the worst measured, under the project's 5e-4
# kernel-level ceiling
LIKE_CEILING = 5e-4
SPLIT_LIKE_BAR = 2.7e-4  # measured 1.339e-4 ((1, 1, 129, 1021, 512), n = 8)


def _ops():
    from apex_studio_amd import ops
    return ops


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _check(out, ref, rel_tol, what, ulp=2.0):
    """rel L2 error, plus max-abs within `ulp` bf16 ulps of the largest reference magnitude (tests/test_gpu_attention_wide.py's)"""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    rel = _rel(out, ref)
    mx = float((out - ref).abs().max())
    bound = ulp * 2.0 ** -8 * float(ref.abs().max()) + 1e-6
    print(f"[attention_wide split] {what}: rel L2 {rel:.3e} (bar {rel_tol}), max abs {mx:.3e} (bound {bound:.3e})")
    assert rel < rel_tol, f"{what}: rel L2 {rel:.3e} >= {rel_tol}"
    assert mx <= bound, f"{what}: max abs {mx:.3e} > {bound:.3e}"


def _allowed(Sq, Sk, ft, B=1, H=1):
    a = frame_allowed(Sq, ft) if ft else torch.ones(Sq, Sk, dtype=torch.bool)
    return a.expand(B, H, Sq, Sk).contiguous()


def _lse_shape(lse, B, H, Sq):
    assert lse.shape == (B, H, Sq) and lse.dtype == torch.float32 and lse.is_contiguous()


def _count_check(name, lse, n):
    """lse against ln n for a probe whose probabilities are all exactly 1; -inf exactly where no key is allowed"""
    lse = lse.double().cpu()
    assert not torch.isnan(lse).any()
    dead = n == 0
    assert torch.equal(lse[dead], torch.full_like(lse[dead], float("-inf"))), f"{name}: a row without keys is not -inf"
    err = (lse[~dead] - torch.log(n[~dead])).abs().max().item()
    print(f"[attention_wide split] lse count {name}: worst |lse - ln count| = {err:.3e}")
    measured(f"wide lse count {name}", err, COUNT_BAR)


def _lse_error(lse, ref_l):
    lse = lse.double().cpu()
    dead = torch.isinf(ref_l)
    assert not torch.isnan(lse).any()
    assert torch.equal(lse[dead], torch.full_like(lse[dead], float("-inf")))
    return (lse[~dead] - ref_l[~dead]).abs().max().item()


# ---- exact probes: membership (and the lse as a key count), selection ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _membership_case(case, D, B=1, H=1):
    _, Sq, Sk, ft = case
    allowed = _allowed(Sq, Sk, ft, B, H)
    w = AP.weights_of(allowed, B, H, Sq, Sk)
    v = AP.code_values(B, H, Sk, D, BF)
    return dict(q=torch.zeros(B, H, Sq, D, dtype=BF).to(DEV), k=seeded((B, H, Sk, D), 311, BF).to(DEV), v=v.to(DEV),
                expect=AP.membership_expected(w, v), count=w.sum(-1))


@pytest.mark.parametrize("D,n", DN + [(384, 1), (512, 1)])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probe_membership_and_key_count(case, D, n):
    """q = 0: every allowed score is 0, out is the mean of the allowed keys' codes and lse = ln(their count).  A wrong tile range,
    a double-counted key or a dropped split is a wrong count in both."""
    c = _membership_case(case, D)
    out, lse = _ops().attention_wide(c["q"], c["k"], c["v"], frame_tokens=case[3], key_splits=n, return_lse=True)
    _lse_shape(lse, 1, 1, case[1])
    ratio, zeros = AP.membership_check(out.cpu(), c["expect"], BF)
    print(f"[attention_wide split] membership {case[0]} D={D} n={n}: worst |err| / (2 u ref) = {ratio:.3f}, zeros exact: {zeros}")
    assert ratio <= 1.0 and zeros
    _count_check(f"{case[0]} D={D} n={n}", lse, c["count"])


@functools.lru_cache(maxsize=None)
def _selection_case(case, D):
    _, Sq, Sk, ft = case
    s = AP.selection_inputs(_allowed(Sq, Sk, ft), 1, D, BF, seed=7)
    return dict(q=s["q"].to(DEV), k=s["k"].to(DEV), v=s["v"].to(DEV), expect=s["expect"], bound=s["bound"], decoys=s["decoys"])


@pytest.mark.parametrize("D,n", DN)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_probe_selection(case, D, n):
    s = _selection_case(case, D)
    out = _ops().attention_wide(s["q"], s["k"], s["v"], softmax_scale=1.0, frame_tokens=case[3], key_splits=n).cpu()
    ratio = AP.selection_ratio(out, s["expect"], s["bound"])
    print(f"[attention_wide split] selection {case[0]} D={D} n={n}: worst |err| / bound = {ratio:.3f} ({s['decoys']} decoys)")
    assert ratio <= 1.0


def test_probe_membership_batches_heads_and_interleaved_layout():
    """B = 3, H = 2, n = 3: the code of V is shifted per (batch, head), so a wrong partial or lse stride is a wrong count; the
    [B, S, H, D] layout (head stride D) once with n = 2"""
    B, H, S, D, ft = 3, 2, 240, 384, 48
    c = _membership_case(("frames 48x5", S, S, ft), D, B, H)
    out, lse = _ops().attention_wide(c["q"], c["k"], c["v"], frame_tokens=ft, key_splits=3, return_lse=True)
    _lse_shape(lse, B, H, S)
    ratio, zeros = AP.membership_check(out.cpu(), c["expect"], BF)
    assert ratio <= 1.0 and zeros, ratio
    _count_check("B3 H2 frames 48x5 n=3", lse, c["count"])
    qi, ki, vi = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (c["q"], c["k"], c["v"]))
    assert vi.stride(1) == D and vi.stride(2) == H * D
    out2, lse2 = _ops().attention_wide(qi, ki, vi, frame_tokens=ft, key_splits=2, return_lse=True)
    ratio, zeros = AP.membership_check(out2.cpu(), c["expect"], BF)
    assert ratio <= 1.0 and zeros, ratio
    _count_check("B3 H2 [B,S,H,D] n=2", lse2, c["count"])


# ---- the lse on seeded inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded_case(case, D, dtype=BF):
    _, Sq, Sk, ft = case
    q, k, v = (seeded((1, 1, S, D), 321 + i, dtype) for i, S in enumerate((Sq, Sk, Sk)))
    w = AP.weights_of(_allowed(Sq, Sk, ft), 1, 1, Sq, Sk)
    return dict(q=q.to(DEV), k=k.to(DEV), v=v.to(DEV), ref_l=lse_ref(q, k, w, 1.0 / math.sqrt(D)))


@pytest.mark.parametrize("D", [384, 512])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lse_seeded_inputs(case, D):
    c = _seeded_case(case, D)
    worst = 0.0
    for n in (1,) + SPLITS:
        out, lse = _ops().attention_wide(c["q"], c["k"], c["v"], frame_tokens=case[3], key_splits=n, return_lse=True)
        _lse_shape(lse, 1, 1, case[1])
        assert torch.isfinite(out.float()).all()
        err = _lse_error(lse, c["ref_l"])
        print(f"[attention_wide split] lse seeded {case[0]} D={D} n={n}: worst |lse - ref| = {err:.3e}")
        worst = max(worst, err)
    assert LSE_BAR <= LSE_CEILING
    measured(f"wide lse seeded {case[0]} D={D}", worst, LSE_BAR)


# ---- bit-identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [256, 384, 512])
def test_bit_identity(D):
    ops = _ops()
    from apex_studio_amd import lib
    case = CASES[0] if D != 384 else CASES[3]
    c = _seeded_case(case, D)
    q, k, v, ft = c["q"], c["k"], c["v"], case[3]
    base = ops.attention_wide(q, k, v, frame_tokens=ft)
    assert torch.equal(base, ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=1))
    with_lse = ops.attention_wide(q, k, v, frame_tokens=ft, return_lse=True)
    assert torch.equal(base, with_lse[0])                      # out does not move with the lse
    # a split call repeats itself to the bit, out and lse
    a = ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=3, return_lse=True)
    b = ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=3, return_lse=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=3))      # and without the lse
    # "auto" is the explicit count of the pure rule on this device's compute-unit count
    _, Sq, Sk, _ = case
    cus = torch.cuda.get_device_properties(q.device).multi_processor_count
    n = lib.load().apexmi_attn_wide_auto_splits((Sq + 127) // 128, (Sk + 63) // 64, cus)
    print(f"[attention_wide split] auto D={D} {case[0]}: {n} splits on {cus} compute units")
    assert 1 <= n <= 8
    auto = ops.attention_wide(q, k, v, frame_tokens=ft, key_splits="auto", return_lse=True)
    expl = ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=n, return_lse=True)
    assert torch.equal(auto[0], expl[0]) and torch.equal(auto[1], expl[1])


def test_no_host_sync():
    c = _seeded_case(CASES[0], 384)
    run = lambda: [_ops().attention_wide(c["q"], c["k"], c["v"], key_splits=n, return_lse=True) for n in (1, 4, "auto")]
    run()                                          # workspace allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = run()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert all(torch.isfinite(o.float()).all() for o, _ in r)


# ---- split against unsplit -------------------------------------------------------------------------------------------------
# (B, H, Sq, Sk, D)
LIKE_SHAPES = ((1, 1, 129, 1021, 512), (2, 1, 1024, 1000, 384), (1, 2, 300, 200, 256))


@functools.lru_cache(maxsize=None)
def _like_case(shape):
    B, H, Sq, Sk, D = shape
    q, k, v = (seeded((B, H, S, D), 181 + n, BF) for n, S in enumerate((Sq, Sk, Sk)))     # tests/test_gpu_attention_wide.py's inputs
    qf, kf, vf = (t.float().to(DEV) for t in (q, k, v))
    return dict(q=q.to(DEV), k=k.to(DEV), v=v.to(DEV), ref=OL.sdpa(qf, kf, vf).cpu(),
                like=OL.sdpa(qf, kf, vf, policy=OL.BF16_STORAGE).cpu().to(BF))


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("shape", LIKE_SHAPES)
def test_split_like_for_like_and_parity(shape, n):
    """f32 partials: a split result differs from the unsplit one only in f32 summation order and the one final rounding, so it
    is held to its own measured bar under the same ceiling, and to the f32 reference at the unsplit test's bar"""
    c = _like_case(shape)
    out = _ops().attention_wide(c["q"], c["k"], c["v"], key_splits=n)
    unsplit = _ops().attention_wide(c["q"], c["k"], c["v"])
    assert out.shape == unsplit.shape and out.dtype == BF and out.permute(0, 2, 1, 3).is_contiguous()
    e, e1 = _rel(out.cpu(), c["like"]), _rel(unsplit.cpu(), c["like"])
    print(f"[attention_wide split] like-for-like {shape} n={n}: {e:.3e} (unsplit {e1:.3e})")
    assert SPLIT_LIKE_BAR <= LIKE_CEILING
    measured(f"attn_wide split like {shape} n={n}", e, SPLIT_LIKE_BAR)
    _check(out, c["ref"], 1e-2, f"wide {shape} n={n}", ulp=3.0)


def test_f16_split_and_lse():
    shape = (1, 2, 300, 200, 256)
    B, H, Sq, Sk, D = shape
    q, k, v = (seeded((B, H, S, D), 191 + n, F16) for n, S in enumerate((Sq, Sk, Sk)))
    out, lse = _ops().attention_wide(q.to(DEV), k.to(DEV), v.to(DEV), key_splits=3, return_lse=True)
    assert out.dtype == F16
    _lse_shape(lse, B, H, Sq)
    ref = OL.sdpa(q.float().to(DEV), k.float().to(DEV), v.float().to(DEV)).cpu()
    _check(out, ref, 1e-2, f"wide f16 {shape} n=3", ulp=3.0)      # the bf16 bar: f16 rounds finer
    err = _lse_error(lse, lse_ref(q, k, torch.ones(B, H, Sq, Sk, dtype=torch.float64), 1.0 / math.sqrt(D)))
    print(f"[attention_wide split] lse f16 {shape} n=3: worst |lse - ref| = {err:.3e}")
    measured(f"wide lse seeded f16 {shape} n=3", err, LSE_BAR)


# ---- attention_chunked at a wide head ---------------------------------------------------------------------------------------
def test_chunked_wide_head():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    B, H, Sq, D, cuts = 2, 2, 200, 384, ((0, 65), (65, 265))
    Sk = cuts[-1][1]
    q, k, v = (seeded((B, H, S, D), 331 + i, BF) for i, S in enumerate((Sq, Sk, Sk)))
    scale = 1.0 / math.sqrt(D)
    ref_o, ref_l = attention_ref(q, k, v, torch.ones(B, H, Sq, Sk, dtype=torch.float64), scale)
    dq, dk, dv = q.to(DEV), k.to(DEV), v.to(DEV)
    single, single_lse = ops.attention_wide(dq, dk, dv, return_lse=True)
    out, lse = ops.attention_chunked(dq, [dk[:, :, a:b] for a, b in cuts], [dv[:, :, a:b] for a, b in cuts])
    assert out.shape == (B, H, Sq, D) and out.dtype == BF
    _lse_shape(lse, B, H, Sq)
    e_single, e_chunked = _rel(single.cpu(), ref_o), _rel(out.cpu(), ref_o)
    print(f"[attention_wide split] chunked D={D}: rel-L2 single {e_single:.3e}, chunked {e_chunked:.3e}, ratio {e_chunked / e_single:.3f}")
    measured("wide chunked D384", e_chunked, 1.5 * e_single)       # every partial out adds one rounding of the store dtype
    _check(out, single, 1e-2, "wide chunked against the single call", ulp=3.0)
    for name, l in (("chunked", lse), ("single", single_lse)):
        err = _lse_error(l, ref_l)
        print(f"[attention_wide split] chunked D={D} lse ({name}): worst |lse - ref| = {err:.3e}")
        measured(f"wide chunked D384 lse {name}", err, LSE_BAR)
    with pytest.raises(ApexMIError, match="no masks"):
        ops.attention_chunked(dq, [dk], [dv], [torch.ones(Sq, Sk, dtype=torch.bool, device=DEV)])
    with pytest.raises(ApexMIError, match="grouped-query"):
        ops.attention_chunked(dq, [dk[:, :1]], [dv[:, :1]], enable_gqa=True)


# ---- model level: the tiny configurations of tests/test_gpu_attention_wide.py ------------------------------------------------
def _split_modes(vae, run, ref, what):
    flash = run(vae.set_mid_attention("flash"))
    assert torch.equal(flash, run(vae.set_mid_attention("flash", key_splits=1)))
    try:
        for ks in (4, "auto"):
            e = _rel(run(vae.set_mid_attention("flash", key_splits=ks)), ref)
            print(f"[attention_wide split] {what} key_splits={ks}: {e:.3e} (flash {_rel(flash, ref):.3e})")
            assert e < 2e-2                                        # the bar of the existing mode tests
    finally:
        vae.set_mid_attention("materialised")
    assert vae.mid_attention == "materialised" and vae.mid_attention_key_splits == 1


def test_wan_vae_key_splits():
    from oracle.vae_wan import AutoencoderKLWanDecoder, AutoencoderKLWanEncoder
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    cfg = dict(base_dim=96, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True])
    dec, enc = AutoencoderKLWanDecoder(**cfg).eval(), AutoencoderKLWanEncoder(**cfg).eval()
    sd = {**vae_synthetic_state_dict(dec, 17), **vae_synthetic_state_dict(enc, 18)}
    dec.load_state_dict({k: v for k, v in sd.items() if k in dec.state_dict()}, strict=True)
    vae = AutoencoderKLWan(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((1, 16, 2, 16, 16), 62).to(BF)                     # mid block: 2 frames of 256 tokens, C = 384
    ref = dec.decode(z.float(), policy=OL.BF16_STORAGE)
    _split_modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu(), ref, "wan decode")


def test_flux_vae_key_splits():
    from oracle.vae_flux import AutoencoderKLDecoder
    from apex_studio_amd.vae_flux import AutoencoderKL
    cfg = dict(latent_channels=16, block_out_channels=(32, 64, 512, 512), layers_per_block=1)
    orc = AutoencoderKLDecoder(**cfg).eval()
    sd = vae_synthetic_state_dict(orc, 19)
    for k in list(sd):                     # GroupNorm affine: weight ~ 1, bias small, bf16-representable (tests/test_gpu_vae.py)
        if ".norm" in k or "group_norm" in k or "conv_norm_out" in k:
            sd[k] = ((torch.ones_like(sd[k]) if k.endswith("weight") else torch.zeros_like(sd[k])) + 0.05 * sd[k].sign()).to(BF).float()
    orc.load_state_dict(sd, strict=True)
    vae = AutoencoderKL(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((1, 16, 20, 24), 63).to(BF)                          # mid block: 480 tokens, C = 512
    ref = orc.decode(z.float(), policy=OL.BF16_STORAGE)
    _split_modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu(), ref, "flux decode")


def test_hunyuan15_vae_key_splits():
    from oracle.vae_hunyuan15 import AutoencoderKLHunyuanVideo15 as Orc
    from apex_studio_amd.vae_hunyuan15 import AutoencoderKLHunyuanVideo15
    cfg = dict(in_channels=3, out_channels=3, latent_channels=32, block_out_channels=(32, 64, 64, 256, 256), layers_per_block=1)
    orc = Orc(**cfg).eval()
    sd = vae_synthetic_state_dict(orc, 23)
    orc.load_state_dict(sd, strict=True)
    vae = AutoencoderKLHunyuanVideo15(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((1, 32, 3, 6, 6), 64).to(BF)                         # mid block: 3 frames of 36 tokens (frame ends inside a tile), C = 256
    ref = orc.decode(z.float(), policy=OL.BF16_STORAGE)
    _split_modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu(), ref, "hunyuan15 decode")
