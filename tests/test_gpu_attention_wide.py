"""ops.attention_wide (attn_wide_kernel, D = 256 / 384 / 512) on the GPU: parity against the f32 reference at the bar the
materialised path's test uses for these head sizes, like-for-like against the oracle's flash rounding, the exact probes of
tests/attention_probes.py (membership, selection) unmasked and under the frame rule, bit-exactness, and the VAEs' "flash" mode.
QB = 128 query rows a workgroup, 64 keys a tile: the shapes put row and key tails, several workgroups, several batches / heads
and frame ends inside tiles and across workgroup boundaries."""
import functools

import pytest
import torch

from oracle import layers as OL
from tests import attention_probes as AP
from tests.conftest import measured
from tests.golden.seeded import seeded, vae_synthetic_state_dict
from tests.test_attention_wide_host import frame_allowed

pytestmark = pytest.mark.gpu

DEV = "cuda"
QB = 128
BF, F16 = torch.bfloat16, torch.float16

# (B, H, Sq, Sk, D)
SHAPES = ((1, 1, QB + 1, 65, 384), (1, 1, 33, 7, 384), (2, 1, 1024, 1000, 384), (1, 2, 300, 200, 256), (1, 1, 129, 1021, 512),
          (3, 1, 64, 64, 512))
# like-for-like working bar: 2 x the worst value measured on the MI355X over SHAPES (1.164e-4 at (2, 1, 1024, 1000, 384); the
# others 0 ... 6.7e-5: profiles/attn_wide_measured.jsonl), under the project's 5e-4 kernel-level ceiling
LIKE_CEILING, LIKE_BAR = 5e-4, 2.4e-4


def _ops():
    from apex_studio_amd import ops
    return ops


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-30))


def _check(out, ref, rel_tol, what, ulp=2.0):
    """rel L2 error, plus max-abs within `ulp` bf16 ulps of the largest reference magnitude (tests/test_gpu_ops.py's helper)"""
    out, ref = out.float().cpu(), ref.float().cpu()
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    rel = _rel(out, ref)
    mx = float((out - ref).abs().max())
    bound = ulp * 2.0 ** -8 * float(ref.abs().max()) + 1e-6
    print(f"[attention_wide] {what}: rel L2 {rel:.3e} (bar {rel_tol}), max abs {mx:.3e} (bound {bound:.3e})")
    assert rel < rel_tol, f"{what}: rel L2 {rel:.3e} >= {rel_tol}"
    assert mx <= bound, f"{what}: max abs {mx:.3e} > {bound:.3e}"


@functools.lru_cache(maxsize=None)
def _case(shape, dtype=BF):
    """inputs, the kernel's output and the two references of one shape, computed once"""
    B, H, Sq, Sk, D = shape
    q, k, v = (seeded((B, H, S, D), 181 + n, dtype) for n, S in enumerate((Sq, Sk, Sk)))
    out = _ops().attention_wide(q.to(DEV), k.to(DEV), v.to(DEV))
    qf, kf, vf = (t.float().to(DEV) for t in (q, k, v))
    return dict(q=q, k=k, v=v, out=out, ref=OL.sdpa(qf, kf, vf).cpu(), like=OL.sdpa(qf, kf, vf, policy=OL.BF16_STORAGE).cpu())


@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_the_f32_reference(shape):
    c = _case(shape)
    assert c["out"].shape == (shape[0], shape[1], shape[2], shape[4]) and c["out"].dtype == BF
    assert c["out"].permute(0, 2, 1, 3).is_contiguous()            # a [B, H, Sq, D] view of a [B, Sq, H, D] buffer
    _check(c["out"], c["ref"], 1e-2, f"wide {shape}", ulp=3.0)


@pytest.mark.parametrize("shape", SHAPES)
def test_like_for_like_with_the_flash_rounding(shape):
    c = _case(shape)
    e = _rel(c["out"].cpu(), c["like"].to(BF))
    print(f"[attention_wide] like-for-like {shape}: {e:.3e}")
    assert LIKE_BAR <= LIKE_CEILING
    measured(f"attn_wide like {shape}", e, LIKE_BAR)


def test_f16():
    shape = (1, 2, 300, 200, 256)
    B, H, Sq, Sk, D = shape
    q, k, v = (seeded((B, H, S, D), 191 + n, F16) for n, S in enumerate((Sq, Sk, Sk)))
    out = _ops().attention_wide(q.to(DEV), k.to(DEV), v.to(DEV))
    assert out.dtype == F16
    ref = OL.sdpa(q.float().to(DEV), k.float().to(DEV), v.float().to(DEV)).cpu()
    _check(out, ref, 1e-2, f"wide f16 {shape}", ulp=3.0)      # the bf16 bar: f16 rounds finer


def test_fused_buffer_slices_and_negative_scale():
    """q, k, v as the three column slices of one [T, 1, S, 3 D] buffer (vae_wan's call), read without a copy; scale < 0"""
    T, S, D = 2, 200, 384
    qkv = seeded((T, 1, S, 3 * D), 201, BF).to(DEV)
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    assert q.stride(2) == 3 * D and k.data_ptr() % 16 == 0
    for scale in (None, -0.07):
        out = _ops().attention_wide(q, k, v, softmax_scale=scale)
        ref = OL.sdpa(q.float(), k.float(), v.float(), softmax_scale=scale).cpu()
        _check(out, ref, 1e-2, f"wide fused slices scale={scale}", ulp=3.0)
        assert torch.equal(out, _ops().attention_wide(q.contiguous(), k.contiguous(), v.contiguous(), softmax_scale=scale))


def test_heads_interleaved_layout():
    """q, k, v as [B, H, S, D] views of [B, S, H, D] buffers (head stride D): V^T of all heads of a batch comes from one
    transpose launch over H D / 128 column slices.  Parity, and bit-equality with the contiguous layout; the membership probe
    (V coded per (batch, head)) pins the slice -> head arithmetic."""
    B, H, S, D, ft = 2, 2, 240, 384, 48
    q, k, v = (seeded((B, S, H, D), 231 + n, BF).to(DEV).permute(0, 2, 1, 3) for n in range(3))
    assert v.stride(1) == D and v.stride(2) == H * D
    out = _ops().attention_wide(q, k, v)
    _check(out, OL.sdpa(q.float(), k.float(), v.float()).cpu(), 1e-2, "wide [B,S,H,D] layout", ulp=3.0)
    assert torch.equal(out, _ops().attention_wide(q.contiguous(), k.contiguous(), v.contiguous()))
    vc = AP.code_values(B, H, S, D, BF)
    expect = AP.membership_expected(AP.weights_of(_allowed(S, S, ft, B, H), B, H, S, S), vc)
    vi = vc.permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3)
    got = _ops().attention_wide(torch.zeros_like(q), k, vi, frame_tokens=ft).cpu()
    ratio, zeros = AP.membership_check(got, expect, BF)
    assert ratio <= 1.0 and zeros, ratio


# ---- exact probes --------------------------------------------------------------------------------------------------------
# (name, S or (Sq, Sk), frame_tokens): frame ends inside tiles (48 x 5) and across tile and workgroup boundaries (160 x 3)
PROBE_RULES = (("plain 65", (QB + 1, 65), 0), ("plain 1021", (QB + 1, 1021), 0), ("frames 48x5", (240, 240), 48),
               ("frames 160x3", (480, 480), 160))


def _allowed(Sq, Sk, ft, B=1, H=1):
    a = frame_allowed(Sq, ft) if ft else torch.ones(Sq, Sk, dtype=torch.bool)
    return a.expand(B, H, Sq, Sk).contiguous()


@pytest.mark.parametrize("D", [384, 512])
@pytest.mark.parametrize("rule", PROBE_RULES, ids=[r[0] for r in PROBE_RULES])
def test_probe_membership(rule, D):
    _, (Sq, Sk), ft = rule
    allowed = _allowed(Sq, Sk, ft)
    v = AP.code_values(1, 1, Sk, D, BF)
    expect = AP.membership_expected(AP.weights_of(allowed, 1, 1, Sq, Sk), v)          # from the rule alone
    q = torch.zeros(1, 1, Sq, D, dtype=BF)
    k = seeded((1, 1, Sk, D), 211, BF)
    out = _ops().attention_wide(q.to(DEV), k.to(DEV), v.to(DEV), frame_tokens=ft).cpu()
    ratio, zeros = AP.membership_check(out, expect, BF)
    print(f"[attention_wide] membership {rule[0]} D={D}: worst |err| / (2 u ref) = {ratio:.3f}, zeros exact: {zeros}")
    assert ratio <= 1.0 and zeros


@pytest.mark.parametrize("D", [384, 512])
@pytest.mark.parametrize("rule", PROBE_RULES, ids=[r[0] for r in PROBE_RULES])
def test_probe_selection(rule, D):
    _, (Sq, Sk), ft = rule
    allowed = _allowed(Sq, Sk, ft)
    s = AP.selection_inputs(allowed, 1, D, BF, seed=7)
    out = _ops().attention_wide(s["q"].to(DEV), s["k"].to(DEV), s["v"].to(DEV), softmax_scale=1.0, frame_tokens=ft).cpu()
    ratio = AP.selection_ratio(out, s["expect"], s["bound"])
    print(f"[attention_wide] selection {rule[0]} D={D}: worst |err| / bound = {ratio:.3f} ({s['decoys']} decoys)")
    assert ratio <= 1.0


def test_probe_membership_batches_and_heads():
    """B = 3, H = 2: the code of V is shifted per (batch, head), so a wrong batch / head stride is a wrong count"""
    B, H, S, D, ft = 3, 2, 240, 384, 48
    allowed = _allowed(S, S, ft, B, H)
    v = AP.code_values(B, H, S, D, BF)
    expect = AP.membership_expected(AP.weights_of(allowed, B, H, S, S), v)
    q, k = torch.zeros(B, H, S, D, dtype=BF), seeded((B, H, S, D), 212, BF)
    out = _ops().attention_wide(q.to(DEV), k.to(DEV), v.to(DEV), frame_tokens=ft).cpu()
    ratio, zeros = AP.membership_check(out, expect, BF)
    assert ratio <= 1.0 and zeros, ratio


# ---- bit-exactness ---------------------------------------------------------------------------------------------------------
def test_bit_exact_repeat_batch_split_and_single_frame():
    ops = _ops()
    B, H, S, D = 3, 1, 200, 384
    q, k, v = (seeded((B, H, S, D), 221 + n, BF).to(DEV) for n in range(3))
    out = ops.attention_wide(q, k, v)
    assert torch.equal(out, ops.attention_wide(q, k, v))
    for b in range(B):
        assert torch.equal(out[b:b + 1], ops.attention_wide(q[b:b + 1], k[b:b + 1], v[b:b + 1])), b
    assert torch.equal(out, ops.attention_wide(q, k, v, frame_tokens=S))      # one frame: the rule excludes nothing
    fc = ops.attention_wide(q, k, v, frame_tokens=40)
    assert not torch.equal(out, fc) and torch.equal(out[:, :, -40:], fc[:, :, -40:])   # the last frame sees every key


# ---- model level -----------------------------------------------------------------------------------------------------------
# The tiny configs of tests/test_gpu_vae.py with wider mid blocks: theirs are 128 channels wide, a head size that belongs to the
# D = 128 flash kernels and not to this one.  Wan runs at its shipped 384, Flux at its shipped 512, HunyuanVideo-1.5 at 256.
def _modes(vae, run):
    base = run(vae)
    assert torch.equal(base, run(vae.set_mid_attention("materialised")))
    flash = run(vae.set_mid_attention("flash"))
    vae.set_mid_attention("materialised")
    return base, flash


def test_wan_vae_modes():
    from oracle.vae_wan import AutoencoderKLWanDecoder, AutoencoderKLWanEncoder
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    cfg = dict(base_dim=96, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True])
    dec, enc = AutoencoderKLWanDecoder(**cfg).eval(), AutoencoderKLWanEncoder(**cfg).eval()
    sd = {**vae_synthetic_state_dict(dec, 17), **vae_synthetic_state_dict(enc, 18)}
    dec.load_state_dict({k: v for k, v in sd.items() if k in dec.state_dict()}, strict=True)
    enc.load_state_dict({k: v for k, v in sd.items() if k in enc.state_dict()}, strict=True)
    vae = AutoencoderKLWan(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((1, 16, 2, 16, 16), 62).to(BF)                     # mid block: 2 frames of 256 tokens, C = 384
    base, flash = _modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu())
    ref = dec.decode(z.float(), policy=OL.BF16_STORAGE)
    print(f"[attention_wide] wan decode: materialised {_rel(base, ref):.3e}, flash {_rel(flash, ref):.3e}")
    assert _rel(flash, ref) < 2e-2                                # test_vae_decode_matches_streaming_reference_and_oracle's bar
    x = seeded((1, 3, 5, 128, 128), 63).to(BF)
    run = lambda m: m.encode(x.to(DEV), return_dict=False)[0].parameters.float().cpu()
    base, flash = _modes(vae, run)
    ref = enc.encode(x.float(), policy=OL.BF16_STORAGE)
    ref = ref.parameters if hasattr(ref, "parameters") else ref
    print(f"[attention_wide] wan encode: materialised {_rel(base, ref):.3e}, flash {_rel(flash, ref):.3e}")
    assert _rel(flash, ref) < 2e-2                                # test_vae_encode...'s bar (e_like)


def test_flux_vae_modes():
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
    base, flash = _modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu())
    ref = orc.decode(z.float(), policy=OL.BF16_STORAGE)
    print(f"[attention_wide] flux decode: materialised {_rel(base, ref):.3e}, flash {_rel(flash, ref):.3e}")
    assert _rel(flash, ref) < 2e-2                                # test_flux_vae_decode_matches_oracle's bar


def test_hunyuan15_vae_modes():
    from oracle.vae_hunyuan15 import AutoencoderKLHunyuanVideo15 as Orc
    from apex_studio_amd.vae_hunyuan15 import AutoencoderKLHunyuanVideo15
    cfg = dict(in_channels=3, out_channels=3, latent_channels=32, block_out_channels=(32, 64, 64, 256, 256), layers_per_block=1)
    orc = Orc(**cfg).eval()
    sd = vae_synthetic_state_dict(orc, 23)
    orc.load_state_dict(sd, strict=True)
    vae = AutoencoderKLHunyuanVideo15(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((1, 32, 3, 6, 6), 64).to(BF)                         # mid block: 3 frames of 36 tokens (frame ends inside a tile), C = 256
    base, flash = _modes(vae, lambda m: m.decode(z.to(DEV), return_dict=False)[0].float().cpu())
    ref = orc.decode(z.float(), policy=OL.BF16_STORAGE)
    print(f"[attention_wide] hunyuan15 decode: materialised {_rel(base, ref):.3e}, flash {_rel(flash, ref):.3e}")
    assert _rel(flash, ref) < 2e-2                                # test_hunyuan15_vae_decode_matches_reference_and_oracle's bar
    # encode (image-to-video conditioning): a 5-frame clip puts 2 latent frames of 36 tokens into the encoder's mid block
    x = seeded((1, 3, 5, 96, 96), 65).clamp(-1, 1).to(BF)
    base, flash = _modes(vae, lambda m: m.encode(x.to(DEV), return_dict=False)[0].parameters.float().cpu())
    ref = orc.encode(x.float(), policy=OL.BF16_STORAGE)
    assert base.shape == ref.shape and base.shape[2] == 2
    print(f"[attention_wide] hunyuan15 encode: materialised {_rel(base, ref):.3e}, flash {_rel(flash, ref):.3e}")
    assert _rel(flash, ref) < 2e-2                                # test_hunyuan15_vae_encode_matches_reference_and_oracle's bar
    # the verification mode set AFTER "flash" raises at the call, as the mixin promises, in this VAE too
    vae.set_mid_attention("flash").set_storage_dtype(torch.float32)
    with pytest.raises(NotImplementedError, match="verification"):
        vae.decode(z.to(DEV), return_dict=False)
    vae.set_storage_dtype(BF).set_mid_attention("materialised")
