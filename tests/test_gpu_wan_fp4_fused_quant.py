"""`WanTransformer3DModel.set_fp4_compute(fused_quant=, mx_ffn=)` on a tiny synthetic bf16 Wan model (width 256,
ffn 512, 2 blocks): both switches change launches and traffic only, so every forward with them is `torch.equal` to the fp4 forward
without them; the `quant_blocks_mxfp4` launches that disappear are counted; off again is never on; a mix with fp6 and a two-step
engine run."""
import pytest
import torch

from tests.test_gpu_wan_fp4_compute import _count
from tests.test_gpu_wan_fp8_compute import BF, CFG, DEV, _fwd

pytestmark = pytest.mark.gpu
LAYERS = 2
SWITCHES = [dict(fused_quant=True), dict(mx_ffn=True), dict(fused_quant=True, mx_ffn=True)]


def _model(affine_norm2=True):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.wan import WanTransformer3DModel
    cfg = dict(CFG, num_layers=LAYERS, cross_attn_norm=affine_norm2)
    return WanTransformer3DModel(**cfg, device=DEV, dtype=BF).init_synthetic(seed=7)


def _quants(m):
    with _count("quant_blocks_mxfp4") as calls:
        out = _fwd(m)
    return out, len(calls["quant_blocks_mxfp4"])


@pytest.mark.parametrize("affine_norm2", [True, False], ids=["affine-norm2", "plain-norm2"])
def test_switches_keep_the_fp4_forward_and_remove_the_quantise_launches(affine_norm2):
    m = _model(affine_norm2)
    m.set_fp4_compute(True)
    base, n_base = _quants(m)
    assert torch.isfinite(base).all() and n_base == 7 * LAYERS
    # the launches a block loses: q|k|v, the cross-attention query (only behind an affine norm2) and FFN-up with fused_quant; the
    # hidden state's with mx_ffn
    fused = 3 if affine_norm2 else 2
    want = {"fused_quant": 7 - fused, "mx_ffn": 6, "fused_quant+mx_ffn": 6 - fused}
    for kw in SWITCHES:
        m.set_fp4_compute(True, **kw)
        out, n = _quants(m)
        name = "+".join(kw)
        assert torch.equal(out, base), name
        assert n == want[name] * LAYERS, f"{name}: {n} quantise launches in {LAYERS} blocks"
    m.set_fp4_compute(True)
    out, n = _quants(m)
    assert torch.equal(out, base) and n == n_base, "the defaults return the earlier launches"
    assert m._fp4_fused_quant is False and m._fp4_mx_ffn is False


def test_off_again_equals_never_on():
    m = _model()
    first = _fwd(m)
    m.set_fp4_compute(True, fused_quant=True, mx_ffn=True)
    _fwd(m)
    m.set_fp4_compute(False)
    assert m._fp4_fused_quant is False and m._fp4_mx_ffn is False
    out, n = _quants(m)
    assert torch.equal(out, first) and n == 0


def test_a_subset_and_a_mix_with_fp6_keep_their_own_forward():
    m = _model()
    m.set_fp4_compute(True, linears=("ffn_up",))                      # no fp4 ffn_down: mx_ffn has nothing to do
    base, n_base = _quants(m)
    m.set_fp4_compute(True, linears=("ffn_up",), fused_quant=True, mx_ffn=True)
    out, n = _quants(m)
    assert torch.equal(out, base) and (n_base, n) == (LAYERS, 0)
    m.set_fp4_compute(False)
    m.set_fp6_compute(True, linears=("qkv", "attn_out", "cross_q", "cross_kv", "cross_out"))
    m.set_fp4_compute(True, linears=("ffn_up", "ffn_down"))
    base, n_base = _quants(m)
    m.set_fp4_compute(True, linears=("ffn_up", "ffn_down"), fused_quant=True, mx_ffn=True)
    out, n = _quants(m)
    assert torch.isfinite(out).all() and torch.equal(out, base) and (n_base, n) == (2 * LAYERS, 0)


def test_engine_run_of_two_steps_equals_the_run_without_the_switches():
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)

    def run(**kw):
        m = _model()
        eng = WanT2VEngine(m, m, vae=vae, fp4_compute=True, **kw)
        assert (m._fp4_fused_quant, m._fp4_mx_ffn) == (bool(kw), bool(kw))
        frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                         height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                         latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
        torch.cuda.synchronize()
        return frames.float().cpu()
    want = run()
    got = run(fp4_fused_quant=True, fp4_mx_ffn=True)
    assert torch.isfinite(got).all() and torch.equal(got, want)
