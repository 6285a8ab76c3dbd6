"""`FluxTransformer2DModel.set_fp4_compute(fused_quant=, mx_ffn=)` on the tiny synthetic bf16 Flux of
tests/test_gpu_flux_fp4_compute.py (width 256, 2 + 2 blocks, 72 and 77 text rows, fused q/k/v on and off): both switches change
launches and traffic only, so every forward with them is `torch.equal` to the fp4 forward without them; the `quant_blocks_mxfp4`
launches that disappear are counted, with the columns each remaining one covers; off again is never on; a two-step engine run."""
import contextlib

import pytest
import torch

from tests.test_gpu_flux_fp4_compute import DIM, MLP, _model
from tests.test_gpu_flux_fp8_compute import DEV, DOUBLE, H2, SINGLE, W2, _fwd

pytestmark = pytest.mark.gpu
SWITCHES = [dict(fused_quant=True), dict(mx_ffn=True), dict(fused_quant=True, mx_ffn=True)]


@contextlib.contextmanager
def _quant_widths():
    """the column count of every `ops.quant_blocks_mxfp4` call made inside"""
    from apex_studio_amd import ops
    real, widths = ops.quant_blocks_mxfp4, []

    def counted(a, *args, **kw):
        widths.append(a.shape[1])
        return real(a, *args, **kw)
    ops.quant_blocks_mxfp4 = counted
    try:
        yield widths
    finally:
        ops.quant_blocks_mxfp4 = real


def _run(m, s_txt):
    with _quant_widths() as widths:
        out = _fwd(m, s_txt)
    return out, sorted(widths)


@pytest.mark.parametrize("fuse_qkv", [True, False], ids=["fused-qkv", "two-pass"])
@pytest.mark.parametrize("s_txt", [72, 77])
def test_switches_keep_the_fp4_forward_and_remove_the_quantise_launches(s_txt, fuse_qkv):
    m = _model()
    m.fuse_qkv = fuse_qkv
    m.set_fp4_compute(True)
    base, w_base = _run(m, s_txt)
    # per double block XN, att, XN (width dim) and FFH (mlp); per single block XN (dim) and CAT (dim + mlp)
    assert torch.isfinite(base).all()
    assert w_base == sorted([DIM] * (3 * DOUBLE + SINGLE) + [MLP] * DOUBLE + [DIM + MLP] * SINGLE)
    want = {
        # the norms in front of the QKV pair, the FF-up pair and QKV + MLP-up quantise themselves: 4 -> 2 and 2 -> 1
        "fused_quant": [DIM] * DOUBLE + [MLP] * DOUBLE + [DIM + MLP] * SINGLE,
        # the hidden state of a double block is never quantised by a launch of its own, and the single block's remaining launch
        # covers the attention columns only
        "mx_ffn": [DIM] * (3 * DOUBLE + SINGLE) + [DIM] * SINGLE,
        "fused_quant+mx_ffn": [DIM] * DOUBLE + [DIM] * SINGLE,      # 4 -> 1 and 2 -> 1
    }
    for kw in SWITCHES:
        m.set_fp4_compute(True, **kw)
        out, widths = _run(m, s_txt)
        name = "+".join(kw)
        assert torch.equal(out, base), name
        assert widths == sorted(want[name]), f"{name}: quantise launches over {widths} columns"
    m.set_fp4_compute(True)
    out, widths = _run(m, s_txt)
    assert torch.equal(out, base) and widths == w_base, "the defaults return the earlier launches"


def test_off_again_equals_never_on_and_a_subset_keeps_its_forward():
    m = _model()
    first = _fwd(m)
    m.set_fp4_compute(True, fused_quant=True, mx_ffn=True)
    _fwd(m)
    m.set_fp4_compute(False)
    assert m._fp4_fused_quant is False and m._fp4_mx_ffn is False
    out, widths = _run(m, 72)
    assert torch.equal(out, first) and widths == []
    # single_in without single_out, ffn_up without ffn_down: mx_ffn has nothing to do, fused_quant serves the two norms
    m.set_fp4_compute(True, linears=("ffn_up", "single_in"))
    base, w_base = _run(m, 72)
    m.set_fp4_compute(True, linears=("ffn_up", "single_in"), fused_quant=True, mx_ffn=True)
    out, widths = _run(m, 72)
    assert torch.equal(out, base) and len(w_base) == DOUBLE + SINGLE and widths == []


def test_engine_run_of_two_steps_equals_the_run_without_the_switches():
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from tests.golden.seeded import seeded

    def run(**kw):
        m = _model()
        eng = FluxT2IEngine(m, fp4_compute=True, **kw)
        assert (m._fp4_fused_quant, m._fp4_mx_ffn) == (bool(kw), bool(kw))
        lat = eng.run(prompt_embeds=seeded((1, 72, 256), 32).to(DEV), pooled_prompt_embeds=seeded((1, 64), 33).to(DEV), height=256,
                      width=256, num_inference_steps=2, guidance_scale=3.5, latents=seeded((1, H2 * W2, 64), 41).to(DEV),
                      return_latents=True)
        torch.cuda.synchronize()
        return lat.float().cpu()
    want = run()
    got = run(fp4_fused_quant=True, fp4_mx_ffn=True)
    assert torch.isfinite(got).all() and torch.equal(got, want)
