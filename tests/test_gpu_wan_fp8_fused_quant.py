"""`WanTransformer3DModel.set_fp8_compute(True, fused_quant=True)` on the tiny resident-fp8 Wan model of
tests/test_gpu_wan_fp8_compute.py (width 256, 3 layers, affine norm2): a launch and traffic change only.  The forward is
bit-identical with and without the switch — plain, with run-time LoRA on the fp8 GEMM, with the documented bf16 fallback and under
the f32 residual stream — and the number of `ops.quant_rows_fp8` launches per block drops from 7 to 4, counted, not assumed."""
import contextlib

import pytest
import torch

from tests.test_gpu_wan_fp8_compute import BF, DEV, DIM, FFN, LAYERS, _fwd, _model

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _count_quant_rows():
    """the number of `ops.quant_rows_fp8` calls made inside (a wrapper around the real op, removed on exit)"""
    from apex_studio_amd import ops
    real, calls = ops.quant_rows_fp8, []

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    ops.quant_rows_fp8 = counted
    try:
        yield calls
    finally:
        ops.quant_rows_fp8 = real


def _lora_state():
    """the adapter set of tests/test_gpu_wan_fp8_compute.py::test_run_time_lora_falls_back_to_the_bf16_path: rank 4 on every block
    Linear"""
    from tests.golden.seeded import spec_tensors
    r, spec = 4, {}
    for i in range(LAYERS):
        for at, n in (("self_attn", "q"), ("self_attn", "o"), ("cross_attn", "q"), ("cross_attn", "k"), ("cross_attn", "v"),
                      ("cross_attn", "o")):
            k = f"diffusion_model.blocks.{i}.{at}.{n}"
            spec.update({k + ".lora_down.weight": (r, DIM), k + ".lora_up.weight": (DIM, r), k + ".alpha": ()})
        spec.update({f"diffusion_model.blocks.{i}.ffn.0.lora_down.weight": (r, DIM), f"diffusion_model.blocks.{i}.ffn.0.lora_up.weight": (FFN, r),
                     f"diffusion_model.blocks.{i}.ffn.2.lora_down.weight": (r, FFN), f"diffusion_model.blocks.{i}.ffn.2.lora_up.weight": (DIM, r)})
    return {k: (v * 0.3 if v.dim() == 2 else v) for k, v in spec_tensors(spec, 3100).items()}


def test_forward_is_bit_identical_and_three_quantise_launches_per_block_disappear(tmp_path):
    m = _model(tmp_path)
    first = _fwd(m)
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        plain = _fwd(m)
    assert len(calls) == 7 * LAYERS, f"fp8 compute without the switch: {len(calls)} quantise launches, expected 7 per block"
    assert not torch.equal(plain, first)
    m.set_fp8_compute(True, fused_quant=True)
    with _count_quant_rows() as calls:
        fused = _fwd(m)
    assert len(calls) == 4 * LAYERS, f"fused_quant: {len(calls)} quantise launches, expected 4 per block"
    assert torch.equal(fused, plain), "fused_quant changed the forward"
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain)
    assert len(calls) == 7 * LAYERS, "the default restores every launch"
    m.set_fp8_compute(False)
    assert torch.equal(_fwd(m), first), "off: the very first forward, bit for bit"


def test_run_time_lora_on_the_fp8_gemm_keeps_the_row_and_the_result(tmp_path):
    m = _model(tmp_path)
    m.load_lora_adapter({k: v.clone() for k, v in _lora_state().items()}, adapter_name="lx")
    assert all(rec.lora_A is not None for rec in m._fp8_records.values())
    bf16_path = _fwd(m)
    # lora=False with adapters loaded: the documented bf16 fallback, with and without the switch, and nothing is quantised
    m.set_fp8_compute(True)
    fallback = _fwd(m)
    assert torch.equal(fallback, bf16_path)
    m.set_fp8_compute(True, fused_quant=True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), bf16_path), "lora=False with adapters: the bf16 fallback is unchanged by fused_quant"
    assert calls == []
    # lora=True: the fp8 GEMM with the adapter tail
    m.set_fp8_compute(True, lora=True)
    with _count_quant_rows() as calls:
        tail = _fwd(m)
    assert len(calls) == 7 * LAYERS and not torch.equal(tail, bf16_path)
    m.set_fp8_compute(True, lora=True, fused_quant=True)
    with _count_quant_rows() as calls:
        fused = _fwd(m)
    assert len(calls) == 4 * LAYERS, f"lora + fused_quant: {len(calls)} quantise launches, expected 4 per block"
    assert torch.equal(fused, tail), "fused_quant changed the forward with run-time LoRA on the fp8 GEMM"


def test_f32_residual_stream_is_bit_identical_too(tmp_path):
    """X is float, XN / QKV / FFH are bf16: the three sites route, through the float-input form of the fused norm"""
    m = _model(tmp_path)
    m.set_residual_dtype(torch.float32)
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        plain = _fwd(m)
    n_plain = len(calls)
    m.set_fp8_compute(True, fused_quant=True)
    with _count_quant_rows() as calls:
        fused = _fwd(m)
    assert torch.equal(fused, plain)
    assert len(calls) == n_plain - 3 * LAYERS, (n_plain, len(calls))


def test_engine_switch_two_steps_equal(tmp_path):
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    m = _model(tmp_path)
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)

    def run(**kw):
        eng = WanT2VEngine(m, m, vae=vae, fp8_compute=True, **kw)
        frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                         height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                         latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
        torch.cuda.synchronize()
        return eng, frames
    eng, plain = run()
    assert eng.fp8_fused_quant is False and m._fp8_fused_quant is False
    with _count_quant_rows() as calls:
        eng, fused = run(fp8_fused_quant=True)
    assert eng.fp8_fused_quant is True and m._fp8_fused_quant is True
    assert len(calls) > 0 and len(calls) % (4 * LAYERS) == 0, len(calls)
    assert torch.equal(fused, plain) and torch.isfinite(fused.float()).all() and float(fused.float().std()) > 0
