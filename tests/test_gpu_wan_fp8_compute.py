"""`WanTransformer3DModel.set_fp8_compute` on a tiny resident-fp8 Wan model: off is bit-identical, on is a
finite, different, bounded forward, run-time LoRA falls back to the bf16 path, and the engines take the switch."""
import hashlib

import pytest
import torch

from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
DIM, FFN, LAYERS = 256, 512, 3
CFG = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=FFN, num_layers=LAYERS, cross_attn_norm=True, eps=1e-6)


def _fp8_scaled_file(tmp_path):
    """An original-format Wan file whose block Linears are fp8-scaled (the Kijai layout), as tests/test_weights.py builds one."""
    from safetensors.torch import save_file
    from tests.golden.make_golden_specs import wan_original_spec
    from tests.golden.seeded import spec_tensors
    wan = {k: v.to(BF) for k, v in spec_tensors(wan_original_spec(dim=DIM, ffn=FFN, text_dim=64, freq=256, layers=LAYERS), 5200).items()}
    for k in [k for k in wan if k.startswith("blocks.") and k.endswith(".weight") and wan[k].dim() == 2]:
        w = wan[k].float()
        s = (w.abs().max() / 448.0).reshape(())
        wan[k] = (w / s).to(torch.float8_e4m3fn)
        wan[k[:-len("weight")] + "scale_weight"] = s
    wan["scaled_fp8"] = torch.zeros(2, dtype=torch.float8_e4m3fn)
    path = str(tmp_path / "wan_fp8.safetensors")
    save_file({k: v.contiguous() for k, v in wan.items()}, path)
    return path


def _model(tmp_path):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import weights
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**CFG, device=DEV, dtype=BF)
    assert weights.load_checkpoint_into(m, [_fp8_scaled_file(tmp_path)], keep_fp8=True) == ([], [])
    return m


def _inputs():
    from tests.golden.seeded import seeded
    return seeded((1, 16, 3, 16, 24), 41).to(BF).to(DEV), seeded((1, 20, 64), 42).to(BF).to(DEV), torch.tensor([537.0], device=DEV)


def _fwd(m):
    x, txt, t = _inputs()
    out = m(hidden_states=x, timestep=t, encoder_hidden_states=txt, return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def _hash(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def test_off_is_bit_identical_and_on_is_bounded(tmp_path):
    from apex_studio_amd import ops
    m = _model(tmp_path)
    recs = {id(r): r for r in m._fp8_records.values()}
    assert len(recs) == 7 * LAYERS and all(isinstance(r, ops.Fp8Weight) and r.compute == "bf16" for r in recs.values())
    first = _fwd(m)
    m.set_fp8_compute(True)
    assert all(r.compute == "fp8" for r in recs.values())
    on = _fwd(m)
    m.set_fp8_compute(False)
    assert all(r.compute == "bf16" for r in recs.values())
    assert _hash(_fwd(m)) == _hash(first), "(a) on, then off: the forward is the first one bit for bit"
    assert torch.isfinite(on).all() and not torch.equal(on, first)
    rel = float((on - first).norm() / first.norm())
    print(f"[wan fp8 compute] {LAYERS} blocks of width {DIM}: rel-L2 of the fp8-compute forward against the bf16-compute one {rel:.3e}")
    # (b) measured 2.700e-2 on the MI355X (profiles/gemm_fp8_measured.jsonl); the bar is 2x that
    measured("wan.fp8_compute.tiny.rel_l2", rel, 5.4e-2)


def test_run_time_lora_falls_back_to_the_bf16_path(tmp_path):
    from tests.golden.seeded import spec_tensors
    m = _model(tmp_path)
    r, spec = 4, {}
    for i in range(LAYERS):
        for at, n in (("self_attn", "q"), ("self_attn", "o"), ("cross_attn", "q"), ("cross_attn", "k"), ("cross_attn", "v"),
                      ("cross_attn", "o")):
            k = f"diffusion_model.blocks.{i}.{at}.{n}"
            spec.update({k + ".lora_down.weight": (r, DIM), k + ".lora_up.weight": (DIM, r), k + ".alpha": ()})
        spec.update({f"diffusion_model.blocks.{i}.ffn.0.lora_down.weight": (r, DIM), f"diffusion_model.blocks.{i}.ffn.0.lora_up.weight": (FFN, r),
                     f"diffusion_model.blocks.{i}.ffn.2.lora_down.weight": (r, FFN), f"diffusion_model.blocks.{i}.ffn.2.lora_up.weight": (DIM, r)})
    raw = {k: (v * 0.3 if v.dim() == 2 else v) for k, v in spec_tensors(spec, 3100).items()}
    plain = _fwd(m)
    m.load_lora_adapter({k: v.clone() for k, v in raw.items()}, adapter_name="lx")
    assert all(rec.lora_A is not None for rec in m._fp8_records.values())
    off = _fwd(m)
    assert not torch.equal(off, plain)
    m.set_fp8_compute(True)
    on = _fwd(m)
    assert torch.equal(on, off), "(c) every block Linear carries LoRA factors: the documented fallback is the bf16 path"
    m.delete_adapters("lx")
    assert not torch.equal(_fwd(m), plain), "without the adapters the switch is live again"
    m.set_fp8_compute(False)
    assert torch.equal(_fwd(m), plain)


def test_engine_switch_runs_two_steps(tmp_path):
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    m = _model(tmp_path)
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)
    eng = WanT2VEngine(m, m, vae=vae, fp8_compute=True)
    assert eng.fp8_compute and all(r.compute == "fp8" for r in m._fp8_records.values())
    frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                     height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                     latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
    torch.cuda.synchronize()
    assert frames.shape[-2:] == (64, 64) and torch.isfinite(frames.float()).all() and float(frames.float().std()) > 0
