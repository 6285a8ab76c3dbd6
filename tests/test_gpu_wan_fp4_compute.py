"""`WanTransformer3DModel.set_fp4_compute` on the tiny synthetic bf16 Wan model of tests/test_gpu_wan_fp8_compute.py:
off is bit-identical, on is a finite, different, bounded forward, a subset of the Linears attaches exactly its records, a merged LoRA
is quantised in, the refusals, the engine switch and the launch counts."""
import contextlib

import pytest
import torch

from tests.conftest import measured
from tests.test_gpu_wan_fp8_compute import BF, CFG, DEV, DIM, FFN, LAYERS, _fwd, _hash
from tests.test_gpu_wan_fp8_compute import _model as _resident_fp8_model

pytestmark = pytest.mark.gpu


def _model():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.wan import WanTransformer3DModel
    return WanTransformer3DModel(**CFG, device=DEV, dtype=BF).init_synthetic(seed=7)


def _records(m):
    if not m._packed:
        return []
    return [w._fp4 for blk in m.blocks for w in m._fp4_weights(blk).values() if getattr(w, "_fp4", None) is not None]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@contextlib.contextmanager
def _count(*names):
    """the number of calls of each named op made inside (wrappers around the real ops, removed on exit)"""
    from apex_studio_amd import ops
    real, calls = {n: getattr(ops, n) for n in names}, {n: [] for n in names}

    def counted(n):
        def f(*a, **k):
            calls[n].append(1)
            return real[n](*a, **k)
        return f
    for n in names:
        setattr(ops, n, counted(n))
    try:
        yield calls
    finally:
        for n in names:
            setattr(ops, n, real[n])


def test_off_is_bit_identical_on_is_bounded_and_a_subset_lies_between():
    from apex_studio_amd import ops
    m = _model()
    first = _fwd(m)
    assert _records(m) == []
    m.set_fp4_compute(True)
    recs = _records(m)
    assert len(recs) == 7 * LAYERS and all(isinstance(r, ops.Mxfp4Weight) and r.compute == "fp4" for r in recs)
    assert m._fp4_bytes == sum(r.nbytes() for r in recs) == LAYERS * (8 * DIM * DIM + 2 * DIM * FFN) * 17 // 32
    on = _fwd(m)
    m.set_fp4_compute(True, linears=("ffn_up", "ffn_down"))
    recs = _records(m)
    assert len(recs) == 2 * LAYERS and {r.shape for r in recs} == {(FFN, DIM), (DIM, FFN)}, "(c) exactly the two FFN Linears of every block"
    ffn = _fwd(m)
    m.set_fp4_compute(False)
    assert _records(m) == [] and m._fp4_bytes == 0
    assert _hash(_fwd(m)) == _hash(first), "(a) on, then off: the forward is the first one bit for bit"
    assert torch.isfinite(on).all() and not torch.equal(on, first), "(b)"
    assert torch.isfinite(ffn).all() and not torch.equal(ffn, first) and not torch.equal(ffn, on), "(c)"
    rel_on, rel_ffn = _rel(on, first), _rel(ffn, first)
    print(f"[wan fp4 compute] {LAYERS} blocks of width {DIM}: rel-L2 against the bf16 forward, all seven Linears {rel_on:.3e}, "
          f"the FFN pair only {rel_ffn:.3e}")
    assert rel_ffn < rel_on, "(c) fewer quantised Linears, a smaller error"
    measured("wan.fp4_compute.tiny.rel_l2", rel_on, ALL_ON_BAR)


# (b) measured 1.589e-2 on the MI355X (the FFN pair alone: 1.362e-2; profiles/gemm_mxfp4_measured.jsonl); the bar is 2x that
ALL_ON_BAR = 3.2e-2


def _lora_state():
    """a rank-4 adapter on every block Linear, as tests/test_gpu_wan_fp8_compute.py builds it"""
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


def test_a_lora_merged_after_the_switch_is_quantised_in():
    m = _model()
    first = _fwd(m)
    m.set_fp4_compute(True)
    on = _fwd(m)
    old = _records(m)
    m.load_lora_adapter(_lora_state(), adapter_name="lx")
    assert _records(m) == [], "the merge drops the records"
    merged = _fwd(m)
    new = _records(m)
    assert len(new) == 7 * LAYERS and all(a is not b for a, b in zip(old, new)), "rebuilt before the forward"
    assert not torch.equal(new[0].q, old[0].q), "from the merged weights"
    assert torch.isfinite(merged).all() and not torch.equal(merged, on), "(d)"
    m.delete_adapters("lx")
    assert torch.equal(_fwd(m), on), "un-merged: the fp4 forward of the base weights again"
    m.set_fp4_compute(False)
    assert _hash(_fwd(m)) == _hash(first), "(d) un-merged and switched off: the first forward bit for bit"


def test_refusals(tmp_path):
    from apex_studio_amd.lib import ApexMIError
    m = _model()
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: .*unknown Linear name\(s\) \['ffn'\]"):
        m.set_fp4_compute(True, linears=("ffn_up", "ffn"))
    m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: .*bfloat16 activation storage"):
        m.set_fp4_compute(True)
    m.set_storage_dtype(BF)
    m.set_residual_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: .*f32 residual stream"):
        m.set_fp4_compute(True)
    m.set_residual_dtype(BF)
    assert _records(m) == [], "a refusal attaches nothing"
    m.set_fp4_compute(True)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp4 compute is on .*bfloat16 activation storage"):
        m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp4 compute is on .*f32 residual stream"):
        m.set_residual_dtype(torch.float32)
    assert m.storage_dtype == BF and m.residual_dtype == BF and len(_records(m)) == 7 * LAYERS
    m.set_fp4_compute(False)
    m.set_residual_dtype(torch.float32).set_residual_dtype(BF)
    resident = _resident_fp8_model(tmp_path)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: .*resident quantised records.*cannot be combined"):
        resident.set_fp4_compute(True)


def test_engine_switch_runs_two_steps():
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    m = _model()
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)
    with pytest.raises(ValueError, match="fp4_linears needs fp4_compute"):
        WanT2VEngine(m, m, vae=vae, fp4_linears=("qkv",))
    eng = WanT2VEngine(m, m, vae=vae, fp4_compute=True)
    assert eng.fp4_compute and eng.fp4_linears is None and len(_records(m)) == 7 * LAYERS
    frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                     height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                     latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
    torch.cuda.synchronize()
    assert frames.shape[-2:] == (64, 64) and torch.isfinite(frames.float()).all() and float(frames.float().std()) > 0


def test_launch_counts_per_block():
    m = _model()
    with _count("quant_blocks_mxfp4", "gemm_mxfp4") as calls:
        _fwd(m)
    assert not calls["quant_blocks_mxfp4"] and not calls["gemm_mxfp4"], "the mode is off: no fp4 launch"
    m.set_fp4_compute(True)
    with _count("quant_blocks_mxfp4", "gemm_mxfp4") as calls:
        _fwd(m)
    assert len(calls["quant_blocks_mxfp4"]) == 7 * LAYERS and len(calls["gemm_mxfp4"]) == 7 * LAYERS, "(g) 7 + 7 per block"
    m.set_fp4_compute(True, linears=("qkv",))
    with _count("quant_blocks_mxfp4", "gemm_mxfp4") as calls:
        _fwd(m)
    assert len(calls["quant_blocks_mxfp4"]) == LAYERS and len(calls["gemm_mxfp4"]) == LAYERS
