"""`WanTransformer3DModel.set_fp6_compute` on the tiny synthetic bf16 Wan model of tests/test_gpu_wan_fp8_compute.py
(width 256, 3 blocks, as tests/test_gpu_wan_fp4_compute.py builds it): off is bit-identical, on is a finite, different, bounded
forward whose error is under half of the fp4 mode's, the mix with fp4 on disjoint Linears, a merged LoRA is quantised in, the
refusals, the engine switch and the launch counts."""
import pytest
import torch

from tests.conftest import measured
from tests.test_gpu_wan_fp4_compute import _count, _lora_state, _model, _rel
from tests.test_gpu_wan_fp8_compute import BF, DEV, DIM, FFN, LAYERS, _fwd, _hash
from tests.test_gpu_wan_fp8_compute import _model as _resident_fp8_model

pytestmark = pytest.mark.gpu
ATTENTION = ("qkv", "attn_out", "cross_q", "cross_kv", "cross_out")
FFN_PAIR = ("ffn_up", "ffn_down")


def _records(m, slot="_fp6"):
    if not m._packed:
        return []
    return [getattr(w, slot) for blk in m.blocks for w in m._fp4_weights(blk).values() if getattr(w, slot, None) is not None]


def test_off_is_bit_identical_on_is_bounded_and_under_half_of_the_fp4_error():
    from apex_studio_amd import ops
    m = _model()
    first = _fwd(m)
    assert _records(m) == []
    m.set_fp6_compute(True)
    recs = _records(m)
    assert len(recs) == 7 * LAYERS and all(isinstance(r, ops.Mxfp6Weight) and r.compute == "fp6" for r in recs)
    assert _records(m, "_fp4") == [], "no fp4 record beside an fp6 one"
    assert m._fp6_bytes == sum(r.nbytes() for r in recs) == LAYERS * (8 * DIM * DIM + 2 * DIM * FFN) * 25 // 32
    on = _fwd(m)
    m.set_fp6_compute(True, linears=FFN_PAIR)
    recs = _records(m)
    assert len(recs) == 2 * LAYERS and {r.shape for r in recs} == {(FFN, DIM), (DIM, FFN)}, "exactly the two FFN Linears of every block"
    ffn = _fwd(m)
    m.set_fp6_compute(False)
    assert _records(m) == [] and m._fp6_bytes == 0 and m._fp6_linears is None
    assert _hash(_fwd(m)) == _hash(first), "on, then off: the forward is the first one bit for bit"
    assert torch.isfinite(on).all() and not torch.equal(on, first)
    assert torch.isfinite(ffn).all() and not torch.equal(ffn, first) and not torch.equal(ffn, on)
    # the fp4 mode of the same model on the same inputs
    m.set_fp4_compute(True)
    on4 = _fwd(m)
    m.set_fp4_compute(True, linears=FFN_PAIR)
    ffn4 = _fwd(m)
    m.set_fp4_compute(False)
    assert _hash(_fwd(m)) == _hash(first)
    rel_on, rel_ffn, rel_on4, rel_ffn4 = _rel(on, first), _rel(ffn, first), _rel(on4, first), _rel(ffn4, first)
    print(f"[wan fp6 compute] {LAYERS} blocks of width {DIM}: rel-L2 against the bf16 forward, all seven Linears {rel_on:.3e} (fp4: "
          f"{rel_on4:.3e}), the FFN pair only {rel_ffn:.3e} (fp4: {rel_ffn4:.3e})")
    assert rel_ffn < rel_on, "fewer quantised Linears, a smaller error"
    assert rel_on < 0.5 * rel_on4 and rel_ffn < 0.5 * rel_ffn4, "three mantissa bits against one: about a quarter is expected"
    measured("wan.fp6_compute.tiny.rel_l2", rel_on, ALL_ON_BAR)
    measured("wan.fp6_compute.tiny.ffn.rel_l2", rel_ffn, FFN_BAR)


# measured on the MI355X (profiles/gemm_mxfp6_measured.jsonl): all seven 6.492e-3 (the fp4 mode: 1.589e-2), the FFN pair alone 5.286e-3
# (fp4: 1.362e-2); the bars are 2x the measured values
ALL_ON_BAR = 1.3e-2
FFN_BAR = 1.06e-2


def test_mixed_mode_fp6_attention_fp4_ffn():
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    m = _model()
    first = _fwd(m)
    m.set_fp6_compute(True)
    on6 = _fwd(m)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp4_compute\(linears=\): \['ffn_up', 'ffn_down'\] multiply as fp6 already"):
        m.set_fp4_compute(True, linears=FFN_PAIR)
    assert _records(m, "_fp4") == [] and len(_records(m)) == 7 * LAYERS, "the refusal changed nothing"
    m.set_fp6_compute(False)
    m.set_fp4_compute(True)
    on4 = _fwd(m)
    m.set_fp4_compute(True, linears=FFN_PAIR)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(linears=\): \['ffn_up', 'ffn_down'\] multiply as fp4 already"):
        m.set_fp6_compute(True)
    m.set_fp6_compute(True, linears=ATTENTION)
    r6, r4 = _records(m), _records(m, "_fp4")
    assert len(r6) == 5 * LAYERS and all(isinstance(r, ops.Mxfp6Weight) for r in r6)
    assert len(r4) == 2 * LAYERS and all(isinstance(r, ops.Mxfp4Weight) for r in r4)
    for blk in m.blocks:
        for w in m._fp4_weights(blk).values():
            assert (getattr(w, "_fp4", None) is None) != (getattr(w, "_fp6", None) is None), "one record per weight, never both"
    names = ("quant_blocks_mxfp6", "gemm_mxfp6", "quant_blocks_mxfp4", "gemm_mxfp4")
    with _count(*names) as calls:
        mixed = _fwd(m)
    assert [len(calls[n]) for n in names] == [5 * LAYERS, 5 * LAYERS, 2 * LAYERS, 2 * LAYERS], "5 + 5 fp6 and 2 + 2 fp4 launches per block"
    rel6, rel4, relm = _rel(on6, first), _rel(on4, first), _rel(mixed, first)
    print(f"[wan fp6 compute] mixed (fp6 attention projections, fp4 FFN pair) rel-L2 {relm:.3e}; fp6 all seven {rel6:.3e}, fp4 all seven {rel4:.3e}")
    assert rel6 < relm < rel4, "the mix lies between the two pure modes"
    m.set_fp6_compute(False)
    assert _records(m) == [] and len(_records(m, "_fp4")) == 2 * LAYERS and m._fp4_linears == FFN_PAIR, "off detaches only the fp6 records"
    with _count(*names) as calls:
        _fwd(m)
    assert [len(calls[n]) for n in names] == [0, 0, 2 * LAYERS, 2 * LAYERS]
    m.set_fp4_compute(False)
    assert _hash(_fwd(m)) == _hash(first)


def test_a_lora_merged_after_the_switch_is_quantised_in():
    m = _model()
    first = _fwd(m)
    m.set_fp6_compute(True)
    on = _fwd(m)
    old = _records(m)
    m.load_lora_adapter(_lora_state(), adapter_name="lx")
    assert _records(m) == [], "the merge drops the records"
    merged = _fwd(m)
    new = _records(m)
    assert len(new) == 7 * LAYERS and all(a is not b for a, b in zip(old, new)), "rebuilt before the forward"
    assert not torch.equal(new[0].q, old[0].q), "from the merged weights"
    assert torch.isfinite(merged).all() and not torch.equal(merged, on)
    m.delete_adapters("lx")
    assert torch.equal(_fwd(m), on), "un-merged: the fp6 forward of the base weights again"
    m.set_fp6_compute(False)
    assert _hash(_fwd(m)) == _hash(first), "un-merged and switched off: the first forward bit for bit"


def test_refusals(tmp_path):
    from apex_studio_amd.lib import ApexMIError
    m = _model()
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(linears=\): unknown Linear name\(s\) \['ffn'\]"):
        m.set_fp6_compute(True, linears=("ffn_up", "ffn"))
    m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute .*bfloat16 activation storage"):
        m.set_fp6_compute(True)
    m.set_storage_dtype(BF)
    m.set_residual_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute .*f32 residual stream"):
        m.set_fp6_compute(True)
    m.set_residual_dtype(BF)
    assert _records(m) == [], "a refusal attaches nothing"
    m.set_fp6_compute(True)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp6 compute is on .*bfloat16 activation storage"):
        m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp6 compute is on .*f32 residual stream"):
        m.set_residual_dtype(torch.float32)
    assert m.storage_dtype == BF and m.residual_dtype == BF and len(_records(m)) == 7 * LAYERS
    m.set_fp6_compute(False)
    m.set_residual_dtype(torch.float32).set_residual_dtype(BF)
    resident = _resident_fp8_model(tmp_path)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute .*resident quantised records.*cannot be combined"):
        resident.set_fp6_compute(True)


def test_engine_kwargs_reach_the_model():
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    m = _model()
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)
    with pytest.raises(ValueError, match="fp6_linears needs fp6_compute"):
        WanT2VEngine(m, m, vae=vae, fp6_linears=("qkv",))
    eng = WanT2VEngine(m, m, vae=vae, fp6_compute=True, fp6_linears=ATTENTION, fp4_compute=True, fp4_linears=FFN_PAIR)
    assert eng.fp6_compute and eng.fp6_linears == ATTENTION and m._fp6_linears == ATTENTION and m._fp4_linears == FFN_PAIR
    assert len(_records(m)) == 5 * LAYERS and len(_records(m, "_fp4")) == 2 * LAYERS
    frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                     height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                     latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
    torch.cuda.synchronize()
    assert frames.shape[-2:] == (64, 64) and torch.isfinite(frames.float()).all() and float(frames.float().std()) > 0


def test_launch_counts_per_block():
    m = _model()
    with _count("quant_blocks_mxfp6", "gemm_mxfp6") as calls:
        _fwd(m)
    assert not calls["quant_blocks_mxfp6"] and not calls["gemm_mxfp6"], "the mode is off: no fp6 launch"
    m.set_fp6_compute(True)
    with _count("quant_blocks_mxfp6", "gemm_mxfp6") as calls:
        _fwd(m)
    assert len(calls["quant_blocks_mxfp6"]) == 7 * LAYERS and len(calls["gemm_mxfp6"]) == 7 * LAYERS, "7 + 7 per block"
    m.set_fp6_compute(True, linears=("qkv",))
    with _count("quant_blocks_mxfp6", "gemm_mxfp6") as calls:
        _fwd(m)
    assert len(calls["quant_blocks_mxfp6"]) == LAYERS and len(calls["gemm_mxfp6"]) == LAYERS
