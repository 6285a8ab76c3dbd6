"""`FluxTransformer2DModel.set_fp4_compute` on the tiny synthetic bf16 Flux of tests/test_gpu_flux_fp8_compute.py (width
256, 2 heads, 2 + 2 blocks: K in {256, 1024, 1280}), built without the fp8 file: off is bit-identical, on is a finite, different,
bounded forward, a subset of the names attaches exactly its records, the fused q/k/v epilogue changes launches and not numbers, a
merged LoRA is quantised in, the refusals, the engine switch and the launch counts."""
import pytest
import torch

from tests.conftest import measured
from tests.test_gpu_flux_fp8_compute import BF, CFG, DEV, DOUBLE, H2, SINGLE, W2, _flux, _fwd, _hash
from tests.test_gpu_flux_fp8_lora import _adapter
from tests.test_gpu_wan_fp4_compute import _count, _rel

pytestmark = pytest.mark.gpu
DIM, MLP = 256, 1024
# weight elements per name: both streams of a double block, or one single block
ELEMS = {"qkv": 2 * 3 * DIM * DIM * DOUBLE, "attn_out": 2 * DIM * DIM * DOUBLE, "ffn_up": 2 * DIM * MLP * DOUBLE,
         "ffn_down": 2 * DIM * MLP * DOUBLE, "single_in": (3 * DIM * DIM + DIM * MLP) * SINGLE, "single_out": (DIM + MLP) * DIM * SINGLE}
RECORDS = {"qkv": 2 * DOUBLE, "attn_out": 2 * DOUBLE, "ffn_up": 2 * DOUBLE, "ffn_down": 2 * DOUBLE, "single_in": 2 * SINGLE,
           "single_out": SINGLE}


def _model():
    from tests.golden.seeded import synthetic_state_dict
    m = _flux()
    m.load_state_dict({k: v.to(BF) for k, v in synthetic_state_dict(m, 5).items()})
    return m


def _records(m):
    if not m._packed:
        return []
    return [w._fp4 for blk in m._fp4_blocks() for ws in m._fp4_weights(blk).values() for w in ws if getattr(w, "_fp4", None) is not None]


@pytest.fixture(scope="module")
def forwards():
    """every forward the tests compare, computed once on one model: off, all six names, the FFN pair, off again"""
    from apex_studio_amd import ops
    m = _model()
    f = {"first": _fwd(m)}
    assert _records(m) == []
    m.set_fp4_compute(True)
    recs = _records(m)
    f["n_all"], f["bytes_all"] = len(recs), m._fp4_bytes
    assert all(isinstance(r, ops.Mxfp4Weight) and r.compute == "fp4" for r in recs) and m._fp4_bytes == sum(r.nbytes() for r in recs)
    f["on"] = _fwd(m)
    f["on77"] = _fwd(m, 77)
    m.fuse_qkv = False
    f["on_two_pass"], f["on77_two_pass"] = _fwd(m), _fwd(m, 77)
    m.fuse_qkv = True
    m.set_fp4_compute(True, linears=("ffn_up", "ffn_down"))
    recs = _records(m)
    f["n_ffn"], f["bytes_ffn"], f["shapes_ffn"] = len(recs), m._fp4_bytes, {r.shape for r in recs}
    f["ffn"] = _fwd(m)
    m.set_fp4_compute(False)
    assert _records(m) == [] and m._fp4_bytes == 0
    f["off_again"] = _fwd(m)
    return f


def test_off_on_off_returns_the_first_forward(forwards):
    f = forwards
    assert _hash(f["off_again"]) == _hash(f["first"]), "on, then off: the forward is the first one bit for bit"
    assert torch.isfinite(f["on"]).all() and not torch.equal(f["on"], f["first"])


def test_a_subset_attaches_exactly_its_records_and_lies_between(forwards):
    f = forwards
    assert f["n_all"] == sum(RECORDS.values()) and f["n_ffn"] == RECORDS["ffn_up"] + RECORDS["ffn_down"]
    assert f["shapes_ffn"] == {(MLP, DIM), (DIM, MLP)}, "exactly the FF Linears of both streams of every double block"
    assert f["bytes_all"] == sum(ELEMS.values()) * 17 // 32, "17/32 of a byte per selected weight element"
    assert f["bytes_ffn"] == (ELEMS["ffn_up"] + ELEMS["ffn_down"]) * 17 // 32
    assert torch.isfinite(f["ffn"]).all() and not torch.equal(f["ffn"], f["first"]) and not torch.equal(f["ffn"], f["on"])
    rel_on, rel_ffn = _rel(f["on"], f["first"]), _rel(f["ffn"], f["first"])
    print(f"[flux fp4 compute] {DOUBLE} + {SINGLE} blocks of width {DIM}: rel-L2 against the bf16 forward, all six names {rel_on:.3e}, "
          f"the FF pair only {rel_ffn:.3e}")
    assert rel_ffn < rel_on, "fewer quantised Linears, a smaller error"
    # an error against the same model's own bf16 forward, never against an fp4 result; not a quality claim
    measured("flux.fp4_compute.tiny.rel_l2", rel_on, ALL_ON_BAR)


# measured 1.390e-1 on the MI355X (the FF pair alone: 9.940e-2; profiles/flux_fp4_measured.jsonl); the bar is 2x that
ALL_ON_BAR = 2.78e-1


@pytest.mark.parametrize("s_txt", [72, 77])
def test_the_fused_qkv_epilogue_changes_launches_not_numbers(forwards, s_txt):
    """s_txt 77: a text stream that is no multiple of 8 rows (the element-wise V^T store)"""
    tag = "on" if s_txt == 72 else "on77"
    assert torch.isfinite(forwards[tag]).all()
    assert _hash(forwards[tag + "_two_pass"]) == _hash(forwards[tag]), "fuse_qkv=False: gemm_mxfp4_grouped + qkv_prepare, the same bits"


def test_a_lora_merged_after_the_switch_is_quantised_in(forwards):
    m = _model()
    m.set_fp4_compute(True)
    on = _fwd(m)
    assert _hash(on) == _hash(forwards["on"])
    old = _records(m)
    m.load_lora_adapter(_adapter(), adapter_name="lx")
    assert _records(m) == [], "the merge drops the records"
    merged = _fwd(m)
    new = _records(m)
    assert len(new) == len(old) == sum(RECORDS.values()) and all(a is not b for a, b in zip(old, new)), "rebuilt before the forward"
    assert not torch.equal(new[0].q, old[0].q), "from the merged weights"
    assert torch.isfinite(merged).all() and not torch.equal(merged, on)
    m.delete_adapters("lx")
    assert torch.equal(_fwd(m), on), "un-merged: the fp4 forward of the base weights again"
    m.set_fp4_compute(False)
    assert _hash(_fwd(m)) == _hash(forwards["first"]), "un-merged and switched off: the first forward bit for bit"


def test_refusals():
    from apex_studio_amd.lib import ApexMIError
    m = _model()
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*unknown Linear name\(s\) \['ffn'\]"):
        m.set_fp4_compute(True, linears=("ffn_up", "ffn"))
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: set_fp4_compute\(False\) takes no `linears`"):
        m.set_fp4_compute(False, linears=("qkv",))
    m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*bfloat16 activation storage"):
        m.set_fp4_compute(True)
    m.set_storage_dtype(BF)
    m.set_residual_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*f32 residual stream"):
        m.set_fp4_compute(True)
    m.set_residual_dtype(BF)
    assert _records(m) == [], "a refusal attaches nothing"
    m.set_fp4_compute(True)
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: fp4 compute is on .*bfloat16 activation storage"):
        m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: fp4 compute is on .*f32 residual stream"):
        m.set_residual_dtype(torch.float32)
    assert m.storage_dtype == BF and m.residual_dtype == BF and len(_records(m)) == sum(RECORDS.values())
    m.set_fp4_compute(False)
    m.set_residual_dtype(torch.float32).set_residual_dtype(BF)


def test_a_resident_model_is_refused(tmp_path_factory):
    """a keep_fp8 load has no bf16 weight to copy, so the mode can never meet the fp8_* switches (the file recipe of
    tests/test_gpu_flux_fp8_compute.py)"""
    from safetensors.torch import save_file
    from apex_studio_amd import weights
    from apex_studio_amd.lib import ApexMIError
    from tests.golden.seeded import synthetic_state_dict
    m = _flux()
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(m, 5).items()}
    for k in [k for k in sd if m._fp8_resident_key(k) and sd[k].dim() == 2]:
        w = sd[k].float()
        s = (w.abs().max() / 448.0).reshape(())
        sd[k] = (w / s).to(torch.float8_e4m3fn)
        sd[k[:-len("weight")] + "scale_weight"] = s
    path = str(tmp_path_factory.mktemp("flux_fp4") / "flux_fp8.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    assert weights.load_checkpoint_into(m, [path], keep_fp8=True) == ([], [])
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*resident quantised records.*cannot be combined"):
        m.set_fp4_compute(True)
    assert m._fp4_linears is None and m._fp4_bytes == 0


def test_engine_switch_runs_two_steps():
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from tests.golden.seeded import seeded
    m = _model()
    with pytest.raises(ValueError, match="fp4_linears needs fp4_compute"):
        FluxT2IEngine(m, fp4_linears=("qkv",))
    with pytest.raises(ValueError, match="fp4_compute and fp8_compute cannot be combined"):
        FluxT2IEngine(m, fp4_compute=True, fp8_compute=True)
    assert m._fp4_linears is None, "refused up front: nothing was switched"
    eng = FluxT2IEngine(m, fp4_compute=True)
    assert eng.fp4_compute and eng.fp4_linears is None and len(_records(m)) == sum(RECORDS.values())
    lat = eng.run(prompt_embeds=seeded((1, 72, 256), 32).to(DEV), pooled_prompt_embeds=seeded((1, 64), 33).to(DEV), height=256,
                  width=256, num_inference_steps=2, guidance_scale=3.5, latents=seeded((1, H2 * W2, 64), 41).to(DEV),
                  return_latents=True)
    torch.cuda.synchronize()
    assert lat.shape == (1, H2 * W2, 64) and torch.isfinite(lat.float()).all() and float(lat.float().std()) > 0
    eng2 = FluxT2IEngine(_model(), fp4_compute=True, fp4_linears=("single_in",))
    assert eng2.fp4_linears == ("single_in",) and len(_records(eng2.transformer)) == RECORDS["single_in"]


NAMES = ("quant_blocks_mxfp4", "gemm_mxfp4_grouped_qkv", "gemm_mxfp4_grouped", "gemm_mxfp4", "gemm_grouped", "gemm_grouped_qkv")


def test_launch_counts_per_block():
    m = _model()
    with _count(*NAMES) as calls:
        _fwd(m)
    assert not any(calls[n] for n in NAMES[:4]), "the mode is off: no fp4 launch"
    assert len(calls["gemm_grouped"]) + len(calls["gemm_grouped_qkv"]) == 4 * DOUBLE + SINGLE
    m.set_fp4_compute(True)
    with _count(*NAMES) as calls:
        _fwd(m)
    n = {k: len(v) for k, v in calls.items()}
    # per double block: 4 quantise launches (XN, att, XN, FFH), the fused QKV pair, 3 grouped pairs; per single block: 2 quantise
    # launches (XN; CAT inside ops.gemm), the fused QKV + MLP-up launch, proj_out through ops.gemm's fp4 route
    assert n["quant_blocks_mxfp4"] == 4 * DOUBLE + 2 * SINGLE and n["gemm_mxfp4_grouped_qkv"] == DOUBLE + SINGLE, n
    assert n["gemm_mxfp4_grouped"] == 3 * DOUBLE and n["gemm_mxfp4"] == SINGLE and n["gemm_grouped"] == 0 and n["gemm_grouped_qkv"] == 0, n
    m.fuse_qkv = False
    with _count(*NAMES) as calls:
        _fwd(m)
    n = {k: len(v) for k, v in calls.items()}
    assert n["gemm_mxfp4_grouped_qkv"] == 0 and n["gemm_mxfp4_grouped"] == 4 * DOUBLE + SINGLE and n["gemm_grouped"] == 0, n
    m.fuse_qkv = True
    m.set_fp4_compute(True, linears=("attn_out", "single_out"))
    with _count(*NAMES) as calls:
        _fwd(m)
    n = {k: len(v) for k, v in calls.items()}
    assert n["quant_blocks_mxfp4"] == DOUBLE + SINGLE and n["gemm_mxfp4_grouped"] == DOUBLE and n["gemm_mxfp4"] == SINGLE, n
    assert n["gemm_mxfp4_grouped_qkv"] == 0 and n["gemm_grouped"] + n["gemm_grouped_qkv"] == 3 * DOUBLE + SINGLE, n
