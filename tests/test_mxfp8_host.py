"""Host-side checks of the MX block-scaled FP8 forms: the reference quantiser of tests/mxfp8_ref.py on planted
rows, the pure routing predicate `ops.fp8_mx_route`, the argument refusals of the new ops, and the exported names.  No GPU."""
import os

import pytest
import torch

from tests import gemm_fp8_probes as P
from tests import mxfp8_ref as R

F8 = torch.float8_e4m3fn
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _weight(N, K, compute="fp8", dtype=F8):
    w = _ops().Fp8Weight(torch.zeros(N, K).to(dtype), torch.ones(N))
    w.compute = compute
    return w


# ---- the reference quantiser --------------------------------------------------------------------------------------------------------
def test_planted_blocks_get_the_stated_scale_bytes():
    a = R.planted_rows()
    codes, sb = R.quant_blocks_ref(a)
    for (r, b, want), (name, _, _) in zip(R.planted_bytes(), R.PLANTS):
        assert int(sb[r, b]) == want, f"{name}: scale byte {int(sb[r, b])}, expected {want}"
    assert int(sb.max()) < 255 and not bool(((codes & 0x7F) == 0x7F).any()), "no byte is 255 and no code is NaN"
    assert not bool(codes[0, :32].any()), "a zero block has zero codes"


@pytest.mark.parametrize("rows", ["planted", "decades", "every-code"])
def test_scaled_maximum_is_at_most_448_and_nothing_is_clipped(rows):
    a = {"planted": R.planted_rows, "decades": R.decade_rows, "every-code": R.every_code_rows}[rows]()
    codes, sb = R.quant_blocks_ref(a)
    M, K = a.shape
    x = a.double().view(M, K // 32, 32)
    amax = x.abs().amax(2)
    e = sb.double() - 127
    scaled = amax / torch.exp2(e)
    assert float(scaled.max()) <= 448.0, "2^e is large enough: the clamp clips nothing"
    live = (amax > 0) & (sb > 1)                      # above the clamp of e at -126, 2^e is the SMALLEST such power of two
    assert bool((scaled[live] > 224.0).all()), "2^(e - 1) would not do"
    assert not bool(((codes & 0x7F) == 0x7F).any()) and int(sb.max()) < 255 and int(sb.min()) >= 1
    if rows == "decades":
        assert float(scaled.max()) > 440.0 and int(sb.max()) - int(sb.min()) > 150, "the rows span the scale range"
    if rows == "planted":
        assert float(scaled.max()) == 448.0, "the 448 x 2^k plants sit exactly on the largest code"


@pytest.mark.parametrize("rows", ["planted", "decades", "every-code"])
def test_dequantised_values_are_within_one_e4m3_step(rows):
    a = {"planted": R.planted_rows, "decades": R.decade_rows, "every-code": R.every_code_rows}[rows]()
    codes, sb = R.quant_blocks_ref(a)
    M, K = a.shape
    back = R.dequant(codes, sb)
    scale = torch.exp2(sb.double() - 127).repeat_interleave(32, dim=1)
    y = a.double() / scale
    err = (back - a.double()).abs() / scale
    assert bool((err <= R.e4m3_step(y)).all()), "every value within one e4m3 step of its input, in units of its block scale"
    assert bool((err <= R.e4m3_step(y) / 2).all()), "and in fact within half a step: round to nearest"


def test_reference_matches_torch_float8_conversion():
    """the definition-based rounding of tests.gemm_fp8_probes against torch's own float8 conversion, on the scaled values"""
    a = R.decade_rows()
    codes, sb = R.quant_blocks_ref(a)
    M, K = a.shape
    inv = torch.exp2((127 - sb.to(torch.int64)).double()).float().repeat_interleave(32, dim=1)
    y = (a.float() * inv).clamp(-448, 448)
    assert torch.equal(codes, y.to(F8).view(torch.uint8))


# ---- the route ------------------------------------------------------------------------------------------------------------------
def test_mx_route_accepts_the_ffn_pair_and_refuses_everything_else():
    ops = _ops()
    a = torch.zeros(200, 256, dtype=BF)
    up, down = _weight(512, 256), _weight(256, 512)
    out = torch.zeros(200, 256, dtype=BF)
    assert ops.fp8_mx_route(a, up, down, "gelu", "gate_res", out=out)
    assert ops.fp8_mx_route(a, up, down, "bias", "bias")
    assert ops.fp8_mx_route((200, 256), up, down, "gelu", "gate_res"), "a shape stands for the bf16 input"
    assert ops.fp8_mx_route((75600, 5120), _weight(13824, 5120), _weight(5120, 13824), "gelu", "gate_res")
    assert not ops.fp8_mx_route(a, up, down, "gate_res", "gate_res"), "the up epilogue is bias or gelu"
    assert not ops.fp8_mx_route(a, up, down, "gelu", "silu"), "a down epilogue the fp8 kernel does not have"
    assert not ops.fp8_mx_route(a, _weight(512, 256, compute="bf16"), down, "gelu", "gate_res"), "up is bf16 compute"
    assert not ops.fp8_mx_route(a, up, _weight(256, 512, compute="bf16"), "gelu", "gate_res"), "down is bf16 compute"
    assert not ops.fp8_mx_route(a, up, _weight(256, 512, dtype=torch.float8_e5m2), "gelu", "gate_res"), "an e5m2 record"
    assert not ops.fp8_mx_route(a, up, torch.zeros(256, 512, dtype=BF), "gelu", "gate_res"), "a bf16 weight"
    assert not ops.fp8_mx_route(a, _weight(528, 256), _weight(256, 528), "gelu", "gate_res"), "N_up % 128 != 0"
    assert not ops.fp8_mx_route(a, up, _weight(256, 640), "gelu", "gate_res"), "down does not read up's output"
    assert not ops.fp8_mx_route(a.float(), up, down, "gelu", "gate_res"), "float activations (the f32-storage mode)"
    assert not ops.fp8_mx_route(a, up, down, "gelu", "gate_res", out=out.float()), "a float residual stream"
    for which in (0, 1):
        pair = [_weight(512, 256), _weight(256, 512)]
        n, k = pair[which].shape
        pair[which].lora_A, pair[which].lora_B = torch.zeros(64, k, dtype=BF), torch.zeros(n, 64, dtype=BF)
        assert not ops.fp8_mx_route(a, pair[0], pair[1], "gelu", "gate_res"), "run-time LoRA factors on either record"


# ---- argument refusals (raised before any device or library is touched) --------------------------------------------------------------
def test_gemm_fp8_refuses_both_scale_kinds_and_lora_with_mx():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    codes, w = torch.zeros(8, 128, dtype=torch.uint8), _weight(128, 128)
    bs = torch.full((8, 4), 127, dtype=torch.uint8)
    with pytest.raises(ApexMIError, match="both given"):
        ops.gemm_fp8(codes, torch.ones(8), w, block_scales=bs)
    t, B = torch.zeros(8, 64, dtype=BF), torch.zeros(128, 64, dtype=BF)
    with pytest.raises(ApexMIError, match="LoRA"):
        ops.gemm_fp8(codes, torch.ones(8), w, lora_t=t, lora_B=B, block_scales=bs)
    with pytest.raises(ApexMIError, match="LoRA"):
        ops.gemm_fp8(codes, torch.ones(8), w, lora_t=t, lora_B=B, out_mx=(torch.zeros(8, 128, dtype=torch.uint8), bs))


def test_gemm_fp8_refuses_wrong_block_scale_dtype_and_shape():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    codes, w = torch.zeros(8, 128, dtype=torch.uint8), _weight(128, 128)
    with pytest.raises(ApexMIError, match=r"block_scales: expected torch.uint8"):
        ops.gemm_fp8(codes, None, w, block_scales=torch.ones(8, 4))
    with pytest.raises(ApexMIError, match=r"block_scales: expected \[8, 4\]"):
        ops.gemm_fp8(codes, None, w, block_scales=torch.zeros(8, 128, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match=r"block_scales: expected \[8, 4\]"):
        ops.gemm_fp8(codes, None, w, block_scales=torch.zeros(4, 4, dtype=torch.uint8))


def test_gemm_fp8_refuses_bad_mx_outputs():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    codes, sa = torch.zeros(8, 128, dtype=torch.uint8), torch.ones(8)
    q, s = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(8, 4, dtype=torch.uint8)
    gate, res = torch.ones(128), torch.zeros(8, 128, dtype=BF)
    with pytest.raises(ApexMIError, match="bias and gelu"):
        ops.gemm_fp8(codes, sa, _weight(128, 128), epilogue="gate_res", gate=gate, residual=res, out_mx=(q, s))
    with pytest.raises(ApexMIError, match=r"N % 128 == 0"):
        ops.gemm_fp8(codes, sa, _weight(144, 128), out_mx=(q, s))
    with pytest.raises(ApexMIError, match=r"out_mx codes: expected torch.uint8"):
        ops.gemm_fp8(codes, sa, _weight(128, 128), out_mx=(q.to(BF), s))
    with pytest.raises(ApexMIError, match=r"out_mx block_scales: expected \[8, 4\]"):
        ops.gemm_fp8(codes, sa, _weight(128, 128), out_mx=(q, torch.zeros(8, 8, dtype=torch.uint8)))
    with pytest.raises(ApexMIError, match=r"out_mx codes: expected \[8, 128\]"):
        ops.gemm_fp8(codes, sa, _weight(128, 128), out_mx=(torch.zeros(8, 256, dtype=torch.uint8), s))
    with pytest.raises(ApexMIError, match="pair"):
        ops.gemm_fp8(codes, sa, _weight(128, 128), out_mx=q)


def test_quantiser_and_grouped_forms_refuse_by_message():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    with pytest.raises(ApexMIError, match="expected torch.bfloat16"):
        ops.quant_blocks_mxfp8(torch.zeros(4, 128))
    with pytest.raises(ApexMIError, match=r"K % 128 == 0"):
        ops.quant_blocks_mxfp8(torch.zeros(4, 96, dtype=BF))
    with pytest.raises(ApexMIError, match=r"block_scales: expected \[4, 4\]"):
        ops.quant_blocks_mxfp8(torch.zeros(4, 128, dtype=BF), out=torch.zeros(4, 128, dtype=torch.uint8),
                               scale_out=torch.zeros(4, 2, dtype=torch.uint8))
    codes, w = torch.zeros(8, 128, dtype=torch.uint8), _weight(128, 128)
    bs = torch.full((8, 4), 127, dtype=torch.uint8)
    with pytest.raises(ApexMIError, match="both given"):
        ops.gemm_fp8_grouped([codes], [torch.ones(8)], [w], None, [None], block_scales_list=[bs])
    with pytest.raises(ApexMIError, match="q/k/v"):
        ops.gemm_fp8_grouped_qkv([codes], [None], [w], None, [None], "bias", [1], None, None, [0], 1, 1e-6, None, None, None, None,
                                 block_scales_list=[bs])


def test_exported_names_in_the_header_and_the_signatures():
    from apex_studio_amd import lib
    header = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    for name, nargs in (("apexmi_quant_blocks_mxfp8", 9), ("apexmi_gemm_fp8_mx", 25), ("apexmi_gemm_fp8_grouped_mx", 26)):
        assert f"int {name}(" in header
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    src = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "fp8_quant.h")).read()
    assert "mx_scale_byte" in src and "0x600000" in src, "the formula has one source"


def test_wan_and_engine_switches_need_fp8_compute():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.wan import WanTransformer3DModel
    import inspect
    sig = inspect.signature(WanTransformer3DModel.set_fp8_compute)
    assert sig.parameters["mx_ffn"].default is False, "off by default"
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    for eng in (WanT2VEngine, WanI2VEngine):
        assert inspect.signature(eng.__init__).parameters["fp8_mx_ffn"].default is False
