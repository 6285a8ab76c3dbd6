"""The MXFP4 reference (tests/mxfp4_ref.py) against itself, the exactness preconditions of the GPU probes (tests/test_gpu_mxfp4.py)
computed in integers, and the host-side surface of the fp4 compute mode (route, exports, switches).  No GPU."""
import inspect
import os

import pytest
import torch

from tests import gemm_probes as G
from tests import mxfp4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def test_planted_scale_bytes():
    q, sb = R.quant_blocks_ref(R.planted_rows())
    for r, b, want in R.planted_bytes():
        assert int(sb[r, b]) == want, R.PLANTS[r][0]
    assert int(sb.max()) < 255
    codes = R.unpack(q)
    assert int(codes[0, :32].max()) == 0, "a zero block has zero codes"
    assert int(codes[5, 5 * 32 + 7]) == 0, "2^-133 x 2^126 = 2^-7 rounds to zero"
    assert int(codes[1, 32 + 7]) == 7 and int(codes[2, 64 + 7]) == 13, "6 x 2^5 -> 6; -6.25 x 2^5 at one scale byte up -> -3"


def test_all_sixteen_codes_are_emitted():
    q, sb = R.quant_blocks_ref(R.every_code_rows())
    wq, ws = R.every_code_want()
    assert torch.equal(q, wq) and torch.equal(sb, ws)
    assert set(R.unpack(q).flatten().tolist()) == set(range(16))


def test_ties_land_on_even_codes():
    a, want = R.tie_row()
    q, sb = R.quant_blocks_ref(a)
    assert bool((sb == 127).all())
    got = R.dequant(q, sb)
    assert torch.equal(got.float(), want)
    tied = torch.isin(a.float().abs(), torch.tensor([v for v, _ in R.TIES]))
    assert int(tied.sum()) == 14 * (a.shape[1] // 32) and bool((R.unpack(q)[tied] % 2 == 0).all())
    assert torch.equal(torch.signbit(R.VALUES[R.unpack(q).long()]), torch.signbit(a.float())), "the sign bit survives a zero magnitude"
    away, _ = R.quant_blocks_ref(a, tie="away")
    assert not torch.equal(away, q), "the ties-away mutant is told apart"


@pytest.mark.parametrize("rows", ["every_code", "decade", "random"])
def test_requantising_fp4_exact_data_is_the_identity(rows):
    a = {"every_code": R.every_code_rows, "decade": R.decade_rows, "random": lambda: R.random_rows(7, 768)}[rows]()
    q, sb = R.quant_blocks_ref(a)
    d = R.dequant(q, sb)
    d16 = d.float().to(BF)
    assert torch.equal(d16.double(), d), "dequant output is bf16-exact"
    q2, sb2 = R.quant_blocks_ref(d16)
    assert torch.equal(R.dequant(q2, sb2), d), "the values are a fixed point"
    # (q, s) itself comes back wherever the block's largest magnitude is 4 or 6 x 2^e: a smaller one re-quantises at a finer scale
    blocks = lambda c: R.unpack(c).view(c.shape[0], -1, 32)          # noqa: E731
    same = (blocks(q) & 7).amax(2) >= 6
    assert bool(same.any()) and (rows != "every_code" or bool(same.all()))
    assert torch.equal(sb2[same], sb[same]) and torch.equal(blocks(q2)[same], blocks(q)[same])


def test_every_bf16_rows_cover_every_scale_byte_and_code():
    q, sb = R.quant_blocks_ref(R.every_bf16_rows())
    assert set(sb.flatten().tolist()) >= set(range(1, 254)) and int(sb.max()) == 253
    for e in R.CODE_EXPONENTS:
        a = R.every_bf16_rows(e)
        q, sb = R.quant_blocks_ref(a)
        used = a.float().view(-1, 32).abs().amax(1) > 0
        assert bool((sb.flatten()[used] == 127 + e).all()) and set(R.unpack(q).flatten().tolist()) == set(range(16))


def test_pack_is_torchs_float4_x2_order():
    codes = torch.arange(16, dtype=torch.uint8).repeat(2).view(1, 32)
    q = R.pack(codes)
    assert int(q[0, 0]) == 0x10 and int(q[0, 1]) == 0x32 and torch.equal(R.unpack(q), codes)


def test_lane_map_probe_is_exact_and_tells_the_four_wrong_permutations_apart():
    L = R.lane_map()
    assert L.span_log2() < G.SPAN_BITS
    want = L.want()
    assert int((want != 0).sum()) == 128 * 4, "C[m, n] is non-zero exactly where m = n mod 32"
    for name, wrong in L.mutants().items():
        assert not torch.equal(wrong.float().to(BF), want), name


@pytest.mark.parametrize("case", R.fixed_cases(), ids=lambda c: "-".join(map(str, c)))
def test_fixed_point_cases_meet_the_exactness_condition(case):
    op = R.fixed_point(*case)
    for epi in ("bias", "gate_res"):
        for bias in (True, False):
            assert op.span_log2(epi, bias) < G.SPAN_BITS
            ref = op.ref(epi, bias)
            assert torch.equal(ref.float().double(), ref), "the exact result is a float32"
    # the integer dot products are what the float64 reference of the format computes
    assert torch.equal(R.gemm_ref(op.qa, op.sa, op.qw, op.sw), op.acc_units.double() * 2.0 ** R.GRID_LOG2)
    assert set(R.unpack(op.qa).flatten().tolist()) <= {0, 2, 4, 5, 6, 7, 10, 12, 13, 14, 15}
    if case[0] * case[1] >= 2048:
        assert G.tie_fraction(op.ref("bias")) > 0, "the bf16 store rounds a tie somewhere"


def test_route_is_pure_and_needs_a_record():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    w = torch.zeros(32, 256, dtype=BF)
    a = torch.zeros(5, 256, dtype=BF)
    assert not ops.mxfp4_route(a, w), "no record attached"
    rec = ops.Mxfp4Weight(torch.zeros(32, 128, dtype=torch.uint8), torch.zeros(32, 8, dtype=torch.uint8))
    assert rec.shape == (32, 256) and rec.nbytes() == 32 * 128 + 32 * 8 and rec.compute == "fp4"
    w._fp4 = rec
    assert ops.mxfp4_route(a, w) and ops.mxfp4_route(a, rec) and ops.mxfp4_route(a, w, torch.zeros(5, 32, dtype=BF), "gate_res")
    assert not ops.mxfp4_route(a.float(), w) and not ops.mxfp4_route(a, w, torch.zeros(5, 32)), "float rows keep the bf16 path"
    assert not ops.mxfp4_route(a, w, None, "silu") and not ops.mxfp4_route(torch.zeros(5, 384, dtype=BF), w)
    w384 = torch.zeros(32, 384, dtype=BF)
    w384._fp4 = ops.Mxfp4Weight(torch.zeros(32, 192, dtype=torch.uint8), torch.zeros(32, 12, dtype=torch.uint8))
    assert not ops.mxfp4_route(torch.zeros(5, 384, dtype=BF), w384), "K % 256"
    w24 = ops.Mxfp4Weight(torch.zeros(24, 128, dtype=torch.uint8), torch.zeros(24, 8, dtype=torch.uint8))
    assert not ops.mxfp4_route(a, w24), "N % 16"
    rec.compute = "bf16"
    assert not ops.mxfp4_route(a, w)
    with pytest.raises(Exception, match="scales"):
        ops.Mxfp4Weight(torch.zeros(32, 128, dtype=torch.uint8), torch.zeros(32, 7, dtype=torch.uint8))


def test_exports_build_lists_and_the_formulas_one_source():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import build, lib
    header = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    for name, nargs in (("apexmi_quant_blocks_mxfp4", 9), ("apexmi_gemm_mxfp4", 19)):
        assert f"int {name}(" in header
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert "gemm_mxfp4.hip" in build.SOURCES and build.NO_SPILL["gemm_mxfp4.hip"] == ["gemm_mxfp4_kernel"]
    src = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "fp8_quant.h")).read()
    assert "mx4_scale_byte" in src and "0x400000" in src, "the formula has one source"
    unit = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "gemm_mxfp4.hip")).read()
    assert '#include "fp8_quant.h"' in unit and "0x400000" not in unit and "fp8_epilogue<EPI, false>" in unit


def test_wan_and_engine_switches():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from apex_studio_amd.wan import WanTransformer3DModel
    sig = inspect.signature(WanTransformer3DModel.set_fp4_compute)
    assert sig.parameters["linears"].default is None
    assert WanTransformer3DModel._FP4_LINEARS == ("qkv", "attn_out", "cross_q", "cross_kv", "cross_out", "ffn_up", "ffn_down")
    for eng in (WanT2VEngine, WanI2VEngine):
        p = inspect.signature(eng.__init__).parameters
        assert p["fp4_compute"].default is False and p["fp4_linears"].default is None
