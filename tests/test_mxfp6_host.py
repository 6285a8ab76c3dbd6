"""The MXFP6 reference (tests/mxfp6_ref.py) against itself, the exactness preconditions of the GPU probes (tests/test_gpu_mxfp6.py)
computed in integers, and the host-side surface of the fp6 compute mode (route, records, exports, switches).  No GPU."""
import inspect
import os

import pytest
import torch

from tests import gemm_probes as G
from tests import mxfp4_ref as R4
from tests import mxfp6_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_the_64_codes_are_the_ocp_e2m3_values_and_round_trip():
    for c in range(64):
        s, e, m = c >> 5, (c >> 3) & 3, c & 7
        v = (m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1)) * (-1 if s else 1)
        assert float(R.VALUES[c]) == v and bool(torch.signbit(R.VALUES[c])) == bool(s)
    codes = torch.arange(64, dtype=torch.uint8).view(2, 32)
    assert torch.equal(R.e2m3_nearest(R.VALUES.view(2, 32)), codes), "every value is its own nearest code, -0 included"
    assert torch.equal(R.VALUES.float().to(BF).double(), R.VALUES), "every value is bf16-exact"


def test_pack_is_the_little_endian_192_bit_block():
    codes = ((torch.arange(64) * 37 + 5) % 64).to(torch.uint8).view(1, 64)
    q = R.pack(codes)
    assert tuple(q.shape) == (1, 48) and torch.equal(R.unpack(q), codes)
    for b in range(2):
        big = int.from_bytes(bytes(q[0, 24 * b:24 * (b + 1)].tolist()), "little")
        assert [(big >> (6 * j)) & 63 for j in range(32)] == codes[0, 32 * b:32 * (b + 1)].tolist()
    q, sb = R.quant_blocks_ref(R.random_rows(7, 768))
    assert tuple(q.shape) == (7, 768 * 3 // 4) and tuple(sb.shape) == (7, 24)


def test_planted_scale_bytes():
    q, sb = R.quant_blocks_ref(R.planted_rows())
    for r, b, want in R.planted_bytes():
        assert int(sb[r, b]) == want, R.PLANTS[r][0]
    assert int(sb.max()) < 255
    codes = R.unpack(q)
    assert int(codes[0, :32].max()) == 0, "a zero block has zero codes"
    assert int(codes[5, 5 * 32 + 7]) == 0, "2^-133 x 2^126 = 2^-7 rounds to zero"
    assert int(codes[1, 32 + 7]) == 31, "7.5 x 2^5 at 2^5 -> 7.5: nothing clips"
    assert int(codes[2, 64 + 7]) == 32 + 23, "-241 at one scale byte up -> -3.75"
    assert int(codes[4, 4 * 32 + 7]) == 24, "bf16 max / 2^126 = 3.98 -> 4"


def test_all_64_codes_are_emitted():
    q, sb = R.quant_blocks_ref(R.every_code_rows())
    wq, ws = R.every_code_want()
    assert torch.equal(q, wq) and torch.equal(sb, ws)
    assert set(R.unpack(q).flatten().tolist()) == set(range(64))


def test_ties_land_on_even_codes():
    a, want = R.tie_row()
    q, sb = R.quant_blocks_ref(a)
    assert bool((sb == 127).all())
    got = R.dequant(q, sb)
    assert torch.equal(got.float(), want)
    tied = a.float().abs() != R.TOP
    assert int(tied.sum()) == 31 * (a.shape[1] // 32) and bool((R.unpack(q)[tied] % 2 == 0).all())
    assert len({v for v, _ in R.TIES}) == 31 and all(R.MAGS[c] in (R.MAGS[i], R.MAGS[i + 1]) for i, (_, c) in enumerate(R.TIES))
    assert torch.equal(torch.signbit(R.VALUES[R.unpack(q).long()]), torch.signbit(a.float())), "the sign bit survives a zero magnitude"
    away, _ = R.quant_blocks_ref(a, tie="away")
    assert not torch.equal(away, q), "the ties-away mutant is told apart"


@pytest.mark.parametrize("rows", ["every_code", "decade", "random"])
def test_requantising_fp6_exact_data_is_the_identity(rows):
    a = {"every_code": R.every_code_rows, "decade": R.decade_rows, "random": lambda: R.random_rows(7, 768)}[rows]()
    q, sb = R.quant_blocks_ref(a)
    d = R.dequant(q, sb)
    d16 = d.float().to(BF)
    assert torch.equal(d16.double(), d), "dequant output is bf16-exact"
    q2, sb2 = R.quant_blocks_ref(d16)
    assert torch.equal(R.dequant(q2, sb2), d), "the values are a fixed point"
    # (q, s) itself comes back wherever the block's largest magnitude is at least 4 x 2^e: a smaller one re-quantises at a finer scale
    blocks = lambda c: R.unpack(c).view(c.shape[0], -1, 32)          # noqa: E731
    same = (blocks(q) & 31).amax(2) >= 24
    assert bool(same.any()) and (rows != "every_code" or bool(same.all()))
    assert torch.equal(sb2[same], sb[same]) and torch.equal(blocks(q2)[same], blocks(q)[same])


def test_every_bf16_rows_cover_every_scale_byte_and_code():
    q, sb = R.quant_blocks_ref(R.every_bf16_rows())
    assert set(sb.flatten().tolist()) >= set(range(1, 254)) and int(sb.max()) == 253
    for e in R.CODE_EXPONENTS:
        a = R.every_bf16_rows(e)
        q, sb = R.quant_blocks_ref(a)
        used = a.float().view(-1, 32).abs().amax(1) > 0
        assert bool((sb.flatten()[used] == 127 + e).all()) and set(R.unpack(q).flatten().tolist()) == set(range(64))


def test_e2m3_product_error_is_at_most_half_of_e2m1_on_the_same_operands():
    g = torch.Generator().manual_seed(20260)
    a, w = torch.randn(256, 1024, generator=g).to(BF), torch.randn(256, 1024, generator=g).to(BF)
    exact = a.double() @ w.double().T
    rel = lambda y: float((y - exact).norm() / exact.norm())          # noqa: E731
    r6 = rel(R.gemm_ref(*R.quant_blocks_ref(a), *R.quant_blocks_ref(w)))
    r4 = rel(R4.gemm_ref(*R4.quant_blocks_ref(a), *R4.quant_blocks_ref(w)))
    print(f"[mxfp6 host] rel-L2 against the f64 product, N(0,1) 256 x 256 x 1024: e2m3 {r6:.3e}, e2m1 {r4:.3e}, ratio {r6 / r4:.3f}")
    assert r6 <= 0.5 * r4


# ------------------------------------------------------------------------------------------- preconditions of the GPU probes
def test_lane_map_probe_is_exact_and_tells_the_wrong_permutations_apart():
    L = R.lane_map()
    assert L.span_log2() < G.SPAN_BITS
    want = L.want()
    assert int((want != 0).sum()) == 128 * 4, "C[m, n] is non-zero exactly where m = n mod 32"
    muts = L.mutants()
    assert len(muts) == 7
    for name, wrong in muts.items():
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
    assert op.gelu_subnormal_share() <= 0.002, "the gelu check would measure the epilogue's flush of bf16 subnormals (see mxfp6_ref)"
    used = set(R.unpack(op.qa).flatten().tolist())
    assert {c >> 3 & 3 for c in used} == {0, 1, 2, 3} and {c & 7 for c in used} == set(range(8)) and {c >> 5 for c in used} == {0, 1}


def test_fixed_point_k_sizes_are_one_two_and_an_odd_number_of_k_tiles():
    assert [k // R.K_TILE for k in R.FIXED_KS] == [1, 2, 5] and R.BAND_CASE == (1100, 144, R.K_TILE)
    unit = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "gemm_mxfp6.hip")).read()
    assert f"constexpr int X6_KT = {R.K_TILE};" in unit


# ------------------------------------------------------------------------------------------------------- predicate and records
def test_route_is_pure_and_needs_a_record():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    w = torch.zeros(32, 128, dtype=BF)
    a = torch.zeros(5, 128, dtype=BF)
    assert not ops.mxfp6_route(a, w), "no record attached"
    rec = ops.Mxfp6Weight(torch.zeros(32, 96, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.uint8))
    assert rec.shape == (32, 128) and rec.nbytes() == 32 * 96 + 32 * 4 and rec.compute == "fp6"
    w._fp6 = rec
    assert ops.mxfp6_route(a, w) and ops.mxfp6_route(a, rec) and ops.mxfp6_route(a, w, torch.zeros(5, 32, dtype=BF), "gate_res")
    assert ops.mxfp6_route(a.to("meta"), rec), "meta tensors are fine"
    assert not ops.mxfp6_route(a.float(), w) and not ops.mxfp6_route(a, w, torch.zeros(5, 32)), "float rows keep the bf16 path"
    assert not ops.mxfp6_route(a, w, None, "silu") and not ops.mxfp6_route(torch.zeros(5, 256, dtype=BF), w)
    assert not ops.mxfp6_route(a[:, ::2], w) and not ops.mxfp6_route(a.view(5, 2, 64), w)
    w384 = ops.Mxfp6Weight(torch.zeros(32, 288, dtype=torch.uint8), torch.zeros(32, 12, dtype=torch.uint8))
    assert ops.mxfp6_route(torch.zeros(5, 384, dtype=BF), w384), "K % 128 is enough: 384 is not a K of the fp4 route"
    w96 = ops.Mxfp6Weight(torch.zeros(32, 72, dtype=torch.uint8), torch.zeros(32, 3, dtype=torch.uint8))
    assert not ops.mxfp6_route(torch.zeros(5, 96, dtype=BF), w96), "K % 128"
    w24 = ops.Mxfp6Weight(torch.zeros(24, 96, dtype=torch.uint8), torch.zeros(24, 4, dtype=torch.uint8))
    assert not ops.mxfp6_route(a, w24), "N % 16"
    assert not ops.mxfp4_route(a, w) and not ops.mxfp6_route(a, torch.zeros(32, 128, dtype=BF)), "the fp4 predicate does not see an fp6 record"
    rec.compute = "bf16"
    assert not ops.mxfp6_route(a, w)


def test_record_shape_refusals_on_cpu_tensors():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    with pytest.raises(ApexMIError, match="scales"):
        ops.Mxfp6Weight(torch.zeros(32, 96, dtype=torch.uint8), torch.zeros(32, 3, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match="scales"):
        ops.Mxfp6Weight(torch.zeros(32, 96, dtype=torch.uint8), torch.zeros(31, 4, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match="whole 24-byte blocks"):
        ops.Mxfp6Weight(torch.zeros(32, 100, dtype=torch.uint8), torch.zeros(32, 4, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match="torch.uint8"):
        ops.Mxfp6Weight(torch.zeros(32, 96, dtype=torch.int8), torch.zeros(32, 4, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match="torch.uint8"):
        ops.Mxfp6Weight(torch.zeros(32, 96, dtype=torch.uint8), None)
    # the record's own dequantiser is the restatement's (plain torch: runs on CPU tensors)
    q, sb = R.quant_blocks_ref(R.decade_rows(4, 128))
    assert torch.equal(ops.Mxfp6Weight(q, sb).dequant().double(), R.dequant(q, sb))
    assert ops.E2M3_VALUES == R.MAGS


def test_exports_build_lists_and_the_formulas_one_source():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import build, lib
    header = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    for name, nargs in (("apexmi_quant_blocks_mxfp6", 9), ("apexmi_gemm_mxfp6", 19)):
        assert f"int {name}(" in header
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs
    assert lib.SIGNATURES["apexmi_gemm_mxfp6"] == lib.SIGNATURES["apexmi_gemm_mxfp4"], "the same signature as the fp4 entry point"
    assert "gemm_mxfp6.hip" in build.SOURCES and build.NO_SPILL["gemm_mxfp6.hip"] == ["gemm_mxfp6_kernel"]
    src = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "fp8_quant.h")).read()
    assert "mx6_scale_byte" in src and "0x700000" in src, "the formula has one source"
    unit = open(os.path.join(ROOT, "apex-studio_amd", "csrc", "gemm_mxfp6.hip")).read()
    assert '#include "fp8_quant.h"' in unit and "0x700000" not in unit and "fp8_epilogue<EPI, false>" in unit
    assert "__launch_bounds__(256, 2) void gemm_mxfp6_kernel" in unit


# --------------------------------------------------------------------------------------------------------------------- switches
SEVEN = ("qkv", "attn_out", "cross_q", "cross_kv", "cross_out", "ffn_up", "ffn_down")


class _NoDevice:
    """stands in for a packed model in the refusal tests: `pack()` (the first step that touches the device) fails the test"""
    _tag = "wan.mi355"
    storage_dtype = residual_dtype = BF

    def pack(self):
        raise AssertionError("a refusal must come before anything touches the device")


def _stub(*bases, **attrs):
    from apex_studio_amd.wan import WanTransformer3DModel
    cls = type("Stub", (_NoDevice,) + bases, {"_FP4_LINEARS": WanTransformer3DModel._FP4_LINEARS})
    m = cls()
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def test_wan_and_engine_switches():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import flux, module_base
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from apex_studio_amd.wan import WanTransformer3DModel
    sig = inspect.signature(WanTransformer3DModel.set_fp6_compute)
    assert list(sig.parameters) == ["self", "on", "linears"] and sig.parameters["linears"].default is None
    assert WanTransformer3DModel._FP4_LINEARS == SEVEN
    assert issubclass(WanTransformer3DModel, module_base.Fp6ComputeMixin) and issubclass(WanTransformer3DModel, module_base.Fp4ComputeMixin)
    assert not hasattr(flux.FluxTransformer2DModel, "set_fp6_compute"), "Flux gets no fp6 switch in this change"
    assert not issubclass(flux.FluxTransformer2DModel, module_base.Fp6ComputeMixin)
    for eng in (WanT2VEngine, WanI2VEngine):
        p = inspect.signature(eng.__init__).parameters
        assert p["fp6_compute"].default is False and p["fp6_linears"].default is None
    with pytest.raises(ValueError, match="fp6_linears needs fp6_compute"):
        WanT2VEngine(None, fp6_linears=("qkv",))


def test_fp6_switch_refusals_come_before_any_device_call():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.lib import ApexMIError
    from apex_studio_amd.module_base import Fp4ComputeMixin, Fp6ComputeMixin
    m = _stub(Fp4ComputeMixin, Fp6ComputeMixin)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(linears=\): unknown Linear name\(s\) \['ffn'\]"):
        m._fp6_switch(True, ("ffn_up", "ffn"))
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(linears=\) takes names out of"):
        m._fp6_switch(True, 7)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(False\) takes no `linears`"):
        m._fp6_switch(False, ("qkv",))
    # the overlap with fp4, in both directions, naming the Linear
    m._fp4_linears = ("ffn_up", "ffn_down")
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute\(linears=\): \['ffn_up'\] multiply as fp4 already"):
        m._fp6_switch(True, ("qkv", "ffn_up"))
    with pytest.raises(ApexMIError, match=r"\['ffn_up', 'ffn_down'\] multiply as fp4 already"):
        m._fp6_switch(True)
    m._fp4_linears, m._fp6_linears = None, ("qkv", "attn_out")
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp4_compute\(linears=\): \['qkv'\] multiply as fp6 already \(set_fp6_compute\)"):
        m._fp4_switch(True, ("qkv", "ffn_up"))
    m._fp6_linears = None
    # resident records, f32 storage, the f32 residual stream
    r = _stub(Fp4ComputeMixin, Fp6ComputeMixin, _fp8_bytes=1, _fp8_options=lambda: "keep_fp8")
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute needs the bf16 block weights.*keep_fp8 load.*for fp6 compute$"):
        r._fp6_switch(True)
    s = _stub(Fp4ComputeMixin, Fp6ComputeMixin, storage_dtype=torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute is for bfloat16 activation storage"):
        s._fp6_switch(True)
    f = _stub(Fp4ComputeMixin, Fp6ComputeMixin, residual_dtype=torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: set_fp6_compute does not take the f32 residual stream.*the fp6 GEMM does not"):
        f._fp6_switch(True)
    # the two dtype setters while the mode is on
    m._fp6_linears = SEVEN
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp6 compute is on and is for bfloat16 activation storage.*set_fp6_compute\(False\) first"):
        m.set_storage_dtype(torch.float32)
    with pytest.raises(ApexMIError, match=r"^wan\.mi355: fp6 compute is on and does not take the f32 residual stream.*set_fp6_compute\(False\) first"):
        m.set_residual_dtype(torch.float32)
    # off detaches only the fp6 records
    w4, w6 = torch.zeros(1), torch.zeros(1)
    w4._fp4, w6._fp6 = object(), object()
    m._fp4_live, m._fp6_live, m._fp4_linears = [w4], [w6], ("ffn_up",)
    m._fp6_switch(False)
    assert m._fp6_linears is None and m._fp6_live == [] and not hasattr(w6, "_fp6")
    assert hasattr(w4, "_fp4") and m._fp4_live == [w4] and m._fp4_linears == ("ffn_up",)


# the messages of the fp4 switch as the parent of this change words them, written out here: the shared implementation must reproduce
# them byte for byte
FP4_MESSAGES = {
    "names": "wan.mi355: set_fp4_compute(linears=) takes names out of " + repr(SEVEN) + ", got 7",
    "unknown": "wan.mi355: set_fp4_compute(linears=): unknown Linear name(s) ['ffn']; the block Linears are " + repr(SEVEN),
    "off": "wan.mi355: set_fp4_compute(False) takes no `linears`: it detaches every record",
    "resident": "wan.mi355: set_fp4_compute needs the bf16 block weights, and this model's are resident quantised records (keep_fp8 "
                "load).  The fp8_* switches need exactly such records, so the two modes cannot be combined: load without those options "
                "for fp4 compute",
    "storage": "wan.mi355: set_fp4_compute is for bfloat16 activation storage; the f32-storage verification mode keeps the bf16 GEMMs "
               "(set_storage_dtype(torch.bfloat16) first)",
    "residual": "wan.mi355: set_fp4_compute does not take the f32 residual stream: its residual GEMMs write float rows, which the fp4 "
                "GEMM does not (set_residual_dtype(torch.bfloat16) first)",
    "set_storage": "wan.mi355: fp4 compute is on and is for bfloat16 activation storage: float rows would quietly return every Linear "
                   "to bf16; set_fp4_compute(False) first",
    "set_residual": "wan.mi355: fp4 compute is on and does not take the f32 residual stream: its residual GEMMs would quietly return to "
                    "bf16; set_fp4_compute(False) first"}


def test_fp4_switch_messages_are_byte_identical():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.lib import ApexMIError
    from apex_studio_amd.module_base import Fp4ComputeMixin, Fp6ComputeMixin

    def message(call):
        with pytest.raises(ApexMIError) as err:
            call()
        return str(err.value)

    for bases in ((Fp4ComputeMixin,), (Fp4ComputeMixin, Fp6ComputeMixin)):          # Flux's bases, Wan's bases
        m = _stub(*bases)
        assert message(lambda: m._fp4_switch(True, 7)) == FP4_MESSAGES["names"]
        assert message(lambda: m._fp4_switch(True, ("ffn_up", "ffn"))) == FP4_MESSAGES["unknown"]
        assert message(lambda: m._fp4_switch(False, ("qkv",))) == FP4_MESSAGES["off"]
        r = _stub(*bases, _fp8_bytes=1, _fp8_options=lambda: "keep_fp8")
        assert message(lambda: r._fp4_switch(True)) == FP4_MESSAGES["resident"]
        s = _stub(*bases, storage_dtype=torch.float32)
        assert message(lambda: s._fp4_switch(True)) == FP4_MESSAGES["storage"]
        f = _stub(*bases, residual_dtype=torch.float32)
        assert message(lambda: f._fp4_switch(True)) == FP4_MESSAGES["residual"]
        m._fp4_linears = SEVEN
        assert message(lambda: m.set_storage_dtype(torch.float32)) == FP4_MESSAGES["set_storage"]
        assert message(lambda: m.set_residual_dtype(torch.float32)) == FP4_MESSAGES["set_residual"]
