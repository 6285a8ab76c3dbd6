"""The norm that quantises its own output (`apexmi_ln_modulate_quant_fp8`), the parts that need no GPU: the
C-ABI tables, every host-side refusal of the entry point, the pairing predicate `ops.fp8_norm_quant_route` and the model and
engine switches."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "apexmi_ln_modulate_quant_fp8"
BF = torch.bfloat16
F8 = torch.float8_e4m3fn


def test_header_bindings_library_and_no_spill_list():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import build, lib
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert "replaces apexmi_ln_modulate2" in header.split(NAME)[1]          # the comment cites what it replaces
    assert NAME in lib.SIGNATURES and len(lib.SIGNATURES[NAME][1]) == len(lib.SIGNATURES["apexmi_ln_modulate2"][1]) + 4
    assert hasattr(lib.load(), NAME)
    assert build.NO_SPILL["elementwise.hip"] == ["ln_modulate_quant_kernel", "ln_modulate_wave_quant_kernel"]
    with open(os.path.join(ROOT, "apex-studio_amd", "csrc", "elementwise.hip")) as f:
        src = f.read()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)
    assert all(k in kernels for k in build.NO_SPILL["elementwise.hip"])
    # the quantiser's formula has one home, which both translation units include
    for unit in ("elementwise.hip", "gemm_fp8.hip"):
        with open(os.path.join(ROOT, "apex-studio_amd", "csrc", unit)) as f:
            text = f.read()
        assert '#include "fp8_quant.h"' in text and "float quant1(" not in text, unit


def test_every_refusal_reports_its_reason_before_any_launch():
    """dummy (never dereferenced) pointers: a call that got as far as a launch would fault or report a HIP error instead"""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000                      # 16-byte aligned dummy address

    def call(x=P, ldx=256, dt=lib.BF16, out=None, ldo=0, codes=P, ldq=256, scales=P, M=4, C=256, scale=None, shift=None, gamma=None,
             beta=None, split=0, scale2=None, shift2=None):
        return L.apexmi_ln_modulate_quant_fp8(x, ldx, dt, out, ldo, codes, ldq, scales, M, C, scale, shift, gamma, beta, 1e-6, 0, split,
                                              scale2, shift2, None)

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and msg.startswith("ln_modulate_quant_fp8:") and needle in msg, (rc, msg)

    bad(call(x=None), "null operand")
    bad(call(codes=None), "null operand")
    bad(call(scales=None), "null operand")
    bad(call(dt=lib.F16), "x_dtype=1")
    bad(call(M=0), "M=0")
    bad(call(M=-3), "M=-3")
    bad(call(C=192, ldx=192, ldq=192), "C=192")
    bad(call(C=8), "C=8")
    bad(call(C=8320, ldx=8320, ldq=8320), "C=8320")
    bad(call(ldx=260), "rows must be 16-byte aligned")                       # bf16 rows: ldx % 8
    bad(call(dt=lib.F32, ldx=258), "rows must be 16-byte aligned")           # float rows: ldx % 4
    bad(call(x=P + 2), "rows must be 16-byte aligned")
    bad(call(codes=P + 8), "rows must be 16-byte aligned")
    bad(call(ldq=264), "rows must be 16-byte aligned")                       # ldq % 16
    bad(call(ldq=128), "at least C wide")
    bad(call(ldx=128), "at least C wide")
    bad(call(out=P, ldo=260), "rows must be 16-byte aligned")
    bad(call(out=P + 4, ldo=256), "rows must be 16-byte aligned")
    bad(call(out=P, ldo=128), "at least C wide")
    bad(call(scale=P + 4), "scale/shift must be 16-byte aligned")
    bad(call(shift=P + 8), "scale/shift must be 16-byte aligned")
    bad(call(split=2, scale2=P + 4), "scale2/shift2 must be 16-byte aligned")
    bad(call(split=2, shift2=P + 12), "scale2/shift2 must be 16-byte aligned")
    bad(call(gamma=P + 2), "gamma/beta must be 16-byte aligned")
    bad(call(beta=P + 6), "gamma/beta must be 16-byte aligned")
    bad(call(split=-1), "split=-1")
    bad(call(split=5), "split=5")


def _weight(N=32, K=256, dt=F8, compute="fp8", lora=False, lora_compute="fp8"):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    w = ops.Fp8Weight(torch.zeros(N, K).to(dt), torch.ones(N))
    w.compute = compute
    if lora:
        w.parts = [("lin", 0, N)]
        w.set_lora([("lin", torch.zeros(4, K), torch.zeros(N, 4), 1.0)])
        w.lora_compute = lora_compute
    return w


def test_pairing_predicate_is_pure_and_right_on_cpu_tensors():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    route = ops.fp8_norm_quant_route
    x, xn = torch.zeros(5, 256, dtype=BF), torch.zeros(5, 256, dtype=BF)
    out = torch.zeros(5, 32, dtype=BF)
    w = _weight()
    assert route(x, xn, w) == (True, False)                                          # a plain record: fuse, no bf16 row
    assert route(x, xn, w, out, "gelu") == (True, False)
    assert route(x, xn, w, row_read_later=True) == (True, True)                      # something else reads xn
    assert route(x.float(), xn, w, out) == (True, False)                             # the f32 residual stream: float x, bf16 xn
    p = torch.nn.Parameter(torch.empty(0), requires_grad=False)
    p._fp8 = w
    assert route(x, xn, p) == (True, False)                                          # a parameter carrying the record
    # a record with LoRA: fuse (the fp8 GEMM with the adapter tail), and the skinny GEMM needs the bf16 row
    lw = _weight(lora=True)
    Rp = lw.lora_A.shape[0]
    buf = torch.zeros(5, 256 + Rp, dtype=BF)
    assert route(x, buf[:, :256], lw, out, "bias", buf) == (True, True)
    assert route(x, buf[:, :256], lw, out, "bias", None) == (False, True)            # no padded buffer: not the fp8 route
    assert route(x, buf[:, :256], _weight(lora=True, lora_compute="bf16"), out, "bias", buf) == (False, True)
    # everything that keeps today's launches
    assert route(x, xn, _weight(dt=torch.float8_e5m2)) == (False, True)              # an e5m2 record
    assert route(x, xn, w, torch.zeros(5, 32)) == (False, True)                      # a float `out`
    assert route(torch.zeros(5, 192, dtype=BF), torch.zeros(5, 192, dtype=BF), _weight(K=192)) == (False, True)   # K % 128
    assert route(x, xn, _weight(compute="bf16")) == (False, True)                    # compute == "bf16"
    assert route(x, xn, torch.zeros(32, 256, dtype=BF)) == (False, True)             # a plain bf16 weight
    assert route(x.float(), xn.float(), w) == (False, True)                          # the f32-storage mode
    assert route(x.half(), xn, w) == (False, True)
    assert route(x, xn, w, None, "silu") == (False, True)
    assert route(torch.zeros(5, 260, dtype=BF)[:, :256], xn, w) == (False, True)     # x rows not 16-byte aligned
    assert route(torch.zeros(4, 256, dtype=BF), xn, w) == (False, True)              # shapes differ
    # pure: no field of the record or of the tensors changed
    assert (w.compute, w.lora_compute, w.lora_A) == ("fp8", "bf16", None) and x.dtype == BF


def test_set_fp8_compute_fused_quant_needs_on():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=1, attention_head_dim=128, in_channels=16, out_channels=16,
                              text_dim=64, freq_dim=256, ffn_dim=256, num_layers=1, cross_attn_norm=True, eps=1e-6,
                              device="cpu", dtype=BF)
    with pytest.raises(ValueError, match="fused_quant=True.*on=True"):
        m.set_fp8_compute(False, fused_quant=True)
    rec = ops.Fp8Weight(torch.zeros(32, 128).to(F8), torch.ones(1))
    m._fp8_records = {"x": rec}
    m.set_fp8_compute(True, fused_quant=True)
    assert m._fp8_fused_quant is True and (rec.compute, rec.lora_compute) == ("fp8", "bf16")
    m.set_fp8_compute(True, lora=True, fused_quant=True)
    assert m._fp8_fused_quant is True and (rec.compute, rec.lora_compute) == ("fp8", "fp8")
    m.set_fp8_compute(True)
    assert m._fp8_fused_quant is False, "the default clears it"
    m.set_fp8_compute(True, fused_quant=True)
    m.set_fp8_compute(False)
    assert m._fp8_fused_quant is False and rec.compute == "bf16"


def test_engines_take_the_fused_quant_switch():
    import inspect
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from tests.test_engines import _FakeWan
    for cls in (WanT2VEngine, WanI2VEngine):
        assert inspect.signature(cls.__init__).parameters["fp8_fused_quant"].default is False

    class Spy(_FakeWan):
        def set_fp8_compute(self, on, lora=False, fused_quant=False):
            self.fp8 = (on, lora, fused_quant)
    for cls in (WanT2VEngine, WanI2VEngine):
        hi, lo = Spy(1.0), Spy(2.0)
        eng = cls(hi, lo, fp8_compute=True, fp8_fused_quant=True)
        assert eng.fp8_fused_quant and hi.fp8 == (True, False, True) and lo.fp8 == (True, False, True)
        hi, lo = Spy(1.0), Spy(2.0)
        cls(hi, lo, fp8_compute=True, fp8_lora=True, fp8_fused_quant=True)
        assert hi.fp8 == (True, True, True)
        hi, lo = Spy(1.0), Spy(2.0)
        assert cls(hi, lo, fp8_compute=True).fp8_fused_quant is False and hi.fp8 == (True, False, False)
        with pytest.raises(ValueError, match="fp8_compute=True"):
            cls(Spy(1.0), Spy(2.0), fp8_fused_quant=True)
