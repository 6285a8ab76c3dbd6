"""The two launch fusions of the MXFP4 mode (`apexmi_ln_modulate_quant_mxfp4`, `apexmi_gemm_mxfp4_mx`,
`apexmi_gemm_mxfp4_grouped_mx`, `apexmi_gemm_mxfp4_grouped_qkv_mx`), the parts that need no GPU: the C-ABI tables, every host-side
refusal of the four entry points, the pairing predicates of `ops` and the model and engine switches."""
import ctypes as C
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16
U8 = torch.uint8
NEW = {"apexmi_ln_modulate_quant_mxfp4": 21, "apexmi_gemm_mxfp4_mx": 23, "apexmi_gemm_mxfp4_grouped_mx": 24,
       "apexmi_gemm_mxfp4_grouped_qkv_mx": 36}
P = 0x100000                      # 16-byte aligned dummy address, never dereferenced


def _lib():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    return lib, lib.load()


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def test_header_signatures_library_and_the_no_spill_lists():
    lib, L = _lib()
    from apex_studio_amd import build
    header = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert "replaces apexmi_" in header.split("/* " + name)[1].split("*/")[0], f"{name}: the comment cites what it replaces"
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), name
    # four more arguments than the entry points they extend (the norm: the scale rows' stride on top of the fp8 form's)
    assert NEW["apexmi_gemm_mxfp4_mx"] == len(lib.SIGNATURES["apexmi_gemm_mxfp4"][1]) + 4
    assert NEW["apexmi_gemm_mxfp4_grouped_mx"] == len(lib.SIGNATURES["apexmi_gemm_mxfp4_grouped"][1]) + 4
    assert NEW["apexmi_gemm_mxfp4_grouped_qkv_mx"] == len(lib.SIGNATURES["apexmi_gemm_mxfp4_grouped_qkv"][1]) + 4
    assert NEW["apexmi_ln_modulate_quant_mxfp4"] == len(lib.SIGNATURES["apexmi_ln_modulate_quant_fp8"][1]) + 1
    # the new kernels are instantiations of the names the no-spill check already matches
    assert build.NO_SPILL["elementwise.hip"] == ["ln_modulate_quant_kernel", "ln_modulate_wave_quant_kernel"]
    assert build.NO_SPILL["gemm_mxfp4.hip"] == ["gemm_mxfp4_kernel"]
    csrc = os.path.join(ROOT, "apex-studio_amd", "csrc")
    kernels = lambda unit: re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", open(os.path.join(csrc, unit)).read())  # noqa: E731
    assert kernels("gemm_mxfp4.hip") == ["quant_blocks_mxfp4_kernel", "gemm_mxfp4_kernel"]
    assert [k for k in kernels("elementwise.hip") if "_quant_" in k] == build.NO_SPILL["elementwise.hip"]
    # the formula keeps one home
    quant = open(os.path.join(csrc, "fp8_quant.h")).read()
    assert "mx4_quant4f" in quant and "mx4_quant8f" in quant
    for unit in ("elementwise.hip", "gemm_mxfp4.hip", "fp8_gemm_tile.h", "ln_modulate_row.inc", "ln_modulate_wave_rows.inc"):
        text = open(os.path.join(csrc, unit)).read()
        assert "0x400000" not in text and "4194304" not in text, unit


def test_the_norm_refuses_every_bad_argument_before_a_launch():
    lib, L = _lib()

    def call(x=P, ldx=256, dt=lib.BF16, out=None, ldo=0, codes=P, ldq=128, scales=P, lds=8, M=4, C_=256, scale=None, shift=None,
             gamma=None, beta=None, split=0, scale2=None, shift2=None):
        return L.apexmi_ln_modulate_quant_mxfp4(x, ldx, dt, out, ldo, codes, ldq, scales, lds, M, C_, scale, shift, gamma, beta, 1e-6, 0,
                                                split, scale2, shift2, None)

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and msg.startswith("ln_modulate_quant_mxfp4:") and needle in msg, (rc, msg)

    bad(call(x=None), "null operand")
    bad(call(codes=None), "null operand")
    bad(call(scales=None), "null operand")
    bad(call(dt=lib.F16), "x_dtype=1")
    bad(call(M=0), "M=0")
    bad(call(M=-3), "M=-3")
    bad(call(C_=192, ldx=192), "C=192")
    bad(call(C_=8), "C=8")
    bad(call(C_=8320, ldx=8320, ldq=4160, lds=260), "C=8320")
    bad(call(ldx=260), "rows must be 16-byte aligned")                       # bf16 rows: ldx % 8
    bad(call(dt=lib.F32, ldx=258), "rows must be 16-byte aligned")           # float rows: ldx % 4
    bad(call(x=P + 2), "rows must be 16-byte aligned")
    bad(call(codes=P + 8), "rows must be 16-byte aligned")
    bad(call(ldq=136), "rows must be 16-byte aligned")                       # ldq % 16
    bad(call(ldq=112), "at least C / 2")
    bad(call(ldx=128), "at least C")
    bad(call(out=P, ldo=260), "rows must be 16-byte aligned")
    bad(call(out=P + 4, ldo=256), "rows must be 16-byte aligned")
    bad(call(out=P, ldo=128), "at least C")
    bad(call(lds=7), "at least C / 32 = 8 wide")
    bad(call(scale=P + 4), "scale/shift must be 16-byte aligned")
    bad(call(shift=P + 8), "scale/shift must be 16-byte aligned")
    bad(call(split=2, scale2=P + 4), "scale2/shift2 must be 16-byte aligned")
    bad(call(split=2, shift2=P + 12), "scale2/shift2 must be 16-byte aligned")
    bad(call(gamma=P + 2), "gamma/beta must be 16-byte aligned")
    bad(call(beta=P + 6), "gamma/beta must be 16-byte aligned")
    bad(call(split=-1), "split=-1")
    bad(call(split=5), "split=5")


def test_the_single_gemm_refuses_every_bad_mx_output_before_a_launch():
    lib, L = _lib()

    def call(C_=None, ldc=0, mq=P, ldmc=64, ms=P, ldms=4, M=8, N=128, K=256, epi=lib.EPI_BIAS, gate=None, R=None, ldr=0, qa=P):
        return L.apexmi_gemm_mxfp4_mx(qa, K // 2, P, K // 32, P, K // 2, P, K // 32, None, C_, ldc, mq, ldmc, ms, ldms, M, N, K, epi, gate, R,
                                      ldr, None)

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and msg.startswith("gemm_mxfp4_mx:") and needle in msg, (rc, msg)

    bad(call(ms=None), "needs codes and block scales")                       # codes without scales
    bad(call(mq=None), "needs codes and block scales")                       # a scale pointer without codes
    bad(call(epi=lib.EPI_BIAS_GATE_RES, gate=P, R=P, ldr=128, C_=P, ldc=128), "not epilogue 2")
    bad(call(N=64, ldmc=32), "N=64 must be a multiple of 128")
    bad(call(N=192, ldmc=96, ldms=8), "N=192 must be a multiple of 128")
    bad(call(ldmc=60), "at least N / 2")
    bad(call(ldmc=66), "4-byte aligned code rows")
    bad(call(mq=P + 2), "4-byte aligned code rows")
    bad(call(ldms=3), "scale rows at least N / 32")
    bad(call(ldms=6), "a multiple of 4")
    bad(call(qa=None), "null operand")
    bad(call(K=384), "K=384 must be a multiple of 256")
    bad(call(M=0), "M=0")
    bad(call(epi=lib.EPI_BIAS_SILU), "epilogues, not epilogue")
    bad(call(C_=P + 4, ldc=128), "operands must be 16-byte aligned")         # a C that is given is still checked
    # without an MX output the entry point is apexmi_gemm_mxfp4 itself, with its own refusals
    rc = call(mq=None, ms=None)
    assert rc != 0 and L.apexmi_last_error().decode().startswith("gemm_mxfp4: null operand")


def _arrays(n, K=256, **over):
    VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
    d = dict(qa=VP(*[P] * n), lda=I64(*[K // 2] * n), sa=VP(*[P] * n), ldsa=I64(*[K // 32] * n), qw=VP(*[P] * n), ldw=I64(*[K // 2] * n),
             sw=VP(*[P] * n), ldsw=I64(*[K // 32] * n), bias=VP(*[None] * n), C=VP(*[P] * n), ldc=I64(*[128] * n),
             mq=VP(*[P] * n), ldmc=I64(*[64] * n), ms=VP(*[P] * n), ldms=I64(*[4] * n), M=INT(*[8] * n),
             N=INT(*[128] * n), K=K, epi=INT(*[0] * n), gate=VP(*[None] * n), R=VP(*[None] * n), ldr=I64(*[0] * n))
    d.update(over)
    return [d[k] for k in ("qa", "lda", "sa", "ldsa", "qw", "ldw", "sw", "ldsw", "bias", "C", "ldc", "mq", "ldmc", "ms", "ldms", "M", "N", "K",
                           "epi", "gate", "R", "ldr")]


def test_the_grouped_gemms_refuse_every_bad_mx_output_before_a_launch():
    lib, L = _lib()
    VP2, I2, L2 = C.c_void_p * 2, C.c_int * 2, C.c_int64 * 2

    def bad(rc, who, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and msg.startswith(who + ":") and needle in msg, (rc, msg)

    g, who = L.apexmi_gemm_mxfp4_grouped_mx, "gemm_mxfp4_grouped_mx"
    bad(g(0, *_arrays(1), None), who, "count=0 not in [1,4]")
    bad(g(2, *_arrays(2, mq=None), None), who, "null argument array")
    bad(g(2, *_arrays(2, ldms=None), None), who, "null argument array")
    bad(g(2, *_arrays(2, ms=VP2(P, None)), None), who, "the MX output of problem 1 needs codes and block scales")
    bad(g(2, *_arrays(2, mq=VP2(None, P)), None), who, "the MX output of problem 0 needs codes and block scales")
    bad(g(2, *_arrays(2, N=I2(128, 64)), None), who, "N=64 of problem 1 must be a multiple of 128")
    bad(g(2, *_arrays(2, epi=I2(0, lib.EPI_BIAS_GATE_RES), gate=VP2(None, P), R=VP2(None, P), ldr=L2(0, 128)), None), who,
        "the MX output of problem 1 exists for the bias (0) and tanh GELU (1) epilogues")
    bad(g(2, *_arrays(2, ldmc=L2(64, 62)), None), who, "4-byte aligned code rows")
    bad(g(2, *_arrays(2, ldms=L2(4, 2)), None), who, "scale rows at least N / 32")
    bad(g(2, *_arrays(2, K=384), None), who, "K=384 must be a multiple of 256")
    # a problem without an MX entry is a problem of apexmi_gemm_mxfp4_grouped: it needs its C
    bad(g(2, *_arrays(2, mq=VP2(P, None), ms=VP2(P, None), C=VP2(None, None)), None), who, "null operand (problem 1)")

    q, who = L.apexmi_gemm_mxfp4_grouped_qkv_mx, "gemm_mxfp4_grouped_qkv_mx"
    tail = [I2(1, 0), VP2(None, None), VP2(None, None), I2(0, 0), 1, 1e-6, P, P, P, P, 8, 8]
    bad(q(2, *_arrays(2, N=I2(384, 128)), *tail, None), who, "a fused q/k/v problem (problem 0) writes q / k / V^T and takes no MX output")
    bad(q(2, *_arrays(2, N=I2(384, 64), mq=VP2(None, P), ms=VP2(None, P)), *tail, None), who, "N=64 of problem 1 must be a multiple of 128")
    tail[6] = None
    bad(q(2, *_arrays(2, N=I2(384, 128), mq=VP2(None, P), ms=VP2(None, P)), *tail, None), who, "null argument")


def _fp4_weight(N, K, compute="fp4"):
    ops = _ops()
    w = torch.zeros(N, K, dtype=BF)
    w._fp4 = ops.Mxfp4Weight(torch.zeros(N, K // 2, dtype=U8), torch.zeros(N, K // 32, dtype=U8))
    w._fp4.compute = compute
    return w


def test_norm_quant_predicate_is_pure_and_right_on_cpu_tensors():
    ops = _ops()
    route = ops.mxfp4_norm_quant_route
    x, xn, out = torch.zeros(5, 256, dtype=BF), torch.zeros(5, 256, dtype=BF), torch.zeros(5, 32, dtype=BF)
    w = _fp4_weight(32, 256)
    assert route(x, xn, w) is True and route(x, xn, w, out, "gelu") is True and route(x, xn, w._fp4, out, "gate_res") is True
    assert route(x.float(), xn, w, out) is True                              # a float x: the norm reads it, the GEMM reads bf16 codes
    # everything that keeps today's launches
    assert not route(x, xn, torch.zeros(32, 256, dtype=BF))                  # no record
    assert not route(x, xn, _fp4_weight(32, 256, compute="bf16"))
    assert not route(x, xn, w, torch.zeros(5, 32))                           # a float `out`
    assert not route(x.float(), xn.float(), w)                               # the f32-storage mode
    assert not route(x.half(), xn, w)
    assert not route(x, xn, w, None, "silu")
    x128, w128 = torch.zeros(5, 128, dtype=BF), _fp4_weight(32, 128)
    assert not route(x128, x128, w128)                                       # K % 256: the GEMM does not route
    x384, w384 = torch.zeros(5, 384, dtype=BF), _fp4_weight(32, 384)
    assert not route(x384, x384, w384)
    big = torch.zeros(2, 8448, dtype=BF)
    assert ops.mxfp4_route(big, _fp4_weight(16, 8448)) and not route(big, big, _fp4_weight(16, 8448))      # the norm's C <= 8192
    assert not route(torch.zeros(5, 260, dtype=BF)[:, :256], xn, w)          # x rows not 16-byte aligned
    assert not route(torch.zeros(4, 256, dtype=BF), xn, w)                   # shapes differ
    assert not route(x, xn, _fp4_weight(24, 256))                            # N % 16
    assert w._fp4.compute == "fp4" and x.dtype == BF and not hasattr(x, "_fp4"), "pure"


def test_mx_predicates_are_pure_and_right_on_cpu_tensors():
    ops = _ops()
    route = ops.mxfp4_mx_route
    a, x = torch.zeros(5, 256, dtype=BF), torch.zeros(5, 256, dtype=BF)
    up, down = _fp4_weight(512, 256), _fp4_weight(256, 512)
    assert route(a, up, down) is True and route((5, 256), up, down, "bias", "bias") is True and route(a, up, down, out=x) is True
    assert not route(a, torch.zeros(512, 256, dtype=BF), down)               # the up weight carries no record
    assert not route(a, up, torch.zeros(256, 512, dtype=BF))                 # nor the down weight
    assert not route(a, up, _fp4_weight(256, 512, compute="bf16"))
    assert not route(a, up, down, "gate_res")                                # the MX output exists for bias and gelu
    assert not route(a, _fp4_weight(384, 256), _fp4_weight(256, 384))        # the up N is no multiple of 256
    assert not route(a, _fp4_weight(128, 256), _fp4_weight(256, 128))
    assert not route(a, up, down, out=x.float())                             # the f32 residual stream
    assert not route(a.float(), up, down)
    assert not route(a, up, _fp4_weight(256, 768))                           # the down K is not the up N
    g = ops.mxfp4_grouped_mx_route
    a2 = torch.zeros(9, 256, dtype=BF)
    assert g([a, a2], [up, up], [down, down]) is True and g([a, a2], [up, up], [down, down], out_list=[x, None]) is True
    assert not g([a, a2], [up, up], [down, torch.zeros(256, 512, dtype=BF)])
    assert not g([a, a2], [up, _fp4_weight(384, 256)], [down, _fp4_weight(256, 384)])
    assert not g([a] * 5, [up] * 5, [down] * 5)                              # a launch holds 1 to 4 problems
    assert not g([a, a2], [up], [down, down])
    assert up._fp4.compute == "fp4" and down._fp4.shape == (256, 512), "pure"


def test_grouped_wrappers_refuse_with_a_reason_before_the_device_is_asked():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    rec = _fp4_weight(128, 256)._fp4
    q, s = torch.zeros(5, 128, dtype=U8), torch.zeros(5, 8, dtype=U8)
    mq, ms = torch.zeros(5, 64, dtype=U8), torch.zeros(5, 4, dtype=U8)
    with pytest.raises(ApexMIError, match="one \\(codes, scales\\) pair or None per problem"):
        ops.gemm_mxfp4_grouped([q], [s], [rec], None, [None], out_mx_list=[(mq, ms), None])
    with pytest.raises(ApexMIError, match="takes no out_mx"):
        ops.gemm_mxfp4_grouped_qkv([q], [s], [rec], None, [None], "bias", [1], None, None, [0], 1, 1e-6, None, None, None, None,
                                   out_mx_list=[(mq, ms)])


def test_model_switches_need_on_and_clear_by_default():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.module_base import Fp4ComputeMixin
    from apex_studio_amd.wan import WanTransformer3DModel
    for cls in (WanTransformer3DModel, FluxTransformer2DModel):
        p = inspect.signature(cls.set_fp4_compute).parameters
        assert list(p) == ["self", "on", "linears", "fused_quant", "mx_ffn"]
        assert p["fused_quant"].default is False and p["mx_ffn"].default is False and issubclass(cls, Fp4ComputeMixin)
    m = WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=1, attention_head_dim=128, in_channels=16, out_channels=16,
                              text_dim=64, freq_dim=256, ffn_dim=256, num_layers=1, cross_attn_norm=True, eps=1e-6,
                              device="cpu", dtype=BF)
    assert m._fp4_fused_quant is False and m._fp4_mx_ffn is False
    with pytest.raises(ValueError, match=r"^wan\.mi355: set_fp4_compute\(fused_quant=True\) needs on=True"):
        m.set_fp4_compute(False, fused_quant=True)
    with pytest.raises(ValueError, match=r"^wan\.mi355: set_fp4_compute\(mx_ffn=True\) needs on=True"):
        m.set_fp4_compute(False, mx_ffn=True)
    assert m._fp4_linears is None and m._fp4_fused_quant is False, "refused up front: nothing was switched"
    m._fp4_fused_quant = m._fp4_mx_ffn = True
    m.set_fp4_compute(False)
    assert m._fp4_fused_quant is False and m._fp4_mx_ffn is False, "off clears both"
    from apex_studio_amd.lib import ApexMIError
    with pytest.raises(ApexMIError, match="unknown Linear name"):
        m.set_fp4_compute(True, linears=("ffn",), fused_quant=True)
    assert m._fp4_fused_quant is False, "the refusals of the switch come first"


def test_engines_take_the_two_switches():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from tests.test_engines import _FakeWan
    for cls in (WanT2VEngine, WanI2VEngine, FluxT2IEngine):
        p = inspect.signature(cls.__init__).parameters
        assert p["fp4_fused_quant"].default is False and p["fp4_mx_ffn"].default is False

    class Spy(_FakeWan):
        def set_fp4_compute(self, on, linears=None, fused_quant=False, mx_ffn=False):
            self.fp4 = (on, linears, fused_quant, mx_ffn)
    for cls in (WanT2VEngine, WanI2VEngine):
        hi, lo = Spy(1.0), Spy(2.0)
        eng = cls(hi, lo, fp4_compute=True, fp4_fused_quant=True)
        assert eng.fp4_fused_quant and not eng.fp4_mx_ffn and hi.fp4 == lo.fp4 == (True, None, True, False)
        hi, lo = Spy(1.0), Spy(2.0)
        cls(hi, lo, fp4_compute=True, fp4_linears=("ffn_up", "ffn_down"), fp4_mx_ffn=True)
        assert hi.fp4 == (True, ("ffn_up", "ffn_down"), False, True)
        hi, lo = Spy(1.0), Spy(2.0)
        assert cls(hi, lo, fp4_compute=True).fp4_fused_quant is False and hi.fp4 == (True, None, False, False)
        with pytest.raises(ValueError, match="fp4_fused_quant=True needs fp4_compute=True"):
            cls(Spy(1.0), Spy(2.0), fp4_fused_quant=True)
        with pytest.raises(ValueError, match="fp4_mx_ffn=True needs fp4_compute=True"):
            cls(Spy(1.0), Spy(2.0), fp4_mx_ffn=True)

    class FluxSpy:
        config = SimpleNamespace(in_channels=64)

        def set_fp4_compute(self, on, linears=None, fused_quant=False, mx_ffn=False):
            self.fp4 = (on, linears, fused_quant, mx_ffn)
    t = FluxSpy()
    eng = FluxT2IEngine(t, fp4_compute=True, fp4_fused_quant=True, fp4_mx_ffn=True)
    assert eng.fp4_fused_quant and eng.fp4_mx_ffn and t.fp4 == (True, None, True, True)
    with pytest.raises(ValueError, match="fp4_fused_quant=True needs fp4_compute=True"):
        FluxT2IEngine(FluxSpy(), fp4_fused_quant=True)
    with pytest.raises(ValueError, match="fp4_mx_ffn=True needs fp4_compute=True"):
        FluxT2IEngine(FluxSpy(), fp4_mx_ffn=True)
