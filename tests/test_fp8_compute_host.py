"""Opt-in FP8 compute on resident fp8 Wan weights, the parts that need no GPU: the C-ABI tables, the host-side
argument checks of the two entry points, the model switch and the routing predicate of `ops.gemm`."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("apexmi_quant_rows_fp8", "apexmi_gemm_fp8")


def test_header_and_bindings_declare_both_entries():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", header), n
        assert n in lib.SIGNATURES, n
    L = lib.load()
    assert all(hasattr(L, n) for n in NAMES)
    with open(os.path.join(ROOT, "apex-studio_amd", "build.py")) as f:
        assert "gemm_fp8.hip" in f.read()
    from apex_studio_amd import build
    assert "gemm_fp8.hip" in build.SOURCES and build.NO_SPILL["gemm_fp8.hip"] == ["gemm_fp8_kernel"]


def test_argument_validation_reports_a_reason():
    """Both entry points validate on the host before touching the device; dummy (never dereferenced) pointers."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000                      # 16-byte aligned dummy address

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    def gemm(M=8, N=16, K=128, fmt=0, epi=lib.EPI_BIAS, gate=None, R=None, ldr=0, lda=None):
        return L.apexmi_gemm_fp8(P, K if lda is None else lda, P, P, K, fmt, P, 1, None, P, N, M, N, K, epi, gate, R, ldr, None)

    bad(gemm(K=100), "K=100")
    bad(gemm(N=12), "N=12")
    bad(gemm(fmt=1), "e5m2")
    bad(gemm(epi=lib.EPI_BIAS_GATE_RES), "needs gate and R")
    bad(gemm(M=0), "M=0")
    bad(gemm(epi=lib.EPI_BIAS | lib.EPI_F32_IO), "f32 output")
    bad(gemm(epi=lib.EPI_BIAS_F32), "f32 output")
    bad(gemm(epi=lib.EPI_BIAS_SILU), "epilogue 5")
    bad(gemm(lda=1 << 23), "2^22")
    bad(L.apexmi_gemm_fp8(P, 128, P, P, 128, 0, P, 3, None, P, 16, 8, 16, 128, 0, None, None, 0, None), "3 values")
    bad(L.apexmi_quant_rows_fp8(P, 100, 4, 100, P, 112, P, None), "K=100")
    bad(L.apexmi_quant_rows_fp8(P, 128, 0, 128, P, 128, P, None), "M=0")
    bad(L.apexmi_quant_rows_fp8(None, 128, 4, 128, P, 128, P, None), "null")


def test_fp8_weight_compute_defaults_to_bf16():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    w = ops.Fp8Weight(torch.zeros(32, 128).to(torch.float8_e4m3fn), torch.ones(1))
    assert w.compute == "bf16" and ops.Fp8Weight.compute == "bf16"
    c = ops.Fp8Weight.cat([w, w])
    assert c.compute == "bf16"


def test_routing_predicate_on_cpu_tensors():
    """`ops.fp8_compute_route` is pure: every documented fallback case answers False, the one eligible case True."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    BF = torch.bfloat16

    def weight(N=32, K=256, dt=torch.float8_e4m3fn, compute="fp8"):
        w = ops.Fp8Weight(torch.zeros(N, K).to(dt), torch.ones(N))
        w.compute = compute
        return w
    a = torch.zeros(5, 256, dtype=BF)
    w = weight()
    assert ops.fp8_compute_route(a, w) and ops.fp8_compute_route(a, w, torch.zeros(5, 32, dtype=BF), "gate_res")
    assert ops.fp8_compute_route(a, w, None, "gelu")
    p = torch.nn.Parameter(torch.empty(0), requires_grad=False)      # a parameter carrying the record, as the models hold them
    p._fp8 = w
    assert ops.fp8_compute_route(a, p)
    assert ops.fp8_compute_route(torch.zeros(5, 512, dtype=BF)[:, :256], w)          # padded row stride
    assert not ops.fp8_compute_route(a, weight(compute="bf16"))                      # the default
    assert not ops.fp8_compute_route(a, weight(dt=torch.float8_e5m2))                # e5m2
    assert not ops.fp8_compute_route(a.float(), w)                                   # f32-storage mode
    assert not ops.fp8_compute_route(a, w, torch.zeros(5, 32))                       # f32 residual stream
    assert not ops.fp8_compute_route(a, torch.zeros(32, 256, dtype=BF))              # a plain bf16 weight
    assert not ops.fp8_compute_route(a, w, None, "silu")                             # an epilogue the fp8 kernel lacks
    assert not ops.fp8_compute_route(torch.zeros(5, 192, dtype=BF), weight(K=192))   # K % 128
    assert not ops.fp8_compute_route(a, weight(N=24))                                # N % 16
    assert not ops.fp8_compute_route(torch.zeros(0, 256, dtype=BF), w)               # M = 0
    assert not ops.fp8_compute_route(torch.zeros(5, 260, dtype=BF)[:, :256], w)      # rows not 16-byte aligned
    lw = weight()
    lw.parts = [("lin", 0, 32)]
    lw.set_lora([("lin", torch.zeros(4, 256), torch.zeros(32, 4), 1.0)])
    assert lw.lora_A is not None and not ops.fp8_compute_route(a, lw)                # run-time LoRA attached
    lw.set_lora([])
    assert ops.fp8_compute_route(a, lw)


def test_set_fp8_compute_needs_resident_records():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=1, attention_head_dim=128, in_channels=16, out_channels=16,
                              text_dim=64, freq_dim=256, ffn_dim=256, num_layers=1, cross_attn_norm=True, eps=1e-6,
                              device="cpu", dtype=torch.bfloat16)
    with pytest.raises(lib.ApexMIError, match="keep_fp8=True"):
        m.set_fp8_compute(True)


def test_engines_take_the_switch():
    import inspect
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from tests.test_engines import _FakeWan
    for cls in (WanT2VEngine, WanI2VEngine):
        assert inspect.signature(cls.__init__).parameters["fp8_compute"].default is False
    assert WanT2VEngine(_FakeWan(1.0), _FakeWan(2.0)).fp8_compute is False

    class Spy(_FakeWan):
        def set_fp8_compute(self, on):
            self.fp8 = on
    hi, lo = Spy(1.0), Spy(2.0)
    WanI2VEngine(hi, lo, fp8_compute=True)
    assert hi.fp8 is True and lo.fp8 is True
