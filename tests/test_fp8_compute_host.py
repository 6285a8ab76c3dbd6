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
    # the remaining refusals of a single launch, at the smallest legal shape (M 1, N 16, K 128) with one argument wrong
    one = dict(qa=P, lda=128, sa=P, qw=P, ldw=128, fmt=0, sw=P, nsw=1, bias=None, C=P, ldc=16, M=1, N=16, K=128, epi=lib.EPI_BIAS,
               gate=None, R=None, ldr=0)
    for change, needle in ((dict(qw=None), "gemm_fp8: null operand"), (dict(lda=136), "rows 16-byte aligned (lda 136, ldw 128, ldc 16)"),
                           (dict(ldc=8), "rows 16-byte aligned (lda 128, ldw 128, ldc 8)"), (dict(C=P + 4), "operands must be 16-byte aligned"),
                           (dict(bias=P + 2), "(scales and bias 8-byte)"),
                           (dict(epi=lib.EPI_BIAS_GATE_RES, gate=P, R=P, ldr=8), "gemm_fp8: gate/R alignment"),
                           (dict(epi=lib.EPI_BIAS_GATE_RES, gate=P + 4, R=P, ldr=16), "gemm_fp8: gate/R alignment")):
        bad(L.apexmi_gemm_fp8(*{**one, **change}.values(), None), needle)
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


def _tiny(which):
    import apex_studio_amd  # noqa: F401
    if which == "wan":
        from apex_studio_amd.wan import WanTransformer3DModel
        m = WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=1, attention_head_dim=128, in_channels=16, out_channels=16,
                                  text_dim=64, freq_dim=256, ffn_dim=256, num_layers=1, cross_attn_norm=True, eps=1e-6,
                                  device="cpu", dtype=torch.bfloat16)
        a1, a2 = m.blocks[0].attn1, m.blocks[0].attn2
        return m, [a1.to_q, a1.to_k, a1.to_v], [a2.to_k, a2.to_v]
    from apex_studio_amd.flux import FluxTransformer2DModel
    m = FluxTransformer2DModel(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128,
                               num_attention_heads=1, joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=False,
                               axes_dims_rope=(16, 56, 56), device="cpu", dtype=torch.bfloat16)
    a = m.transformer_blocks[0].attn
    return m, [a.to_q, a.to_k, a.to_v], [a.add_q_proj, a.add_k_proj, a.add_v_proj]


@pytest.mark.parametrize("case", ["first-group", "later-group"])
@pytest.mark.parametrize("which", ["wan", "flux"])
def test_adopt_refuses_a_mixed_group_and_releases_nothing(which, case):
    """A fused projection with a record on ONE of its parts is refused, and the refusal leaves every parameter's bf16 storage in
    place: every group is checked before any is released.  first-group: a record on to_q only.  later-group: q | k | v all
    resident (a group that would be released if groups were adopted one by one) and a record on the first part of the next
    group only.  `_packed` is set by hand: `pack()` itself needs a ROCm device and is not what is tested."""
    from apex_studio_amd import lib, ops
    m, first, second = _tiny(which)
    m._packed = True

    def record(lin):
        lin.weight._fp8 = ops.Fp8Weight(torch.zeros(lin.weight.shape).to(torch.float8_e4m3fn), torch.ones(1))
    if case == "first-group":
        record(first[0])
    else:
        for lin in first:
            record(lin)
        record(second[0])
    sizes = {k: p.numel() for k, p in m.named_parameters()}
    assert all(n > 0 for n in sizes.values())
    with pytest.raises(lib.ApexMIError, match="mixes"):
        m._fp8_adopt()
    assert {k: p.numel() for k, p in m.named_parameters()} == sizes, "a refused adopt released bf16 storage"
    assert not getattr(m, "_fp8_bytes", 0) and not getattr(m, "_fp8_records", None)
    assert all(hasattr(lin.weight, "_fp8") for lin in (first if case == "later-group" else first[:1]))


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
