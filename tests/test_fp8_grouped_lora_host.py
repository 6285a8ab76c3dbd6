"""The grouped run-time LoRA form of the FP8 GEMM and Flux run-time LoRA on resident fp8 weights, the parts that
need no GPU: the routing predicate `ops.fp8_grouped_lora_route`, the model switch, the conditions under which the probes of
tests/gemm_fp8_grouped_lora_probes.py are exact for every case tests/test_gpu_gemm_fp8_grouped_lora.py runs, that the comparison
rejects single wrong decisions of a grouped kernel, the C ABI and the host-side argument checks of the two new entry points."""
import inspect
import os
import re

import pytest
import torch

from tests import gemm_fp8_grouped_lora_probes as GL
from tests import gemm_fp8_lora_probes as L
from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn


def _weight(N=32, K=256, dt=F8, compute="fp8", lora_compute="fp8", factors=True):
    from apex_studio_amd import ops
    w = ops.Fp8Weight(torch.zeros(N, K).to(dt), torch.ones(N))
    w.compute, w.lora_compute = compute, lora_compute
    w.parts = [("lin", 0, N)]
    if factors:
        w.set_lora([("lin", torch.zeros(4, K), torch.zeros(N, 4), 1.0)])
    return w


# ------------------------------------------------------------------------------------------------------------------ the route
def test_fp8_grouped_lora_route_truth_table():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    a, b = torch.zeros(5, 256, dtype=BF), torch.zeros(9, 256, dtype=BF, device="meta")
    wl, wp = _weight(), _weight(N=48, factors=False)
    route = ops.fp8_grouped_lora_route
    assert route([a, b], [wl, wp])                                                # a mixed group: adapter + plain
    assert route([a, b], [wp, wl]) and route([a], [wl]) and route([a, b, a, b], [wl, wl, wp, wl])
    assert route([a, a], [wl, wp], [None, torch.zeros(5, 48, dtype=BF)], ["bias", "gelu"])      # shared rows (QKV + MLP-up)
    buf = torch.zeros(14, 256, dtype=BF)
    assert route([buf[9:], buf[:9]], [wl, wl], None, "gate_res")                  # row slices of one joint buffer
    p = torch.nn.Parameter(torch.empty(0), requires_grad=False)
    p._fp8 = wl
    assert route([a, b], [p, wp])                                                 # a parameter carrying the record
    assert not route([a, b], [wp, wp])                                            # no problem with factors: fp8_grouped_route's case
    assert ops.fp8_grouped_route([a, b], [wp, wp]) and not ops.fp8_grouped_route([a, b], [wl, wp])
    assert not route([a, b], [_weight(lora_compute="bf16"), wp])                  # the flag is off
    assert not route([a, b], [_weight(compute="bf16"), wp])                       # fp8 compute is off
    assert not route([a, b], [wl, _weight(compute="bf16", factors=False)])        # a plain problem that is not routed
    assert not route([a, b], [wl, wp], [torch.zeros(5, 32), None])                # a float out
    assert not route([a, b], [wl, wp], [None, torch.zeros(9, 48)])
    assert not route([a, b], [_weight(dt=torch.float8_e5m2), wp])                 # e5m2
    assert not route([a, b], [wl, _weight(dt=torch.float8_e5m2, factors=False)])
    assert not route([a, torch.zeros(9, 384, dtype=BF)], [wl, _weight(K=384, factors=False)])        # unequal K
    assert not route([a] * 5, [wl] * 5)                                           # 5 problems
    assert not route([], []) and not route([a, b], [wl])
    assert not route([a.float(), b], [wl, wp])                                    # f32 activations
    assert not route([a, b], [wl, wp], None, ["bias", "silu"])                    # an epilogue the kernel lacks
    assert not route([torch.zeros(5, 192, dtype=BF)], [_weight(K=192)])           # K % 128
    assert not route([a], [_weight(N=24)])                                        # N % 16
    # the single-problem predicates are unchanged
    assert not ops.fp8_lora_route(a, wl) and not ops.fp8_compute_route(a, wl) and ops.fp8_compute_route(a, wp)


def test_grouped_wrappers_refuse_mx_lists_and_half_pairs_before_any_launch():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib, ops
    w = _weight(factors=False)
    q, s = torch.zeros(5, 256, dtype=torch.uint8), torch.ones(5)
    t, lb = torch.zeros(5, 64, dtype=BF), torch.zeros(32, 64, dtype=BF)
    mx = (torch.zeros(5, 32, dtype=torch.uint8), torch.zeros(5, 1, dtype=torch.uint8))
    with pytest.raises(lib.ApexMIError, match="block_scales_list / out_mx_list"):
        ops.gemm_fp8_grouped([q], [s], [w], [None], [None], lora_t_list=[t], lora_B_list=[lb], out_mx_list=[mx])
    with pytest.raises(lib.ApexMIError, match="block_scales_list / out_mx_list"):
        ops.gemm_fp8_grouped([q], [None], [w], [None], [None], lora_t_list=[t], lora_B_list=[lb],
                             block_scales_list=[torch.zeros(5, 8, dtype=torch.uint8)])
    with pytest.raises(lib.ApexMIError, match="block_scales_list / out_mx_list"):
        ops.gemm_fp8_grouped_qkv([q], [s], [w], [None], [None], "bias", [1], None, None, [0], 1, 1e-6, None, None, None, None,
                                 out_mx_list=[mx], lora_t_list=[t], lora_B_list=[lb])


# ---------------------------------------------------------------------------------------------------------- model and engine
_TINY = dict(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=1,
             joint_attention_dim=64, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))


def test_set_fp8_compute_lora_needs_on_and_keeps_the_positional_order():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    from apex_studio_amd.flux import FluxTransformer2DModel
    sig = inspect.signature(FluxTransformer2DModel.set_fp8_compute)
    assert list(sig.parameters) == ["self", "on", "fused_quant", "mx_ffn", "lora"]
    assert [sig.parameters[k].default for k in ("fused_quant", "mx_ffn", "lora")] == [False, False, False]
    m = FluxTransformer2DModel(**_TINY, device="cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="on=True"):
        m.set_fp8_compute(False, lora=True)
    rec = ops.Fp8Weight(torch.zeros(32, 128).to(F8), torch.ones(1))
    m._fp8_records = {"x": rec}
    m.set_fp8_compute(True, lora=True)
    assert (rec.compute, rec.lora_compute) == ("fp8", "fp8") and m._fp8_lora is True
    m.set_fp8_compute(True)
    assert (rec.compute, rec.lora_compute) == ("fp8", "bf16") and m._fp8_lora is False
    m.set_fp8_compute(True, False, False, True)
    assert rec.lora_compute == "fp8"
    m.set_fp8_compute(False)
    assert (rec.compute, rec.lora_compute) == ("bf16", "bf16")


def test_switching_off_with_resident_factors_is_refused_and_changes_nothing():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    from apex_studio_amd.flux import FluxTransformer2DModel
    m = FluxTransformer2DModel(**_TINY, device="cpu", dtype=torch.bfloat16)
    rec = _weight()
    m._fp8_records = {"lin": rec}
    m.set_fp8_compute(True, lora=True)
    rec.set_lora([("lin", torch.zeros(4, 256), torch.zeros(32, 4), 1.0)])
    for args in ((False,), (True,)):
        with pytest.raises(lib.ApexMIError, match="delete"):
            m.set_fp8_compute(*args)
        assert (rec.compute, rec.lora_compute) == ("fp8", "fp8") and m._fp8_lora and m._fp8_compute and rec.lora_A is not None
    with pytest.raises(lib.ApexMIError, match="float32"):
        m.set_residual_dtype(torch.float32)
    assert m.residual_dtype == torch.bfloat16
    with pytest.raises(lib.ApexMIError, match="bf16 storage"):
        m.set_storage_dtype(torch.float32)
    assert m.storage_dtype == torch.bfloat16
    rec.set_lora([])
    m.set_fp8_compute(False)
    assert (rec.compute, rec.lora_compute) == ("bf16", "bf16")


def test_engine_takes_the_lora_switch():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_flux import FluxT2IEngine
    assert inspect.signature(FluxT2IEngine.__init__).parameters["fp8_lora"].default is False

    class Spy:
        config = type("C", (), {"in_channels": 64, "guidance_embeds": True})()

        def set_fp8_compute(self, on, fused_quant=False, mx_ffn=False, lora=False):
            self.fp8 = (on, fused_quant, mx_ffn, lora)
    s = Spy()
    eng = FluxT2IEngine(s, fp8_compute=True, fp8_lora=True)
    assert eng.fp8_lora is True and s.fp8 == (True, False, False, True)
    s = Spy()
    assert FluxT2IEngine(s, fp8_compute=True).fp8_lora is False and s.fp8 == (True, False, False, False)
    with pytest.raises(ValueError, match="fp8_compute=True"):
        FluxT2IEngine(Spy(), fp8_lora=True)


# ------------------------------------------------------------------------------------------------------- the probes' conditions
@pytest.mark.parametrize("name", sorted(GL.GROUPS))
def test_every_problem_of_every_launch_is_exact_in_float32(name):
    """span below 2^22 for every (problem, epilogue, scale kind, bias) the GPU file launches; a tie of the bf16 rounding in every
    exact result; the problems of a group share K and differ where the group says they do"""
    shapes, K = GL.GROUPS[name]
    probs = GL.group(name)
    assert len(probs) == len(shapes) <= 4 and all(p.K == K and p.op.K == K for p in probs)
    for launch in GL.LAUNCHES[name]:
        assert len(launch) == len(probs)
        for p, (epi, per_row, bias) in zip(probs, launch):
            span = p.span_log2(epi, per_row, bias)
            assert span < GL.SPAN_BITS, (name, p.M, p.N, epi, span)
            if epi != "gelu":
                ref = p.ref(epi, per_row, bias)
                assert torch.equal(ref.float().double(), ref) and P.G.tie_fraction(ref) > 0
                assert p.want(epi, per_row, bias).dtype == BF
    for p, (M, N, Rp) in zip(probs, shapes):
        assert (p.lo is None) == (Rp == 0)
        if Rp:
            assert tuple(p.lo.t.shape) == (M, Rp) and tuple(p.lo.lb.shape) == (N, Rp)
            assert not torch.equal(p.want(), P.want(M, N, K)), "the adapter term matters"


def test_groups_cover_what_they_claim():
    (mixed, K), (twin, Kt) = GL.MIXED, GL.TWIN
    assert K == 256 and mixed == ((130, 144, 64), (1, 16, 0), (257, 272, 128)) and Kt == 128 and twin == ((130, 144, 128),) * 2
    tiles = [(-(-M // P.BM), -(-N // P.BN), Rp // 64) for M, N, Rp in mixed]
    assert tiles == [(2, 2, 1), (1, 1, 0), (3, 3, 2)]
    # every problem of MIXED sees every epilogue, with both scale kinds somewhere
    for i in range(3):
        assert {launch[i][0] for launch in GL.MIXED_LAUNCHES} == {"bias", "gelu", "gate_res"}
    assert {v[1] for launch in GL.MIXED_LAUNCHES for v in launch} == {True, False}
    a, b = GL.group("twin")
    assert a.op is b.op and not torch.equal(a.lo.t, b.lo.t) and not torch.equal(a.lo.lb, b.lo.lb)
    assert not torch.equal(a.want(), b.want())
    # the one-hot pair: different rank counts, every position of a rank tile in each
    x, y = GL.one_hot_group()
    assert (x.Rp, y.Rp) == (128, 64) and x.K == y.K == GL.ONE_HOT_K
    for oh in (x, y):
        assert int(((oh.t != 0).float() @ (oh.lb != 0).float().T).max()) == 1 and bool((oh.ref() != 0).all())
        assert torch.equal(P.expected(oh.ref()).double(), oh.ref())
    # a kernel that gives the second problem the first one's t (its first rank tile) stores other numbers, and one that gives the
    # first problem the second one's rank count drops every product of its second rank tile
    assert not torch.equal(x.t[:y.M, :64].double() @ y.lb.double().T, y.ref())
    assert int((x.t[:, :64].double() @ x.lb[:, :64].double().T != x.ref()).sum()) >= x.M * x.N // 4


# --------------------------------------------------------------------------------------------- what the comparison rejects
def test_single_wrong_decisions_of_a_grouped_kernel_change_the_expected_buffer():
    """Each mutant differs from the contract in ONE decision for ONE problem.  Stated minimum: half of the problem's M x N
    elements (two different operand sets give different sums but for coincidences, and the bf16 rounding hides a difference only
    where it is under half an ulp)."""
    got = {}
    for k, (p, y, per_row, bias) in GL.grouped_mutants().items():
        got[k] = (GL.changed(p, y, per_row, bias), p.M * p.N)
    print(got)
    for k in ("the adapter term dropped for one problem", "the problems' t swapped", "the rank tiles swapped"):
        assert k in got
    for k, (n, size) in got.items():
        assert n >= size // 2, (k, n, size)


def test_the_in_place_scaling_order_on_a_plain_problem_is_visible_on_random_operands():
    """In the fixed-point family both orders are exact, so THAT comparison cannot tell them apart; the random-operand comparison
    of a no-adapter problem against its own plain launch (torch.equal, tests/test_gpu_gemm_fp8_grouped_lora.py) can: the two
    orders round differently somewhere."""
    (shapes, K) = GL.RANDOM
    M, N, Rp = shapes[1]
    fused, in_place = GL.scaling_orders(GL.random_case(M, N, K, Rp))
    n = int((fused != in_place).sum())
    print(f"[{M}x{N}x{K}] the two scaling orders differ in {n} of {M * N} bf16 outputs")
    assert n > 0


def test_random_case_adapter_matters():
    shapes, K = GL.RANDOM
    for M, N, Rp in shapes:
        c = GL.random_case(M, N, K, Rp)
        matters = float((c["ref"] - c["ref_plain"]).norm() / c["ref"].norm())
        assert matters > 0.3, matters


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_bindings_and_kernel_name():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import build, lib
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    for name in ("apexmi_gemm_fp8_grouped_lora", "apexmi_gemm_fp8_grouped_qkv_lora"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and hasattr(lib.load(), name)
    for base, lora in (("apexmi_gemm_fp8_grouped", "apexmi_gemm_fp8_grouped_lora"),
                       ("apexmi_gemm_fp8_grouped_qkv", "apexmi_gemm_fp8_grouped_qkv_lora")):
        b, l_ = lib.SIGNATURES[base][1], lib.SIGNATURES[lora][1]
        assert len(l_) == len(b) + 5 and l_[:len(b) - 1] == b[:-1] and l_[-1] == b[-1]
    with open(os.path.join(ROOT, "apex-studio_amd", "csrc", "gemm_fp8.hip")) as f:
        src = f.read()
    # the grouped LoRA form is an instantiation of the ONE GEMM kernel the no-spill list names, so the build's check covers it
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)
    assert [k for k in kernels if "gemm" in k] == ["gemm_fp8_kernel"], kernels
    assert "gemm_fp8_kernel" in build.NO_SPILL["gemm_fp8.hip"] and "gemm_fp8_kernel<0, Fp8LoraGroup>" in src


def test_argument_validation_reports_a_reason():
    """both entry points validate every problem on the host before any launch; dummy (never dereferenced) pointers"""
    import ctypes as C
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    Lb = lib.load()
    Pp = 0x100000                     # 16-byte aligned dummy address

    def bad(rc, needle):
        msg = Lb.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    def grouped(n=2, K=128, Rp=(64, 0), t=(Pp, None), lb=(Pp, None), ldt=None, ldb=None, fmt=0, qkv=False):
        VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
        ldt = ldt or [r for r in Rp]
        ldb = ldb or [r for r in Rp]
        N = 384 if qkv else 16
        base = (n, VP(*[Pp] * n), I64(*[K] * n), VP(*[Pp] * n), VP(*[Pp] * n), I64(*[K] * n), INT(*[fmt] * n), VP(*[Pp] * n),
                I64(*[1] * n), None, VP(*[Pp] * n), I64(*[N] * n), INT(*[8] * n), INT(*[N] * n), K, INT(*[lib.EPI_BIAS] * n), None, None,
                None)
        lora = (VP(*t), I64(*ldt), VP(*lb), I64(*ldb), INT(*Rp))
        if qkv:
            return Lb.apexmi_gemm_fp8_grouped_qkv_lora(*base, INT(*[1] * n), None, None, INT(*[8 * i for i in range(n)]), 1, 1e-6, Pp, Pp,
                                                       Pp, Pp, 8 * n, 8 * n, *lora, None)
        return Lb.apexmi_gemm_fp8_grouped_lora(*base, *lora, None)

    for qkv in (False, True):
        bad(grouped(qkv=qkv, Rp=(0, 0), t=(None, None), lb=(None, None)), "no problem carries an adapter")
        bad(grouped(qkv=qkv, Rp=(64, 32), t=(Pp, Pp), lb=(Pp, Pp)), "Rp=32 of problem 1")
        bad(grouped(qkv=qkv, Rp=(96, 0)), "Rp=96 of problem 0")
        bad(grouped(qkv=qkv, ldt=[56, 0]), "at least Rp=64 wide")
        bad(grouped(qkv=qkv, ldb=[56, 0]), "at least Rp=64 wide")
        bad(grouped(qkv=qkv, ldt=[68, 0]), "multiples of 8")
        bad(grouped(qkv=qkv, t=(Pp + 8, None)), "16-byte aligned")
        bad(grouped(qkv=qkv, t=(None, None)), "null adapter operand")
        bad(grouped(qkv=qkv, ldb=[(1 << 22) + 8, 0]), "2^22")
        bad(grouped(qkv=qkv, n=5, Rp=(64,) * 5, t=(Pp,) * 5, lb=(Pp,) * 5), "count=5")
        # everything apexmi_gemm_fp8_grouped checks
        bad(grouped(qkv=qkv, K=100), "K=100")
        bad(grouped(qkv=qkv, fmt=1), "e5m2")
