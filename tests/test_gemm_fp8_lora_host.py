"""The run-time LoRA form of the FP8 GEMM, the parts that need no GPU: the conditions under which the probes of
tests/gemm_fp8_lora_probes.py are exact, for every case tests/test_gpu_gemm_fp8_lora.py runs; that the comparison rejects single
wrong decisions; the routing predicate; the model and engine switches; the host-side argument checks of apexmi_gemm_fp8_lora."""
import os
import re

import pytest
import torch

from tests import gemm_fp8_lora_probes as L
from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------------------------------------- the probes' conditions
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_fixed_point_cases_are_exact_in_float32(case):
    """span below 2^22 for all eight exact variants (and for the four gelu pre-activations), the adapter sum on its 2^-4 grid and
    non-zero nearly everywhere, the padding columns zero, a tie of the bf16 rounding in every result"""
    M, N, K, Rp = case
    lo = L.fixed_point(*case)
    assert Rp % 64 == 0 and tuple(lo.t.shape) == (M, Rp) and tuple(lo.lb.shape) == (N, Rp)
    assert not bool(lo.t[:, Rp - L.PAD:].any()) and not bool(lo.lb[:, Rp - L.PAD:].any())
    assert torch.equal((lo.term / L.GA).round() * L.GA, lo.term), "the adapter sum is a multiple of 2^-4"
    spans = {v: L.span_log2(lo, *v) for v in L.EXACT_VARIANTS}
    assert max(spans.values()) < L.SPAN_BITS, spans
    nonzero = float((lo.term != 0).double().mean())
    ties = L.tie_fractions(lo)
    print(f"[{L.case_id(case)}] worst span 2^{max(spans.values()):.1f}, adapter term non-zero on {100 * nonzero:.2f} %, "
          f"ties {min(ties.values()):.3f} .. {max(ties.values()):.3f}")
    assert nonzero > 0.99 and min(ties.values()) > 0
    for v in L.EXACT_VARIANTS:
        ref = L.gemm_ref(lo, *v)
        assert torch.equal(ref.float().double(), ref)
        assert L.want(M, N, K, Rp, *v).dtype == BF
    # the adapter term matters: the expected buffer is not the one of the plain kernel
    assert not torch.equal(L.want(M, N, K, Rp), P.want(M, N, K))


def test_cases_cover_what_they_claim():
    tiles = [(-(-M // P.BM), -(-N // P.BN), K // P.BK, Rp // 64) for M, N, K, Rp in L.CASES]
    assert (2, 2, 2, 1) in tiles            # edge rows and columns behind one full tile
    assert (2, 2, 1, 2) in tiles            # nk = 1: from the only K-tile straight into two rank tiles
    assert (3, 3, 3, 2) in tiles            # a 3 x 3 tile grid
    assert (1, 16, 128, 64) in L.CASES      # the smallest legal problem
    assert all(M % P.BM and N % P.BN for M, N, _, _ in L.CASES)


def test_one_hot_family_has_one_product_per_output():
    oh = L.one_hot()
    M, N, K, Rp = L.ONE_HOT
    ref = oh.ref()
    assert int(((oh.t != 0).float() @ (oh.lb != 0).float().T).max()) == 1
    m = torch.arange(M)
    assert torch.equal(ref, (oh.t[m, oh.hot].double().view(-1, 1) * oh.lb[:, oh.hot].double().T))
    assert bool((ref != 0).all()) and torch.equal(P.expected(ref).double(), ref), "every output is one bf16-exact product"
    # a lane map that swaps the two 8-element halves of a k-step, or k-steps, or the two rank tiles, reads a zero or another B'
    for perm in (lambda r: r ^ 8, lambda r: r ^ 16, lambda r: r ^ 64, lambda r: (r + 1) % Rp):
        r = perm(torch.arange(Rp))
        wrong = oh.t[:, r].double() @ oh.lb.double().T
        assert int((wrong != ref).sum()) >= M * N // 4


# --------------------------------------------------------------------------------------------- what the comparison rejects
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_single_wrong_decisions_change_the_expected_buffer(case):
    """Each mutant differs from the contract in ONE decision.  Stated minimum: half of the elements it can touch — M x N, or
    (M - 1) x N for a row shift of t, M x 4 for the clamp of the last 4-column group, nothing for the bias mutant without a bias.
    Reason: two different operand rows give different sums but for coincidences (the terms are random integers on a grid), and
    the bf16 rounding hides a difference only where it is under half an ulp of the result."""
    M, N, K, Rp = case
    lo = L.fixed_point(*case)
    for per_row in (True, False):
        for bias in (True, False):
            got = {k: L.changed(lo, y, per_row, bias) for k, y in L.mutants(lo, per_row, bias).items()}
            floor = {k: M * N // 2 for k in got}
            floor["t a row above"] = (M - 1) * N // 2
            floor["B' with a wrong 4-column clamp"] = M * 4 // 2
            if not bias:
                floor["bias before the scales"] = 0
            if Rp == 64:
                assert got["last rank tile dropped"] == got["adapter term omitted"]
            print(f"[{L.case_id(case)} per_row={per_row} bias={bias}] {got}")
            for k in got:
                assert got[k] >= floor[k] and (got[k] > 0 or floor[k] == 0), (k, got[k], floor[k])


# ------------------------------------------------------------------------------------------------------------------ the route
def _weight(N=32, K=256, dt=F8, compute="fp8", lora_compute="fp8", factors=True):
    from apex_studio_amd import ops
    w = ops.Fp8Weight(torch.zeros(N, K).to(dt), torch.ones(N))
    w.compute, w.lora_compute = compute, lora_compute
    w.parts = [("lin", 0, N)]
    if factors:
        w.set_lora([("lin", torch.zeros(4, K), torch.zeros(N, 4), 1.0)])
    return w


def test_fp8_lora_route_truth_table():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    assert ops.Fp8Weight.lora_compute == "bf16"
    buf = torch.zeros(5, 256 + 64, dtype=BF)
    a = buf[:, :256]
    w = _weight()
    assert w.lora_A.shape == (64, 256) and w.lora_B.shape == (32, 64)
    assert ops.fp8_lora_route(a, w, None, "bias", buf)
    assert ops.fp8_lora_route(a, w, torch.zeros(5, 32, dtype=BF), "gate_res", buf) and ops.fp8_lora_route(a, w, None, "gelu", buf)
    p = torch.nn.Parameter(torch.empty(0), requires_grad=False)
    p._fp8 = w
    assert ops.fp8_lora_route(a, p, lora_buf=buf)
    assert not ops.fp8_lora_route(a, _weight(lora_compute="bf16"), lora_buf=buf)             # the flag is off (the default)
    assert not ops.fp8_lora_route(a, _weight(compute="bf16"), lora_buf=buf)                  # fp8 compute is off
    assert not ops.fp8_lora_route(a, _weight(factors=False), lora_buf=buf)                   # no factors: fp8_compute_route's case
    assert not ops.fp8_lora_route(a, w, torch.zeros(5, 32), "bias", buf)                     # f32 out
    assert not ops.fp8_lora_route(a.float(), w, lora_buf=buf)                                # f32 activations
    assert not ops.fp8_lora_route(a, _weight(dt=torch.float8_e5m2), lora_buf=buf)            # e5m2
    assert not ops.fp8_lora_route(a, w, None, "silu", buf)                                   # an epilogue the kernel lacks
    assert not ops.fp8_lora_route(a, w)                                                      # no lora_buf
    assert not ops.fp8_lora_route(a, w, lora_buf=torch.zeros(5, 320, dtype=BF))              # another buffer
    assert not ops.fp8_lora_route(a, w, lora_buf=buf[:, :256 + 32])                          # too narrow for K + Rp
    assert not ops.fp8_lora_route(a[:4], w, lora_buf=buf)                                    # other rows
    buf192 = torch.zeros(5, 192 + 64, dtype=BF)
    assert not ops.fp8_lora_route(buf192[:, :192], _weight(K=192), lora_buf=buf192)          # K % 128
    assert not ops.fp8_lora_route(a, _weight(N=24), lora_buf=buf)                            # N % 16
    # fp8_compute_route is unchanged: False with factors attached, whatever the flag
    assert not ops.fp8_compute_route(a, w) and not ops.fp8_compute_route(a, _weight(lora_compute="bf16"))
    w.set_lora([])
    assert ops.fp8_compute_route(a, w) and not ops.fp8_lora_route(a, w, lora_buf=buf)


def test_gemm_fp8_takes_both_adapter_operands_or_neither():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib, ops
    w = _weight(factors=False)
    q, s = torch.zeros(5, 256, dtype=torch.uint8), torch.ones(5)
    with pytest.raises(lib.ApexMIError, match="both or neither"):
        ops.gemm_fp8(q, s, w, lora_t=torch.zeros(5, 64, dtype=BF))
    with pytest.raises(lib.ApexMIError, match="both or neither"):
        ops.gemm_fp8(q, s, w, lora_B=torch.zeros(32, 64, dtype=BF))


# ---------------------------------------------------------------------------------------------------------- model and engines
def test_set_fp8_compute_lora_needs_on():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(patch_size=(1, 2, 2), num_attention_heads=1, attention_head_dim=128, in_channels=16, out_channels=16,
                              text_dim=64, freq_dim=256, ffn_dim=256, num_layers=1, cross_attn_norm=True, eps=1e-6,
                              device="cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="on=True"):
        m.set_fp8_compute(False, lora=True)
    # with records: the flag lands on them, and lora=False (the default) clears it
    from apex_studio_amd import ops
    rec = ops.Fp8Weight(torch.zeros(32, 128).to(F8), torch.ones(1))
    m._fp8_records = {"x": rec}
    m.set_fp8_compute(True, lora=True)
    assert (rec.compute, rec.lora_compute) == ("fp8", "fp8")
    m.set_fp8_compute(True)
    assert (rec.compute, rec.lora_compute) == ("fp8", "bf16")
    m.set_fp8_compute(True, lora=True)
    m.set_fp8_compute(False)
    assert (rec.compute, rec.lora_compute) == ("bf16", "bf16")


def test_engines_take_the_lora_switch():
    import inspect
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    from tests.test_engines import _FakeWan
    for cls in (WanT2VEngine, WanI2VEngine):
        assert inspect.signature(cls.__init__).parameters["fp8_lora"].default is False

    class Spy(_FakeWan):
        def set_fp8_compute(self, on, lora=False):
            self.fp8 = (on, lora)
    for cls in (WanT2VEngine, WanI2VEngine):
        hi, lo = Spy(1.0), Spy(2.0)
        eng = cls(hi, lo, fp8_compute=True, fp8_lora=True)
        assert eng.fp8_lora and hi.fp8 == (True, True) and lo.fp8 == (True, True)
        hi, lo = Spy(1.0), Spy(2.0)
        assert cls(hi, lo, fp8_compute=True).fp8_lora is False and hi.fp8 == (True, False)
        with pytest.raises(ValueError, match="fp8_compute=True"):
            cls(Spy(1.0), Spy(2.0), fp8_lora=True)


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_header_bindings_and_kernel_name():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import build, lib
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+apexmi_gemm_fp8_lora\s*\(", header) and "manager.py:454-606" in header
    base, lora = lib.SIGNATURES["apexmi_gemm_fp8"][1], lib.SIGNATURES["apexmi_gemm_fp8_lora"][1]
    assert len(lora) == len(base) + 5 and lora[:len(base) - 1] == base[:-1] and lora[-1] == base[-1]
    assert hasattr(lib.load(), "apexmi_gemm_fp8_lora")
    # the LoRA form is an instantiation of the ONE kernel the no-spill list names, so the build's check covers it
    with open(os.path.join(ROOT, "apex-studio_amd", "csrc", "gemm_fp8.hip")) as f:
        src = f.read()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)
    assert sorted(kernels) == ["gemm_fp8_kernel", "quant_rows_fp8_kernel"], kernels
    # (the form is chosen by the argument type: LORA = the kernel was given an Fp8LoraGemm, which gemm_fp8_run launches it with)
    assert "gemm_fp8_kernel" in build.NO_SPILL["gemm_fp8.hip"] and re.search(r"gemm_fp8_kernel<\w+, Args>", src)
    assert "LORA = std::is_same_v<Args, Fp8LoraGemm>" in src and re.search(r"Fp8LoraGemm L\{.*\n(.*\n)*?\s*fp8_launch\(epilogue, L, stream\)", src)


def test_argument_validation_reports_a_reason():
    """apexmi_gemm_fp8_lora validates on the host before any launch; dummy (never dereferenced) pointers"""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    Lb = lib.load()
    Pp = 0x100000                     # 16-byte aligned dummy address

    def bad(rc, needle):
        msg = Lb.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    def gemm(M=8, N=16, K=128, Rp=64, t=Pp, lb=Pp, ldt=None, ldb=None, fmt=0, epi=lib.EPI_BIAS):
        return Lb.apexmi_gemm_fp8_lora(Pp, K, Pp, Pp, K, fmt, Pp, 1, None, Pp, N, M, N, K, epi, None, None, 0, t,
                                       Rp if ldt is None else ldt, lb, Rp if ldb is None else ldb, Rp, None)

    bad(gemm(Rp=32), "Rp=32")
    bad(gemm(Rp=96), "Rp=96")
    bad(gemm(Rp=0), "Rp=0")
    bad(gemm(t=None), "null adapter operand")
    bad(gemm(lb=None), "null adapter operand")
    bad(gemm(ldt=64 - 8), "at least Rp=64 wide")
    bad(gemm(ldb=64 - 8), "at least Rp=64 wide")
    bad(gemm(ldb=68), "multiples of 8")
    bad(gemm(ldt=68), "multiples of 8")
    bad(gemm(t=Pp + 8), "16-byte aligned")
    bad(gemm(ldt=(1 << 22) + 8), "2^22")
    # everything apexmi_gemm_fp8 checks
    bad(gemm(K=100), "K=100")
    bad(gemm(N=12), "N=12")
    bad(gemm(fmt=1), "e5m2")
    bad(gemm(M=0), "M=0")
    bad(gemm(epi=lib.EPI_BIAS_GATE_RES), "needs gate and R")
    bad(gemm(epi=lib.EPI_BIAS | lib.EPI_F32_IO), "f32 output")
