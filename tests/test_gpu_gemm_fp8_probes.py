"""Exact probes of the opt-in FP8 compute path on the GPU (operands and references: tests/gemm_fp8_probes.py; what the
comparison rejects and the older pair of bars accepts: tests/test_gemm_fp8_probes_host.py).

GEMM: every output is a column slice of a wider buffer pre-filled with a sentinel (ldc > N, one guard row above and below, 8 guard
columns on each side), qa has a padded row stride, and the WHOLE buffer, sentinels included, must equal what a correct run leaves:
torch.equal, no bar, no element excluded.  The only assertions that are not exact are the tanh-GELU ones, under the bars of
test_gemm_epilogue_activations_on_every_bf16_code_point (at most 1 bf16 ulp from the float64 definition, more than 99 % equal).
Quantiser: codes and scales bit for bit against the definition-based reference, into a wider byte buffer whose columns past K
must stay untouched.

Found by these probes: no kernel or wrapper bug.  One observation, pinned by test_nan_codes_stay_in_their_row_and_column and
written into DESIGN.md §3.6: an output whose dot product reads a NaN code (0x7f or 0xff, in either operand, whatever the partner
code) is NaN - 542 of 542 such outputs - and every other output is bit-equal to the run without the NaN codes.

Measured on the MI355X (profiles/gemm_fp8_probes_measured.jsonl; `measured` records them):
  * exact ties of the bf16 rounding, the smallest share among the eight exact results of a case: 2.7 % (1 x 112 x 1152) to 16.0 %
    (1 x 144 x 128) over the 82 cases; asserted non-zero for every result of every case;
  * tanh GELU on the fixed-point pre-activations, per case over its four launches: worst distance 1 bf16 ulp in 17 of the 77
    cases and under 2e-5 in the other 60, smallest share of points equal to the float64 definition rounded to bf16 99.22 %
    (1 x 128 x 384: one of 128 elements) to 100 %;
  * tanh GELU on all 65 536 bf16 patterns: worst distance 4.6e-6 bf16 ulp, 99.992 % equal (the unequal ones are results below
    2^-100, where the distance is counted in units of 2^-107)."""
import pytest
import torch

from tests import gemm_fp8_probes as P
from tests.conftest import measured
from tests.gemm_fp8_probes import BF, F8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _padded_codes(codes, extra=128):
    """the codes [M, K] as a view of a wider byte buffer: lda = K + extra, the padding holds a NaN code"""
    M, K = codes.shape
    buf = torch.full((M, K + extra), P.SENTINEL_CODE, dtype=U8, device=DEV)
    buf[:, :K] = codes.to(DEV)
    return buf[:, :K]


class Dev:
    """the operands of one fixed-point case on the device"""

    def __init__(self, op):
        ops = _ops()
        self.op = op
        self.qa = _padded_codes(P.codes_of(op.qa))
        self.qw = P.codes_of(op.qw).view(F8).to(DEV)
        self.w = {True: ops.Fp8Weight(self.qw, op.sw.to(DEV)), False: ops.Fp8Weight(self.qw, op.sw_one.to(DEV))}
        assert self.w[True].scale.numel() == op.N and self.w[False].scale.numel() == 1
        self.sa, self.bias, self.gate = op.sa.to(DEV), op.bias.to(BF).to(DEV), op.gate.to(DEV)
        self.res = op.res.to(BF).to(DEV)


def _launch(d, view, epilogue, per_row, bias, inplace):
    ops = _ops()
    kw = {}
    if epilogue == "gate_res":
        if inplace:
            view.copy_(d.res)
        kw = dict(gate=d.gate, residual=view if inplace else d.res)
    out = ops.gemm_fp8(d.qa, d.sa, d.w[per_row], d.bias if bias else None, out=view, epilogue=epilogue, **kw)
    assert out.data_ptr() == view.data_ptr()


def _check_exact(buf, want, what):
    torch.cuda.synchronize()
    msg = P.buffer_mismatches(buf.cpu(), want)
    assert not msg, f"{what}: {msg}"


def _check_gelu(buf, x, what):
    """the view under the project's GELU bars, everything around it still the sentinel"""
    torch.cuda.synchronize()
    host = buf.cpu()
    M, N = x.shape
    got = host[1:M + 1, P.GUARD:P.GUARD + N]
    full = torch.full_like(host, P.SENTINEL)
    full[1:M + 1, P.GUARD:P.GUARD + N] = got
    assert torch.equal(torch.nan_to_num(host), torch.nan_to_num(full)), f"{what}: store outside the output view"
    assert not bool(((got == P.SENTINEL) & (x != P.SENTINEL)).any()), f"{what}: elements left at the sentinel"
    worst, equal = P.gelu_judge(got, x)
    print(f"[{what}] worst {worst} bf16 ulp from the float64 definition, {100 * equal:.3f} % equal")
    assert worst <= P.GELU_MAX_ULP and equal > P.GELU_MIN_EQUAL, (what, worst, equal)
    return worst, equal


def _run_variants(M, N, K, variants):
    """every variant of one fixed-point case: returns (worst gelu ulp, smallest share of equal gelu points)"""
    op = P.fixed_point(M, N, K)
    d = Dev(op)
    worst, equal = 0.0, 1.0
    for epilogue, per_row, bias, inplace in variants:
        what = f"gemm_fp8 {M}x{N}x{K} {epilogue} sw={'row' if per_row else 'one'} bias={bias} inplace={inplace}"
        buf, view = P.sentinel_buffer(M, N, DEV)
        _launch(d, view, epilogue, per_row, bias, inplace)
        if epilogue == "gelu":
            x = P.pre_activation(op, per_row, bias)
            assert P.span_log2(op, "bias", per_row, bias) < P.SPAN_BITS
            w, e = _check_gelu(buf, x, what)
            worst, equal = max(worst, w), min(equal, e)
        else:
            _check_exact(buf, P.want(M, N, K, epilogue, per_row, bias), what)
    ties = P.tie_fractions(op)
    print(f"[gemm_fp8 {M}x{N}x{K}] exact ties of the bf16 rounding: {min(ties.values()):.4f} .. {max(ties.values()):.4f}")
    measured(f"gemm_fp8_probes.no_tie.{M}x{N}x{K}", 1.0 - min(ties.values()), 1.0)          # every variant holds a tie
    if any(v[0] == "gelu" for v in variants):
        measured(f"gemm_fp8_probes.gelu_worst_ulp.{M}x{N}x{K}", worst, P.GELU_MAX_ULP + 0.25)      # distances are multiples of 0.5
        measured(f"gemm_fp8_probes.gelu_not_equal.{M}x{N}x{K}", 1.0 - equal, 1.0 - P.GELU_MIN_EQUAL)


# --------------------------------------------------------------------------------------------------- scales and epilogues
@pytest.mark.parametrize("N", P.EDGE_NS)
@pytest.mark.parametrize("M", P.EDGE_MS)
def test_scales_and_epilogue_operands_at_every_edge(M, N):
    """per-row sa, per-column and single sw, bias (present and None), gate and residual (separate and in place) under bias, gelu
    and gate_res at 1, 3 and 9 K-tiles: M and N one short of, at and one past a tile, a lone row, a lone 16-column group"""
    for K in P.EDGE_KS:
        _run_variants(M, N, K, P.VARIANTS)


def test_long_k():
    """32 K-tiles: the span condition holds through integers in [-3, 3]"""
    _run_variants(*P.LONG_K, P.VARIANTS)


# --------------------------------------------------------------------------------------------------------------- tile order
@pytest.mark.parametrize("N", P.ORDER_NS)
@pytest.mark.parametrize("M", P.ORDER_MS)
def test_tile_order_past_one_band(M, N):
    """tiles_m 9, 10 and 17 (a part-filled band of 1 and of 2 tile rows, two full bands plus one) x tiles_n 1 and 3: every tile
    written once, from its own operands"""
    _run_variants(M, N, P.ORDER_K, [("bias", True, True, False), ("gate_res", False, True, True), ("gate_res", True, False, False)])


# -------------------------------------------------------------------------------------------------------- the C entry point
def test_c_entry_point_with_padded_weight_rows_and_its_own_residual_stride():
    """apexmi_gemm_fp8 called directly: ldw > K (ops.Fp8Weight always packs), ldr != ldc, lda > K"""
    _ops()
    from apex_studio_amd import lib
    M, N, K = P.ABI
    op = P.fixed_point(M, N, K)
    d = Dev(op)
    qw = _padded_codes(P.codes_of(op.qw), extra=64)
    sw = op.sw.to(BF).to(DEV)
    rbuf = torch.full((M, N + 40), P.SENTINEL, dtype=BF, device=DEV)
    res = rbuf[:, 4:4 + N]
    res.copy_(d.res)
    st = torch.cuda.current_stream().cuda_stream
    for epi, name in ((lib.EPI_BIAS, "bias"), (lib.EPI_BIAS_GATE_RES, "gate_res")):
        buf, view = P.sentinel_buffer(M, N, DEV)
        assert qw.stride(0) == K + 64 and res.stride(0) != view.stride(0) and d.qa.stride(0) == K + 128
        rc = lib.load().apexmi_gemm_fp8(d.qa.data_ptr(), d.qa.stride(0), d.sa.data_ptr(), qw.data_ptr(), qw.stride(0), 0, sw.data_ptr(), N,
                                        d.bias.data_ptr(), view.data_ptr(), view.stride(0), M, N, K, epi, d.gate.data_ptr(),
                                        res.data_ptr(), res.stride(0), st)
        lib.check(rc, "gemm_fp8")
        _check_exact(buf, P.want(M, N, K, name), f"C entry point {name}")
    torch.cuda.synchronize()
    keep = torch.full((M, N + 40), P.SENTINEL, dtype=BF)
    keep[:, 4:4 + N] = op.res.to(BF)
    assert torch.equal(rbuf.cpu(), keep), "the residual buffer is read only"


# -------------------------------------------------------------------------------------------------------------- code points
@pytest.mark.parametrize("role", ["act", "weight"])
def test_every_finite_e4m3_code_through_the_mfma(role):
    """254 codes (subnormals, +-448, -0 included), one non-zero product per output, at every byte position of a K-tile"""
    ops = _ops()
    cp = P.code_points(role)
    want = P.expected(cp.ref())
    buf, view = P.sentinel_buffer(cp.M, cp.N, DEV)
    w = ops.Fp8Weight(cp.qw_codes.view(F8).to(DEV), cp.sw.to(DEV))
    ops.gemm_fp8(_padded_codes(cp.qa_codes), cp.sa.to(DEV), w, None, out=view)
    _check_exact(buf, want, f"every code as {role}")
    assert int((want != 0).sum()) >= 252 * min(cp.M, cp.N)


def test_nan_codes_stay_in_their_row_and_column():
    """0x7f and 0xff planted into both operands: every output whose dot product reads none of them is bit-equal to the run
    without them (and to the exact expectation); every output that reads one is NaN"""
    ops = _ops()
    M, N, K = P.NAN_SHAPE
    op = P.fixed_point(M, N, K)
    d = Dev(op)
    qa, qw = P.codes_of(op.qa).clone(), P.codes_of(op.qw).clone()
    for which, r, k, code in P.NAN_PLANTS:
        (qa if which == "a" else qw)[r, k] = code
    clean_buf, clean = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(d.qa, d.sa, d.w[True], d.bias, out=clean)
    _check_exact(clean_buf, P.want(M, N, K), "the run without NaN codes")
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(_padded_codes(qa), d.sa, ops.Fp8Weight(qw.view(F8).to(DEV), op.sw.to(DEV)), d.bias, out=view)
    torch.cuda.synchronize()
    host, touched = buf.cpu(), P.nan_touched(M, N)
    got = host[1:M + 1, P.GUARD:P.GUARD + N]
    print(f"[nan codes] {int(torch.isnan(got[touched]).sum())} of {int(touched.sum())} touched outputs are NaN")
    assert bool(torch.isnan(got[touched]).all()), "an output that reads a NaN code must be NaN"
    got[touched] = 0.0                                           # `got` is a view: the whole buffer is compared
    untouched = torch.where(touched, torch.zeros((), dtype=BF), clean_buf.cpu()[1:M + 1, P.GUARD:P.GUARD + N])
    msg = P.buffer_mismatches(host, untouched)
    assert not msg, f"outputs that read no NaN code changed: {msg}"


def test_gelu_instance_on_every_bf16_code_point():
    """all codes zero, bias = the 65 536 bf16 patterns: the pre-activation is exactly the code point (512 tile columns)"""
    ops = _ops()
    M, N, K = 2, 65536, 128
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    g = torch.Generator().manual_seed(3)
    sw = torch.tensor(P.SW)[P._walk(N, 1, 8, g)]
    w = ops.Fp8Weight(torch.zeros(N, K, dtype=U8, device=DEV).view(F8), sw.to(DEV))
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(_padded_codes(torch.zeros(M, K, dtype=U8)), torch.tensor([1.5, 0.75], device=DEV), w, bits.to(DEV), out=view,
                 epilogue="gelu")
    worst, equal = _check_gelu(buf, bits.float().double().expand(M, N), "gemm_fp8 gelu, every bf16 code point")
    measured("gemm_fp8_probes.gelu_worst_ulp.codepoints", worst, P.GELU_MAX_ULP + 0.25)
    measured("gemm_fp8_probes.gelu_not_equal.codepoints", 1.0 - equal, 1.0 - P.GELU_MIN_EQUAL)


# ---------------------------------------------------------------------------------------------------------------- quantiser
def _quantise(a):
    """ops.quant_rows_fp8 of bf16 a (CPU) through a padded input, into guarded outputs -> (codes, scales) on the CPU"""
    ops = _ops()
    M, K = a.shape
    src = torch.zeros(M, K + 64, dtype=BF, device=DEV)
    src[:, :K] = a.to(DEV)
    qbuf, q = P.byte_buffer(M, K, DEV)
    sbuf = torch.full((M + 2,), -1.0, dtype=torch.float32, device=DEV)
    ops.quant_rows_fp8(src[:, :K], out=q, scale_out=sbuf[1:M + 1])
    torch.cuda.synchronize()
    qh, sh = qbuf.cpu(), sbuf.cpu()
    assert bool((qh[:, K:] == P.SENTINEL_CODE).all()), "the columns past K of the code buffer were written"
    assert float(sh[0]) == -1.0 and float(sh[M + 1]) == -1.0, "a scale outside the M rows was written"
    return qh[:, :K], sh[1:M + 1]


def _same_codes(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        r, k = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} codes differ; first at (row {r}, k {k}): got {int(got[r, k]):#04x} want {int(want[r, k]):#04x}")


@pytest.mark.parametrize("K", P.QUANT_KS)
@pytest.mark.parametrize("M", P.QUANT_MS)
def test_quantiser_past_the_first_k_step(M, K):
    """K = 1152 and 2176: a second and a third step of the K loop; the row's absmax in the second step only, the third only, the
    last 16 columns; adjacent rows six decades apart; odd M and more than one workgroup"""
    a = P.quant_rows(M, K)
    want_q, want_s = P.quant_ref(a)
    q, s = _quantise(a)
    assert torch.equal(s, want_s), (s, want_s)
    _same_codes(q, want_q, f"quantiser {M}x{K}")
    assert int((want_q[:, 1024:] & 0x7F != 0).sum()) > 0 and not bool(((q & 0x7F) == 0x7F).any())


@pytest.mark.parametrize("e", P.CODEPOINT_EXPONENTS)
def test_quantiser_on_every_bf16_value(e):
    """all finite bf16 values with |x| <= 448, times 2^e, in rows that hold 448 x 2^e: scale = 2^e exactly, so every rounding
    tie, the subnormal range, underflow to +-0 and saturation at +-448 are met"""
    a = P.quant_codepoint_rows(e)
    want_q, want_s = P.quant_ref(a)
    assert bool((want_s == 2.0 ** e).all())
    q, s = _quantise(a)
    assert torch.equal(s, want_s), (s, want_s)
    _same_codes(q, want_q, f"quantiser, every bf16 value x 2^{e}")
    assert not bool(((q & 0x7F) == 0x7F).any()), "no NaN code"


# -------------------------------------------------------------------------------------------------------------------- route
def test_route_through_ops_gemm_is_exact():
    """ops.gemm with compute = 'fp8' on bf16 activations that quantise losslessly: out= a column slice, and gate_res in place"""
    ops = _ops()
    op, a = P.routed()
    M, N, K = P.ROUTE
    w = ops.Fp8Weight(P.codes_of(op.qw).view(F8).to(DEV), op.sw.to(DEV))
    w.compute = "fp8"
    abuf = torch.zeros(M, K + 64, dtype=BF, device=DEV)
    abuf[:, :K] = a.to(DEV)
    av, bias = abuf[:, :K], op.bias.to(BF).to(DEV)
    buf, view = P.sentinel_buffer(M, N, DEV)
    assert ops.fp8_compute_route(av, w, view, "bias") and ops.fp8_compute_route(av, w, view, "gate_res")
    ops.gemm(av, w, bias, out=view)
    _check_exact(buf, P.routed_want("bias"), "route, bias")
    buf, view = P.sentinel_buffer(M, N, DEV)
    view.copy_(op.res.to(BF).to(DEV))
    ops.gemm(av, w, bias, out=view, epilogue="gate_res", gate=op.gate.to(DEV), residual=view)
    _check_exact(buf, P.routed_want("gate_res"), "route, gate_res in place")
