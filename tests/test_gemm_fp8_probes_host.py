"""The FP8 probes have teeth (no GPU): every case the GPU file runs meets the conditions that make its expected output exact;
the definition-based quantiser reference equals torch's float8_e4m3fn cast on every finite bf16 value up to 448; the whole-buffer
comparison rejects every single wrong decision planted into the reference path and names a coordinate, a tile and a band.

The gap this closes.  tests/test_gpu_gemm_fp8.py checks the scales, bias, gate and residual only under
test_random_operands_under_every_epilogue: rel-L2 under _BARS (3.3e-3) and at least 99 % of the elements within 1 bf16 ulp.
On its (129, 5120, 256) per-row case, evaluated here on the CPU (test_the_older_bars_accept_wrong_epilogue_indices):
  * one whole output column taking its neighbour's weight scale is ACCEPTED (rel-L2 1.7e-3 .. 2.6e-3 for n +- 1 and n + 4);
  * one lane's wrong index - the 4-column group x 2 rows whose sw / bias / gate one lane loads, the 32 columns of one row one
    lane's sa load feeds, the 4 residual values of one load - is ACCEPTED at 32 of 32 placements for sw and for bias, 23 of 32
    for the gate, 62 of 128 rows for sa and 108 of 128 rows for the residual (the rows with the largest activation scales
    carry the norm; elsewhere the error drowns);
  * a whole column on a neighbour's bias (4.9e-3) or gate (9.4e-3), a whole row on a neighbour's sa or residual (8e-2) and the
    last 4-column group on the group before it (4.8e-3 .. 3.4e-2) are rejected by the rel-L2 bar at this size: for those the older
    test has teeth only when the whole column or row is wrong, not when one wave's or one lane's share of it is.
The exact comparison rejects all of them, whatever their extent."""
import pytest
import torch

from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF, F8


def _buffer(out):
    """what a run that stored `out` leaves in the sentinel-filled buffer"""
    buf, view = P.sentinel_buffer(*out.shape)
    view.copy_(out)
    return buf


def _rejected(mutant, want):
    """the whole-buffer comparison rejects the mutant and names a coordinate, a tile, a band and a position in the tile"""
    assert not P.buffer_mismatches(_buffer(want), want)
    msg = P.buffer_mismatches(_buffer(mutant), want)
    assert msg and "got" in msg and "want" in msg and "tiles (m // 128, n // 128)" in msg and "band" in msg, msg
    return msg


# ------------------------------------------------------------------------------------------------ conditions of every case
@pytest.mark.parametrize("case", P.all_fixed_cases(), ids=P.case_id)
def test_every_fixed_point_case_meets_the_exactness_conditions(case):
    M, N, K = case
    op = P.fixed_point(M, N, K)            # the constructor asserts the round trips and the neighbour differences
    assert torch.equal(P.values_of(P.codes_of(op.qa)), op.qa) and torch.equal(P.values_of(P.codes_of(op.qw)), op.qw)
    assert float(op.qa.abs().max()) <= P.int_range(K) and float(op.qw.abs().max()) <= P.int_range(K)
    assert op.sa.unique().numel() >= min(6, M) and (N < 64 or op.sw.unique().numel() >= 6)
    if M > 1:
        assert bool((op.sa[1:] != op.sa[:-1]).all()) and bool((op.res[M - 1] != op.res[M - 2]).all())
    for t in (op.sw, op.bias, op.gate):
        assert bool((t[1:] != t[:-1]).all()) and bool((t[4:] != t[:-4]).all()) and bool((t[N - 4:] != t[N - 8:N - 4]).all())
    ties = P.tie_fractions(op)
    for (epilogue, per_row, bias), tie in ties.items():
        assert P.span_log2(op, epilogue, per_row, bias) < P.SPAN_BITS
        ref = P.gemm_ref(op, epilogue, per_row, bias)
        assert float(ref.abs().max()) <= P.SENTINEL / 4
        assert torch.equal(P.expected(ref).float().to(BF), P.want(M, N, K, epilogue, per_row, bias))
        assert tie > 0, (epilogue, per_row, bias)
        # float32 arithmetic in two orders, scales first and scales last, reproduces the exact value
        sw = (op.sw if per_row else op.sw_one).view(1, -1)
        acc = op.qa @ op.qw.T
        y1 = acc * op.sa.view(-1, 1) * sw + (op.bias if bias else 0)
        y2 = (op.qa * op.sa.view(-1, 1)) @ (op.qw * sw.view(-1, 1)).T + (op.bias if bias else 0) if per_row else y1
        for y in (y1, y2):
            assert torch.equal((y if epilogue == "bias" else op.res + op.gate * y).double(), ref)
    print(f"[{P.case_id(case)}] ties {min(ties.values()):.4f} .. {max(ties.values()):.4f}")


def test_route_case_quantises_losslessly():
    op, a = P.routed()                     # asserts scale = sa (a power of two) and codes = qa through the quantiser reference
    assert a.dtype == BF and float(op.qa.abs().max()) == 448 and bool((op.qa.abs().amax(1) == 448).all())
    assert bool((op.sa[1:] != op.sa[:-1]).all())
    for epilogue in ("bias", "gate_res"):
        assert P.span_log2(op, epilogue) < P.SPAN_BITS and P.tie_fraction(P.gemm_ref(op, epilogue)) > 0
        assert P.routed_want(epilogue).dtype == BF


@pytest.mark.parametrize("role", ["act", "weight"])
def test_code_point_family(role):
    cp = P.code_points(role)               # the constructor asserts 254 finite codes, every byte position, both K-tiles
    ref = cp.ref()                         # asserts one non-zero product per output
    want = P.expected(ref)
    hot = P.values_of(cp.qa_codes if role == "act" else cp.qw_codes)
    assert sorted(hot[hot != 0].tolist()) == sorted(v for v in P.values_of(P.FINITE).tolist() if v != 0)
    codes = (cp.qa_codes if role == "act" else cp.qw_codes)
    assert int((codes == 0x80).sum()) == 1 and not bool(((codes & 0x7F) == 0x7F).any())
    other = P.values_of(cp.qw_codes if role == "act" else cp.qa_codes)
    assert set(other.unique().tolist()) == {1.0, -2.0}
    assert not torch.equal(other[:, :128], other[:, 128:]) and not torch.equal(other[0], other[1])
    assert float(want.float().abs().max()) <= 448 * 2 * 1.5 * 1.5 and int((want != 0).sum()) >= 252 * min(cp.M, cp.N)
    # a partner read at the wrong k, or a code's neighbour in the table, is another result
    shifted = ((P.values_of(cp.qa_codes).double() @ P.values_of(cp.qw_codes).double().roll(1, 1).T)
               * cp.sa.double().view(-1, 1) * cp.sw.double().view(1, -1)).float().to(BF)
    _rejected(shifted, want)


def test_nan_plants():
    M, N, K = P.NAN_SHAPE
    t = P.nan_touched(M, N)
    assert 0 < int(t.sum()) < M * N // 10 and {c for *_, c in P.NAN_PLANTS} == {0x7F, 0xFF}
    assert all(bool(torch.isnan(P.values_of(torch.tensor([c], dtype=torch.uint8))).all()) for *_, c in P.NAN_PLANTS)
    assert all(r < (M if which == "a" else N) and k < K for which, r, k, _ in P.NAN_PLANTS)


# --------------------------------------------------------------------------------------------------------------- quantiser
def test_quantiser_reference_is_torch_cast_on_every_bf16_value():
    x = P.bf16_upto_448()
    got = P.e4m3_nearest(x.float())
    assert torch.equal(got, x.float().to(F8).view(torch.uint8))
    assert not bool(((got & 0x7F) == 0x7F).any()) and int((got == 0x80).sum()) > 1, "underflow keeps the sign"
    # ties: the midpoints of neighbouring e4m3 values are bf16 values; they go to the even code
    v = P.E4M3_POS
    mid = ((v[1:] + v[:-1]) / 2).float()
    assert torch.equal(mid.to(BF).float(), mid)
    m = P.e4m3_nearest(mid)
    assert bool((m % 2 == 0).all()) and torch.equal(m, mid.to(F8).view(torch.uint8))
    away = P.e4m3_nearest(mid, tie="away")
    assert torch.equal(away.long(), torch.arange(1, 127))


@pytest.mark.parametrize("e", P.CODEPOINT_EXPONENTS)
def test_quantiser_code_point_rows(e):
    a = P.quant_codepoint_rows(e)
    codes, scale = P.quant_ref(a)
    assert bool((scale == 2.0 ** e).all()) and not bool(((codes & 0x7F) == 0x7F).any())
    body = a.float() / 2.0 ** e
    assert torch.equal(codes, body.to(F8).view(torch.uint8)), "scale 2^e: the codes are torch's cast of the unscaled values"
    have = set(body.to(BF).view(torch.int16).flatten().tolist())
    every = set(P.bf16_upto_448().view(torch.int16).tolist())
    assert have == every if e >= 0 else len(every - have) < 1200, "the values the row layout carries"
    assert set(codes.flatten().tolist()) == set(P.FINITE.tolist()), "every finite code is produced, -0 included"
    # mutant: a tie rounded away from even
    assert int((P.quant_ref(a, tie="away")[0] != codes).sum()) >= 126


@pytest.mark.parametrize("K", P.QUANT_KS)
@pytest.mark.parametrize("M", P.QUANT_MS)
def test_quantiser_rows_and_the_absmax_mutant(M, K):
    a = P.quant_rows(M, K)                  # asserts the absmax column of every row and its margin
    codes, scale = P.quant_ref(a)
    cols = [P.absmax_column(r, K) for r in range(M)]
    assert all(c >= 1024 for r, c in enumerate(cols) if r % 4 in (0, 1, 3)) and all(c >= K - 16 for r, c in enumerate(cols) if r % 4 == 1)
    assert K <= 2048 or all(c >= 2048 for r, c in enumerate(cols) if r % 4 == 3)
    assert all(int(codes[r, c]) & 0x7F == 0x7E for r, c in enumerate(cols)), "the absmax quantises to +-448"
    if M > 1:
        assert bool(((scale[1:] / scale[:-1]).log10().abs() > 4).all()), "adjacent rows differ by decades"
    # mutant: absmax over the first 1024 columns only
    c2, s2 = P.quant_ref(a, absmax_cols=1024)
    wrong = [r for r in range(M) if cols[r] >= 1024]
    assert all(float(s2[r]) != float(scale[r]) for r in wrong) and not torch.equal(c2, codes)
    # mutant: a row pair mixed up (row 2p + 1 quantised with the scale of row 2p)
    if M > 1:
        swapped = P.e4m3_nearest((a[1].float() / scale[0]).clamp(-448, 448))
        assert not torch.equal(swapped, codes[1])


# --------------------------------------------------------------------------------------------------------------- the mutants
def _out(op, acc=None, sa=None, sw=None, bias=None, gate=None, res=None, epilogue="bias"):
    acc = op.acc if acc is None else acc
    sa, sw = (op.sa if sa is None else sa).double(), (op.sw if sw is None else sw).double()
    y = acc * sa.view(-1, 1) * sw.view(1, -1) + (op.bias if bias is None else bias).double()
    if epilogue == "gate_res":
        y = (op.res if res is None else res).double() + (op.gate if gate is None else gate).double() * y
    return y.float().to(BF)


def _moved(t, n, d):
    t = t.clone()
    t[n] = t[n + d]
    return t


def _clamped(t):
    t = t.clone()
    t[-4:] = t[-8:-4]
    return t


@pytest.mark.parametrize("M,N,K", [(257, 272, 384), (129, 144, 1152), (127, 16, 128)])
def test_epilogue_index_mutants_are_rejected(M, N, K):
    op = P.fixed_point(M, N, K)
    want, wantg = P.want(M, N, K), P.want(M, N, K, "gate_res")
    assert torch.equal(_out(op), want) and torch.equal(_out(op, epilogue="gate_res"), wantg)
    for n, d in ((N - 6, 1), (N - 6, -1), (N - 6, 4), (N - 6, -4), (0, 1), (N - 1, -1)):
        msg = _rejected(_out(op, sw=_moved(op.sw, n, d)), want)                          # column n takes sw[n + d]
        assert f", {n})" in msg
        _rejected(_out(op, bias=_moved(op.bias, n, d)), want)
        _rejected(_out(op, gate=_moved(op.gate, n, d), epilogue="gate_res"), wantg)
    msg = _rejected(_out(op, sw=_clamped(op.sw)), want)                                 # the last group takes the clamped group's
    assert f", {N - 4})" in msg
    _rejected(_out(op, bias=_clamped(op.bias)), want)
    _rejected(_out(op, gate=_clamped(op.gate), epilogue="gate_res"), wantg)
    if M > 1:
        for m, d in ((M - 1, -1), (0, 1), (M // 2, 1), (M // 2, -1)):
            msg = _rejected(_out(op, sa=_moved(op.sa, m, d)), want)                      # row m takes sa[m + d]
            assert f"({m}, " in msg
        for src in (M - 2, 0):
            if src != M - 1:
                r2 = op.res.clone()
                r2[M - 1] = op.res[src]                                                   # row M - 1 takes another row's residual
                msg = _rejected(_out(op, res=r2, epilogue="gate_res"), wantg)
                assert f"({M - 1}, 0)" in msg
    # the single-sw form applied as per-row, and the reverse
    _rejected(_out(op), P.want(M, N, K, per_row=False))
    _rejected(_out(op, sw=op.sw_one.expand(N)), want)
    # the bias added before the scales
    y = (op.acc + op.bias.double()) * op.sa.double().view(-1, 1) * op.sw.double().view(1, -1)
    _rejected(y.float().to(BF), want)
    # one K-tile skipped
    lo = K - 128 if K > 128 else 0
    acc = op.acc - op.qa[:, lo:lo + 128].double() @ op.qw[:, lo:lo + 128].double().T
    _rejected(_out(op, acc=acc), want)


def test_tile_mutants_are_rejected():
    M, N, K = 1153, 272, P.ORDER_K
    op = P.fixed_point(M, N, K)
    want = P.want(M, N, K)
    # one 128 x 128 tile left unwritten, in the second band
    left = want.clone()
    left[1024:1152, 128:256] = P.SENTINEL
    msg = _rejected(left, want)
    assert msg.startswith(f"{128 * 128} of") and "[(8, 1)]" in msg and "band 1 at (0, 0)" in msg
    # the part-filled band's tile written from the operands of the tile above it (a duplicate in the tile map)
    twice = want.clone()
    twice[1152:, 128:256] = want[1024:1024 + (M - 1152), 128:256]
    msg = _rejected(twice, want)
    assert "[(9, 1)]" in msg and "band 1" in msg
    # two tiles of the second band swapped
    swap = want.clone()
    swap[1024:1152, 0:128], swap[1024:1152, 128:256] = want[1024:1152, 128:256], want[1024:1152, 0:128]
    _rejected(swap, want)
    # a store one column past the view breaks a guard
    buf = _buffer(want)
    buf[5, P.GUARD + N] = 1.0
    assert "store outside the output view" in P.buffer_mismatches(buf, want)


# ------------------------------------------------------------------------------------- what the older pair of bars accepts
def test_the_older_bars_accept_wrong_epilogue_indices():
    """See the module docstring.  The operands are test_random_operands_under_every_epilogue's own (129, 5120, 256) per-row case,
    the 'output' is its f32 reference rounded to bf16 - a perfect kernel - with ONE wrong decision planted."""
    from tests.test_gpu_gemm_fp8 import _BARS, _case
    M, N, K = 129, 5120, 256
    c = _case(M, N, K, True)
    acc = c["qa"].view(F8).float() @ c["qw"].view(F8).float().T
    sa, sw, b, gate, res = c["sa"], c["sw"].float(), c["bias"].float(), c["gate"], c["res"].float()

    def y(sa=sa, sw=sw, b=b):
        return acc * sa.view(-1, 1) * sw.view(1, -1) + b

    ref, refg = c["ref"]["bias"], c["ref"]["gate_res"]
    assert torch.equal(y(), ref)
    ideal, idealg = ref.to(BF), refg.to(BF)
    assert P.old_bars_accept(ideal, ref, _BARS["bias"]) and P.old_bars_accept(idealg, refg, _BARS["gate_res"])

    def accepted(out, r=ref, epi="bias"):
        assert not torch.equal(out, ideal if r is ref else idealg), "the mutant changes the output"
        return P.old_bars_accept(out, r, _BARS[epi])

    # a whole column on a neighbour's weight scale
    n0 = 2000
    for d in (1, -1, 4):
        assert sw[n0 + d] != sw[n0]
        assert accepted(y(sw=_moved(sw, n0, d)).to(BF)), "the gap: one column on its neighbour's weight scale"
    # one lane's share of a wrong column index: rows m0 and m0 + 32 x the 4-column group at n0, for every m0 of the lane's wave
    taken = {}
    for name, wrong in (("sw", y(sw=sw.roll(4))), ("bias", y(b=b.roll(4))), ("gate", res + gate.roll(4) * y())):
        base, r, epi = (idealg, refg, "gate_res") if name == "gate" else (ideal, ref, "bias")
        taken[name] = 0
        for m0 in range(32):
            out = base.clone()
            out[[m0, m0 + 32], n0:n0 + 4] = wrong.to(BF)[[m0, m0 + 32], n0:n0 + 4]
            taken[name] += accepted(out, r, epi)
    # one lane's sa: row m, the 32 columns its two weight tiles hold inside one 128-column tile, taken from row m - 1
    lane_cols = [n0 - n0 % 128 + 32 * i + 8 * g + e for i in range(2) for g in range(4) for e in range(4)]
    wrong, taken["sa"] = y(sa=sa.roll(1)).to(BF), 0
    for m in range(1, M):
        out = ideal.clone()
        out[m, lane_cols] = wrong[m, lane_cols]
        taken["sa"] += accepted(out)
    # one residual load: 4 values of row m from the row above
    wrong, taken["res"] = (res.roll(1, 0) + gate * y()).to(BF), 0
    for m in range(1, M):
        out = idealg.clone()
        out[m, N - 4:] = wrong[m, N - 4:]
        taken["res"] += accepted(out, refg, "gate_res")
    print(f"accepted by the older bars: {taken} of sw 32, bias 32, gate 32, sa {M - 1}, res {M - 1} placements")
    # measured here: sw 32, bias 32, gate 23, sa 62, res 108 (the rows with the largest activation scales carry the norm)
    assert taken["sw"] == 32 and taken["bias"] == 32 and taken["gate"] > 16 and taken["sa"] > 40 and taken["res"] > 96, taken
    # the same wrong index over a whole column / row / the last group is caught by the rel-L2 bar at this size
    assert not accepted(y(b=_moved(b, n0, 1)).to(BF)) and not accepted(y(sw=_clamped(sw)).to(BF))
    assert not accepted(y(sa=_moved(sa, M - 1, -1)).to(BF))
    # ... and the exact comparison rejects every one of them on a fixed-point case (test_epilogue_index_mutants_are_rejected)
