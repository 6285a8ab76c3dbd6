"""The MX block-scaled forms of the FP8 GEMM on the GPU: `ops.quant_blocks_mxfp8`, `ops.gemm_fp8(block_scales=)`,
`ops.gemm_fp8(out_mx=)` and their grouped forms.  Every comparison is torch.equal: against the CPU restatement of the quantiser
(tests/mxfp8_ref.py), against float64 references whose every partial sum is exact in float32, or against the composition of
the public ops the fused launch replaces.  Outputs are views of wider sentinel-filled buffers that must come back untouched
outside the view.

The scale-map probe runs first in the file: which codes the MFMA's scale operand scales is exercised by nothing else in the
tree.  On the MI355X the instruction's scale block 0 is registers 0..3 of BOTH lane halves (scaled by lanes 0..31's byte) and
block 1 is registers 4..7 of both (lanes 32..63's byte), not one block per lane half; the kernel's block-scaled fragment order
(lds_frag_blocks, csrc/gemm_fp8.hip) puts memory block b into scale block b.  DESIGN.md §3.6 records the map."""
import functools

import pytest
import torch

from tests import gemm_fp8_probes as P
from tests import mxfp8_ref as R
from tests.gemm_fp8_probes import BF, F8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8
SCALE_SENTINEL = 0xFF            # a scale byte the quantiser never writes


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _weight(codes, sw):
    return _ops().Fp8Weight(codes.view(F8).to(DEV), sw.to(DEV))


def _padded(t, extra, fill):
    """t [M, K] on the device as a view of a wider buffer (row stride K + extra) filled with `fill`"""
    M, K = t.shape
    buf = torch.full((M, K + extra), fill, dtype=t.dtype, device=DEV)
    buf[:, :K] = t.to(DEV)
    return buf[:, :K]


def _mx_buffers(M, N, rows_below=2):
    """sentinel-filled (codes buffer, codes view [M, N], scales buffer, scales view [M, N / 32]): wider rows, rows below M"""
    qb = torch.full((M + rows_below, N + 64), P.SENTINEL_CODE, dtype=U8, device=DEV)
    sb = torch.full((M + rows_below, N // 32 + 12), SCALE_SENTINEL, dtype=U8, device=DEV)
    return qb, qb[:M, :N], sb, sb[:M, :N // 32]


def _mx_check(qb, sb, want_q, want_s, what):
    """the whole buffers, sentinels included, against what a correct run leaves"""
    torch.cuda.synchronize()
    M, N = want_q.shape
    fq, fs = torch.full_like(qb, P.SENTINEL_CODE).cpu(), torch.full_like(sb, SCALE_SENTINEL).cpu()
    fq[:M, :N], fs[:M, :N // 32] = want_q.cpu(), want_s.cpu()
    gq, gs = qb.cpu(), sb.cpu()
    if not torch.equal(gs, fs):
        bad = (gs != fs).nonzero()[:6].tolist()
        raise AssertionError(f"{what}: scale bytes differ at (row, block) {bad}: got {[int(gs[r, c]) for r, c in bad]}, "
                             f"expected {[int(fs[r, c]) for r, c in bad]}")
    if not torch.equal(gq, fq):
        bad = (gq != fq).nonzero()[:6].tolist()
        raise AssertionError(f"{what}: codes differ at (row, column) {bad}: got {[int(gq[r, c]) for r, c in bad]}, "
                             f"expected {[int(fq[r, c]) for r, c in bad]}")


# ---- 2. the scale-map probe (first: everything below relies on the map) ---------------------------------------------------------------
@pytest.mark.parametrize("case", [(128, 128, 128), (130, 144, 384)], ids=P.case_id)
def test_scale_map_probe_every_lane_byte_and_k_tile(case):
    """codes all 1.0, block_scales[m, b] = 127 + (7 m + 3 b) mod 5, weight row n one-hot (1.0) at k = 32 (n mod K/32) +
    (n div K/32) mod 32: out[m, n] = 2^((7 m + 3 b) mod 5) with b = n mod K/32, exactly.  A wrong lane, byte or K-tile is a
    different power of two at a named (m, n)."""
    ops = _ops()
    M, N, K = case
    nb = K // 32
    m, b, n = torch.arange(M).view(-1, 1), torch.arange(nb).view(1, -1), torch.arange(N)
    bs = (127 + (7 * m + 3 * b) % 5).to(U8)
    qa = torch.full((M, K), 1.0)
    qw = torch.zeros(N, K)
    qw[n, 32 * (n % nb) + (n // nb) % 32] = 1.0
    want = torch.exp2(((7 * m + 3 * (n % nb).view(1, -1)) % 5).float()).to(BF)
    buf, view = P.sentinel_buffer(M, N, DEV)
    out = ops.gemm_fp8(_padded(P.codes_of(qa), 128, P.SENTINEL_CODE), None, _weight(P.codes_of(qw), torch.ones(N)), out=view,
                       block_scales=_padded(bs, 4, SCALE_SENTINEL))
    assert out.data_ptr() == view.data_ptr()
    torch.cuda.synchronize()
    msg = P.buffer_mismatches(buf.cpu(), want)
    if msg:
        got = buf.cpu()[1:M + 1, P.GUARD:P.GUARD + N].float()
        bad = (got != want.float()).nonzero()[:8].tolist()
        detail = "; ".join(f"(m {r}, n {c}): block {c % nb} k {32 * (c % nb) + (c // nb) % 32} scale got 2^{float(torch.log2(got[r, c])):.0f} "
                           f"expected 2^{float(torch.log2(want[r, c].float())):.0f}" for r, c in bad)
        raise AssertionError(f"scale map {M}x{N}x{K}: {msg} :: {detail}")


# ---- 1. the quantiser -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quant_case(which):
    if which == "M1-K128":
        return R.planted_rows(128)
    a = torch.cat([R.planted_rows(384), R.every_code_rows(384), R.decade_rows(120, 384)])
    assert a.shape == (130, 384)
    return a


@pytest.mark.parametrize("which", ["M1-K128", "M130-K384"])
def test_quantiser_matches_the_reference_bit_for_bit(which):
    """planted blocks (zero, 448 x 2^k, 450 x 2^k, a bf16 subnormal, the bf16 maximum), every e4m3 code point at three scales and
    blocks over 60 decades; M 1 / K 128 quantises each planted row in a launch of its own; M 130 / K 384 reads a padded row
    stride.  Bytes beyond the rows stay at their sentinels."""
    ops = _ops()
    a = _quant_case(which)
    launches = [a[r:r + 1] for r in range(a.shape[0])] if which == "M1-K128" else [a]
    for i, rows in enumerate(launches):
        M, K = rows.shape
        want_q, want_s = R.quant_blocks_ref(rows)
        qb, qv, sb, sv = _mx_buffers(M, K)
        src = _padded(rows, 8, 7.0) if M > 1 else rows.to(DEV)
        got = ops.quant_blocks_mxfp8(src, out=qv, scale_out=sv)
        assert got[0].data_ptr() == qv.data_ptr() and got[1].data_ptr() == sv.data_ptr()
        _mx_check(qb, sb, want_q, want_s, f"quant_blocks_mxfp8 {which} launch {i}")
    q, s = ops.quant_blocks_mxfp8(a.to(DEV))                 # the allocating form
    want_q, want_s = R.quant_blocks_ref(a)
    assert torch.equal(q.cpu(), want_q) and torch.equal(s.cpu(), want_s) and s.shape == (a.shape[0], a.shape[1] // 32)


# ---- 3. unit block scales: the same K-loop and epilogue ---------------------------------------------------------------------------
@pytest.mark.parametrize("epilogue", ["bias", "gelu", "gate_res"])
def test_unit_block_scales_equal_unit_row_scales(epilogue):
    ops = _ops()
    M, N, K = 130, 144, 384
    op = P.fixed_point(M, N, K)
    qa, w = _padded(P.codes_of(op.qa), 128, P.SENTINEL_CODE), _weight(P.codes_of(op.qw), op.sw)
    bias, gate, res = op.bias.to(BF).to(DEV), op.gate.to(DEV), op.res.to(BF).to(DEV)
    kw = dict(gate=gate, residual=res) if epilogue == "gate_res" else {}
    ref = ops.gemm_fp8(qa, torch.ones(M, device=DEV), w, bias, epilogue=epilogue, **kw)
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(qa, None, w, bias, out=view, epilogue=epilogue, block_scales=torch.full((M, K // 32), 127, dtype=U8, device=DEV), **kw)
    torch.cuda.synchronize()
    msg = P.buffer_mismatches(buf.cpu(), ref.cpu())
    assert not msg, f"unit block scales, {epilogue}: {msg}"


# ---- 4. fixed-point exactness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,pad", [(384, 4), (1152, 12), (1152, 4)], ids=["K384", "K1152-rows16", "K1152-rows8"])
def test_power_of_two_block_scales_are_exact(K, pad):
    """integer codes (tests.gemm_fp8_probes.int_range) and block scales 2^-2 .. 2^1 that change with the row and with the block:
    every product and every partial sum is a multiple of 2^-2, times sw (odd part <= 5, lowest bit >= 2^-2) plus a bias on the
    2^-4 grid; the span condition below is evaluated on the operands, so float32 holds every intermediate exactly in any order
    and the output is the float64 reference rounded once to bf16.  K 1152 = 9 K-tiles: the kernel fetches the scale dwords four
    K-tiles at a time, so two whole groups and a part-filled one, with 16-byte scale rows (one wide load per group) and with
    8-byte-aligned rows (dword by dword)."""
    ops = _ops()
    M, N = 130, 144
    op = P.fixed_point(M, N, K)
    m, b = torch.arange(M).view(-1, 1), torch.arange(K // 32).view(1, -1)
    bs = (125 + (3 * m + 5 * b + (m * b) % 3) % 4).to(U8)
    assert set(bs.unique().tolist()) == {125, 126, 127, 128} and bool((bs[1:] != bs[:-1]).any(1).all()) and bool((bs[:, 1:] != bs[:, :-1]).any())
    qa = P.codes_of(op.qa)
    ref = R.gemm_ref(qa, bs, P.codes_of(op.qw), op.sw, op.bias)
    mag = (R.dequant(qa, bs).abs() @ op.qw.double().abs().T) * op.sw.double().abs().view(1, -1) + op.bias.double().abs()
    grid = (0.25 * op.sw_lsb.double()).clamp_max(P.GB).view(1, -1)
    assert float((mag / grid).max().log2()) < P.SPAN_BITS, "the span condition: every float32 intermediate is exact"
    want = P.expected(ref)
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(_padded(qa, 128, P.SENTINEL_CODE), None, _weight(P.codes_of(op.qw), op.sw), op.bias.to(BF).to(DEV), out=view,
                 block_scales=_padded(bs, pad, SCALE_SENTINEL))
    torch.cuda.synchronize()
    msg = P.buffer_mismatches(buf.cpu(), want)
    assert not msg, f"block-scaled fixed point {M}x{N}x{K}: {msg}"


# ---- 5. MX output ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_problem(M, N, K, seed):
    """bf16 activations whose 32-column blocks differ by decades (so block scales differ inside a row), e4m3 weights, bias"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-6, 7, (M, K // 32), generator=g).float()).repeat_interleave(32, dim=1)
    qw = (torch.randn(N, K, generator=g) * 0.5).to(F8).view(U8)
    sw = (torch.rand(N, generator=g) * 0.02 + 0.005).to(BF).float()
    bias = torch.randn(N, generator=g).to(BF)
    return a.to(BF), qw, sw, bias


@pytest.mark.parametrize("epilogue", ["bias", "gelu"])
@pytest.mark.parametrize("case", [(130, 256, 128), (64, 128, 256)], ids=P.case_id)
def test_mx_output_equals_bf16_output_then_quantiser(case, epilogue):
    """M 130 / N 256: both wave columns, both i, two tile rows with an M edge.  Rows >= M of both outputs stay untouched."""
    ops = _ops()
    M, N, K = case
    a, qw, sw, bias = _random_problem(M, N, K, 11)
    qa, sa = ops.quant_rows_fp8(a.to(DEV))
    w, bias = _weight(qw, sw), bias.to(DEV)
    y = ops.gemm_fp8(qa, sa, w, bias, epilogue=epilogue)
    want_q, want_s = ops.quant_blocks_mxfp8(y)
    assert int(want_s.max()) - int(want_s.min()) >= 2, "the blocks of the output carry different scales"
    rq, rs = R.quant_blocks_ref(y.cpu())
    assert torch.equal(want_q.cpu(), rq) and torch.equal(want_s.cpu(), rs), "the quantiser itself, on this output"
    qb, qv, sb, sv = _mx_buffers(M, N)
    got = ops.gemm_fp8(qa, sa, w, bias, epilogue=epilogue, out_mx=(qv, sv))
    assert got[0].data_ptr() == qv.data_ptr() and got[1].data_ptr() == sv.data_ptr()
    _mx_check(qb, sb, want_q, want_s, f"out_mx {M}x{N}x{K} {epilogue}")


# ---- 6. the chain ---------------------------------------------------------------------------------------------------------------
def test_up_mx_then_down_block_scaled_equals_the_three_launch_composition():
    ops = _ops()
    M, D, F = 130, 256, 384
    a, qw1, sw1, b1 = _random_problem(M, F, D, 21)
    _, qw2, sw2, b2 = _random_problem(M, D, F, 22)
    g = torch.Generator().manual_seed(23)
    gate, x0 = torch.randn(D, generator=g).to(DEV), torch.randn(M, D, generator=g).to(BF).to(DEV)
    w1, w2, b1, b2 = _weight(qw1, sw1), _weight(qw2, sw2), b1.to(DEV), b2.to(DEV)
    qa, sa = ops.quant_rows_fp8(a.to(DEV))
    # the composition of the public ops
    h = ops.gemm_fp8(qa, sa, w1, b1, epilogue="gelu")
    hq, hs = ops.quant_blocks_mxfp8(h)
    want = x0.clone()
    ops.gemm_fp8(hq, None, w2, b2, out=want, epilogue="gate_res", gate=gate, residual=want, block_scales=hs)
    # the two fused launches, the down projection in place in a sentinel buffer
    mq, ms = ops.gemm_fp8(qa, sa, w1, b1, epilogue="gelu", out_mx=(torch.empty(M, F, dtype=U8, device=DEV),
                                                                   torch.empty(M, F // 32, dtype=U8, device=DEV)))
    buf, view = P.sentinel_buffer(M, D, DEV)
    view.copy_(x0)
    ops.gemm_fp8(mq, None, w2, b2, out=view, epilogue="gate_res", gate=gate, residual=view, block_scales=ms)
    torch.cuda.synchronize()
    assert torch.isfinite(want.float()).all() and not torch.equal(want, x0)
    msg = P.buffer_mismatches(buf.cpu(), want.cpu())
    assert not msg, f"chain {M}: {D} -> {F} -> {D}: {msg}"
    # and it is close to the per-row path it replaces: the same product, another quantisation of h
    hq2, hs2 = ops.quant_rows_fp8(h)
    row = ops.gemm_fp8(hq2, hs2, w2, b2, epilogue="gate_res", gate=gate, residual=x0)
    rel = float((want.float() - row.float()).norm() / row.float().norm())
    print(f"[mx chain] rel-L2 of the MX chain against the per-row chain {rel:.3e}")
    assert rel < 0.1


# ---- 7. grouped -----------------------------------------------------------------------------------------------------------------
def test_grouped_mixes_mx_and_bf16_problems_bit_identically():
    """problem 0: per-row scales in, gelu, MX out (M 130, N 256); problem 1: block scales in, gate_res in place, bf16 out (M 72,
    N 144).  K 256 shared.  Each result is what the single launch leaves."""
    ops = _ops()
    K = 256
    a0, qw0, sw0, b0 = _random_problem(130, 256, K, 31)
    a1, qw1, sw1, b1 = _random_problem(72, 144, K, 32)
    g = torch.Generator().manual_seed(33)
    gate, x1 = torch.randn(144, generator=g).to(DEV), torch.randn(72, 144, generator=g).to(BF).to(DEV)
    w0, w1, b0, b1 = _weight(qw0, sw0), _weight(qw1, sw1), b0.to(DEV), b1.to(DEV)
    qa0, sa0 = ops.quant_rows_fp8(a0.to(DEV))
    qa1, bs1 = ops.quant_blocks_mxfp8(a1.to(DEV))
    sq, ss = ops.gemm_fp8(qa0, sa0, w0, b0, epilogue="gelu", out_mx=(torch.empty(130, 256, dtype=U8, device=DEV),
                                                                     torch.empty(130, 8, dtype=U8, device=DEV)))
    single1 = x1.clone()
    ops.gemm_fp8(qa1, None, w1, b1, out=single1, epilogue="gate_res", gate=gate, residual=single1, block_scales=bs1)
    qb, qv, sb, sv = _mx_buffers(130, 256)
    buf, view = P.sentinel_buffer(72, 144, DEV)
    view.copy_(x1)
    ops.gemm_fp8_grouped([qa0, qa1], [sa0, None], [w0, w1], [b0, b1], [None, view], ["gelu", "gate_res"], gate_list=[None, gate],
                         residual_list=[None, view], block_scales_list=[None, bs1], out_mx_list=[(qv, sv), None])
    _mx_check(qb, sb, sq, ss, "grouped problem 0 (MX out)")
    msg = P.buffer_mismatches(buf.cpu(), single1.cpu())
    assert not msg, f"grouped problem 1 (block scales in, bf16 out): {msg}"
    # a launch with no MX problem is the launch of today
    o0, o1 = torch.empty(130, 256, dtype=BF, device=DEV), torch.empty(72, 144, dtype=BF, device=DEV)
    qa1r, sa1r = ops.quant_rows_fp8(a1.to(DEV))
    ops.gemm_fp8_grouped([qa0, qa1r], [sa0, sa1r], [w0, w1], [b0, b1], [o0, o1], ["gelu", "bias"], block_scales_list=[None, None])
    assert torch.equal(o0, ops.gemm_fp8(qa0, sa0, w0, b0, epilogue="gelu")) and torch.equal(o1, ops.gemm_fp8(qa1r, sa1r, w1, b1))


def test_entry_points_refuse_by_message():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    a = torch.zeros(8, 128, dtype=BF, device=DEV)
    with pytest.raises(ApexMIError, match="fp8_mx_route"):
        ops.gemm(a, torch.zeros(128, 128, dtype=BF, device=DEV),
                 out_mx=(torch.zeros(8, 128, dtype=U8, device=DEV), torch.zeros(8, 4, dtype=U8, device=DEV)))
    from apex_studio_amd import lib as L
    lib = L.load()
    q, s = torch.zeros(8, 128, dtype=U8, device=DEV), torch.zeros(8, 4, dtype=U8, device=DEV)
    w, sw, sa = torch.zeros(128, 128, dtype=U8, device=DEV), torch.ones(1, dtype=BF, device=DEV), torch.ones(8, device=DEV)
    c = torch.zeros(8, 128, dtype=BF, device=DEV)

    def args(sa_, abs_, mq, ms, n=128):
        return (q.data_ptr(), 128, sa_, abs_, 4, w.data_ptr(), 128, 0, sw.data_ptr(), 1, None, c.data_ptr(), 128, mq, 128, ms, 4, 8, n,
                128, 0, None, None, 0, None)
    for bad, text in ((args(sa.data_ptr(), s.data_ptr(), None, None), "both given"),
                      (args(None, None, None, None), "null operand"),
                      (args(sa.data_ptr(), None, q.data_ptr(), None), "codes and block scales"),
                      (args(sa.data_ptr(), None, q.data_ptr(), s.data_ptr(), n=64), "multiple of 128")):
        assert lib.apexmi_gemm_fp8_mx(*bad) != 0
        msg = lib.apexmi_last_error().decode("utf-8", "replace")
        assert text in msg, (text, msg)
