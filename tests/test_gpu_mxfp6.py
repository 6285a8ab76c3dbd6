"""The MXFP6 quantiser and GEMM (csrc/gemm_mxfp6.hip; ops.quant_blocks_mxfp6, ops.gemm_mxfp6, the fp6 route of ops.gemm) against the
CPU restatement of the format (tests/mxfp6_ref.py): bit-exact codes and scale bytes, the operand lane map and scale wiring of the
block-scaled MFMA with 6-bit operands on one-hot data, exact fixed-point products under every epilogue and edge, like-for-like random
operands against the bf16 kernel, and the refusals.  The exactness preconditions are proven in tests/test_mxfp6_host.py."""
import pytest
import torch

from tests import gemm_fp8_probes as P
from tests import mxfp6_ref as R
from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _quantise_wide(a):
    """ops.quant_blocks_mxfp6 on a copy of `a` with lda > K into sentinel-filled buffers with ldq > 3 K / 4 and lds > K / 32; returns
    the host copies of (codes, scales, whole code buffer, whole scale buffer)"""
    ops = _ops()
    M, K = a.shape
    kb = K * 3 // 4
    abuf = torch.full((M, K + 24), 7.0, dtype=BF, device=DEV)
    abuf[:, :K] = a.to(DEV)
    qbuf = torch.full((M, kb + 40), 0x5A, dtype=torch.uint8, device=DEV)          # rows 8-byte aligned, not 16
    sbuf = torch.full((M, K // 32 + 5), 0x5A, dtype=torch.uint8, device=DEV)
    q, s = ops.quant_blocks_mxfp6(abuf[:, :K], out=qbuf[:, :kb], scale_out=sbuf[:, :K // 32])
    torch.cuda.synchronize()
    assert q.data_ptr() == qbuf.data_ptr() and s.data_ptr() == sbuf.data_ptr()
    return q.cpu(), s.cpu(), qbuf.cpu(), sbuf.cpu()


def _check_quantiser(a):
    M, K = a.shape
    q, s, qbuf, sbuf = _quantise_wide(a)
    wq, ws = R.quant_blocks_ref(a)
    assert torch.equal(s, ws), f"scale bytes: {int((s != ws).sum())} of {ws.numel()} differ"
    if not torch.equal(q, wq):
        bad = (R.unpack(q) != R.unpack(wq)).nonzero()[:4]
        what = [(int(r), int(k), float(a[r, k].float()), int(R.unpack(q)[r, k]), int(R.unpack(wq)[r, k])) for r, k in bad]
        assert False, f"codes: {int((R.unpack(q) != R.unpack(wq)).sum())} of {M * K} differ; first (row, k, value, got, want): {what}"
    assert bool((qbuf[:, K * 3 // 4:] == 0x5A).all()) and bool((sbuf[:, K // 32:] == 0x5A).all()), "a store behind the row"


# ------------------------------------------------------------------------------------------------------------------- 1. quantiser
@pytest.mark.parametrize("rows", ["planted", "tie", "every_code", "decade"])
def test_quantiser_on_the_planted_rows(rows):
    a = {"planted": R.planted_rows, "tie": lambda: R.tie_row()[0], "every_code": R.every_code_rows, "decade": R.decade_rows}[rows]()
    _check_quantiser(a)
    if rows == "every_code":
        q, s = _quantise_wide(a)[:2]
        wq, ws = R.every_code_want()
        assert torch.equal(q, wq) and torch.equal(s, ws)
    if rows == "planted":
        s = _quantise_wide(a)[1]
        for r, b, want in R.planted_bytes():
            assert int(s[r, b]) == want, R.PLANTS[r][0]


@pytest.mark.parametrize("K", [32, 256, 768])
@pytest.mark.parametrize("M", [1, 7, 130])
def test_quantiser_on_random_rows(M, K):
    a = R.random_rows(M, K).clone()
    if K == 256 and M >= 7:
        a[:len(R.PLANTS)] = R.planted_rows()
    _check_quantiser(a)


@pytest.mark.parametrize("e", [None, 0, 6, -4], ids=["own-scales", "e0", "e6", "e-4"])
def test_quantiser_on_every_bf16_bit_pattern(e):
    """all 65 280 finite bf16 patterns: in blocks of neighbours (every scale byte), and against one known scale 2^e (every rounding
    decision of the code grid, down to the subnormals)"""
    _check_quantiser(R.every_bf16_rows(e))


def test_weight_record_round_trip():
    ops = _ops()
    w = R.decade_rows(16, 256)
    rec = ops.Mxfp6Weight.from_bf16(w.to(DEV))
    wq, ws = R.quant_blocks_ref(w)
    assert rec.shape == (16, 256) and rec.nbytes() == 16 * 192 + 16 * 8 and rec.q.stride(0) % 16 == 0
    assert torch.equal(rec.q.cpu(), wq) and torch.equal(rec.s.cpu(), ws)
    d = rec.dequant()
    assert d.dtype == BF and torch.equal(d.cpu().double(), R.dequant(wq, ws)), "fp6 x 2^e is exact in bf16"
    out = torch.empty(16, 256, dtype=BF, device=DEV)
    assert rec.dequant(out=out) is out and torch.equal(out, d)


# -------------------------------------------------------------------------------------------------------------------- 2. lane map
def _gemm(op_qa, op_sa, op_qw, op_sw, M, N, **kw):
    """ops.gemm_mxfp6 on device copies with strides wider than the rows, into a sentinel-filled buffer; returns the host buffer"""
    ops = _ops()
    qa, sa = R.wide(op_qa.to(DEV), 32), R.wide(op_sa.to(DEV), 8)
    w = ops.Mxfp6Weight(R.wide(op_qw.to(DEV), 16), R.wide(op_sw.to(DEV), 4))
    buf, out = R.sentinel_buffer(M, N, DEV)
    if kw.pop("in_place", False):
        out.copy_(kw["residual"])
        kw["residual"] = out
    got = ops.gemm_mxfp6(qa, sa, w, out=out, **kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    return buf.cpu()


def _buffer_mismatches(host_buf, want):
    M, N = want.shape
    full = torch.full_like(host_buf, R.SENTINEL)
    full[1:M + 1, R.GUARD:R.GUARD + N] = want
    if torch.equal(host_buf, full):
        return ""
    return P.mismatches(host_buf[1:M + 1, R.GUARD:R.GUARD + N], want) or "store outside the output view"


def test_lane_map_with_one_hot_blocks_and_distinct_scales():
    L = R.lane_map()
    M, N, K = R.LANE
    want = L.want()
    for name, wrong in L.mutants().items():
        assert not torch.equal(wrong.float().to(BF), want), f"the probe cannot see a wrong {name}"
    buf = _gemm(R.pack(L.ca), L.sa, R.pack(L.cw), L.sw, M, N)
    got = buf[1:M + 1, R.GUARD:R.GUARD + N]
    if not torch.equal(got, want):
        same_as = [name for name, wrong in L.mutants().items() if torch.equal(wrong.float().to(BF), got)]
        nz_got, nz_want = (got != 0), (want != 0)
        print(f"[mxfp6 lane map] {int((got != want).sum())} wrong; equals the mutant {same_as}; non-zero pattern equal "
              f"{torch.equal(nz_got, nz_want)}; ratios got / want on the diagonal rows 0, 1, 33: "
              f"{[float(got[m, m].float() / want[m, m].float()) for m in (0, 1, 33)]}")
    assert _buffer_mismatches(buf, want) == ""


# --------------------------------------------------------------------------------------------------------- 3. exact fixed point
@pytest.mark.parametrize("case", R.fixed_cases(), ids=lambda c: "-".join(map(str, c)))
def test_fixed_point_products_are_exact_under_every_epilogue(case):
    M, N, K = case
    op = R.fixed_point(M, N, K)
    bias, gate, res = op.bias.to(BF).to(DEV), op.gate.to(DEV), op.res.to(BF).to(DEV)
    for with_bias in (True, False):
        buf = _gemm(op.qa, op.sa, op.qw, op.sw, M, N, bias=bias if with_bias else None)
        assert _buffer_mismatches(buf, op.want("bias", with_bias)) == "", f"bias epilogue, bias {with_bias}"
    for in_place in (False, True):
        buf = _gemm(op.qa, op.sa, op.qw, op.sw, M, N, bias=bias, epilogue="gate_res", gate=gate, residual=res.clone(), in_place=in_place)
        assert _buffer_mismatches(buf, op.want("gate_res")) == "", f"gate_res, residual aliasing out: {in_place}"
    # gelu: the activation is not exact arithmetic; its bars are those of the fp8 probes (1 bf16 ulp of the float64 definition rounded once)
    buf = _gemm(op.qa, op.sa, op.qw, op.sw, M, N, bias=bias, epilogue="gelu")
    got = buf[1:M + 1, R.GUARD:R.GUARD + N]
    worst, equal = P.gelu_judge(got, op.ref("bias"))
    assert worst <= P.GELU_MAX_ULP and equal >= P.GELU_MIN_EQUAL, (worst, equal)
    full = torch.full_like(buf, R.SENTINEL)
    full[1:M + 1, R.GUARD:R.GUARD + N] = got
    assert torch.equal(buf, full), "store outside the output view"


# -------------------------------------------------------------------------------------------------------------------- 4. route
def test_route_through_ops_gemm_is_the_two_launches():
    ops = _ops()
    M, N, K = 129, 144, 384                       # three K-tiles; not a K of the fp4 route
    a, w = R.random_rows(M, K).to(DEV), R.random_rows(N, K, seed=12).to(DEV)
    plain, plain32 = ops.gemm(a, w), ops.gemm(a, w, out=torch.empty(M, N, device=DEV))
    w._fp6 = ops.Mxfp6Weight.from_bf16(w)
    assert ops.mxfp6_route(a, w)
    routed = ops.gemm(a, w)
    qa, sa = ops.quant_blocks_mxfp6(a)
    direct = ops.gemm_mxfp6(qa, sa, w._fp6)
    assert torch.equal(routed, direct) and not torch.equal(routed, plain)
    assert torch.equal(ops.gemm(a, w, out=torch.empty(M, N, device=DEV)), plain32), "a float `out` keeps the bf16 path"
    from apex_studio_amd.lib import ApexMIError
    q8 = ops.quant_rows_fp8(a)
    with pytest.raises(ApexMIError, match="belong to the fp8 route.*MXFP6 route"):
        ops.gemm(a, w, quantised=q8)
    with pytest.raises(ApexMIError, match="belong to the fp8 route.*MXFP6 route"):
        ops.gemm(a, w, out_mx=(torch.empty(M, N, dtype=torch.uint8, device=DEV), torch.empty(M, N // 32, dtype=torch.uint8, device=DEV)))
    del w._fp6
    assert torch.equal(ops.gemm(a, w), plain), "without the record the call is the earlier one"


@pytest.mark.parametrize("mode", ["fp4", "fp6"])
def test_the_shared_front_end_routes_either_format_as_its_explicit_pair(mode):
    """`ops.gemm` on a weight carrying the format's record against `quant_blocks_mxfpN` + `gemm_mxfpN` with fresh buffers, bit for
    bit, under bias / gelu / gate_res at M = 130 (a tile and two edge rows), N = 144 (a tile and one 16-column group), K = 512 (two
    fp4 K-tiles, four fp6 K-tiles); again after an M = 64 call on the same stream has taken smaller views of the per-stream
    activation scratch; and with a call of the OTHER format in between, whose scratch is a store of its own."""
    ops = _ops()
    M, N, K = 130, 144, 512
    kinds = {"fp4": (ops.Mxfp4Weight, "_fp4", ops.quant_blocks_mxfp4, ops.gemm_mxfp4, ops.mxfp4_route),
             "fp6": (ops.Mxfp6Weight, "_fp6", ops.quant_blocks_mxfp6, ops.gemm_mxfp6, ops.mxfp6_route)}
    a, wdata = R.random_rows(M, K).to(DEV), R.random_rows(N, K, seed=12)
    bias, gate = R.random_rows(1, N, seed=13).view(N).to(DEV), R.random_rows(1, N, seed=14).view(N).float().to(DEV)
    res = R.random_rows(M, N, seed=15).to(DEV)
    weights = {}
    for m, (cls, slot, _, _, route) in kinds.items():
        w = wdata.to(DEV)
        setattr(w, slot, cls.from_bf16(w))
        assert route(a, w) and route(a[:64], w)
        weights[m] = w
    epilogues = {"bias": {}, "gelu": {}, "gate_res": {"gate": gate}}

    def explicit(m, rows, epi, extra):
        _, slot, quant, gemm, _ = kinds[m]
        qa, sa = quant(a[:rows])
        kw = dict(extra, residual=res[:rows]) if epi == "gate_res" else extra
        return gemm(qa, sa, getattr(weights[m], slot), bias, epilogue=epi, **kw)

    def routed(m, rows, epi, extra):
        kw = dict(extra, residual=res[:rows]) if epi == "gate_res" else extra
        return ops.gemm(a[:rows], weights[m], bias, epilogue=epi, **kw)

    other = "fp6" if mode == "fp4" else "fp4"
    for epi, extra in epilogues.items():
        want = {(m, rows): explicit(m, rows, epi, extra) for m in kinds for rows in (M, 64)}
        assert not torch.equal(want[mode, M], want[other, M]), "the two formats round differently: the comparison can tell them apart"
        assert torch.equal(routed(mode, M, epi, extra), want[mode, M]), (epi, "the route is its explicit pair")
        assert torch.equal(routed(mode, 64, epi, extra), want[mode, 64]), (epi, "a smaller view of the same scratch")
        assert torch.equal(routed(mode, M, epi, extra), want[mode, M]), (epi, "the larger view again")
        first, second, third = routed(mode, M, epi, extra), routed(other, M, epi, extra), routed(mode, M, epi, extra)
        assert torch.equal(first, want[mode, M]) and torch.equal(second, want[other, M]) and torch.equal(third, want[mode, M]), \
            (epi, "back to back on one stream, each format still matches its own pair")
    # the stores themselves: the two formats' views of this stream's scratch do not overlap
    spans = []
    for fmt in ops._MX_FORMATS:
        for t in ops._act_scratch_mx(fmt, a.device, M, K):
            spans.append((t.data_ptr(), t.data_ptr() + t.numel()))
    spans.sort()
    assert len(spans) == 4 and all(hi <= lo for (_, hi), (lo, _) in zip(spans, spans[1:])), spans


# ------------------------------------------------------------------------------------------------------------- 5. like for like
@pytest.mark.parametrize("case", [(300, 272, 1280), (129, 528, 512)], ids=["300-272-1280", "129-528-512"])
def test_random_operands_like_for_like_with_the_bf16_kernel(case):
    ops = _ops()
    M, N, K = case
    x, w = R.random_rows(M, K, seed=21).to(DEV), R.random_rows(N, K, seed=22).to(DEV)
    xq, xs = ops.quant_blocks_mxfp6(x)
    rec = ops.Mxfp6Weight.from_bf16(w)
    # the precondition of the equality bar, on the operands as quantised: sum |a| |w| in units of the finest product grid 2^(min sa +
    # min sw - 254 - 6) is below 2^20, so float32 holds every partial sum exactly in either kernel, whatever its order
    xd64, wd64 = R.dequant(xq.cpu(), xs.cpu()), R.dequant(rec.q.cpu(), rec.s.cpu())
    grid = 2.0 ** (int(xs.min()) + int(rec.s.min()) - 254 - 6)
    span = float((xd64.abs() @ wd64.abs().T).max() / grid)
    assert span < 2 ** 20, f"the exact-sum precondition does not hold: {span:.3e} units"
    got = ops.gemm_mxfp6(xq, xs, rec).float()
    xd = ops.Mxfp6Weight(xq, xs).dequant()
    assert torch.equal(xd.cpu().double(), xd64)
    like = ops.gemm(xd, rec.dequant()).float()            # the shipped bf16 kernel on operands holding the same values exactly
    rel = float((got - like).norm() / like.norm())
    f32 = x.float() @ w.float().T
    approx = float((got - f32).norm() / f32.norm())
    x4, s4 = ops.quant_blocks_mxfp4(x)
    got4 = ops.gemm_mxfp4(x4, s4, ops.Mxfp4Weight.from_bf16(w)).float()
    approx4 = float((got4 - f32).norm() / f32.norm())
    print(f"[mxfp6 like-for-like] {M}x{N}x{K}: rel-L2 against the bf16 kernel on the dequantised operands {rel:.3e}; the approximation "
          f"itself, against the f32 product of the unquantised operands, {approx:.3e} (the fp4 path on the same operands: {approx4:.3e})")
    assert approx < 0.5 * approx4, "three mantissa bits against one: about a quarter of the fp4 error is expected"
    measured(f"gemm_mxfp6.like_for_like.{M}x{N}x{K}", rel, LIKE_BARS[case])


# Both kernels hold the EXACT sum in float32 (the precondition asserted above) and round it once, so the outputs are bit-identical and
# rel-L2 is 0.  The strict `<` of `measured` cannot express 0; the bar is a value below the smallest rel-L2 one differing bf16 element
# can produce (one ulp of the smallest non-zero output against the norm of 1e5 elements of order 36 is above 1e-9), i.e. equality —
# the form of the fp4 test.
LIKE_BARS = {(300, 272, 1280): 1e-9, (129, 528, 512): 1e-9}


# ------------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_launch_nothing():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError

    def operands(M, N, K):
        return (torch.zeros(M, K * 3 // 4, dtype=torch.uint8, device=DEV), torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV),
                ops.Mxfp6Weight(torch.zeros(N, K * 3 // 4, dtype=torch.uint8, device=DEV),
                                torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV)))

    qa, sa, w = operands(8, 32, 128)
    out = torch.full((8, 32), 3.0, dtype=BF, device=DEV)
    with pytest.raises(ApexMIError, match=r"K=64 must be a multiple of 128 \(a K-tile is 96 bytes of e2m3 codes\)"):
        ops.gemm_mxfp6(*operands(8, 32, 64))
    with pytest.raises(ApexMIError, match="N=24 must be a multiple of 16"):
        ops.gemm_mxfp6(*operands(8, 24, 128))
    with pytest.raises(ApexMIError, match="f32 output"):
        ops.gemm_mxfp6(qa, sa, w, out=torch.zeros(8, 32, device=DEV))
    with pytest.raises(ApexMIError, match="null operand"):
        ops.gemm_mxfp6(None, sa, w, out=out)
    with pytest.raises(ApexMIError, match="scales"):
        ops.gemm_mxfp6(qa, None, w, out=out)
    with pytest.raises(ApexMIError, match=r"scales must be \[8, 4\]"):
        ops.gemm_mxfp6(qa, sa[:, :3], w, out=out)
    with pytest.raises(ApexMIError, match=r"scales must be \[8, 4\]"):
        ops.gemm_mxfp6(qa, sa[:4], w, out=out)
    with pytest.raises(ApexMIError, match=r"codes must be \[8, 96\]"):
        ops.gemm_mxfp6(torch.zeros(8, 64, dtype=torch.uint8, device=DEV), sa, w, out=out)
    with pytest.raises(ApexMIError, match="Mxfp6Weight"):
        ops.gemm_mxfp6(qa, sa, torch.zeros(32, 128, dtype=BF, device=DEV), out=out)
    with pytest.raises(ApexMIError, match="Mxfp6Weight"):
        ops.gemm_mxfp6(qa, sa, ops.Mxfp4Weight(torch.zeros(32, 64, dtype=torch.uint8, device=DEV),
                                               torch.full((32, 4), 127, dtype=torch.uint8, device=DEV)), out=out)
    with pytest.raises(ApexMIError, match="gate_res epilogue needs"):
        ops.gemm_mxfp6(qa, sa, w, out=out, epilogue="gate_res")
    with pytest.raises(ApexMIError, match="epilogue 'silu' is not one of"):
        ops.gemm_mxfp6(qa, sa, w, out=out, epilogue="silu")
    with pytest.raises(ApexMIError, match="K % 32"):
        ops.quant_blocks_mxfp6(torch.zeros(4, 48, dtype=BF, device=DEV))
    with pytest.raises(ApexMIError, match="bfloat16"):
        ops.quant_blocks_mxfp6(torch.zeros(4, 64, device=DEV))
    # the C entry points themselves: null pointers, misaligned or narrow rows, an unknown epilogue
    import apex_studio_amd.lib as lib
    L = lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    args = [qa.data_ptr(), 96, sa.data_ptr(), 4, w.q.data_ptr(), 96, w.s.data_ptr(), 4, None, out.data_ptr(), 32, 8, 32, 128, 0, None, None, 0,
            stream]

    def refused(i, value, what):
        bad = list(args)
        bad[i] = value
        assert L.apexmi_gemm_mxfp6(*bad) != 0
        with pytest.raises(ApexMIError, match=what):
            lib.check(1, "gemm_mxfp6")

    for i in (0, 2, 4, 6, 9):
        refused(i, None, "null operand")
    refused(0, qa.data_ptr() + 8, "operands must be 16-byte aligned")
    refused(1, 88, r"code rows at least 3 K / 4 = 96 bytes")
    refused(5, 104, r"leading dimensions must keep rows 16-byte aligned")
    refused(3, 2, "block scales must be 4-byte aligned rows of at least K / 32 = 4 bytes")
    refused(7, 6, "block scales must be 4-byte aligned rows")
    refused(13, 192, "K=192 must be a multiple of 128")
    refused(14, 5, "epilogue 5 is not one of bias")
    refused(10, 16, "ldc 16")
    a16 = torch.ones(8, 128, dtype=BF, device=DEV)
    qargs = [a16.data_ptr(), 128, 8, 128, qa.data_ptr(), 96, sa.data_ptr(), 4, stream]
    for i, value, what in ((0, None, "null operand"), (4, None, "null operand"), (6, None, "null operand"), (3, 48, "K=48 must be a multiple of 32"),
                           (5, 88, "at least 3 K / 4 bytes wide"), (5, 100, "code rows 8-byte aligned"), (4, qa.data_ptr() + 4, "8-byte aligned"),
                           (7, 3, "block scales must be at least K / 32 = 4 wide"), (2, 0, "M=0 must be at least 1")):
        bad = list(qargs)
        bad[i] = value
        assert L.apexmi_quant_blocks_mxfp6(*bad) != 0
        with pytest.raises(ApexMIError, match=what):
            lib.check(1, "quant_blocks_mxfp6")
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((qa == 0).all()) and bool((sa == 127).all()), "nothing was launched"
