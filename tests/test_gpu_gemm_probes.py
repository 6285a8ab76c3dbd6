"""Exact fixed-point probes of every bf16 GEMM tiling, epilogue class and edge (operands and references: tests/gemm_probes.py).
Every output element must equal the exact result rounded ONCE to nearest-even, bit for bit: torch.equal, no bar, no element
excluded.  Every output is a view into a buffer pre-filled with a sentinel, one guard row above and below and 8 guard columns on
each side: a tile that is never written shows the sentinel, a store outside the view breaks a guard.  (What the comparison
rejects and the older two-number bar accepts: tests/test_gemm_probes_host.py.)

Tilings are forced through the tune keys (gemm_probes.TILINGS); `tuned` restores the shipped values.  The ring schedules
(gemm.config 9 and 10) have tests of their own at the end of the file."""
import contextlib
import functools

import pytest
import torch

from tests import gemm_probes as G
from tests.conftest import measured
from tests.gemm_probes import BF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
DEFAULTS = {"gemm.config": 0, "gemm.x288": 0, "gemm.x384": 1, "gemm.x384_dist": -1, "gemm.group_m": 0, "gemm.x384_group_m": 0}
# gelu_erf (0.5 x (1 + erff(x / sqrt 2)) in float32) against the float64 definition, in bf16 code points, on |x| <= 4.  Measured on
# the MI355X: 0 on every tiling, K and bias setting (profiles/gemm_probes_measured.jsonl); the bar is that plus 1 code point of
# margin for other seeds.
GELU_ERF_ULP_BAR = 1


@contextlib.contextmanager
def tuned(**kv):
    from apex_studio_amd import lib
    try:
        for key, v in kv.items():
            lib.tune_set("gemm." + key, v)
        yield
    finally:
        for key, v in DEFAULTS.items():
            lib.tune_set(key, v)


class Dev:
    """the operands of one case on the device"""

    def __init__(self, op, act=BF):
        self.op = op
        self.a, self.w, self.bias = op.a.to(act).to(DEV), op.w.to(BF).to(DEV), op.bias.to(BF).to(DEV)
        self.gate = op.gate.to(DEV)
        self._res = {}

    def res(self, dtype=BF):
        if dtype not in self._res:
            self._res[dtype] = self.op.res.to(dtype).to(DEV)
        return self._res[dtype]


@functools.lru_cache(maxsize=None)
def dev(family, M, N, K, salt=0, act=BF):
    return Dev(G.operands(family, M, N, K, salt), act)


class Out:
    """Views [M_i, N_i] into ONE sentinel-filled buffer: row ranges stacked in `order`, one guard row above and below, 8 guard
    columns to the left and at least 8 to the right.  check(): every view equals its reference bit for bit (or lies within `ulp`
    code points of a float64 reference), and everything else still holds the sentinel."""

    def __init__(self, shapes, dtype=BF, order=None):
        self.shapes, self.dtype = list(shapes), dtype
        order = list(order) if order is not None else list(range(len(self.shapes)))
        self.sentinel = G.SENTINEL
        width = max(n for _, n in self.shapes) + 16
        self.buf = torch.full((sum(m for m, _ in self.shapes) + 2, width), self.sentinel, dtype=dtype, device=DEV)
        self.rows, r = [0] * len(self.shapes), 1
        for i in order:
            self.rows[i] = r
            r += self.shapes[i][0]
        self.views = [self.buf[self.rows[i]:self.rows[i] + m, 8:8 + n] for i, (m, n) in enumerate(self.shapes)]
        assert all(v.data_ptr() % 16 == 0 for (_, n), v in zip(self.shapes, self.views) if n % 8 == 0)

    def check(self, wants, what, tile, ulp=None):
        torch.cuda.synchronize()
        host = self.buf.cpu()
        full = torch.full_like(host, self.sentinel)
        worst = 0
        for i, ((m, n), want) in enumerate(zip(self.shapes, wants)):
            got = host[self.rows[i]:self.rows[i] + m, 8:8 + n]
            if want.dtype == torch.float64:          # an activation epilogue: code points from the float64 definition
                assert not (got == self.sentinel).any(), f"{what}: problem {i}: elements left at the sentinel"
                d, at = G.ulp_worst(got, want)
                worst = max(worst, d)
                assert d <= ulp, f"{what}: problem {i}: {d} bf16 code points from the float64 definition at (m, n) = {at}"
                full[self.rows[i]:self.rows[i] + m, 8:8 + n] = got
            else:
                assert want.dtype == self.dtype
                msg = G.mismatches(got, want, tile=tile, prob=i if len(self.shapes) > 1 else None)
                assert not msg, f"{what}: {msg}"
                full[self.rows[i]:self.rows[i] + m, 8:8 + n] = want
        msg = G.mismatches(host, full)
        assert not msg, f"{what}: store outside the output view (buffer coordinates, guards included): {msg}"
        return worst


def _tiling(name):
    keys, BM, BN = G.ALL_TILINGS[name]
    return keys, (BM, BN)


def _gemm(d, out, epilogue="bias", bias=True, res=None, a=None, w=None):
    from apex_studio_amd import ops
    kw = {}
    if epilogue == "gate_res":
        kw = dict(gate=d.gate, residual=res if res is not None else d.res(out.dtype))
    ops.gemm(d.a if a is None else a, d.w if w is None else w, d.bias if bias else None, out=out, epilogue=epilogue, **kw)


def _run(name, family, M, N, K, epilogue="bias", bias=True, dtype=BF, inplace=False, a=None, w=None, what=""):
    """one launch into a guarded buffer, compared exactly"""
    keys, tile = _tiling(name)
    d = dev(family, M, N, K)
    out = Out([(M, N)], dtype)
    res = None
    if inplace:
        out.views[0].copy_(d.res(dtype))
        res = out.views[0]
    with tuned(**keys):
        _gemm(d, out.views[0], epilogue, bias, res, a, w)
    out.check([G.want(family, M, N, K, epilogue, bias, dtype)], f"{name} {family} {M}x{N}x{K} {epilogue} {what}", tile)


# ------------------------------------------------------------------------------------------------------------ shared bodies
def _edges(name):
    _, (BM, BN) = _tiling(name)
    for M, N, K in G.edge_cases(BM, BN):
        for family in ("selector", "fixed"):
            _run(name, family, M, N, K)
            _run(name, family, M, N, K, "gate_res")


def _tile_order(name):
    _, (BM, BN) = _tiling(name)
    M, N, K = G.order_shape(BM, BN)
    for family in ("selector", "fixed"):
        _run(name, family, M, N, K)
        _run(name, family, M, N, K, "gate_res", inplace=True)


def _epilogues(name, float_out=True):
    _, (BM, BN) = _tiling(name)
    M, N = BM + 37, BN + 8
    for K in G.EPI_KS:
        d = dev("fixed", M, N, K)
        _run(name, "fixed", M, N, K)
        _run(name, "fixed", M, N, K, bias=False)
        _run(name, "fixed", M, N, K, "gate_res", what="separate residual, ldr != ldc")
        _run(name, "fixed", M, N, K, "gate_res", inplace=True, what="in place")
        _run(name, "fixed", M, N, K, "gate_res", bias=False, inplace=True, what="in place, no bias")
        big = torch.full((M, K + 64), 3.0, dtype=BF, device=DEV)
        big[:, 32:32 + K] = d.a
        av = big[:, 32:32 + K]                           # lda > K, 64-byte offset
        assert av.stride(0) == K + 64 and (av.data_ptr() - big.data_ptr()) == 64
        _run(name, "fixed", M, N, K, a=av, what="a through a view")
        bigw = torch.full((N, K + 64), 3.0, dtype=BF, device=DEV)
        bigw[:, :K] = d.w
        _run(name, "fixed", M, N, K, "gate_res", w=bigw[:, :K], what="w through a view")
        if float_out:                                    # the f32 residual stream: bf16 operand, float C / R, no rounding at all
            _run(name, "fixed", M, N, K, dtype=F32)
            _run(name, "fixed", M, N, K, bias=False, dtype=F32)
            _run(name, "fixed", M, N, K, "gate_res", dtype=F32, what="separate residual")
            _run(name, "fixed", M, N, K, "gate_res", dtype=F32, inplace=True, what="in place")


def _activations(name):
    keys, tile = _tiling(name)
    M, N = tile[0] + 37, tile[1] + 8
    for K in G.EPI_KS:
        d = dev("act", M, N, K)
        for epi in ("gelu", "silu", "quick_gelu", "gelu_erf"):
            for bias in (True, False):
                out = Out([(M, N)])
                with tuned(**keys):
                    _gemm(d, out.views[0], epi, bias)
                ref = G.act_ref(d.op, epi, bias)
                what = f"gemm_probes.{epi}.{name}.k{K}" + ("" if bias else ".nobias")
                if epi == "gelu_erf":
                    worst = out.check([ref], what, tile, ulp=1 << 16)
                    measured(what, worst, GELU_ERF_ULP_BAR + 1)      # worst <= GELU_ERF_ULP_BAR
                else:
                    # the bar test_gemm_epilogue_activations_on_every_bf16_code_point pins: one bf16 step from the float64 definition
                    out.check([ref], what, tile, ulp=1)


def _grouped(name, count):
    from apex_studio_amd import ops
    keys, tile = _tiling(name)
    shapes = list(G.group_shapes(*tile)[:count])
    K = G.GROUP_K
    order = [(i * 3 + 1) % count for i in range(count)] if count != 3 else [2, 0, 1]
    assert sorted(order) == list(range(count))
    # bias class, the activation flag mixed: exact problems beside activation problems
    epis = ["bias", "silu", "bias", "gelu"][:count]
    ds = [dev("fixed" if e == "bias" else "act", M, N, K, i) for i, ((M, N), e) in enumerate(zip(shapes, epis))]
    out = Out(shapes, order=order)
    with tuned(**keys):
        ops.gemm_grouped([d.a for d in ds], [d.w for d in ds], [d.bias if i != 2 else None for i, d in enumerate(ds)], out.views,
                         epilogue=epis)
    wants = [G.want("fixed", M, N, K, "bias", i != 2, BF, i) if e == "bias" else G.act_ref(d.op, e)
             for i, ((M, N), e, d) in enumerate(zip(shapes, epis, ds))]
    out.check(wants, f"{name} grouped x{count} bias class", tile, ulp=1)
    # gate_res, per-problem gates: once with separate residuals, once in place
    ds = [dev("fixed", M, N, K, i) for i, (M, N) in enumerate(shapes)]
    wants = [G.want("fixed", M, N, K, "gate_res", True, BF, i) for i, (M, N) in enumerate(shapes)]
    for inplace in (False, True):
        out = Out(shapes, order=order)
        if inplace:
            for v, d in zip(out.views, ds):
                v.copy_(d.res())
        res = out.views if inplace else [d.res() for d in ds]
        with tuned(**keys):
            ops.gemm_grouped([d.a for d in ds], [d.w for d in ds], [d.bias for d in ds], out.views, epilogue="gate_res",
                             gate_list=[d.gate for d in ds], residual_list=res)
        out.check(wants, f"{name} grouped x{count} gate_res inplace={inplace}", tile)


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", list(G.TILINGS))
def test_edges(name):
    """(BM + 37, BN + 8), (BM - 1, BN - 8), (1, 8) at 1, 2, 3, 4, 5, 9 K-tiles, and 64 K-tiles on the first: selector and
    fixed-point operands, the bias and the gate / residual class"""
    _edges(name)


@pytest.mark.parametrize("name", list(G.TILINGS))
def test_tile_order(name):
    """a last tile group shorter than group_m, a tile count that is no multiple of 8"""
    _tile_order(name)
    keys, tile = _tiling(name)
    M, N, K = G.order_shape(*tile)
    d = dev("selector", M, N, K)
    gm = {"x384_group_m": 2} if "x384" in name else {"group_m": 4}      # another group height: the last group is short again
    out = Out([(M, N)])
    with tuned(**keys, **gm):
        _gemm(d, out.views[0])
    out.check([G.want("selector", M, N, K)], f"{name} tile order {gm}", tile)


@pytest.mark.parametrize("name", list(G.TILINGS))
def test_epilogues(name):
    """bias, no bias, gate_res with a separate residual (ldr != ldc) and in place, strided a and w; bf16 outputs equal the RNE
    expected value, float outputs (the f32 residual stream) the exact value.  288 x 192 has no float epilogue."""
    _epilogues(name, float_out=name != "x288")


@pytest.mark.parametrize("name", list(G.TILINGS))
def test_activations(name):
    """gelu, silu, quick_gelu on the exact pre-activation (|y| <= 4): one bf16 code point from the float64 definition; gelu_erf:
    the measured distance plus one"""
    _activations(name)


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("name", ["cfg1", "cfg7", "x384d1"])
def test_verification_mode(name, K):
    """float a = three bf16 parts (hi and mid non-zero), float C / R: exact"""
    from apex_studio_amd import ops
    assert not ops.shipped_verification()
    keys, tile = _tiling(name)
    M, N = tile[0] + 37, tile[1] + 8
    d = dev("verify", M, N, K, 0, F32)
    assert d.a.dtype == F32
    for epilogue, bias in (("bias", True), ("bias", False), ("gate_res", True)):
        out = Out([(M, N)], F32)
        with tuned(**keys):
            _gemm(d, out.views[0], epilogue, bias)
        out.check([G.want("verify", M, N, K, epilogue, bias, F32)], f"{name} verification mode {M}x{N}x{K} {epilogue} bias={bias}", tile)


@pytest.mark.parametrize("count", [2, 3, 4])
@pytest.mark.parametrize("name", ["cfg1", "cfg3", "cfg7", "cfg8", "x288", "x384d0", "x384d1"])
def test_grouped(name, count):
    """2, 3 and 4 problems with their own operands, M = (BM + 37, 1, 2 BM + 3, 80), different N, outputs = row ranges of one joint
    buffer in permuted order"""
    _grouped(name, count)


@pytest.mark.parametrize("name", ["cfg1", "cfg2", "cfg3", "cfg6", "cfg7", "cfg8"])
def test_batched(name):
    """apexmi_gemm_bf16_batched: three batch elements with different operands, contiguous and interleaved-head layout, bf16 and
    float outputs"""
    from apex_studio_amd import lib
    keys, tile = _tiling(name)
    st = torch.cuda.current_stream().cuda_stream
    B = G.BATCH
    for M, N, K in G.BATCHED:
        ds = [dev("fixed", M, N, K, z) for z in range(B)]
        a, w = torch.stack([d.a for d in ds]), torch.stack([d.w for d in ds])                 # [B, M, K], [B, N, K]
        a2 = a.permute(1, 0, 2).reshape(M, B * K).contiguous()                                 # heads interleaved: stride K
        w2 = w.permute(1, 0, 2).reshape(N, B * K).contiguous()
        for dtype, epi in ((BF, lib.EPI_BIAS), (F32, lib.EPI_BIAS_F32)):
            wants = [G.want("fixed", M, N, K, "bias", False, dtype, z) for z in range(B)]
            for layout in ("contiguous", "interleaved"):
                ldc = N + 16                     # every batch element brings its own guards: batch stride (M + 2)(N + 16)
                buf = torch.full((B, M + 2, ldc), G.SENTINEL, dtype=dtype, device=DEV)
                c0 = buf[0, 1:, 8:]
                with tuned(**keys):
                    if layout == "contiguous":
                        rc = lib.load().apexmi_gemm_bf16_batched(a.data_ptr(), K, M * K, w.data_ptr(), K, N * K, c0.data_ptr(), ldc,
                                                                 (M + 2) * ldc, B, M, N, K, epi, st)
                    else:
                        rc = lib.load().apexmi_gemm_bf16_batched(a2.data_ptr(), B * K, K, w2.data_ptr(), B * K, K, c0.data_ptr(), ldc,
                                                                 (M + 2) * ldc, B, M, N, K, epi, st)
                lib.check(rc, "gemm_batched")
                torch.cuda.synchronize()
                host = buf.cpu()
                full = torch.full_like(host, G.SENTINEL)
                for z in range(B):
                    msg = G.mismatches(host[z, 1:M + 1, 8:8 + N], wants[z], tile=tile, prob=z)
                    assert not msg, f"{name} batched {layout} {dtype} {M}x{N}x{K}: {msg}"
                    full[z, 1:M + 1, 8:8 + N] = wants[z]
                assert torch.equal(host, full), f"{name} batched {layout}: store outside the output views"


def test_auto_dispatch_tail_split():
    """gemm.config 0: the lead fills 256 tiles of 256 x 256, the small tail goes out as its own 128 x 128 launch on eight waves"""
    from apex_studio_amd import ops
    (M0, N0), (M1, N1), K = G.AUTO_TAIL
    shapes = [(M0, N0), (M1, N1)]
    ds = [dev("fixed", M, N, K, i) for i, (M, N) in enumerate(shapes)]
    out = Out(shapes, order=[1, 0])
    with tuned():
        ops.gemm_grouped([d.a for d in ds], [d.w for d in ds], [d.bias for d in ds], out.views)
    out.check([G.want("fixed", M, N, K, "bias", True, BF, i) for i, (M, N) in enumerate(shapes)], "auto dispatch, tail split", (256, 256))


@pytest.mark.parametrize("M,N,K", G.GEMV)
def test_gemv_and_gemv_rows(M, N, K):
    """ops.gemv, one row and many (the multi-row kernel), accumulate on and off: fixed-point float x, exact float y"""
    from apex_studio_amd import ops
    op = G.gemv_operands(M, N, K)
    y = G.gemm_ref(op)
    x, w, b, y0 = op.a.to(DEV), op.w.to(BF).to(DEV), op.bias.to(BF).to(DEV), op.res.to(DEV)
    for rows in (slice(0, M), slice(M - 1, M)):
        m = rows.stop - rows.start
        for accum in (False, True):
            out = Out([(m, N)], F32)
            if accum:
                out.views[0].copy_(y0[rows])
            ops.gemv(w, x[rows], b, out=out.views[0], accum=accum)
            want = G.expected(y[rows] + op.res[rows].double() if accum else y[rows], F32)
            out.check([want], f"gemv {m} rows of {M}x{N}x{K} accum={accum}", (8, 64))
        out = Out([(m, N)], F32)
        ops.gemv(w, x[rows], None, out=out.views[0])
        out.check([G.expected(G.gemm_ref(op, bias=False)[rows], F32)], f"gemv {m} rows of {M}x{N}x{K} no bias", (8, 64))


# ------------------------------------------------------------------------------------------- the ring schedules, run last
@pytest.mark.parametrize("name", list(G.RING))
def test_ring_edges(name):
    """gemm.config 9 / 10 (also reachable as gemm.large): the edges of the 256 x 256 tilings, K from 2 to 128 sub-tiles"""
    _edges(name)


@pytest.mark.parametrize("name", list(G.RING))
def test_ring_tile_order_epilogues_activations(name):
    _tile_order(name)
    _epilogues(name)
    _activations(name)
