"""Exact fixed-point probes of the bf16 GEMM family (ops.gemm, gemm_grouped, the batched launch, ops.gemv): operands whose correct
result is known bit for bit, and the references, written from the documented semantics (ops.gemm's docstring, the header of
gemm.hip), never from a kernel:

    C = epi(A W^T + bias)            and            C = R + gate * (A W^T + bias)   for gate_res.

Pure torch on the CPU; the GPU tests feed the operands to every tiling and compare with torch.equal, the host tests evaluate the
conditions below for every case the GPU tests run and prove that the comparison rejects single wrong decisions which the
two-number bar of the older GEMM tests (rel-L2 < 3e-3, max-abs within 2 bf16 ulps of the largest magnitude) lets through.

Why no tolerance.  Every operand lies on a power-of-two grid and is bf16-exact: a = integers in [-32, 32] x 2^-3, w = integers in
[-16, 16] x 2^-6, bias = integers in [-64, 64] x 2^-4, residual = integers in [-64, 64] x 2^-3, gate (f32) per column from
{1, -1, 0.5, -2, 1.5, 0.75, -0.25, 1.25}.  Every product a * w is a multiple of 2^-9, hence every partial sum in ANY order, and
acc + bias; gate * y is a multiple of 2^-9 x (lowest set bit of the gate), and so is r + gate * y.  A multiple of a grid g whose
magnitude stays below 2^24 g is a float32, so as long as the SPAN (sum of magnitudes / grid, `span_log2`) stays below 2^22 - two
bits of headroom - every float32 intermediate is exact, with or without FMA contraction, and the ONLY inexact step is the one bf16
rounding at the store.  The expected bf16 output is exact.float().to(bfloat16) bit for bit, the expected float output the exact
value.  4 - 12 % of the elements are exact ties of that rounding (`tie_fraction`), so the tie rule is exercised.

Selector weights tell K positions apart: every output column has exactly one non-zero weight per chosen K-tile t, at
k = 64 t + (11 n + 23 t + 3 (n // 7)) % 64, with a coefficient from {1, -2, 2, -1}; a[m, k] is an integer formula in [-4, 4].  A
mismatch names the missed K-tile and position through its value and sign."""
import functools
from typing import Optional

import torch

from tests.conv_probes import BF, _ordered, mismatches as _elementwise, ulp_distance  # noqa: F401  (ulp_distance: re-exported)

BK = 64
SENTINEL = 32768.0            # bf16-exact, outside every reference's range (asserted per case: |ref| <= 8192)
GATES = (1.0, -1.0, 0.5, -2.0, 1.5, 0.75, -0.25, 1.25)
GATE_LSB = (1.0, 1.0, 0.5, 2.0, 0.5, 0.25, 0.25, 0.25)       # lowest set bit of each gate: gate * (multiple of g) is a multiple of lsb * g
SPAN_BITS = 22                # float32 holds 24; two bits of headroom
ACT_RANGE = 4.0               # |pre-activation| of the activation probes, see act_operands


# ------------------------------------------------------------------------------------------------------------------ operands
class Operands:
    """a [M, K], w [N, K], bias [N], res [M, N]: float32 holding bf16-exact values; gate [N] float32; g*: the grid of each"""

    def __init__(self, a, w, bias, gate, res, ga, gw, gb, gr, gate_idx):
        self.a, self.w, self.bias, self.gate, self.res = a, w, bias, gate, res
        self.ga, self.gw, self.gb, self.gr = ga, gw, gb, gr
        self.gate_lsb = torch.tensor(GATE_LSB)[gate_idx]
        self.M, self.K, self.N = a.shape[0], a.shape[1], w.shape[0]
        for t, g in ((a, ga), (w, gw), (bias, gb), (res, gr)):      # conditions, not measurements
            assert torch.equal(t.to(BF).float(), t), "operand does not round-trip through bf16"
            assert torch.equal((t / g).round() * g, t), "operand off its grid"
        assert torch.equal(self.gate, torch.tensor(GATES)[gate_idx])


def _ints(shape, seed, lim):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _seed(M, N, K, salt):
    return (M * 7919 + N * 104729 + K * 31 + salt * 1299709) % (2 ** 31 - 1)


def w_grid(K):
    """(largest integer, grid) of the fixed-point weights: coarser above K = 4096 so that the span condition holds"""
    return (16, 2.0 ** -6) if K <= 4096 else (8, 2.0 ** -5)


@functools.lru_cache(maxsize=None)
def fixed_point(M, N, K, salt=0):
    """the main family: the default grids of the module docstring"""
    s = _seed(M, N, K, salt)
    wl, gw = w_grid(K)
    g = torch.Generator().manual_seed(s + 4)
    gi = torch.randint(0, 8, (N,), generator=g)
    return Operands(_ints((M, K), s, 32) * 2.0 ** -3, _ints((N, K), s + 1, wl) * gw, _ints((N,), s + 2, 64) * 2.0 ** -4,
                    torch.tensor(GATES)[gi], _ints((M, N), s + 3, 64) * 2.0 ** -3, 2.0 ** -3, gw, 2.0 ** -4, 2.0 ** -3, gi)


@functools.lru_cache(maxsize=None)
def act_operands(M, N, K, salt=0):
    """Pre-activations for the activation epilogues, |y| <= ACT_RANGE (asserted by pre_activation): a = integers in [-4, 4] x 2^-3,
    w = integers in [-4, 4] x 2^-6, bias = integers in [-40, 40] x 2^-4.  Inside that range none of the four activations loses
    its result to float32 itself: gelu_erf's 1 + erf(x / sqrt 2) >= 6e-5 keeps the cancellation error 2^-24 / 6e-5 under half
    a bf16 step (2^-9), and no exp2 / rcp operand comes near the float32 exponent limits (gelu(tanh) reaches them at |x| ~ 9.6)."""
    s = _seed(M, N, K, salt + 50)
    gi = torch.zeros(N, dtype=torch.long)
    return Operands(_ints((M, K), s, 4) * 2.0 ** -3, _ints((N, K), s + 1, 4) * 2.0 ** -6, _ints((N,), s + 2, 40) * 2.0 ** -4,
                    torch.ones(N), torch.zeros(M, N), 2.0 ** -3, 2.0 ** -6, 2.0 ** -4, 2.0 ** -3, gi)


@functools.lru_cache(maxsize=None)
def verify_operands(M, N, K, salt=0):
    """f32-storage verification mode: float a = integers in +-2047 x 2^-9 (12 significant bits: the hi AND mid parts of the
    three-way bf16 split carry it), w = integers in [-4, 4] x 2^-4; K <= 256"""
    assert K <= 256
    s = _seed(M, N, K, salt + 100)
    g = torch.Generator().manual_seed(s + 4)
    gi = torch.randint(0, 8, (N,), generator=g)
    a = _ints((M, K), s, 2047) * 2.0 ** -9
    op = Operands.__new__(Operands)
    op.a, op.w, op.bias = a, _ints((N, K), s + 1, 4) * 2.0 ** -4, _ints((N,), s + 2, 64) * 2.0 ** -4
    op.gate, op.res = torch.tensor(GATES)[gi], _ints((M, N), s + 3, 64) * 2.0 ** -3          # res: float storage here
    op.ga, op.gw, op.gb, op.gr, op.gate_lsb = 2.0 ** -9, 2.0 ** -4, 2.0 ** -4, 2.0 ** -3, torch.tensor(GATE_LSB)[gi]
    op.M, op.K, op.N = M, K, N
    assert torch.equal(op.w.to(BF).float(), op.w) and torch.equal(op.bias.to(BF).float(), op.bias)
    hi = a.to(BF).float()
    mid = (a - hi).to(BF).float()
    assert not torch.equal(hi, a) and torch.equal(hi + mid, a), "a must need exactly the hi and mid parts"
    return op


# ---- selector weights
def int_a(M, K, salt=0):
    """a[m, k] in [-4, 4]: one step along either axis changes the value (4 and 7 are units mod 9), rows and columns enter
    differently, the period along both axes is 9 or a multiple of it, which divides no tile extent"""
    m, k = torch.arange(M).view(-1, 1) + salt, torch.arange(K).view(1, -1)
    return ((m * 4 + k * 7 + (m * k) % 5 + (m // 9 + k // 9) % 3) % 9 - 4).float()


def selector_tiles(N, T):
    """chosen[n, t]: the K-tiles column n reads.  All of them up to 12 K-tiles; above: the first, the last and a walk of ten that
    starts at another tile for every column - at most 12, so |sum| <= 12 * 2 * 4 = 96"""
    if T <= 12:
        return torch.ones(N, T, dtype=torch.bool)
    chosen = torch.zeros(N, T, dtype=torch.bool)
    chosen[:, 0] = chosen[:, T - 1] = True
    n = torch.arange(N)
    for j in range(10):
        chosen[n, (7 * n + j * (T // 10) + j) % T] = True
    return chosen


def selector_positions(N, T):
    """(pos [N, T] in 0..63, coef [N, T]) of the one non-zero weight of column n in K-tile t"""
    n, t = torch.arange(N).view(-1, 1), torch.arange(T).view(1, -1)
    pos = (11 * n + 23 * t + 3 * (n // 7)) % BK
    coef = torch.tensor([1.0, -2.0, 2.0, -1.0])[(n * 3 + t * 5 + (n * t) % 7) % 4]
    return pos, coef


@functools.lru_cache(maxsize=None)
def selector(M, N, K, salt=0):
    """integer operands: |a| <= 4, one weight of magnitude <= 2 per chosen K-tile, |bias| <= 8, |residual| <= 16, |gate| <= 2:
    |R + gate (y + b)| <= 16 + 2 (96 + 8) = 224 <= 256"""
    T = K // BK
    chosen = selector_tiles(N, T)
    pos, coef = selector_positions(N, T)
    w = torch.zeros(N, T, BK)
    w.scatter_(2, pos.unsqueeze(2), (coef * chosen).unsqueeze(2))
    n, m = torch.arange(N), torch.arange(M).view(-1, 1)
    gi = (n * 3 + n // 8 + salt) % 8
    bias = ((n * 5 + 3 + salt) % 17 - 8).float()
    res = ((m * 5 + n.view(1, -1) * 7 + (m * n.view(1, -1)) % 5 + salt) % 33 - 16).float()
    op = Operands(int_a(M, K, salt), w.view(N, K), bias, torch.tensor(GATES)[gi], res, 1.0, 1.0, 1.0, 1.0, gi)
    assert int(chosen.sum(1).max()) <= 12
    return op


FAMILIES = {"fixed": fixed_point, "selector": selector, "act": act_operands, "verify": verify_operands}


def operands(family, M, N, K, salt=0):
    return FAMILIES[family](M, N, K, salt)


# ---------------------------------------------------------------------------------------------------------------- references
def pre_activation(op, bias=True):
    """A W^T (+ bias) in float64: exact (every term a multiple of the grid, sums far below 2^53 grids)"""
    y = op.a.double() @ op.w.double().T
    return y + op.bias.double() if bias else y


def gemm_ref(op, epilogue="bias", bias=True, res=None):
    """the exact float64 result of the bias or gate_res epilogue"""
    y = pre_activation(op, bias)
    if epilogue == "gate_res":
        return (op.res if res is None else res).double() + op.gate.double() * y
    assert epilogue == "bias", epilogue
    return y


def act_ref(op, epilogue, bias=True):
    """the float64 definition of an activation epilogue on the exact pre-activation"""
    x = pre_activation(op, bias)
    assert float(x.abs().max()) <= ACT_RANGE, float(x.abs().max())
    if epilogue == "gelu":        # 0.5 (1 + tanh u) = sigmoid(2 u)
        return x * torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x ** 3))
    if epilogue == "gelu_erf":
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if epilogue == "silu":
        return x * torch.sigmoid(x)
    assert epilogue == "quick_gelu", epilogue
    return x * torch.sigmoid(1.702 * x)


def span_log2(op, epilogue="bias", bias=True):
    """log2 of the largest (sum of magnitudes) / grid over the output elements: every float32 partial result of any summation
    order is a multiple of its column's grid no larger than that sum"""
    mag = op.a.double().abs() @ op.w.double().abs().T
    grid = torch.full((op.N,), op.ga * op.gw, dtype=torch.float64)
    if bias:
        mag = mag + op.bias.double().abs()
        grid = grid.clamp_max(op.gb)
    if epilogue == "gate_res":
        mag = mag * op.gate.double().abs() + op.res.double().abs()
        grid = (grid * op.gate_lsb.double()).clamp_max(op.gr)
    return float((mag / grid).max().log2())


def expected(ref, dtype=BF):
    """what the kernel must store: the exact value as float32 (asserted to hold it), rounded ONCE to nearest-even for bf16"""
    f = ref.float()
    assert torch.equal(f.double(), ref), "the exact result is no float32: the span condition is violated"
    assert float(ref.abs().max()) <= SENTINEL / 4
    return f.to(dtype)


def tie_fraction(ref):
    """fraction of elements whose exact value lies exactly halfway between two bf16 neighbours"""
    b = ref.float().to(BF).double()
    _, ex = torch.frexp(ref)                             # |ref| = m 2^ex, m in [0.5, 1): bf16 spacing 2^(ex - 8) in that binade
    half = torch.ldexp(torch.ones_like(ref), ex - 9)
    return float((((ref - b).abs() == half) & (ref != 0)).double().mean())


def exact_fraction(ref):
    """fraction of elements that are bf16 values already"""
    return float((ref.float().to(BF).double() == ref).double().mean())


@functools.lru_cache(maxsize=None)
def want(family, M, N, K, epilogue="bias", bias=True, dtype=BF, salt=0):
    """expected output of one case, computed once and shared (callers do not modify it)"""
    op = operands(family, M, N, K, salt)
    assert span_log2(op, epilogue, bias) < SPAN_BITS
    return expected(gemm_ref(op, epilogue, bias), dtype)


# --------------------------------------------------------------------------------------------------------------- comparisons
def mismatches(got, want_, tile=None, prob=None, n=6):
    """'' when got == want bit for bit; else the count and the first n entries as (m, n) got / want (conv_probes.mismatches),
    the problem or batch element, and the tile coordinates (m // BM, n // BN) of the tiling under test"""
    msg = _elementwise(got, want_, n)
    if not msg or got.shape != want_.shape:
        return msg
    msg = msg.replace("(t, h, w, co)", "(m, n)")
    if prob is not None:
        msg = f"problem / batch {prob}: " + msg
    if tile is not None:
        bad = (got != want_).nonzero()
        tiles = sorted({(int(i[-2]) // tile[0], int(i[-1]) // tile[1]) for i in bad})
        msg += f"; tiles (m // {tile[0]}, n // {tile[1]}): {tiles[:8]}" + (" ..." if len(tiles) > 8 else "")
    return msg


def ulp_worst(got, want64):
    """(largest distance in bf16 code points from the float64 reference rounded to bf16, its coordinate)"""
    d = (_ordered(got) - _ordered(want64.to(BF))).abs()
    i = int(d.argmax())
    return int(d.flatten()[i]), (i // got.shape[-1], i % got.shape[-1])


def old_bar_accepts(out, ref, rel_tol=3e-3, ulp=2.0):
    """the two-number bar every older bf16 GEMM test ends in (tests/test_gpu_ops.py, _check), as a predicate"""
    out, ref = out.float(), ref.float()
    rel = float((out - ref).norm() / (ref.norm() + 1e-30))
    mx = float((out - ref).abs().max())
    return bool(torch.isfinite(out).all()) and rel < rel_tol and mx <= ulp * 2.0 ** -8 * float(ref.abs().max()) + 1e-6


# ------------------------------------------------------------------------------------------------ the cases of the GPU suite
# name: (tune keys without the "gemm." prefix, BM, BN).  The ring schedules (9, 10) stand apart: they run last.
TILINGS = {
    "cfg1": ({"config": 1}, 128, 128), "cfg8": ({"config": 8}, 128, 128),
    "cfg2": ({"config": 2}, 256, 256), "cfg3": ({"config": 3}, 256, 256), "cfg6": ({"config": 6}, 256, 256),
    "cfg7": ({"config": 7}, 256, 256),
    "x288": ({"x288": 2}, 288, 192),
    "x384d0": ({"x384": 2, "x384_dist": 0}, 384, 256), "x384d1": ({"x384": 2, "x384_dist": 1}, 384, 256),
}
RING = {"ring9": ({"config": 9}, 256, 256), "ring10": ({"config": 10}, 256, 256)}
ALL_TILINGS = {**TILINGS, **RING}
EDGE_KS = tuple(BK * t for t in (1, 2, 3, 4, 5, 9))      # prologue only .. the peeled last tile .. past the ring's 3 - 4 sub-tile lead
DEEP_K = 4096
EPI_KS = (64, 320)
GROUP_K = 192
BATCHED = ((77, 72, 128), (300, 264, 192))
BATCH = 3
AUTO_TAIL = ((4096, 4096), (80, 4096), 256)             # lead fills 256 tiles of 256 x 256, the tail goes out on CFG_128E
GEMV = ((2, 70, 256), (5, 301, 768), (3, 40, 16384))


def edge_shapes(BM, BN):
    return ((BM + 37, BN + 8), (BM - 1, BN - 8), (1, 8))


def edge_cases(BM, BN):
    """(M, N, K) of the edge probes of one tiling"""
    out = [(M, N, K) for (M, N) in edge_shapes(BM, BN) for K in EDGE_KS]
    return out + [(BM + 37, BN + 8, DEEP_K)]


def order_shape(BM, BN):
    """tile order: the last tile group is shorter than group_m and the tile count is no multiple of 8 (xcd_remap)"""
    return ((3 * 384 + 5) if BM == 384 else 6 * BM + 5, BN + 8, BK)


def group_shapes(BM, BN):
    """(M, N) of the four problems of a grouped launch (the first `count` are used)"""
    return ((BM + 37, BN + 8), (1, 72), (2 * BM + 3, BN - 8), (80, 136))


def all_exact_cases():
    """every (family, M, N, K, salt) the GPU file compares exactly, for the host tests"""
    cases = set()
    for _, BM, BN in ALL_TILINGS.values():
        for M, N, K in edge_cases(BM, BN):
            cases |= {("fixed", M, N, K, 0), ("selector", M, N, K, 0)}
        cases.add(("selector", *order_shape(BM, BN), 0))
        cases.add(("fixed", *order_shape(BM, BN), 0))
        for K in EPI_KS:
            cases.add(("fixed", BM + 37, BN + 8, K, 0))
        for i, (M, N) in enumerate(group_shapes(BM, BN)):
            cases.add(("fixed", M, N, GROUP_K, i))
    for M, N, K in BATCHED:
        cases |= {("fixed", M, N, K, z) for z in range(BATCH)}
    (M0, N0), (M1, N1), K = AUTO_TAIL
    cases |= {("fixed", M0, N0, K, 0), ("fixed", M1, N1, K, 1)}
    return sorted(cases)


def gemv_operands(M, N, K):
    """x [M, K] float32 = integers in [-32, 32] x 2^-3, w bf16 on w_grid(K), bias, and y0 [M, N] (the accumulate operand)"""
    return fixed_point(M, N, K, 7)


def case_id(c):
    return "-".join(str(v) for v in c)


def sentinel_of(dtype) -> Optional[float]:
    return float(torch.tensor(SENTINEL).to(dtype))
