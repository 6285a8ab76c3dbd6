"""Exact probes of the opt-in FP8 compute path (gemm_fp8.hip: apexmi_quant_rows_fp8 and apexmi_gemm_fp8; ops.quant_rows_fp8,
ops.gemm_fp8 and the fp8 route of ops.gemm): operands whose correct result is known bit for bit, and the references, written from
the documented semantics (ops.gemm_fp8's and ops.quant_rows_fp8's docstrings), never from a kernel:

    out = epi((qa . qw^T) * sa[m] * sw[n] + bias[n])        and        out = R + gate[n] * (...)   for gate_res,
    scale = absmax / 448 (1 for a zero row),  code = the nearest finite e4m3 value of clamp(x / scale, +-448), ties to even.

Pure torch on the CPU.  The GPU tests (tests/test_gpu_gemm_fp8_probes.py) feed the operands to the kernels and compare whole
sentinel-filled buffers with torch.equal; the host tests (tests/test_gemm_fp8_probes_host.py) evaluate the conditions below for
every case the GPU tests run and prove that the comparison rejects single wrong decisions.

Fixed-point family, why no tolerance.  qa and qw hold the codes of integers in [-L, L] (L = 8 up to K = 384, 6 up to 1152, 3 above: `int_range`),
so every product and every partial sum of the dot product is an integer.  sa[m] is drawn per row from SA, sw[n] per column from
SW (or is the single value SW_ONE), gate[n] from gemm_probes.GATES: odd x 2^e values with an odd part of at most 3 / 5 / 5, so
acc * sa * sw is a multiple of lsb(sa) lsb(sw) (`lsb`: the lowest set bit).  bias = integers in [-64, 64] x 2^-4 and R = integers in
[-64, 64] x 2^-3 lie on the grids gemm_probes uses.  `span_log2` evaluates, per output element and on the actual operands,
(sum |qa| |qw|) |sa| |sw| (+ |bias|) (x |gate| + |R|) in units of the finest grid of that element's final sum and asserts it below
2^22: every float32 intermediate is then a multiple of its grid below 2^24 grids, i.e. exact, in any accumulation order and with
or without FMA contraction of acc * sa * sw + bias.  The ONLY rounding left is the bf16 store: expected = exact.float().to(bf16).

Neighbours differ by construction (asserted, `Fixed.__init__`): sa[m] != sa[m - 1]; sw, bias and gate differ between columns n and
n - 1 and between n and n - 4 (the epilogue loads 4-column groups and clamps the group index: the last group against the group a
wrong clamp would read); every element of R differs from the one a row above.  A wrong index of any of them is a different number.

Code-point family: every finite e4m3 code (254: 0 .. 448 and -0 .. -448) once as an activation and once as a weight.  The
operand under test is one-hot per row (the code at a k that depends on the code: the 254 between them reach all 128 byte
positions of a K-tile in both K-tiles), the partner is dense, 1.0 or -2.0 by a formula in (row, k): every output's dot product has
exactly ONE non-zero product and is value(code) x partner x sa x sw exactly."""
import functools

import torch

from tests import gemm_probes as G
from tests.gemm_probes import BF, GATES, GATE_LSB, SPAN_BITS, tie_fraction, exact_fraction  # noqa: F401  (re-exported)

F8 = torch.float8_e4m3fn
BM = BN = BK = 128            # the kernel's output tile and K-tile (bytes)
BAND = 8                      # tile rows per band of the tile order
SENTINEL = 2.0 ** 30          # bf16-exact, outside every reference's range (asserted per case: |ref| <= 2^28)
SENTINEL_CODE = 0x7F          # a NaN code: the quantiser never writes one
GUARD = 8                     # guard columns on each side of an output view (16 bytes), one guard row above and below

SA = (1.0, 0.5, 1.5, 0.75, 0.25, 0.375, 0.1875, 0.125)          # float32 activation scales, odd part <= 3
SW = (1.0, -1.0, 0.5, 1.5, 0.75, -0.25, 1.25, -0.5)           # bf16-exact weight scales, odd part <= 5
SW_ONE = 0.75                                                 # the single-value form
GB, GR = 2.0 ** -4, 2.0 ** -3                                 # grids of bias and residual (gemm_probes.fixed_point's)


def lsb(v: float) -> float:
    """lowest set bit of a binary fraction: v = odd x lsb(v)"""
    v, e = abs(float(v)), 0
    assert v != 0
    while v != int(v):
        v, e = v * 2, e - 1
    v = int(v)
    while v % 2 == 0:
        v, e = v // 2, e + 1
    return 2.0 ** e


SA_LSB, SW_LSB = tuple(lsb(v) for v in SA), tuple(lsb(v) for v in SW)
assert len(set(SA)) == 8 and len(set(SW)) == 8 and 1.5 in SA and 0.75 in SA and tuple(lsb(g) for g in GATES) == GATE_LSB


def codes_of(x: torch.Tensor) -> torch.Tensor:
    """float values that e4m3 holds exactly -> their code bytes (asserted)"""
    q = x.float().to(F8)
    assert torch.equal(q.float(), x.float()), "operand does not round-trip through e4m3"
    return q.view(torch.uint8)


def values_of(codes: torch.Tensor) -> torch.Tensor:
    return codes.view(F8).float()


def int_range(K: int) -> int:
    """largest integer of the fixed-point codes: narrower as K grows so that the span condition holds"""
    return 8 if K <= 384 else 6 if K <= 1152 else 3


# ------------------------------------------------------------------------------------------------------- fixed-point family
def _walk(n, lo, hi, gen):
    """n indices in 0 .. hi - 1 whose adjacent entries differ: a cumulative sum of steps in lo .. hi - 1, modulo hi"""
    return torch.randint(lo, hi, (n,), generator=gen).cumsum(0) % hi


def _columns(N, mod, gen):
    """N values in 0 .. mod - 1 that differ from the value 1 and the value 4 columns before"""
    draw = torch.randint(0, mod, (N,), generator=gen).tolist()
    for n in range(N):
        while (n >= 1 and draw[n] == draw[n - 1]) or (n >= 4 and draw[n] == draw[n - 4]):
            draw[n] = (draw[n] + 1) % mod
    return torch.tensor(draw)


class Fixed:
    """qa [M, K], qw [N, K]: float32 holding integers in [-L, L]; sa [M] float32; sw [N] and sw_one [1] bf16-exact float32;
    bias [N], res [M, N] bf16-exact float32; gate [N] float32; *_lsb: the lowest set bit of each scale"""

    def __init__(self, M, N, K, salt=0, lossless_a=False):
        self.M, self.N, self.K, self.salt = M, N, K, salt
        g = torch.Generator().manual_seed(G._seed(M, N, K, salt + 200))
        L = int_range(K)
        self.qa = torch.randint(-L, L + 1, (M, K), generator=g).float()
        self.qw = torch.randint(-L, L + 1, (N, K), generator=g).float()
        if lossless_a:            # the route case: every row holds +-448 once and a power-of-two scale, see `routed`
            m = torch.arange(M)
            self.qa[m, (m * 37 + 11) % K] = torch.where(m % 3 == 0, -448.0, 448.0)
            pw = torch.tensor([1.0, 0.5, 0.25, 0.125])[_walk(M, 1, 4, g)]
            self.sa, self.sa_lsb = pw, pw
        else:
            si = _walk(M, 1, 8, g)
            self.sa, self.sa_lsb = torch.tensor(SA)[si], torch.tensor(SA_LSB)[si]
        wi = _columns(N, 8, g)
        self.sw, self.sw_lsb = torch.tensor(SW)[wi], torch.tensor(SW_LSB)[wi]
        self.sw_one, self.sw_one_lsb = torch.tensor([SW_ONE]), torch.tensor([lsb(SW_ONE)])
        self.bias = (_columns(N, 129, g) - 64).float() * GB
        gi = _columns(N, 8, g)
        self.gate, self.gate_lsb = torch.tensor(GATES)[gi], torch.tensor(GATE_LSB)[gi]
        self.res = ((torch.randint(1, 129, (M, N), generator=g).cumsum(0) % 129) - 64).float() * GR
        # conditions, not measurements
        for t in (self.qa, self.qw):
            assert torch.equal(values_of(codes_of(t)), t)
        for t in (self.sw, self.sw_one, self.bias, self.res):
            assert torch.equal(t.to(BF).float(), t), "operand does not round-trip through bf16"
        assert self.sa.dtype == torch.float32 and len(set(SA)) >= 6
        assert bool((self.sa[1:] != self.sa[:-1]).all()), "adjacent rows must differ in sa"
        assert bool((self.res[1:] != self.res[:-1]).all()), "every residual element must differ from the row above"
        for t in (self.sw, self.bias, self.gate):
            assert bool((t[1:] != t[:-1]).all()) and bool((t[4:] != t[:-4]).all()), "columns 1 and 4 apart must differ"
            assert not torch.equal(t[N - 4:], t[N - 8:N - 4]), "the last 4-column group against the one a wrong clamp reads"
        assert float(self.sw_one) != 1.0 and bool((self.sw != self.sw_one).any()), "the two sw forms must differ"

    @functools.cached_property
    def acc(self):
        """qa . qw^T in float64: exact integers"""
        return self.qa.double() @ self.qw.double().T

    @functools.cached_property
    def mag(self):
        return self.qa.double().abs() @ self.qw.double().abs().T


def pre_activation(op, per_row=True, bias=True):
    """(qa . qw^T) sa[m] sw[n] (+ bias[n]) in float64: exact"""
    sw = op.sw if per_row else op.sw_one
    y = op.acc * op.sa.double().view(-1, 1) * sw.double().view(1, -1)
    return y + op.bias.double() if bias else y


def gemm_ref(op, epilogue="bias", per_row=True, bias=True):
    """the exact float64 result of the bias or gate_res epilogue"""
    y = pre_activation(op, per_row, bias)
    if epilogue == "gate_res":
        return op.res.double() + op.gate.double() * y
    assert epilogue == "bias", epilogue
    return y


def gelu_ref(x):
    """the float64 definition of the tanh GELU in the x sigmoid(2 u) form (0.5 (1 + tanh u) = sigmoid(2 u) exactly)"""
    x = x.double()
    return x * torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x ** 3))


def span_log2(op, epilogue="bias", per_row=True, bias=True):
    """log2 of the largest (sum of magnitudes) / grid over the output elements, grid = the finest grid of that element's final
    sum: every float32 partial result of any order is a multiple of its grid no larger than that sum"""
    sw, sw_lsb = (op.sw, op.sw_lsb) if per_row else (op.sw_one, op.sw_one_lsb)
    mag = op.mag * op.sa.double().abs().view(-1, 1) * sw.double().abs().view(1, -1)
    grid = (op.sa_lsb.double().view(-1, 1) * sw_lsb.double().view(1, -1)).expand(op.M, op.N)
    if bias:
        mag = mag + op.bias.double().abs()
        grid = grid.clamp_max(GB)
    if epilogue == "gate_res":
        mag = mag * op.gate.double().abs() + op.res.double().abs()
        grid = (grid * op.gate_lsb.double()).clamp_max(GR)
    return float((mag / grid).max().log2())


def expected(ref):
    """what the kernel must store: the exact value as float32 (asserted to hold it), rounded ONCE to nearest-even to bf16"""
    f = ref.float()
    assert torch.equal(f.double(), ref), "the exact result is no float32: the span condition is violated"
    assert float(ref.abs().max()) <= SENTINEL / 4
    return f.to(BF)


EXACT_VARIANTS = tuple((e, p, b) for e in ("bias", "gate_res") for p in (True, False) for b in (True, False))


def tie_fractions(op):
    """{(epilogue, per-row sw, bias): fraction of exact ties of the bf16 rounding} of the eight exact results of one case"""
    return {v: tie_fraction(gemm_ref(op, *v)) for v in EXACT_VARIANTS}


def _has_ties(op):
    """every exact result holds a tie, and no dot product is zero in a whole row or column (a wrong scale would not show there)"""
    return min(tie_fractions(op).values()) > 0 and bool((op.acc != 0).any(0).all()) and bool((op.acc != 0).any(1).all())


@functools.lru_cache(maxsize=None)
def fixed_point(M, N, K):
    """the case of one shape.  Small outputs (M = 1, N = 16 has 16 elements) take the first salt whose eight exact results
    all hold an exact tie of the bf16 rounding and whose rows and columns all hold a non-zero dot product: a condition on the operands, evaluated on the CPU reference alone"""
    for salt in range(4096):
        op = Fixed(M, N, K, salt)
        if _has_ties(op):
            return op
    raise AssertionError(f"no draw of {M}x{N}x{K} holds a tie")


@functools.lru_cache(maxsize=None)
def want(M, N, K, epilogue="bias", per_row=True, bias=True):
    """expected bf16 output of one variant of one case, computed once and shared (callers do not modify it)"""
    op = fixed_point(M, N, K)
    assert span_log2(op, epilogue, per_row, bias) < SPAN_BITS
    return expected(gemm_ref(op, epilogue, per_row, bias))


# ---- the route through ops.gemm: bf16 activations that quantise losslessly
ROUTE = (129, 144, 384)


@functools.lru_cache(maxsize=None)
def routed():
    """(op, a): a = qa * sa[m] in bf16, every row holding +-448 sa[m] once with sa[m] a power of two, so the quantiser's scale
    is exactly sa[m] and its codes are exactly qa (asserted here on the CPU with the definition-based reference)"""
    op = Fixed(*ROUTE, salt=0, lossless_a=True)
    a = op.qa * op.sa.view(-1, 1)
    assert torch.equal(a.to(BF).float(), a)
    codes, scale = quant_ref(a.to(BF))
    assert torch.equal(scale, op.sa) and torch.equal(codes, codes_of(op.qa))
    assert bool((torch.log2(scale) == torch.log2(scale).round()).all())
    return op, a.to(BF)


@functools.lru_cache(maxsize=None)
def routed_want(epilogue="bias"):
    op, _ = routed()
    assert span_log2(op, epilogue) < SPAN_BITS and _has_ties(op)
    return expected(gemm_ref(op, epilogue))


# ------------------------------------------------------------------------------------------------------- code-point family
FINITE = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)          # 254 codes, NaN left out
CODE_K = 256                                                                                   # two K-tiles
CODE_OTHER = {"act": 144, "weight": 130}     # N of the activation role, M of the weight role


def code_k(i):
    """k of the one non-zero of the row that carries FINITE[i]: 37 is a unit modulo 256, so the 254 rows take 254 different k"""
    return (i * 37 + 5) % CODE_K


def partner(r, k):
    """the dense partner operand: 1.0 or -2.0 by (row, k)"""
    return torch.where((r + 3 * k + (r * k) % 5) % 2 == 0, 1.0, -2.0)


class CodePoints:
    """role 'act': qa [254, K] one-hot rows of the 254 codes, qw [144, K] dense partner;
    role 'weight': qw [256, K] one-hot rows (rows 254, 255 all zero: N is a multiple of 16), qa [130, K] dense partner"""

    def __init__(self, role):
        self.role, self.K = role, CODE_K
        i = torch.arange(254)
        hot = torch.zeros(256 if role == "weight" else 254, CODE_K, dtype=torch.uint8)
        hot[i, code_k(i)] = FINITE
        other = CODE_OTHER[role]
        dense = partner(torch.arange(other).view(-1, 1), torch.arange(CODE_K).view(1, -1))
        self.qa_codes, self.qw_codes = (hot, codes_of(dense)) if role == "act" else (codes_of(dense), hot)
        self.M, self.N = self.qa_codes.shape[0], self.qw_codes.shape[0]
        g = torch.Generator().manual_seed(31 + (role == "act"))
        si, wi = _walk(self.M, 1, 8, g), _columns(self.N, 8, g)
        self.sa, self.sw = torch.tensor(SA)[si], torch.tensor(SW)[wi]
        # conditions: all finite codes, every value a bf16, all byte positions of a K-tile, both K-tiles
        v = values_of(FINITE)
        assert bool(torch.isfinite(v).all()) and torch.equal(v.to(BF).float(), v) and FINITE.numel() == 254
        assert float(v.abs().max()) == 448 and float(v[v != 0].abs().min()) == 2.0 ** -9 and int((FINITE == 0x80).sum()) == 1
        ks = code_k(i)
        assert ks.unique().numel() == 254 and (ks % BK).unique().numel() == BK and set((ks // BK).tolist()) == {0, 1}
        assert int((values_of(hot) != 0).sum(1).max()) == 1

    def ref(self):
        """float64: one non-zero product per output, value(code) x partner x sa x sw"""
        a, w = values_of(self.qa_codes).double(), values_of(self.qw_codes).double()
        assert int(((a != 0).float() @ (w != 0).float().T).max()) == 1, "exactly one non-zero product per output"
        return (a @ w.T) * self.sa.double().view(-1, 1) * self.sw.double().view(1, -1)


@functools.lru_cache(maxsize=None)
def code_points(role):
    return CodePoints(role)


# NaN codes: planted into the fixed-point case NAN_SHAPE; (operand, row, k, code)
NAN_SHAPE = (129, 144, 384)
NAN_PLANTS = (("a", 5, 3, 0x7F), ("a", 128, 383, 0xFF), ("w", 17, 130, 0xFF), ("w", 143, 64, 0x7F))


def nan_touched(M, N):
    """mask [M, N] of the outputs whose dot product reads a NaN code"""
    t = torch.zeros(M, N, dtype=torch.bool)
    for which, r, _, _ in NAN_PLANTS:
        if which == "a":
            t[r, :] = True
        else:
            t[:, r] = True
    return t


# ----------------------------------------------------------------------------------------------------------- the quantiser
E4M3_POS = torch.arange(0, 127, dtype=torch.uint8).view(F8).double()       # the 127 non-negative finite values, ascending: 0 .. 448


def e4m3_nearest(y, tie="even"):
    """codes of the nearest finite e4m3 value of y (|y| <= 448), from the definition: ties go to the even mantissa (the even
    code: the mantissa's last bit is the code's), the sign is kept, also of a result that rounds to zero.
    tie = 'away' is the mutant of the host tests."""
    mag = y.double().abs()
    assert float(mag.max()) <= 448
    hi = torch.searchsorted(E4M3_POS, mag.contiguous()).clamp(max=126)          # the first value >= |y|
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = mag - E4M3_POS[lo], E4M3_POS[hi] - mag
    tie_up = (hi % 2 == 0) if tie == "even" else torch.ones_like(hi, dtype=torch.bool)
    idx = torch.where((dhi < dlo) | ((dhi == dlo) & tie_up), hi, lo)
    return (idx + 128 * torch.signbit(y).long()).to(torch.uint8)


def quant_ref(a, absmax_cols=None, tie="even"):
    """ops.quant_rows_fp8's documented formula on bf16 a [M, K] -> (codes uint8 [M, K], scales float32 [M]); IEEE float32,
    every operation rounded on its own.  absmax_cols = 1024 is the mutant 'absmax over the first step only'."""
    x = a.float()
    amax = x[:, :absmax_cols].abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))       # tensor / tensor: true division
    y = torch.minimum(torch.maximum(x / scale, torch.full_like(x, -448.0)), torch.full_like(x, 448.0))
    return e4m3_nearest(y, tie), scale.reshape(-1)


def bf16_upto_448():
    """every finite bf16 value with |x| <= 448, -0 and the subnormals included: 34 754 points"""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = x[torch.isfinite(x.float()) & (x.float().abs() <= 448)]
    assert x.numel() == 34754
    return x


QUANT_KS = (1152, 2176)           # one and two full 1024-steps plus a 128 remainder
QUANT_MS = (1, 2, 3, 9)
CODEPOINT_K = 1152
CODEPOINT_EXPONENTS = (0, 6, -4)


@functools.lru_cache(maxsize=None)
def quant_rows(M, K):
    """bf16 [M, K]: adjacent rows six decades apart; the row's absmax sits at ONE column, by row: in the second step only, in the
    last 16 columns, in the first step, in the third step only (K = 2176; else in the second)"""
    g = torch.Generator().manual_seed(977 * M + K)
    a = torch.randn(M, K, generator=g)
    a = a * torch.tensor([1e3 if r % 2 == 0 else 1e-3 for r in range(M)]).view(-1, 1)
    for r in range(M):
        k = absmax_column(r, K)
        a[r, k] = 8.0 * float(a[r].abs().max()) * (-1.0 if r % 3 == 1 else 1.0)
    a = a.to(BF)
    for r in range(M):
        rest = torch.cat([a[r, :absmax_column(r, K)], a[r, absmax_column(r, K) + 1:]]).float().abs().max()
        assert int(a[r].float().abs().argmax()) == absmax_column(r, K) and float(a[r].float().abs().max()) > 4 * float(rest)
    return a


def absmax_column(r, K):
    return (1024 + (37 + 16 * r) % 128, K - 1 - (r % 16), 5 + 16 * r, (2048 if K > 2048 else 1024) + 99 - r)[r % 4]


@functools.lru_cache(maxsize=None)
def quant_codepoint_rows(e):
    """every finite bf16 value with |x| <= 448, times 2^e (where that is a bf16 again: all of them for e >= 0), laid out in rows
    of CODEPOINT_K that each hold 448 x 2^e once, at a column that moves with the row: the scale is exactly 2^e"""
    v = bf16_upto_448().float() * 2.0 ** e
    v = v[v.to(BF).float() == v]
    assert e < 0 or v.numel() == 34754
    per = CODEPOINT_K - 1
    rows = -(-v.numel() // per)
    body = torch.zeros(rows * per)
    body[:v.numel()] = v
    a = torch.zeros(rows, CODEPOINT_K)
    for r in range(rows):
        k = (r * 131 + 1030) % CODEPOINT_K
        a[r, :k], a[r, k], a[r, k + 1:] = body[r * per:r * per + k], 448.0 * 2.0 ** e, body[r * per + k:(r + 1) * per]
    a = a.to(BF)
    assert torch.equal(a.float().abs().amax(1), torch.full((rows,), 448.0 * 2.0 ** e))
    return a


# --------------------------------------------------------------------------------------------------------------- comparisons
def mismatches(got, want_, n=6):
    """'' when got == want bit for bit; else gemm_probes.mismatches with the 128 x 128 tiles, and for the first n wrong elements
    their tile, the band of 8 tile rows the tile order walks, and the position inside the tile"""
    msg = G.mismatches(got, want_, tile=(BM, BN), n=n)
    if not msg or got.shape != want_.shape:
        return msg
    bad = (got != want_).nonzero()[:n]
    at = [f"({int(m)}, {int(c)}): tile ({int(m) // BM}, {int(c) // BN}) band {int(m) // BM // BAND} at ({int(m) % BM}, {int(c) % BN})"
          for m, c in bad]
    return msg + "; where: " + "; ".join(at)


def sentinel_buffer(M, N, device="cpu", extra=0):
    """(buffer [M + 2, N + 2 GUARD + extra] filled with SENTINEL, its view [M, N]): ldc > N, 16-byte aligned"""
    buf = torch.full((M + 2, N + 2 * GUARD + extra), SENTINEL, dtype=BF, device=device)
    return buf, buf[1:M + 1, GUARD:GUARD + N]


def buffer_mismatches(host_buf, want_):
    """'' when the whole buffer, sentinels included, is what a correct run leaves (torch.equal); else the report"""
    M, N = want_.shape
    full = torch.full_like(host_buf, SENTINEL)
    full[1:M + 1, GUARD:GUARD + N] = want_
    if torch.equal(host_buf, full):
        return ""
    msg = mismatches(host_buf[1:M + 1, GUARD:GUARD + N], want_)
    return msg or "store outside the output view (buffer coordinates, guards included): " + G.mismatches(host_buf, full)


def byte_buffer(M, K, device="cpu", extra=64):
    """(uint8 buffer [M, K + extra] filled with SENTINEL_CODE, its view [M, K]): ldq > K"""
    buf = torch.full((M, K + extra), SENTINEL_CODE, dtype=torch.uint8, device=device)
    return buf, buf[:, :K]


def gelu_judge(got, x):
    """the bars of test_gemm_epilogue_activations_on_every_bf16_code_point for the bf16 output `got` of the tanh GELU on the
    exact pre-activation x (float64): returns (largest distance from the float64 definition rounded to bf16, in bf16 ulps of the
    reference; share of exactly equal points) over the finite points, after asserting NaN -> NaN and +inf -> +inf"""
    got, x = got.float().flatten(), x.double().flatten()
    ref = gelu_ref(x)
    assert bool(torch.isnan(got[torch.isnan(x)]).all()), "NaN must stay NaN"
    assert bool((got[x == float("inf")] == float("inf")).all()), "+inf must go to +inf"
    r16 = ref.to(BF).float()
    ok = torch.isfinite(x) & torch.isfinite(r16) & ((x.abs() >= 2.0 ** -120) | (x == 0))
    ulp = torch.maximum(r16.abs(), torch.tensor(2.0 ** -100)).log2().floor().exp2() * 2.0 ** -7
    d = ((got - r16).abs() / ulp)[ok]
    return float(d.max()), float((d == 0).float().mean())


GELU_MAX_ULP, GELU_MIN_EQUAL = 1.0, 0.99


def old_bars_accept(out, ref, rel_bar):
    """the pair of bars test_random_operands_under_every_epilogue ends in, as a predicate: rel-L2 against the f32 reference under
    its bar and at least 99 % of the elements within 1 bf16 ulp"""
    rel = float((out.float() - ref).norm() / ref.norm())
    within = float(((G._ordered(out) - G._ordered(ref.to(BF))).abs() <= 1).float().mean())
    return rel < rel_bar and within >= 0.99


# ------------------------------------------------------------------------------------------------ the cases of the GPU suite
EDGE_MS, EDGE_NS, EDGE_KS = (1, 127, 128, 129, 257), (16, 112, 128, 144, 272), (128, 384, 1152)
LONG_K = (130, 272, 4096)
ORDER_MS, ORDER_NS, ORDER_K = (1025, 1153, 2177), (16, 272), 128        # tiles_m 9, 10, 17 x tiles_n 1, 3
ABI = (129, 144, 384)             # through the C entry point with ldw > K and ldr != ldc
# (epilogue, per-row sw, bias present, gate_res in place)
VARIANTS = tuple((e, p, b, i) for e in ("bias", "gelu", "gate_res") for p in (True, False) for b in (True, False)
                 for i in ((False, True) if e == "gate_res" else (False,)))


def edge_cases():
    return [(M, N, K) for M in EDGE_MS for N in EDGE_NS for K in EDGE_KS] + [LONG_K]


def order_cases():
    return [(M, N, ORDER_K) for M in ORDER_MS for N in ORDER_NS]


def all_fixed_cases():
    """every (M, N, K) the GPU file compares exactly with the fixed-point family, for the host tests"""
    return sorted(set(edge_cases() + order_cases() + [ABI, NAN_SHAPE]))


def case_id(c):
    return "-".join(str(v) for v in c)
