"""Exact probes of the run-time LoRA form of the FP8 GEMM (gemm_fp8.hip: apexmi_gemm_fp8_lora; ops.gemm_fp8(lora_t=, lora_B=) and
the fp8-LoRA route of ops.gemm), on top of tests/gemm_fp8_probes.py: operands whose correct result is known bit for bit and the
references, written from the documented contract, never from a kernel:

    acc = qa . qw^T;   acc = (acc * sa[m]) * sw[n];   acc += sum_r t[m, r] B'[n, r];   out = epi(acc + bias[n])

Pure torch on the CPU.  tests/test_gpu_gemm_fp8_lora.py feeds the operands to the kernel and compares whole sentinel-filled
buffers with torch.equal; tests/test_gemm_fp8_lora_host.py evaluates the conditions below for every case the GPU file runs and
shows that the comparison rejects single wrong decisions.

Fixed-point family.  The `Fixed` operands of a shape (gemm_fp8_probes.fixed_point) plus t [M, Rp] and B' [N, Rp] = integers in
[-4, 4] x 2^-2, so every product of the adapter term and every partial sum of it is a multiple of 2^-4.  Every element of t
differs from the one a row above; every element of B' differs from the one 1 row and the one 4 rows above (the rows of B' are the
output columns: a wrong column or a wrong clamp of a 4-column group reads another number).  The last 8 rank columns of both are
zero, as set_lora's padding leaves them.  `span_log2` adds sum |t| |B'| to the magnitude of gemm_fp8_probes.span_log2 and clamps
the grid to 2^-4; below 2^22 every float32 intermediate is exact in any order, and the only rounding is the bf16 store.

One-hot rank family.  All codes zero; t is one-hot per row, at rank index (37 m + 5) % Rp — the rows between them reach all 64
positions of a rank tile in both tiles of Rp = 128 — and B' is dense, +-1 or +-2 by a formula in (n, r): every output is exactly
ONE product t[m, hot(m)] B'[n, hot(m)].  This pins the bf16 operand lane map and the order of the rank tiles."""
import functools

import torch

from tests import gemm_probes as G
from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF, SPAN_BITS, GB, GR  # noqa: F401

GT = 2.0 ** -2            # grid of t and of B'
GA = GT * GT              # grid of the adapter sum
PAD = 8                   # zero rank columns at the end of t and B'

# (M, N, K, Rp): edge rows and columns behind one full tile; nk = 1 straight into two rank tiles; a 3 x 3 tile grid; the smallest
# legal problem
CASES = ((130, 144, 256, 64), (130, 144, 128, 128), (257, 272, 384, 128), (1, 16, 128, 64))
ONE_HOT = (130, 144, 128, 128)
# (epilogue, per-row sw, bias present): the eight exact variants, and the four gelu ones
EXACT_VARIANTS = P.EXACT_VARIANTS
GELU_VARIANTS = tuple(("gelu", p, b) for p in (True, False) for b in (True, False))


def case_id(c):
    return "-".join(str(v) for v in c)


class Lora:
    """t [M, Rp], lb [N, Rp]: bf16-exact float32 on the 2^-2 grid, for the Fixed operands `op`"""

    def __init__(self, op, Rp, salt=0):
        self.op, self.Rp, self.salt = op, Rp, salt
        M, N = op.M, op.N
        g = torch.Generator().manual_seed(G._seed(M, N, op.K, 900 + 16 * salt + Rp // 64))
        t = ((torch.randint(1, 9, (M, Rp), generator=g).cumsum(0) % 9) - 4).float() * GT
        d = torch.randint(0, 9, (N, Rp), generator=g)
        for n in range(1, N):
            while True:
                clash = d[n] == d[n - 1]
                if n >= 4:
                    clash |= d[n] == d[n - 4]
                if not bool(clash.any()):
                    break
                d[n] = torch.where(clash, (d[n] + 1) % 9, d[n])
        lb = (d - 4).float() * GT
        t[:, Rp - PAD:] = 0
        lb[:, Rp - PAD:] = 0
        self.t, self.lb = t, lb
        live = Rp - PAD
        for x in (t, lb):
            assert torch.equal(x.to(BF).float(), x) and float(x.abs().max()) <= 1.0
        assert M == 1 or bool((t[1:, :live] != t[:-1, :live]).all()), "every element of t must differ from the row above"
        assert bool((lb[1:, :live] != lb[:-1, :live]).all()) and bool((lb[4:, :live] != lb[:-4, :live]).all())

    @functools.cached_property
    def term(self):
        """sum_r t[m, r] B'[n, r] in float64: exact multiples of 2^-4"""
        return self.t.double() @ self.lb.double().T

    @functools.cached_property
    def mag(self):
        return self.t.double().abs() @ self.lb.double().abs().T


def pre_activation(lo, per_row=True, bias=True, term=None):
    """(qa . qw^T) sa[m] sw[n] + t . B'^T (+ bias[n]) in float64: exact"""
    y = P.pre_activation(lo.op, per_row, False) + (lo.term if term is None else term)
    return y + lo.op.bias.double() if bias else y


def gemm_ref(lo, epilogue="bias", per_row=True, bias=True, term=None):
    y = pre_activation(lo, per_row, bias, term)
    if epilogue == "gate_res":
        return lo.op.res.double() + lo.op.gate.double() * y
    assert epilogue == "bias", epilogue
    return y


def span_log2(lo, epilogue="bias", per_row=True, bias=True):
    """gemm_fp8_probes.span_log2 with the adapter term: log2 of the largest (sum of magnitudes) / grid over the outputs"""
    op = lo.op
    sw, sw_lsb = (op.sw, op.sw_lsb) if per_row else (op.sw_one, op.sw_one_lsb)
    mag = op.mag * op.sa.double().abs().view(-1, 1) * sw.double().abs().view(1, -1) + lo.mag
    grid = (op.sa_lsb.double().view(-1, 1) * sw_lsb.double().view(1, -1)).expand(op.M, op.N).clamp_max(GA)
    if bias:
        mag = mag + op.bias.double().abs()
        grid = grid.clamp_max(GB)
    if epilogue == "gate_res":
        mag = mag * op.gate.double().abs() + op.res.double().abs()
        grid = (grid * op.gate_lsb.double()).clamp_max(GR)
    return float((mag / grid).max().log2())


def tie_fractions(lo):
    return {v: G.tie_fraction(gemm_ref(lo, *v)) for v in EXACT_VARIANTS}


@functools.lru_cache(maxsize=None)
def fixed_point(M, N, K, Rp):
    """the adapter operands of one case: the first salt whose eight exact results all hold an exact tie of the bf16 rounding and
    whose adapter term is non-zero in every row and every column (conditions on the operands, evaluated on the CPU alone)"""
    op = P.fixed_point(M, N, K)
    for salt in range(4096):
        lo = Lora(op, Rp, salt)
        if min(tie_fractions(lo).values()) > 0 and bool((lo.term != 0).any(0).all()) and bool((lo.term != 0).any(1).all()):
            return lo
    raise AssertionError(f"no draw of {M}x{N}x{K} rank {Rp} holds a tie")


@functools.lru_cache(maxsize=None)
def want(M, N, K, Rp, epilogue="bias", per_row=True, bias=True):
    """expected bf16 output of one variant of one case, computed once and shared (callers do not modify it)"""
    lo = fixed_point(M, N, K, Rp)
    assert span_log2(lo, epilogue, per_row, bias) < SPAN_BITS
    return P.expected(gemm_ref(lo, epilogue, per_row, bias))


# ---------------------------------------------------------------------------------------------------------- one-hot rank family
def hot_rank(m, Rp):
    """rank index of the one non-zero of row m of t: 37 is a unit modulo 128"""
    return (m * 37 + 5) % Rp


def dense_b(n, r):
    """+-1 or +-2 by (n, r)"""
    mag = torch.where((n + 3 * r + (n * r) % 5) % 2 == 0, 1.0, 2.0)
    return torch.where((2 * n + r + (n * r) % 3) % 3 == 0, -mag, mag)


class OneHot:
    """t [M, Rp] one-hot rows with values (1 + m % 7) / 4, negative on every third row; lb [N, Rp] dense; all codes zero"""

    def __init__(self, M, N, K, Rp):
        self.M, self.N, self.K, self.Rp = M, N, K, Rp
        m = torch.arange(M)
        self.hot = hot_rank(m, Rp)
        self.t = torch.zeros(M, Rp)
        self.t[m, self.hot] = (1 + m % 7).float() * 0.25 * torch.where(m % 3 == 1, -1.0, 1.0)
        self.lb = dense_b(torch.arange(N).view(-1, 1), torch.arange(Rp).view(1, -1))
        g = torch.Generator().manual_seed(77)
        self.sa, self.sw = torch.tensor(P.SA)[P._walk(M, 1, 8, g)], torch.tensor(P.SW)[P._columns(N, 8, g)]
        assert int((self.t != 0).sum(1).min()) == 1 == int((self.t != 0).sum(1).max())
        assert (self.hot % 64).unique().numel() == 64 and set((self.hot // 64).tolist()) == set(range(Rp // 64))
        assert self.hot.unique().numel() == min(M, Rp)
        assert set(self.lb.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
        for x in (self.t, self.lb):
            assert torch.equal(x.to(BF).float(), x)

    def ref(self):
        """float64: exactly one product per output"""
        return self.t.double() @ self.lb.double().T


@functools.lru_cache(maxsize=None)
def one_hot():
    return OneHot(*ONE_HOT)


# ------------------------------------------------------------------------------- single wrong decisions (for the host tests)
def _shift_rows(x):
    """row r reads row r - 1 (row 0 reads itself)"""
    return torch.cat([x[:1], x[:-1]])


def mutants(lo, per_row=True, bias=True):
    """{name: float64 pre-epilogue result y of a kernel that takes ONE wrong decision}; the correct one is `pre_activation`"""
    op = lo.op
    t, lb = lo.t.double(), lo.lb.double()
    sw = (op.sw if per_row else op.sw_one).double().view(1, -1)
    scale = op.sa.double().view(-1, 1) * sw
    b = op.bias.double() if bias else torch.zeros(op.N, dtype=torch.float64)
    clamp = lb.clone()
    clamp[op.N - 4:] = lb[op.N - 8:op.N - 4]
    half = t.clone()
    half[:, lo.Rp - 64:] = 0
    return {
        "t a row above": op.acc * scale + _shift_rows(t) @ lb.T + b,
        "B' a row above": op.acc * scale + t @ _shift_rows(lb).T + b,
        "B' with a wrong 4-column clamp": op.acc * scale + t @ clamp.T + b,
        "last rank tile dropped": op.acc * scale + half @ lb.T + b,
        "scales on the adapter term too": (op.acc + lo.term) * scale + b,
        "adapter term omitted": op.acc * scale + b,
        "bias before the scales": (op.acc + b) * scale + lo.term,
    }


def changed(lo, y, per_row=True, bias=True):
    """number of elements of the expected bf16 buffer (bias epilogue) that the wrong result y changes"""
    return int((y.float().to(BF) != pre_activation(lo, per_row, bias).float().to(BF)).sum())
