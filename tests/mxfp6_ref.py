"""The MXFP6 format of the opt-in fp6 compute path (csrc/fp8_quant.h, ops.quant_blocks_mxfp6, ops.gemm_mxfp6), restated in torch on the
CPU from the OCP definition, never from a kernel.

Codes: OCP e2m3, 6 bits = sign << 5 | exp << 3 | man, bias 1: exp = 0 is man / 8, otherwise (1 + man / 8) 2^(exp - 1); the magnitudes
MAGS = 0, 0.125 .. 0.875, 1 .. 1.875, 2 .. 3.75, 4 .. 7.5 are indexed by the low five bits.  Packing: a row of K codes is 3 K / 4 bytes,
block b is bytes 24 b .. 24 b + 23, and code j of the block is bits 6 j .. 6 j + 5 of the block's 192-bit little-endian integer (so four
codes fill three bytes).  Scales: one e8m0 byte per 32 consecutive k.  Per block of 32 consecutive bf16 values of one row (blocks
aligned to 32 columns):

    amax = max |x|, E = its unbiased float32 exponent, man = its 23 mantissa bits
    e    = clamp(E - 2 + (man > 0x700000), -126, 127), 0 for a zero block          (7.5 = 1.875 x 2^2: no element clips)
    byte = e + 127                                                                  (127 for a zero block, never 255)
    code = e2m3_rne(clamp(x * 2^-e, -7.5, 7.5))   nearest, ties to the even code; the sign bit of x is kept, also on a zero magnitude

Also the planted rows the host and GPU tests share, the float64 reference of the GEMM, the one-hot lane-map probe with its wrong
permutations, and the exact fixed-point GEMM family (`Fixed`) with its integer exactness bound."""
import functools

import torch

from tests import gemm_probes as G

BF = torch.bfloat16
BLOCK = 32
BLOCK_BYTES = 24
MAGS = tuple(m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1) for e in range(4) for m in range(8))
VALUES = torch.tensor(MAGS + tuple(-v for v in MAGS), dtype=torch.float64)          # value of code c; code 32 is -0
_POS = torch.tensor(MAGS, dtype=torch.float64)
TOP = 7.5
assert MAGS[0] == 0 and MAGS[7] == 0.875 and MAGS[8] == 1 and MAGS[15] == 1.875 and MAGS[16] == 2 and MAGS[23] == 3.75 and MAGS[31] == TOP
assert all(b > a for a, b in zip(MAGS, MAGS[1:]))


# ---- the format -----------------------------------------------------------------------------------------------------------------
def scale_bytes(amax: torch.Tensor) -> torch.Tensor:
    """float32 amax >= 0 -> the e8m0 scale byte (uint8), by integer arithmetic on the float's bits"""
    assert amax.dtype == torch.float32 and bool((amax >= 0).all()) and bool(torch.isfinite(amax).all())
    bits = amax.contiguous().view(torch.int32).to(torch.int64)
    E = (bits >> 23) - 127                     # a float32 subnormal (every bf16 subnormal is one) has the exponent field 0
    man = bits & 0x7FFFFF
    e = (E - 2 + (man > 0x700000).to(torch.int64)).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return (e + 127).to(torch.uint8)


def e2m3_nearest(y: torch.Tensor, tie: str = "even") -> torch.Tensor:
    """codes (uint8, 0..63) of the nearest e2m3 value of y (|y| <= 7.5), from the definition: a tie goes to the even code (the code's
    last bit is the last mantissa bit), the sign bit is kept, also of a result that rounds to zero.  tie = 'away' is the host tests'
    mutant."""
    mag = y.double().abs()
    assert float(mag.max()) <= TOP
    hi = torch.searchsorted(_POS, mag.contiguous()).clamp(max=31)               # the first value >= |y|
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = mag - _POS[lo], _POS[hi] - mag
    tie_up = (hi % 2 == 0) if tie == "even" else torch.ones_like(hi, dtype=torch.bool)
    idx = torch.where((dhi < dlo) | ((dhi == dlo) & tie_up), hi, lo)
    return (idx + 32 * torch.signbit(y).long()).to(torch.uint8)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [M, K] (0..63) -> bytes [M, 3 K / 4]: bits 6 j .. 6 j + 5 of a block's little-endian 192-bit integer hold code j, so
    codes 4 i .. 4 i + 3 are the 24-bit little-endian integer in bytes 3 i .. 3 i + 2"""
    assert codes.dtype == torch.uint8 and int(codes.max()) <= 63 and codes.shape[1] % BLOCK == 0
    c = codes.long().view(codes.shape[0], -1, 4)
    v = c[..., 0] | c[..., 1] << 6 | c[..., 2] << 12 | c[..., 3] << 18
    return torch.stack([v & 255, (v >> 8) & 255, v >> 16], dim=-1).to(torch.uint8).view(codes.shape[0], -1).contiguous()


def unpack(q: torch.Tensor) -> torch.Tensor:
    """bytes [M, 3 K / 4] -> codes uint8 [M, K]"""
    b = q.long().view(q.shape[0], -1, 3)
    v = b[..., 0] | b[..., 1] << 8 | b[..., 2] << 16
    return torch.stack([(v >> s) & 63 for s in (0, 6, 12, 18)], dim=-1).to(torch.uint8).view(q.shape[0], -1)


def quant_blocks_ref(a: torch.Tensor, tie: str = "even"):
    """bf16 [M, K] (K % 32 == 0) -> (packed codes uint8 [M, 3 K / 4], scale bytes uint8 [M, K / 32])"""
    assert a.dtype == BF and a.dim() == 2 and a.shape[1] % BLOCK == 0
    M, K = a.shape
    x = a.float().view(M, K // BLOCK, BLOCK)
    sb = scale_bytes(x.abs().amax(dim=2))
    inv = torch.exp2((127 - sb.to(torch.int64)).double()).float()          # 2^-e: |e| <= 126, a normal float32
    assert bool(torch.isfinite(inv).all()) and bool((inv > 0).all())
    y = x * inv.unsqueeze(2)                                               # exact: a power-of-two factor, float32 subnormals kept
    y = torch.minimum(torch.maximum(y, torch.full_like(y, -TOP)), torch.full_like(y, TOP))
    return pack(e2m3_nearest(y.reshape(M, K), tie)), sb


def values_of(q: torch.Tensor) -> torch.Tensor:
    """float64 values of packed codes, without the scales: [M, K]"""
    return VALUES[unpack(q).long()]


def dequant(q: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """float64 values of MXFP6 (packed codes, scale bytes)"""
    M, K = q.shape[0], q.shape[1] // 3 * 4
    v = values_of(q).view(M, K // BLOCK, BLOCK)
    return (v * torch.exp2(sb.double() - 127).unsqueeze(2)).reshape(M, K)


def gemm_ref(qa, sa, qw, sw, bias=None):
    """float64: sum_k value(a[m, k]) 2^(sa[m, k / 32] - 127) value(w[n, k]) 2^(sw[n, k / 32] - 127) (+ bias[n])"""
    y = dequant(qa, sa) @ dequant(qw, sw).T
    return y if bias is None else y + bias.double().view(1, -1)


# ---- planted rows ----------------------------------------------------------------------------------------------------------------
def _const_block(v, rest=0.0):
    b = torch.full((BLOCK,), float(rest))
    b[7] = float(v)
    return b


# (name, the 32 values of the block, expected scale byte).  By hand: 7.5 x 2^5 = 240 = 1.875 x 2^7 has E = 7 and man = 0x700000, not
# above it: e = 5, byte 132.  The next bf16 above 240 is 241 (8 significant bits: 11110001b): man > 0x700000, e = 6, byte 133, and
# 241 / 64 = 3.765625 rounds to 3.75.  7.5 x 2^-9: E = -7, e = -9, byte 118.  bf16 max = 1.9921875 x 2^127: E = 127, man = 0x7f0000 >
# 0x700000, e = 126, byte 253.  2^-133: E = -133 (the exponent field is 0, so the integer formula gives -127 - 2, clamped), e = -126,
# byte 1, and 2^-133 x 2^126 = 2^-7 is below half of 0.125: code 0.
PLANTS = (("zero", _const_block(0.0), 127),
          ("7.5 x 2^5", _const_block(TOP * 32, rest=3.0), 132),
          ("the next bf16 above 7.5 x 2^5", _const_block(-241.0, rest=3.0), 133),
          ("7.5 x 2^-9", _const_block(TOP * 2.0 ** -9, rest=2.0 ** -12), 118),
          ("bf16 max", _const_block(float(torch.finfo(BF).max), rest=1.0), 253),
          ("2^-133 (bf16 subnormal)", _const_block(2.0 ** -133), 1))


@functools.lru_cache(maxsize=None)
def planted_rows(K=256):
    """bf16 [len(PLANTS), K]: row r holds plant r in block r mod K/32 and small integers x 2^-20 elsewhere, so the other blocks
    of the row have scales of their own"""
    g = torch.Generator().manual_seed(4242)
    a = (torch.randint(-8, 9, (len(PLANTS), K), generator=g).float() * 2.0 ** -20)
    for r, (_, blk, _) in enumerate(PLANTS):
        b = r % (K // BLOCK)
        a[r, BLOCK * b:BLOCK * (b + 1)] = blk
    assert torch.equal(a.to(BF).float(), a), "planted values must be bf16"
    return a.to(BF)


def planted_bytes(K=256):
    """[(row, block, expected scale byte)] of `planted_rows`"""
    return [(r, r % (K // BLOCK), want) for r, (_, _, want) in enumerate(PLANTS)]


CODE_EXPONENTS = (0, 6, -4)


def _code_block(b):
    """the 32 codes of block b of `every_code_rows`: the non-negative codes in even blocks, the negative ones (-0 included) in odd
    blocks, rotated by the block index; either half holds +-7.5"""
    return (torch.arange(32) + 32 * (b & 1)).roll(3 * b + 1)


@functools.lru_cache(maxsize=None)
def every_code_rows(K=256):
    """bf16 [3, K]: row r = every e2m3 value (64 codes, -0 included, 32 to a block) times 2^CODE_EXPONENTS[r], rotated by the block
    index; each block holds 7.5 x 2^e or its negative: the block's scale is exactly 2^e and its codes are the values' own codes"""
    nb = K // BLOCK
    assert nb % 2 == 0
    row = torch.cat([VALUES[_code_block(b)].float() for b in range(nb)])
    a = torch.stack([row * 2.0 ** e for e in CODE_EXPONENTS])
    assert torch.equal(a.to(BF).float(), a) and int(torch.signbit(a).sum()) == 3 * (nb // 2) * 32
    return a.to(BF)


def every_code_want(K=256):
    """(packed codes, scale bytes) `every_code_rows` must quantise to, written down without the quantiser"""
    nb = K // BLOCK
    codes = torch.cat([_code_block(b) for b in range(nb)]).to(torch.uint8)
    sb = torch.tensor([[127 + e] * nb for e in CODE_EXPONENTS], dtype=torch.uint8)
    return pack(codes.repeat(3, 1)), sb


# every midpoint of the grid and the code it rounds to: the even one of its two neighbours
TIES = tuple(((MAGS[i] + MAGS[i + 1]) / 2, i if i % 2 == 0 else i + 1) for i in range(31))


@functools.lru_cache(maxsize=None)
def tie_row(K=128):
    """bf16 [1, K]: an even block holds the 31 midpoints and 7.5, an odd block their negatives and -7.5 (so every scale is 2^0), at
    positions that move with the block; returns (row, the values each element must round to)"""
    a, want = torch.zeros(1, K), torch.zeros(1, K)
    for b in range(K // BLOCK):
        sign = -1.0 if b & 1 else 1.0
        at = (torch.arange(32) * 5 + 3 * b) % BLOCK                # a permutation of the 32 positions (5 is odd)
        a[0, BLOCK * b + at] = sign * torch.tensor([v for v, _ in TIES] + [TOP])
        want[0, BLOCK * b + at] = sign * torch.tensor([MAGS[c] for _, c in TIES] + [TOP])
    assert torch.equal(a.to(BF).float(), a)
    return a.to(BF), want


@functools.lru_cache(maxsize=None)
def decade_rows(M=16, K=256, seed=7):
    """random bf16 rows whose blocks span 60 decades: normal values times 10^u, u uniform in [-30, 30] per block"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K // BLOCK, BLOCK, generator=g).double()
    u = torch.rand(M, K // BLOCK, 1, generator=g).double() * 60 - 30
    return (x * 10.0 ** u).float().reshape(M, K).to(BF)


@functools.lru_cache(maxsize=None)
def every_bf16_rows(e=None, K=256):
    """Every finite bf16 bit pattern (65 280, -0 and the subnormals included) through the quantiser.  e = None: in ascending order
    of the bit pattern, so a block holds neighbours of one binade and takes its own scale — every scale byte 1 .. 253 occurs.
    e = an exponent: the patterns with |x| <= 7.5 x 2^e, 31 to a block, each block also holding 7.5 x 2^e at a position that moves with
    the block, so the scale is exactly 2^e and every value down to the subnormals meets the rounding at that one scale."""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = x[torch.isfinite(x.float())]
    assert x.numel() == 65280
    if e is None:
        return x.view(-1, K)
    top = TOP * 2.0 ** e
    v = x.float()
    v = v[v.abs() <= top]
    nb = -(-v.numel() // 31)
    body = torch.zeros(nb * 31)
    body[:v.numel()] = v
    blocks = torch.empty(nb, BLOCK)
    for b in range(nb):
        at = (5 * b + 3) % BLOCK
        blocks[b] = torch.cat([body[31 * b:31 * b + at], torch.tensor([top]), body[31 * b + at:31 * (b + 1)]])
    pad = -nb % (K // BLOCK)
    blocks = torch.cat([blocks, torch.zeros(pad, BLOCK)])
    a = blocks.view(-1, K)
    assert torch.equal(a.to(BF).float(), a)
    return a.to(BF)


@functools.lru_cache(maxsize=None)
def random_rows(M, K, seed=11):
    g = torch.Generator().manual_seed(seed + 1000 * M + K)
    return torch.randn(M, K, generator=g).to(BF)


# ---- the lane-map probe ------------------------------------------------------------------------------------------------------------
# M = N = 128, K = 512: 16 blocks of 32 k, four K-tiles of the kernel, two k-steps each, two lane halves per k-step.  Row m of A holds
# ONE non-zero per block b, at k = 32 b + pos(m, b), with a code that cycles through the 62 non-zero codes by (m, b); row n of W holds
# ONE non-zero per block at pos(n, b).  pos(m, b) == pos(n, b) exactly when (m - n) % 32 == 0, so C[m, n] is a sum of 16 single
# products for those pairs and 0 elsewhere, and every position of a block is hit by some row.  The scale bytes differ from block to
# block and between the operands (A: 126 .. 128 by block and row, W: 124 .. 125), so the products of a sum have weights of their own;
# a product of two values in eighths is below 2^12 units, the weights span 3 bits and the sum of 16 another 4, so every float32 partial
# sum is exact in any order (`span_log2`, asserted below gemm_probes.SPAN_BITS).
LANE = (128, 128, 512)
NONZERO = torch.tensor([c for c in range(64) if c & 31], dtype=torch.uint8)          # the 62 codes with a non-zero value


class LaneMap:
    def __init__(self):
        M, N, K = LANE
        nb = K // BLOCK
        m, n, b = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(nb).view(1, -1)
        self.ca, self.cw = torch.zeros(M, K, dtype=torch.uint8), torch.zeros(N, K, dtype=torch.uint8)
        pa, pw = (m * 5 + b * 7) % BLOCK, (n * 5 + b * 7) % BLOCK
        self.ca[m.expand(M, nb), BLOCK * b + pa] = NONZERO[(m * 3 + b) % 62]
        self.cw[n.expand(N, nb), BLOCK * b + pw] = NONZERO[(n * 5 + 2 * b + 1) % 62]          # asymmetric: another cycle than A's
        self.sa = (126 + (b + m) % 3).to(torch.uint8)
        self.sw = (124 + (b + n) % 2).to(torch.uint8)
        # conditions: one non-zero per block and row, all 32 positions and all 62 codes in use, A / W scales differ in every block
        for c in (self.ca, self.cw):
            assert bool(((c & 31) != 0).view(M, nb, BLOCK).sum(2).eq(1).all())
            assert set(c[c != 0].tolist()) == set(NONZERO.tolist())
        assert pa.unique().numel() == BLOCK and bool((self.sa != self.sw).all())
        assert bool((self.sa[:, 1:] != self.sa[:, :-1]).all()) and bool((self.sw[:, 1:] != self.sw[:, :-1]).all())

    def ref(self, qa=None, sa=None, qw=None, sw=None):
        return gemm_ref(pack(self.ca) if qa is None else qa, self.sa if sa is None else sa,
                        pack(self.cw) if qw is None else qw, self.sw if sw is None else sw)

    def span_log2(self):
        """log2 of the largest sum of |products| in units of the smallest product weight 2^(126 + 124 - 254 - 6), in int64"""
        va, vw = (VALUES[self.ca.long()].abs() * 8).long(), (VALUES[self.cw.long()].abs() * 8).long()      # eighths
        M, N, K = LANE
        ua = (va.view(M, -1, BLOCK) * (1 << (self.sa.long() - 126)).unsqueeze(2)).reshape(M, K)
        uw = (vw.view(N, -1, BLOCK) * (1 << (self.sw.long() - 124)).unsqueeze(2)).reshape(N, K)
        return float((ua @ uw.T).max().double().log2())

    def want(self):
        ref = self.ref()
        assert self.span_log2() < G.SPAN_BITS and torch.equal(ref.float().double(), ref)
        return ref.float().to(BF)

    def mutants(self):
        """{name: the float64 result of a kernel with ONE wrong decision}; each must differ from `ref()` (asserted by the tests)"""
        M, N, K = LANE
        p = lambda c: pack(c.contiguous())                                                     # noqa: E731
        rev4 = lambda c: c.view(-1, K // 4, 4).flip(2).reshape(-1, K)                          # noqa: E731 big-endian groups of four codes
        rev32 = lambda c: c.view(-1, K // 32, 32).flip(2).reshape(-1, K)                       # noqa: E731 the block read from the top bit down
        half = lambda c: c.view(-1, K // 64, 2, 32).flip(2).reshape(-1, K)                     # noqa: E731 blocks b and b ^ 1 swapped, A only
        pair = lambda c: c.view(-1, K // 128, 2, 2, 32).flip(2).reshape(-1, K)                 # noqa: E731 blocks b and b ^ 2 swapped, A only
        nxt = lambda s: s.roll(1, dims=1)                                                      # noqa: E731 scale of the block before
        return {"code order inside three bytes": self.ref(qa=p(rev4(self.ca))),
                "code order inside the 24 bytes": self.ref(qa=p(rev32(self.ca))),
                "lane halves of a k-step (blocks b, b ^ 1)": self.ref(qa=p(half(self.ca))),
                "lane halves of a k-step (blocks b, b ^ 2)": self.ref(qa=p(pair(self.ca))),
                "swapped A/B scales": self.ref(sa=self.sw[:M], sw=self.sa[:N]),
                "scale of the neighbouring block": self.ref(sa=nxt(self.sa)),
                "block boundary shifted by 8 bytes": self.ref(qa=pack(self.ca).roll(8, dims=1))}


@functools.lru_cache(maxsize=None)
def lane_map():
    return LaneMap()


# ---- the exact fixed-point GEMM family ---------------------------------------------------------------------------------------------
# Values from EIGHTHS / 8 (every exponent of the format, every mantissa bit, the subnormals, 7.5; small values more often, which keeps
# the sums short), either sign; scale bytes 128 .. 129 on A and 127 .. 128 on W, drawn per block: every product is an integer times
# 2^(sa + sw - 254 - 6) with sa + sw - 254 in 1 .. 3, so every partial sum in any order is a multiple of 2^-5.  bias on the grid 2^-4,
# the residual on 2^-3, gates from gemm_probes.GATES.  `span_log2` bounds sum |a| |w| 2^(..) (+ |bias|) (x |gate| + |R|) in units of the
# finest grid of the element's final sum, in int64 / float64, and the tests assert it below gemm_probes.SPAN_BITS: every float32
# intermediate is exact, in any order, with or without FMA contraction.  The ONLY rounding left is the bf16 store.  The scale bytes sit
# above 127 so that the dot products of the shortest K spread over hundreds: the GELU epilogue shared with the fp8 and fp4 kernels
# flushes a result that is a bf16 subnormal (pre-activations near -10.2) to zero, which gemm_fp8_probes.gelu_judge counts as unequal,
# and a family whose pre-activations crowd that window would test the activation's corner instead of the product
# (`gelu_subnormal_share`, bounded in tests/test_mxfp6_host.py).
EIGHTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 18, 22, 30, 32, 36, 60)
SA_BYTES, SW_BYTES = (128, 129), (127, 128)
GB, GR = 2.0 ** -4, 2.0 ** -3
GRID_LOG2 = -5                                              # of the dot product: 2^(128 - 127 + 127 - 127) / 64
K_TILE = 128                                                # codes of a K-tile of gemm_mxfp6_kernel
FIXED_MS, FIXED_NS, FIXED_KS = (1, 127, 129, 300), (16, 144, 272), (K_TILE, 2 * K_TILE, 5 * K_TILE)
BAND_CASE = (1100, 144, K_TILE)                             # 9 tile rows: more than one band of the tile order
SENTINEL, GUARD = 2.0 ** 30, 8
assert all(v / 8 in MAGS for v in EIGHTHS)


def fixed_cases():
    return [(M, N, K) for M in FIXED_MS for N in FIXED_NS for K in FIXED_KS] + [BAND_CASE]


class Fixed:
    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        g = torch.Generator().manual_seed(G._seed(M, N, K, 600))
        vals = torch.tensor(EIGHTHS)

        def draw(rows):
            return vals[torch.randint(0, len(EIGHTHS), (rows, K), generator=g)] * (1 - 2 * torch.randint(0, 2, (rows, K), generator=g))

        self.a, self.w = draw(M), draw(N)                                    # int64 values in eighths
        self.sa = torch.tensor(SA_BYTES)[torch.randint(0, 2, (M, K // BLOCK), generator=g)].to(torch.uint8)
        self.sw = torch.tensor(SW_BYTES)[torch.randint(0, 2, (N, K // BLOCK), generator=g)].to(torch.uint8)
        self.qa, self.qw = pack(self.codes(self.a)), pack(self.codes(self.w))
        col = torch.arange(N)
        self.bias = (((col * 37 + 11) % 129) - 64).float() * GB
        gi = (col * 3 + col // 4) % 8
        self.gate, self.gate_lsb = torch.tensor(G.GATES)[gi], torch.tensor(G.GATE_LSB)[gi]
        self.res = ((torch.randint(1, 129, (M, N), generator=g).cumsum(0) % 129) - 64).float() * GR
        assert torch.equal(self.bias.to(BF).float(), self.bias) and torch.equal(self.res.to(BF).float(), self.res)
        assert bool((self.bias[1:] != self.bias[:-1]).all()) and bool((self.gate[1:] != self.gate[:-1]).all())

    @staticmethod
    def codes(v):
        """integers in eighths -> e2m3 codes (a zero keeps the sign +)"""
        idx = torch.searchsorted(_POS, v.abs().double() / 8)
        assert torch.equal(_POS[idx] * 8, v.abs().double())
        return (idx + 32 * (v < 0).long()).to(torch.uint8)

    def _shifted(self, v, sb, lo):
        """integers v [R, K] times 2^(sb - lo) per block: int64"""
        R = v.shape[0]
        return (v.view(R, -1, BLOCK) * (1 << (sb.long() - lo)).unsqueeze(2)).reshape(R, self.K)

    @functools.cached_property
    def acc_units(self):
        """the dot products in units of 2^GRID_LOG2: exact int64"""
        return self._shifted(self.a, self.sa, SA_BYTES[0]) @ self._shifted(self.w, self.sw, SW_BYTES[0]).T

    @functools.cached_property
    def mag_units(self):
        return self._shifted(self.a.abs(), self.sa, SA_BYTES[0]) @ self._shifted(self.w.abs(), self.sw, SW_BYTES[0]).T

    def ref(self, epilogue="bias", bias=True):
        """the exact float64 result of the bias or gate_res epilogue, or the pre-activation of gelu"""
        y = self.acc_units.double() * 2.0 ** GRID_LOG2
        if bias:
            y = y + self.bias.double()
        if epilogue == "gate_res":
            return self.res.double() + self.gate.double() * y
        return y

    def span_log2(self, epilogue="bias", bias=True):
        """log2 of the largest (sum of magnitudes) / (finest grid of the element's final sum); the dot product's part in int64"""
        g0 = 2.0 ** GRID_LOG2                                                # finer than GB and GR
        mag = self.mag_units.double() * g0                                   # exact: below 2^53 units
        if bias:
            mag = mag + self.bias.double().abs()
        grid = torch.full((self.N,), g0, dtype=torch.float64)
        if epilogue == "gate_res":
            mag = mag * self.gate.double().abs() + self.res.double().abs()
            grid = (grid * self.gate_lsb.double()).clamp_max(GR)
        return float((mag / grid).max().log2())

    def gelu_subnormal_share(self):
        """the share of pre-activations whose tanh GELU (float64, rounded to bf16) is a non-zero bf16 subnormal"""
        from tests import gemm_fp8_probes as P
        r16 = P.gelu_ref(self.ref("bias").flatten()).to(BF).float()
        return float(((r16 != 0) & (r16.abs() < 2.0 ** -126)).float().mean())

    def want(self, epilogue="bias", bias=True):
        assert self.span_log2(epilogue, bias) < G.SPAN_BITS
        ref = self.ref(epilogue, bias)
        f = ref.float()
        assert torch.equal(f.double(), ref) and float(ref.abs().max()) <= SENTINEL / 4
        return f.to(BF)


@functools.lru_cache(maxsize=None)
def fixed_point(M, N, K):
    return Fixed(M, N, K)


def sentinel_buffer(M, N, device="cpu"):
    """(buffer [M + 2, N + 2 GUARD] filled with SENTINEL, its view [M, N]): ldc > N, 16-byte aligned"""
    buf = torch.full((M + 2, N + 2 * GUARD), SENTINEL, dtype=BF, device=device)
    return buf, buf[1:M + 1, GUARD:GUARD + N]


def wide(t: torch.Tensor, extra: int, fill: int = 0x77):
    """a copy of uint8 `t` [R, C] inside a buffer whose rows are `extra` bytes wider (filled with `fill`): a stride wider than the row"""
    buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=torch.uint8, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]
