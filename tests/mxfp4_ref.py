"""The MXFP4 format of the opt-in fp4 compute path (csrc/fp8_quant.h, ops.quant_blocks_mxfp4, ops.gemm_mxfp4), restated in torch on the
CPU from the documented definition, never from a kernel.

Codes: OCP e2m1, bit 3 = sign, the low three bits index MAGS = (0, 0.5, 1, 1.5, 2, 3, 4, 6); packed two to a byte as torch's
float4_e2m1fn_x2 does, byte j of a row = code[2 j] | code[2 j + 1] << 4.  Scales: one e8m0 byte per 32 consecutive k.  Per block of 32
consecutive bf16 values of one row (blocks aligned to 32 columns):

    amax = max |x|, E = its unbiased float32 exponent, man = its 23 mantissa bits
    e    = clamp(E - 2 + (man > 0x400000), -126, 127), 0 for a zero block          (6 = 1.5 x 2^2)
    byte = e + 127                                                                  (127 for a zero block, never 255)
    code = e2m1_rne(clamp(x * 2^-e, -6, 6))      nearest, ties to the even code; the sign bit of x is kept, also on a zero magnitude

Also the planted rows the host and GPU tests share, the float64 reference of the GEMM, the one-hot lane-map probe with its four
wrong permutations, and the exact fixed-point GEMM family (`Fixed`) with its integer exactness bound."""
import functools

import torch

from tests import gemm_probes as G

BF = torch.bfloat16
BLOCK = 32
MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
VALUES = torch.tensor(MAGS + tuple(-v for v in MAGS), dtype=torch.float64)          # value of code c; code 8 is -0
_POS = torch.tensor(MAGS, dtype=torch.float64)


# ---- the format -----------------------------------------------------------------------------------------------------------------
def scale_bytes(amax: torch.Tensor) -> torch.Tensor:
    """float32 amax >= 0 -> the e8m0 scale byte (uint8), by integer arithmetic on the float's bits"""
    assert amax.dtype == torch.float32 and bool((amax >= 0).all()) and bool(torch.isfinite(amax).all())
    bits = amax.contiguous().view(torch.int32).to(torch.int64)
    E = (bits >> 23) - 127                     # a float32 subnormal (every bf16 subnormal is one) has the exponent field 0
    man = bits & 0x7FFFFF
    e = (E - 2 + (man > 0x400000).to(torch.int64)).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return (e + 127).to(torch.uint8)


def e2m1_nearest(y: torch.Tensor, tie: str = "even") -> torch.Tensor:
    """codes (uint8, 0..15) of the nearest e2m1 value of y (|y| <= 6), from the definition: a tie goes to the even code (the code's
    last bit is the mantissa bit), the sign bit is kept, also of a result that rounds to zero.  tie = 'away' is the host tests' mutant."""
    mag = y.double().abs()
    assert float(mag.max()) <= 6
    hi = torch.searchsorted(_POS, mag.contiguous()).clamp(max=7)                # the first value >= |y|
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = mag - _POS[lo], _POS[hi] - mag
    tie_up = (hi % 2 == 0) if tie == "even" else torch.ones_like(hi, dtype=torch.bool)
    idx = torch.where((dhi < dlo) | ((dhi == dlo) & tie_up), hi, lo)
    return (idx + 8 * torch.signbit(y).long()).to(torch.uint8)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [M, K] (0..15) -> bytes [M, K / 2]: byte j = code[2 j] | code[2 j + 1] << 4"""
    assert codes.dtype == torch.uint8 and int(codes.max()) <= 15 and codes.shape[1] % 2 == 0
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack(q: torch.Tensor) -> torch.Tensor:
    """bytes [M, K / 2] -> codes uint8 [M, K]"""
    return torch.stack([q & 15, q >> 4], dim=-1).reshape(q.shape[0], 2 * q.shape[1])


def quant_blocks_ref(a: torch.Tensor, tie: str = "even"):
    """bf16 [M, K] (K % 32 == 0) -> (packed codes uint8 [M, K / 2], scale bytes uint8 [M, K / 32])"""
    assert a.dtype == BF and a.dim() == 2 and a.shape[1] % BLOCK == 0
    M, K = a.shape
    x = a.float().view(M, K // BLOCK, BLOCK)
    sb = scale_bytes(x.abs().amax(dim=2))
    inv = torch.exp2((127 - sb.to(torch.int64)).double()).float()          # 2^-e: |e| <= 126, a normal float32
    assert bool(torch.isfinite(inv).all()) and bool((inv > 0).all())
    y = x * inv.unsqueeze(2)                                               # exact: a power-of-two factor, float32 subnormals kept
    y = torch.minimum(torch.maximum(y, torch.full_like(y, -6.0)), torch.full_like(y, 6.0))
    return pack(e2m1_nearest(y.reshape(M, K), tie)), sb


def values_of(q: torch.Tensor) -> torch.Tensor:
    """float64 values of packed codes, without the scales: [M, K]"""
    return VALUES[unpack(q).long()]


def dequant(q: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """float64 values of MXFP4 (packed codes, scale bytes)"""
    M, K = q.shape[0], 2 * q.shape[1]
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


# (name, the 32 values of the block, expected scale byte)
PLANTS = (("zero", _const_block(0.0), 127),
          ("6 x 2^5", _const_block(6.0 * 32, rest=3.0), 132),
          ("6.25 x 2^5", _const_block(-6.25 * 32, rest=3.0), 133),
          ("6 x 2^-9", _const_block(6.0 * 2.0 ** -9, rest=2.0 ** -12), 118),
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


@functools.lru_cache(maxsize=None)
def every_code_rows(K=256):
    """bf16 [3, K]: row r = every e2m1 value (16 codes, -0 included) times 2^CODE_EXPONENTS[r] in every block, rotated by the block
    index, each block also holding 6 x 2^e: the block's scale is exactly 2^e and its codes are the values' own codes"""
    nb = K // BLOCK
    row = torch.zeros(K)
    for b in range(nb):
        blk = torch.cat([VALUES.float(), VALUES.float()]).roll(3 * b + 1)
        row[BLOCK * b:BLOCK * (b + 1)] = blk
    a = torch.stack([row * 2.0 ** e for e in CODE_EXPONENTS])
    assert torch.equal(a.to(BF).float(), a) and int(torch.signbit(a).sum()) == 3 * nb * 16
    return a.to(BF)


def every_code_want(K=256):
    """(packed codes, scale bytes) `every_code_rows` must quantise to, written down without the quantiser"""
    nb = K // BLOCK
    codes = torch.cat([torch.cat([torch.arange(16), torch.arange(16)]).roll(3 * b + 1) for b in range(nb)]).to(torch.uint8)
    sb = torch.tensor([[127 + e] * nb for e in CODE_EXPONENTS], dtype=torch.uint8)
    return pack(codes.repeat(3, 1)), sb


TIES = ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0))       # (value, what it rounds to)


@functools.lru_cache(maxsize=None)
def tie_row(K=64):
    """bf16 [1, K]: every block holds the seven ties with both signs, 6 (so the scale is 2^0) and zeros, at positions that move with
    the block; returns (row, the values each element must round to)"""
    a, want = torch.zeros(1, K), torch.zeros(1, K)
    for b in range(K // BLOCK):
        at = (torch.arange(15) * 2 + 3 * b) % BLOCK                # 15 distinct positions (a step of 2 inside 32, from 3 b)
        vals = [v for v, _ in TIES] + [-v for v, _ in TIES] + [6.0]
        to = [t for _, t in TIES] + [-t for _, t in TIES] + [6.0]
        a[0, BLOCK * b + at] = torch.tensor(vals)
        want[0, BLOCK * b + at] = torch.tensor(to)
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
    e = an exponent: the patterns with |x| <= 6 x 2^e, 31 to a block, each block also holding 6 x 2^e at a position that moves with
    the block, so the scale is exactly 2^e and every value down to the subnormals meets the rounding at that one scale."""
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF)
    x = x[torch.isfinite(x.float())]
    assert x.numel() == 65280
    if e is None:
        return x.view(-1, K)
    top = 6.0 * 2.0 ** e
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
# M = N = 128, K = 512: 16 blocks of 32 k, two K-tiles of the kernel, four k-steps each, two lane halves per k-step.  Row m of A holds
# ONE non-zero per block b, at k = 32 b + pos_a(m, b), with a value that cycles through the 14 non-zero codes by (m, b); row n of W holds
# ONE non-zero per block at pos_w(n, b).  pos_a(m, b) == pos_w(n, b) exactly when (m - n) % 32 == 0, so C[m, n] is a sum of 16 single
# products for those pairs and 0 elsewhere, and every position of a block is hit by some row.  The scale bytes differ per block and
# between the operands (A: 124 .. 131 by block and row, W: 123 .. 127), so the products of a sum have weights of their own; the
# weights span 11 bits, a product 6 and the sum of 16 another 4, so every float32 partial sum is exact in any order (`span_log2`).
LANE = (128, 128, 512)
NONZERO = torch.tensor([c for c in range(16) if c & 7], dtype=torch.uint8)          # the 14 codes with a non-zero value


class LaneMap:
    def __init__(self):
        M, N, K = LANE
        nb = K // BLOCK
        m, n, b = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(nb).view(1, -1)
        self.ca, self.cw = torch.zeros(M, K, dtype=torch.uint8), torch.zeros(N, K, dtype=torch.uint8)
        pa, pw = (m * 5 + b * 7) % BLOCK, (n * 5 + b * 7) % BLOCK
        self.ca[m.expand(M, nb), BLOCK * b + pa] = NONZERO[(m * 3 + b) % 14]
        self.cw[n.expand(N, nb), BLOCK * b + pw] = NONZERO[(n * 5 + 2 * b + 1) % 14]          # asymmetric: another cycle than A's
        self.sa = (124 + (b + m) % 8).to(torch.uint8)
        self.sw = (123 + (3 * b + n) % 5).to(torch.uint8)
        # conditions: one non-zero per block and row, all 32 positions and all 14 codes in use, A / W scales differ in every block
        for c in (self.ca, self.cw):
            assert bool(((c & 7) != 0).view(M, nb, BLOCK).sum(2).eq(1).all())
            assert set(c[c != 0].tolist()) == set(NONZERO.tolist())
        assert pa.unique().numel() == BLOCK and bool((self.sa != self.sw).any(1).all())
        assert bool((self.sa[:, 1:] != self.sa[:, :-1]).all()) and bool((self.sw[:, 1:] != self.sw[:, :-1]).all())

    def ref(self, ca=None, sa=None, cw=None, sw=None):
        return gemm_ref(pack(self.ca if ca is None else ca), self.sa if sa is None else sa,
                        pack(self.cw if cw is None else cw), self.sw if sw is None else sw)

    def span_log2(self):
        """log2 of the largest sum of |products| in units of the smallest product weight 2^(124 + 123 - 254), in int64"""
        va, vw = (VALUES[self.ca.long()].abs() * 2).long(), (VALUES[self.cw.long()].abs() * 2).long()      # halves
        M, N, K = LANE
        ua = (va.view(M, -1, BLOCK) * (1 << (self.sa.long() - 124)).unsqueeze(2)).reshape(M, K)
        uw = (vw.view(N, -1, BLOCK) * (1 << (self.sw.long() - 123)).unsqueeze(2)).reshape(N, K)
        return float((ua @ uw.T).max().double().log2())

    def want(self):
        ref = self.ref()
        assert self.span_log2() < G.SPAN_BITS and torch.equal(ref.float().double(), ref)
        return ref.float().to(BF)

    def mutants(self):
        """{name: the float64 result of a kernel with ONE wrong decision}; each must differ from `ref()` (asserted by the tests)"""
        M, N, K = LANE
        swap_nib = lambda c: c.view(-1, K // 2, 2).flip(2).reshape(-1, K)                      # noqa: E731 nibble order, A only
        half = lambda c: c.view(-1, K // 64, 2, 32).flip(2).reshape(-1, K)                     # noqa: E731 lane halves of a k-step, A only
        nxt = lambda s: s.roll(1, dims=1)                                                      # noqa: E731 scale of the block before
        return {"nibble order": self.ref(ca=swap_nib(self.ca)), "k-to-lane map": self.ref(ca=half(self.ca)),
                "swapped A/B scales": self.ref(sa=self.sw[:M], sw=self.sa[:N]), "scale of the wrong block": self.ref(sa=nxt(self.sa))}


@functools.lru_cache(maxsize=None)
def lane_map():
    return LaneMap()


# ---- the exact fixed-point GEMM family ---------------------------------------------------------------------------------------------
# Codes of the integers {0, +-1, +-2, +-3, +-4, +-6}; scale bytes 126 .. 128 on A and 125 .. 127 on W, drawn per block: every product is
# an integer times 2^(sa + sw - 254) with sa + sw - 254 in -3 .. 1, so every partial sum in any order is a multiple of 2^-3.  bias on
# the grid 2^-4, the residual on 2^-3, gates from gemm_probes.GATES.  `span_log2` bounds sum |a| |w| 2^(..) (+ |bias|) (x |gate| + |R|)
# in units of the finest grid, in int64, and the tests assert it below 2^22: every float32 intermediate is exact, in any order, with
# or without FMA contraction.  The ONLY rounding left is the bf16 store: expected = exact.float().to(bf16).
INTS = (0, 1, 2, 3, 4, 6)
SA_BYTES, SW_BYTES = (126, 127, 128), (125, 126, 127)
GB, GR = 2.0 ** -4, 2.0 ** -3
GRID_LOG2 = -3                                              # of the dot product: 2^(126 - 127 + 125 - 127)
FIXED_MS, FIXED_NS, FIXED_KS = (1, 127, 129, 300), (16, 144, 272), (256, 512, 1280)
BAND_CASE = (1100, 144, 256)                                # 9 tile rows: more than one band of the tile order
SENTINEL, GUARD = 2.0 ** 30, 8


def fixed_cases():
    return [(M, N, K) for M in FIXED_MS for N in FIXED_NS for K in FIXED_KS] + [BAND_CASE]


class Fixed:
    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        g = torch.Generator().manual_seed(G._seed(M, N, K, 400))
        ints = torch.tensor(INTS)

        def draw(rows):
            v = ints[torch.randint(0, 6, (rows, K), generator=g)] * (1 - 2 * torch.randint(0, 2, (rows, K), generator=g))
            return v

        self.a, self.w = draw(M), draw(N)                                    # int64 values
        self.sa = torch.tensor(SA_BYTES)[torch.randint(0, 3, (M, K // BLOCK), generator=g)].to(torch.uint8)
        self.sw = torch.tensor(SW_BYTES)[torch.randint(0, 3, (N, K // BLOCK), generator=g)].to(torch.uint8)
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
        idx = torch.tensor([0, 2, 4, 5, 6, 0, 7])[v.abs()]                    # value -> code of its magnitude (5 does not occur)
        return (idx + 8 * (v < 0).long()).to(torch.uint8)

    def _shifted(self, v, sb, lo):
        """integers v [R, K] times 2^(sb - lo) per block: int64"""
        R = v.shape[0]
        return (v.view(R, -1, BLOCK) * (1 << (sb.long() - lo)).unsqueeze(2)).reshape(R, self.K)

    @functools.cached_property
    def acc_units(self):
        """the dot products in units of 2^GRID_LOG2: exact int64"""
        return self._shifted(self.a, self.sa, 126) @ self._shifted(self.w, self.sw, 125).T

    @functools.cached_property
    def mag_units(self):
        return self._shifted(self.a.abs(), self.sa, 126) @ self._shifted(self.w.abs(), self.sw, 125).T

    def ref(self, epilogue="bias", bias=True):
        """the exact float64 result of the bias or gate_res epilogue, or the pre-activation of gelu"""
        y = self.acc_units.double() * 2.0 ** GRID_LOG2
        if bias:
            y = y + self.bias.double()
        if epilogue == "gate_res":
            return self.res.double() + self.gate.double() * y
        return y

    def span_log2(self, epilogue="bias", bias=True):
        """log2 of the largest (sum of magnitudes) / (finest grid of the element's final sum), the sum bounded in int64"""
        mag = self.mag_units * 2                                             # units of GB = 2^-4
        if bias:
            mag = mag + (self.bias.abs() / GB).long()
        mag, grid = mag.double() * GB, torch.full((self.N,), GB, dtype=torch.float64)
        if epilogue == "gate_res":
            mag = mag * self.gate.double().abs() + self.res.double().abs()
            grid = (grid * self.gate_lsb.double()).clamp_max(GR)
        return float((mag / grid).max().log2())

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
