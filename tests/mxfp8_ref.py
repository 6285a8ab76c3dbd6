"""The MX block quantiser of the opt-in FP8 compute path (csrc/fp8_quant.h, ops.quant_blocks_mxfp8, the `out_mx` epilogue of
ops.gemm_fp8), restated in torch on the CPU from the documented formula, never from a kernel.  Per block of 32 consecutive bf16
values of one row (blocks aligned to 32 columns):

    amax = max |x|, E = its unbiased float32 exponent, man = its 23 mantissa bits
    e    = clamp(E - 8 + (man > 0x600000), -126, 127), 0 for a zero block        (448 = 1.75 x 2^8)
    byte = e + 127                                                                (127 for a zero block, never 255)
    code = e4m3fn_rne(clamp(x * 2^-e, -448, 448))                                 (an exact power-of-two multiplication)

Also the planted rows the host and GPU tests share, and the float64 reference of a GEMM on block-scaled activations."""
import functools

import torch

from tests import gemm_fp8_probes as P

BF = torch.bfloat16
BLOCK = 32


def scale_bytes(amax: torch.Tensor) -> torch.Tensor:
    """float32 amax >= 0 -> the e8m0 scale byte (uint8), by integer arithmetic on the float's bits"""
    assert amax.dtype == torch.float32 and bool((amax >= 0).all()) and bool(torch.isfinite(amax).all())
    bits = amax.contiguous().view(torch.int32).to(torch.int64)
    E = (bits >> 23) - 127                     # a float32 subnormal (every bf16 subnormal is one) has the exponent field 0
    man = bits & 0x7FFFFF
    e = (E - 8 + (man > 0x600000).to(torch.int64)).clamp(-126, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    return (e + 127).to(torch.uint8)


def quant_blocks_ref(a: torch.Tensor):
    """bf16 [M, K] (K % 32 == 0) -> (codes uint8 [M, K], scale bytes uint8 [M, K / 32])"""
    assert a.dtype == BF and a.dim() == 2 and a.shape[1] % BLOCK == 0
    M, K = a.shape
    x = a.float().view(M, K // BLOCK, BLOCK)
    sb = scale_bytes(x.abs().amax(dim=2))
    inv = torch.exp2((127 - sb.to(torch.int64)).double()).float()          # 2^-e: bf16 inputs give e <= 120, a normal float32
    assert bool(torch.isfinite(inv).all()) and bool((inv > 0).all())
    y = x * inv.unsqueeze(2)                                               # exact unless the product is a float32 subnormal
    y = torch.minimum(torch.maximum(y, torch.full_like(y, -448.0)), torch.full_like(y, 448.0))
    return P.e4m3_nearest(y.reshape(M, K)), sb


def dequant(codes: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """float64 values of MX (codes, scale bytes)"""
    M, K = codes.shape
    v = P.values_of(codes).double().view(M, K // BLOCK, BLOCK)
    return (v * torch.exp2(sb.double() - 127).unsqueeze(2)).reshape(M, K)


def e4m3_step(y: torch.Tensor) -> torch.Tensor:
    """the spacing of the e4m3 grid at |y| <= 448 (float64): 2^(floor(log2 |y|) - 3), and 2^-9 in the subnormal range"""
    ex = torch.floor(torch.log2(y.double().abs().clamp_min(2.0 ** -6))).clamp(-6, 8)
    return torch.exp2(ex - 3)


# ---- planted rows --------------------------------------------------------------------------------------------------------------
# (name, the 32 values of the block, expected scale byte)
def _const_block(v, rest=0.0):
    b = torch.full((BLOCK,), float(rest))
    b[7] = float(v)
    return b


PLANTS = (("zero", _const_block(0.0), 127),
          ("448 x 2^5", _const_block(448.0 * 32, rest=3.0), 132),
          ("450 x 2^5", _const_block(-450.0 * 32, rest=3.0), 133),
          ("448 x 2^-9", _const_block(448.0 * 2.0 ** -9, rest=2.0 ** -12), 118),
          ("450 x 2^-9", _const_block(450.0 * 2.0 ** -9, rest=2.0 ** -12), 119),
          ("bf16 max", _const_block(float(torch.finfo(BF).max), rest=1.0), 247),
          ("2^-133 (bf16 subnormal)", _const_block(2.0 ** -133), 1))


@functools.lru_cache(maxsize=None)
def planted_rows(K=128):
    """bf16 [len(PLANTS), K]: row r holds plant r in block r mod K/32 and small integers x 2^-20 elsewhere, so the other blocks
    of the row have scales of their own"""
    g = torch.Generator().manual_seed(4242)
    a = (torch.randint(-8, 9, (len(PLANTS), K), generator=g).float() * 2.0 ** -20)
    for r, (_, blk, _) in enumerate(PLANTS):
        b = r % (K // BLOCK)
        a[r, BLOCK * b:BLOCK * (b + 1)] = blk
    assert torch.equal(a.to(BF).float(), a), "planted values must be bf16"
    return a.to(BF)


def planted_bytes(K=128):
    """[(row, block, expected scale byte)] of `planted_rows`"""
    return [(r, r % (K // BLOCK), want) for r, (_, _, want) in enumerate(PLANTS)]


@functools.lru_cache(maxsize=None)
def decade_rows(M=16, K=256, seed=7):
    """random bf16 rows whose blocks span 60 decades: normal values times 10^u, u uniform in [-30, 30] per block"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K // BLOCK, BLOCK, generator=g).double()
    u = torch.rand(M, K // BLOCK, 1, generator=g).double() * 60 - 30
    return (x * 10.0 ** u).float().reshape(M, K).to(BF)


CODE_EXPONENTS = (0, 6, -4)


@functools.lru_cache(maxsize=None)
def every_code_rows(K=384):
    """bf16 [3, K]: row r = every finite e4m3 value (tests.gemm_fp8_probes.FINITE, 254 codes) times 2^CODE_EXPONENTS[r], 31 to a
    block, each block also holding 448 x 2^e at a position that moves with the block: the block's scale is exactly 2^e and its
    codes are the values' own codes, so the quantiser must emit all 254 (asserted on the reference)"""
    v = P.values_of(P.FINITE)
    nb = K // BLOCK
    assert 31 * nb >= v.numel()
    body = torch.zeros(31 * nb)
    body[:v.numel()] = v
    row = torch.zeros(K)
    for b in range(nb):
        at = (5 * b + 3) % BLOCK
        blk = torch.cat([body[31 * b:31 * b + at], torch.tensor([448.0]), body[31 * b + at:31 * (b + 1)]])
        row[BLOCK * b:BLOCK * (b + 1)] = blk
    a = torch.stack([row * 2.0 ** e for e in CODE_EXPONENTS])
    assert torch.equal(a.to(BF).float(), a)
    codes, sb = quant_blocks_ref(a.to(BF))
    for r, e in enumerate(CODE_EXPONENTS):
        assert bool((sb[r] == 127 + e).all()) and set(codes[r].tolist()) >= set(P.FINITE.tolist())
    return a.to(BF)


# ---- GEMM on block-scaled activations ----------------------------------------------------------------------------------------------
def gemm_ref(codes, sb, w_codes, sw, bias=None):
    """float64: (sum_k value(code[m, k]) 2^(sb[m, k / 32] - 127) value(w[n, k])) sw[n] + bias[n]"""
    y = dequant(codes, sb) @ P.values_of(w_codes).double().T * sw.double().view(1, -1)
    return y if bias is None else y + bias.double().view(1, -1)
