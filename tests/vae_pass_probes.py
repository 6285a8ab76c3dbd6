"""Per-element probes of the channels-last passes of the VAEs: groupnorm_cl (csrc/conv.hip), upsample2x_cl, time_interleave_cl,
pixel_shuffle_clamp, crossfade_, tanh_clamp (conv.hip), group_mean and frames_to_u8 (csrc/elementwise.hip).  Case tables, operands,
float64 references, envelopes and the mutation helpers, written from the docstrings of ops.py and the comment headers of conv.hip,
elementwise.hip and include/apexmi.h, never from a kernel body.  Pure torch on the CPU; the GPU tests feed the operands to the
kernels, the host tests prove the conditions below for every GPU case and that the verdict rejects single wrong decisions.  The
verdict, the sentinel and the grid are those of tests/norm_rope_probes.py.

A. GroupNorm.  x [P, C] channels-last, G groups of cpg = C / G channels, one sample: every leading dimension is a position.
   Documented order: 1024-row blocks of per-channel partial sums of x and x^2, a float64 combine per group into mean and
   rstd = 1 / sqrt(max(E[x^2] - mean^2, 0) + eps), both stored as f32, then (x - mean) rstd gamma + beta [SiLU] in f32 and one
   store rounding.  u = 2^-24.

   The contract (a decision, not a description of the code): the normalised value n = (x - mean) rstd is accurate relative to
   the SPREAD of its group, not to its magnitude.  With d = x - mean over the group
        e_n = (K u (|d| + mean|d|) + 4 u |mean|) rstd,        env = e_n |gamma| + u (2 |n gamma| + |out|)
   The 4 u |mean| term is the f32 mean every f32 evaluation subtracts (torch's and the kernel's alike).  K = GN_K = 24: the
   kernel's partial sums are float64 from the first addition (a float squares exactly in float64, a 1024-row chain of float64
   additions is off by < 2^-42), so its longest f32 chain in the statistics has L = 0 terms; what is left is the rounding of rstd
   to f32 (u), the subtraction (u |d|) and the product (u |d|): 3 u |d|.  K = L / 2 + 24 is the form of norm_rope_probes'
   envelope ((n + 24) there, n >= L / 2); the 21 u of slack is what lets an f32 two-pass evaluation on the CPU through (condition
   2 below), whose sums of squared deviations are off by a few u.  The parent kernel summed x and x^2 in f32 in
   chains of up to 260 terms (K would be 154) and formed E[x^2] - mean^2 from them: its variance was accurate relative to
   E[x^2], not to the spread, which no K repairs.
   With SiLU: silu_f is documented (common.h) as one v_exp_f32 and one v_rcp_f32, 1 ulp (2 u) each, on an argument pre-scaled
   by log2(e).  For r = n gamma + beta, s = sigmoid(r): the scaled argument is off by u |z|, which exp2 turns into a relative
   ln2 u |z| = u |r|; with the exp's own 2 u and the weight (1 - s) of exp in 1 + exp, the add (u), the rcp (2 u) and the product
   (u): |silu_f(r) - silu(r)| <= u |silu(r)| ((1 - s)(|r| + 2) + 4).  The envelope of r goes through the derivative,
   silu' = s (1 + r (1 - s)), with |silu''| <= 1/2 for the second order:
        env_silu = |silu'(r)| env + env^2 / 4 + u |silu(r)| ((1 - s)(|r| + 2) + 4 + 1)        (+ 1: the store of a float out)

   Family 1, exact sums (reach and mapping).  The base image is grid_x / 8 (|x| <= 1/2, multiples of 2^-6); group g gets the
   offset and scale GROUP_TABLE[g % 5], the second half of a group's channels a further quarter of the scale, so no two adjacent
   groups and no two halves of a group share statistics.  Marker rows at positions 0, r - 1, r, 1023, 1024, P - 1 (r = 256 /
   (C / 8); those below P) carry +-4 in the channels of one thin group each (a different one per marker while G allows):
   dropping any one of them from the statistics moves that group's variance by more than ten percent (asserted).  Every value is a
   multiple of 2^-8 and every f32 partial sum of x and x^2 over a 1024-row block is exact in any order (asserted: three orders
   against float64), so the statistics are known to float64 accuracy and the envelope holds only the rounding steps after them:
        e_n = (K1 u |d| + |mean - f32(mean)| + 2^-40 |mean|) rstd,   K1 = GN_K_EXACT = 6
   the rounding of the mean to f32 is KNOWN here, not merely bounded by u |mean| (zero for a constant group, whose output is
   then beta bit for bit; the bound is attained where d is small: measured ratios of 0.99 are this term); the variance to f32, the eps add, the square root and the division (u/2 + u/2 + u + u = 3 u when the
   finish is f32; u when it is float64 rounded once), the subtraction (u) and the product (u): 5 u, + 1 u for second order.  The
   three affine steps are in env as above.

   Family 2, conditioning.  f32 storage: 64 + 0.125 N(0, 1) (mean / spread = 512) and a "groups" image with group means in
   {-6, -3, 0, 3, 6} and spreads 0.25 .. 1.75.  bf16 storage: 128 + 4 k, |k| <= 2 (with 128 + k the 4 u |mean| term alone leaves 3.3
   to 5.6 % of the elements undecided, over the cap; at mean / spread = 23 it is 0 to 2.7 %), and the groups image.  Both: 3 N(0, 1) + 0.5 and
   2^-10 N(0, 1) (eps is a tens-of-percent effect).  Fixed seeds.  A constant image (1.5) and P = 1 with one channel per group have
   variance exactly 0: the output is beta (or silu(beta)), bit for bit in bf16.  beta is never zero: at a zero reference every
   envelope is undecided.

   Two conditions, asserted by the host tests for every GPU case: (1) at most UNDECIDED_CAP of a case's elements are undecided;
   (2) three f32 evaluations on the CPU, rounded to the output type, are accepted everywhere: torch's group_norm in float32, a
   two-pass evaluation in 1024-row blocks (per channel: chunks of 8 rows in sequence, then a pairwise tree over the 128 chunks)
   whose partials are combined in float64, and the same with a pairwise tree over all rows.  (One sequence over the 1024 rows
   of a block is not among them: its 1023 roundings are outside what K = 24 admits, and on family 1, where a marker's 16 comes
   first, it lands 1.5 envelopes out.)  Family 1 and the constant images are judged by their own tighter envelope, which the
   documented route (float64 sums and combine, f32 statistics and apply) must meet; the three evaluations are judged by the
   contract there as everywhere.

   MUTATIONS the host test rejects (test_vae_pass_probes_host.py prints the table); * = the old bar of
   tests/test_gpu_vae.py::test_groupnorm_cl, rel-L2 < 4e-3, ACCEPTS what the verdict rejects:
       one marker row left out of the statistics, each marker in turn (the markers move a variance by > 10 %: both bars see it)
     * the tail row of the plain 1025-row image left out (a 1e-3 effect): every case
       the last block's rows counted, the divisor taken as nblk 1024
       channels mapped to group c // (2 cpg), and to (c // cpg + 1) % G; the two halves of a group swapped in the apply
     * eps dropped, eps doubled: on family 1 in f32 storage (a 1e-4 effect; below the resolution of a bf16 output, where two of
       the sixteen bf16 cases happen to be rejected); on the 2^-10 image both bars reject
       the variance not clamped: the constant 1.5 sums exactly, so the clamp cannot matter there and the host test asserts
       that; on the constant BIG_CONST the float64 E[x^2] - mean^2 falls below -eps in 7 of the 8 (C, G): NaN
       gamma and beta swapped; SiLU applied when off and the reverse
     * the bf16 store done by truncation: every case
     * the parent kernel's one-pass f32 order (sums of x and x^2 in f32 chains of up to 260 terms, float64 combine): rejected
       on the f32 offset image at every (C, G, P), 160 to 3400 envelopes out (the old bar accepts 4 of the 24, it is at
       rel-L2 4e-3 itself on the others), and on the f32 groups image at every (C, G) at P = 1025 (23 of 24 over all P; * on
       all).  On the bf16 offset image it is exact: 8-bit integers square to 16 bits and 260 of them sum exactly in f32.

B. Passes with nothing to tolerate: torch.equal on WHOLE sentinel-filled buffers, guard elements before and after included.
   Operands on the grid_x grid, so one step along any axis changes the value; element counts no multiple of 256, odd extents.
   crossfade with E in {4, 8}: the weights e / E are exact, a (1 - w) and b w are multiples of 2^-6 <= 4 and so is their sum,
   exact in f32 with or without contraction; one store rounding remains.  E in {5, 6}: interval verdict with
   env = 4 u (|a (1 - w)| + |b w|) (the division, 1 - w, two products, the sum: at most 4 roundings touch either term).
   group_mean: the sequential f32 sum of up to 64 grid values (multiples of 2^-3, |sum| <= 256) is exact, so the output is
   store(f32(sum) / f32(gs)) with IEEE division.  frames_to_u8: every bf16 code point in [-2, 2] against the reference chain of
   oracle/postprocess.py.  tanh_clamp: properties over every finite bf16 code point, no tolerance."""
import functools
from typing import NamedTuple

import torch
import torch.nn.functional as F

from tests.conv_probes import mismatches, ulp_distance  # noqa: F401  (re-exported for the two test files)
from tests.norm_rope_probes import (BF, EPS, F32, F64, SENTINEL, U, UNDECIDED_CAP, all_bf16_codes, check_grid,  # noqa: F401
                                    describe, grid_x, store, truncate_bf16, verdict)

GN_K = 24
GN_K_EXACT = 6
OLD_BAR = 4e-3                      # tests/test_gpu_vae.py::test_groupnorm_cl
BLOCK_ROWS = 1024
GN_CG = ((32, 32), (64, 32), (128, 32), (256, 32), (512, 32), (512, 64), (16, 2), (8, 1))
FOUR_BLOCKS = 3 * BLOCK_ROWS + 7
# (offset, scale) of group g % 5; entries 0 and 2 are the thin groups that carry the markers
GROUP_TABLE = ((0.25, 0.25), (0.0, 1.0), (-0.25, 0.5), (-1.0, 1.0), (0.25, 2.0))
MARKER = 4.0
CONST_VALUE = 1.5
BIG_CONST = 99999.8984375        # a float whose 48-bit square does not sum exactly even in float64: E[x^2] - mean^2 comes out at
#                                  +-1e-5 instead of 0, below -eps in most summation orders: the probe of the clamp (f32 storage)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def old_bar_accepts(out, ref):
    return bool(torch.isfinite(out.double()).all()) and rel_l2(out, ref) < OLD_BAR


def rows_per_pass(C):
    """positions one pass of a 256-thread block covers: one 16-byte chunk of 8 channels per thread"""
    return 256 // (C // 8)


def gn_positions(C):
    """P = 1, a P below rows_per_pass(C), 61, one block, one block and a row, four blocks"""
    return (1, 5 if rows_per_pass(C) > 5 else 3, 61, BLOCK_ROWS, BLOCK_ROWS + 1, FOUR_BLOCKS)


@functools.lru_cache(maxsize=None)
def gn_affine(C):
    """(gamma, beta) bf16 [C]: the steps over 1, 2, 4, 8 and 16 channels are non-zero modulo 13 and 17; beta is an odd multiple of
    1/32, never zero (at a zero reference every envelope is undecided)"""
    c = torch.arange(C)
    return (0.5 + ((c * 7) % 13).float() / 8).to(BF), (((c * 5 + 3) % 17 - 8).float() / 16 + 1.0 / 32).to(BF)


class GnCase(NamedTuple):
    C: int
    G: int
    P: int
    image: str            # exact | const | bigconst | plain | tiny | offset | groups
    f32: bool
    silu: bool

    @property
    def id(self):
        return f"C{self.C}.G{self.G}.P{self.P}.{self.image}.{'f32' if self.f32 else 'bf16'}.{'silu' if self.silu else 'lin'}"

    @property
    def dtype(self):
        return F32 if self.f32 else BF


@functools.lru_cache(maxsize=None)
def gn_cases(C, G):
    """every GroupNorm case of one (C, G): family 1 at every P in both storages (SiLU alternating, both at P = 1 and 1025), the
    constant image at P = 1 and 1025, family 2 at P = 61 and 1025 and, for the offset and groups images, at four blocks"""
    out, i = [], 0
    for P in gn_positions(C):
        for f32 in (False, True):
            for silu in ((False, True) if P in (1, BLOCK_ROWS + 1) else (bool(i % 2),)):
                out.append(GnCase(C, G, P, "exact", f32, silu))
            i += 1
        i += 1
    for P in (1, BLOCK_ROWS + 1):
        out += [GnCase(C, G, P, "const", f32, silu) for f32 in (False, True) for silu in (False, True)]
    out.append(GnCase(C, G, BLOCK_ROWS + 1, "bigconst", True, False))
    for image in ("plain", "tiny", "offset", "groups"):
        for P in (61, BLOCK_ROWS + 1) + ((FOUR_BLOCKS,) if image in ("offset", "groups") else ()):
            for f32 in (False, True):
                out.append(GnCase(C, G, P, image, f32, bool(i % 2)))
                i += 1
            i += 1
    return tuple(out)


def marker_rows(P, C):
    r = rows_per_pass(C)
    rows = []
    for p in (0, r - 1, r, BLOCK_ROWS - 1, BLOCK_ROWS, P - 1):
        if 0 <= p < P and p not in rows:
            rows.append(p)
    return rows


def thin_groups(G):
    return [g for g in range(G) if g % 5 in (0, 2)]


def markers(P, C, G):
    """[(row, group, value)]: marker i sits in thin group i (cycling while G has fewer), its sign alternating"""
    thin = thin_groups(G)
    return [(p, thin[i % len(thin)], MARKER if i % 2 == 0 else -MARKER) for i, p in enumerate(marker_rows(P, C))]


def _group_of(C, G):
    return torch.arange(C) // (C // G)


@functools.lru_cache(maxsize=None)
def gn_image(image, P, C, G, f32):
    """float64 [P, C], exact in the storage type"""
    cpg = C // G
    grp = _group_of(C, G)
    g = torch.Generator().manual_seed(5000 + 7 * P + 3 * C + G + 1000 * ("plain", "tiny", "offset", "groups", "exact", "const", "bigconst").index(image))
    if image == "exact":
        tab = torch.tensor(GROUP_TABLE, dtype=F64)[grp % 5]
        half = ((torch.arange(C) % cpg) >= (cpg + 1) // 2).double() if cpg > 1 else torch.zeros(C, dtype=F64)
        x = tab[:, 0] + tab[:, 1] * (grid_x(P, C, salt=C // 8) / 8 + half / 4)
        for p, gi, val in markers(P, C, G):
            x[p, grp == gi] = val
    elif image in ("const", "bigconst"):
        x = torch.full((P, C), CONST_VALUE if image == "const" else BIG_CONST, dtype=F64)
    elif image == "plain":
        x = torch.randn(P, C, generator=g) * 3 + 0.5
    elif image == "tiny":
        x = torch.randn(P, C, generator=g) * 2.0 ** -10
    elif image == "offset":
        if f32:
            x = 64 + 0.125 * torch.randn(P, C, generator=g)
        else:
            p, c = torch.arange(P).view(-1, 1), torch.arange(C).view(1, -1)
            x = 128.0 + 4 * ((p * 3 + c * 2 + c // 8 + p // 5 + (p * c) % 7) % 5 - 2)
    elif image == "groups":
        m = torch.tensor([-6.0, -3.0, 0.0, 3.0, 6.0])[(grp * 2 + grp // 5) % 5]
        s = 0.25 + 0.25 * ((grp * 3 + 1) % 7).float()
        x = m + s * torch.randn(P, C, generator=g)
    else:
        raise ValueError(image)
    x = x.to(F32 if f32 else BF).double() if image not in EXACT_IMAGES else x.double()
    assert torch.equal(x.to(F32 if f32 else BF).double(), x), (image, "not exact in the storage type")
    return x


def case_image(case):
    return gn_image(case.image, case.P, case.C, case.G, case.f32 and case.image not in ("exact", "const"))


EXACT_IMAGES = ("exact", "const", "bigconst")        # judged by family 1's envelope: their statistics are known exactly


def silu64(r):
    return r * torch.sigmoid(r)


def silu_env(r, env, store_u=1.0):
    """the envelope of silu_f(r') for |r' - r| <= env: module docstring"""
    s = torch.sigmoid(r)
    d1 = (s * (1 + r * (1 - s))).abs()
    return d1 * env + env * env / 4 + U * silu64(r).abs() * ((1 - s) * (r.abs() + 2) + 4 + store_u) + 1e-37


def gn_stats64(x, G):
    """(mean, var, d) float64 over the groups of x [P, C]: mean, var [1, G, 1], d [P, G, cpg]"""
    P, C = x.shape
    xg = x.view(P, G, C // G)
    mean = xg.mean((0, 2), keepdim=True)
    d = xg - mean
    return mean, d.pow(2).mean((0, 2), keepdim=True), d


def gn_ref(x, G, silu, eps=EPS, exact=False):
    """(ref, env) float64 [P, C] of groupnorm_cl on x with gn_affine(C): the contract's envelope, or family 1's (exact)"""
    P, C = x.shape
    cpg = C // G
    gamma, beta = (t.double().view(1, G, cpg) for t in gn_affine(C))
    mean, var, d = gn_stats64(x, G)
    rstd = (var + eps).rsqrt()
    n = d * rstd
    if exact:
        e_n = (GN_K_EXACT * U * d.abs() + (mean - mean.float().double()).abs() + 2.0 ** -40 * mean.abs()) * rstd
    else:
        e_n = (GN_K * U * (d.abs() + d.abs().mean((0, 2), keepdim=True)) + 4 * U * mean.abs()) * rstd
    r = n * gamma + beta
    env = e_n * gamma.abs() + U * (2 * (n * gamma).abs() + r.abs())
    if silu:
        r, env = silu64(r), silu_env(r, env)
    assert float(r.abs().max()) < SENTINEL / 4
    return r.reshape(P, C), env.reshape(P, C)


@functools.lru_cache(maxsize=256)
def gn_case_ref(case, exact=None):
    return gn_ref(case_image(case), case.G, case.silu, exact=case.image in EXACT_IMAGES if exact is None else exact)


# ------------------------------------------------------------------------------------------- f32 evaluations and mutations
ORDERS = ("torch", "blocks", "tree")


def _blocks(v):
    """[P, C] -> [nblk, 1024, C], zero rows appended (a zero term changes no f32 sum)"""
    P, C = v.shape
    nblk = (P + BLOCK_ROWS - 1) // BLOCK_ROWS
    return torch.cat([v, torch.zeros(nblk * BLOCK_ROWS - P, C, dtype=v.dtype)]).view(nblk, BLOCK_ROWS, C)


def block_sums32(v, order):
    """f32 per-channel sums over each 1024-row block of v [P, C] -> [nblk, C]: 'seq' rows in sequence, 'tree' pairwise,
    'strided' four interleaved sequences then their sum, 'chunk8' 8 rows in sequence then a pairwise tree over the 128 chunks"""
    b = _blocks(v.float())
    if order == "chunk8":
        c = b.view(b.shape[0], BLOCK_ROWS // 8, 8, b.shape[2])
        acc = c[:, :, 0]
        for j in range(1, 8):
            acc = acc + c[:, :, j]
        b = acc
    if order == "seq":
        acc = torch.zeros(b.shape[0], b.shape[2], dtype=F32)
        for r in range(min(BLOCK_ROWS, v.shape[0])):
            acc = acc + b[:, r]
        return acc
    if order == "strided":
        q = b.view(b.shape[0], BLOCK_ROWS // 4, 4, b.shape[2])
        acc = torch.zeros(b.shape[0], 4, b.shape[2], dtype=F32)
        for r in range(min(BLOCK_ROWS // 4, (v.shape[0] + 3) // 4)):
            acc = acc + q[:, r]
        return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    while b.shape[1] > 1:
        b = b[:, 0::2] + b[:, 1::2]
    return b[:, 0]


def _combine64(part, G):
    """[nblk, C] partials -> float64 [G] group sums"""
    return part.double().sum(0).view(G, -1).sum(1)


def gn_stats32(x, G, order, eps=EPS, mut=None):
    """(mean, rstd) f32 [G] of x float64 [P, C] (exact in f32), two-pass: 'blocks' chunks of 8 rows | 'tree' pairwise.
    mut: None | ('drop_row', p) | 'div_nblk' | 'noeps' | 'eps2'"""
    P, C = x.shape
    cpg = C // G
    x32 = x.float()
    keep = torch.ones(P, dtype=torch.bool)
    if isinstance(mut, tuple) and mut[0] == "drop_row":
        keep[mut[1]] = False
    count = float((((P + BLOCK_ROWS - 1) // BLOCK_ROWS) * BLOCK_ROWS if mut == "div_nblk" else P) * cpg)
    e = torch.tensor(0.0 if mut == "noeps" else 2 * eps if mut == "eps2" else eps, dtype=F32)
    xk = x32[keep]
    seq = "tree" if order == "tree" else "chunk8"
    mean = (_combine64(block_sums32(xk, seq), G) / count).float()
    d = xk - mean.repeat_interleave(cpg).view(1, C)
    var = (_combine64(block_sums32(d * d, seq), G) / count).float()
    return mean, 1.0 / torch.sqrt(var + e)


def onepass_stats(x, G, eps=EPS, clamp=True, f64=False):
    """The one-pass form: per 1024-row block and channel, the thread of row-lane j sums rows j, j + r, .. (r = rows_per_pass) of x
    and x^2 (a fused multiply-add) in sequence, the lanes are then added in sequence, the partials combined in float64 and
    var = E[x^2] - mean^2 [clamped at 0].  f64 = False: the parent kernel's f32 sums (MUTATION 'onepass'); True: float64 sums."""
    P, C = x.shape
    cpg, r = C // G, rows_per_pass(C)
    dt = F64 if f64 else F32
    b = _blocks(x).view(-1, BLOCK_ROWS // r, r, C)
    s = torch.zeros(b.shape[0], r, C, dtype=dt)
    q = torch.zeros(b.shape[0], r, C, dtype=dt)
    for i in range(min(BLOCK_ROWS // r, (P + r - 1) // r)):
        v = b[:, i]
        s = (s.double() + v).to(dt)
        q = (q.double() + v * v).to(dt)
    ss, qq = s[:, 0], q[:, 0]
    for j in range(1, r):
        ss, qq = ss + s[:, j], qq + q[:, j]
    n = float(P * cpg)
    mean = _combine64(ss, G) / n
    var = _combine64(qq, G) / n - mean * mean
    if clamp:
        var = var.clamp_min(0.0)
    return mean.float(), (1.0 / torch.sqrt(var + eps)).float()


def gn_apply32(x, G, mean, rstd, silu, dtype, mut=None):
    """the apply in f32 in the documented order, one store rounding.  mut: 'map_pair' | 'map_next' | 'swap_halves' |
    'swap_affine' | 'silu_flip' | 'trunc'"""
    P, C = x.shape
    cpg = C // G
    gamma, beta = (t.float() for t in gn_affine(C))
    if mut == "swap_affine":
        gamma, beta = beta, gamma
    grp = _group_of(C, G)
    if mut == "map_pair":
        grp = torch.arange(C) // (cpg * 2)
    elif mut == "map_next":
        grp = (grp + 1) % G
    y = (x.float() - mean[grp].view(1, C)) * rstd[grp].view(1, C) * gamma + beta
    if mut == "swap_halves":
        assert cpg > 1
        c = torch.arange(C)
        y = y[:, grp * cpg + (c % cpg + cpg // 2) % cpg]
    if silu != (mut == "silu_flip"):
        y = F.silu(y)
    if mut == "trunc":
        assert dtype == BF
        return truncate_bf16(y)
    return y.to(dtype)


def gn_emulate(case, order="blocks", mut=None, x=None):
    """The case's output from an f32 evaluation on the CPU, or with ONE wrong decision planted (mut: those of gn_stats32,
    gn_apply32, 'onepass', 'noclamp')."""
    x = case_image(case) if x is None else x
    if mut in ("onepass", "noclamp"):     # the parent's f32 sums (clamped) | the documented float64 sums without the clamp
        mean, rstd = onepass_stats(x, case.G, clamp=mut != "noclamp", f64=mut == "noclamp")
        return gn_apply32(x, case.G, mean, rstd, case.silu, case.dtype)
    stat_mut = mut if (isinstance(mut, tuple) or mut in ("div_nblk", "noeps", "eps2")) else None
    if order == "torch" and mut is None:
        gamma, beta = (t.float() for t in gn_affine(case.C))
        # torch.group_norm: F.group_norm's operation without its refusal of one value per group (P = 1, one channel per group)
        y = torch.group_norm(x.float().t().reshape(1, case.C, case.P), case.G, gamma, beta, EPS, False)[0].t()
        return (F.silu(y) if case.silu else y).contiguous().to(case.dtype)
    mean, rstd = gn_stats32(x, case.G, "blocks" if order == "torch" else order, mut=stat_mut)
    return gn_apply32(x, case.G, mean, rstd, case.silu, case.dtype, mut=None if stat_mut is not None else mut)


def gn_documented(case):
    """the documented route on the CPU: one-pass float64 sums, float64 combine, f32 statistics, f32 apply"""
    x = case_image(case)
    mean, rstd = onepass_stats(x, case.G, f64=True)
    return gn_apply32(x, case.G, mean, rstd, case.silu, case.dtype)


def _units(v):
    """per column of v [P, C]: the largest 2^-k (k <= 16) of which every entry is a multiple"""
    unit = torch.full((v.shape[1],), 2.0 ** -16, dtype=F64)
    for k in range(16, -1, -1):
        ok = (v * 2.0 ** k == (v * 2.0 ** k).round()).all(0)
        unit = torch.where(ok, torch.full_like(unit, 2.0 ** -k), unit)
    assert bool((v / unit == (v / unit).round()).all())
    return unit


def exact_sums_hold(x):
    """family 1: in every channel the sum of magnitudes of x and of x^2 over a 1024-row block is below 2^24 units of that
    channel's grid, which makes every partial sum of every order exact in f32; and the f32 sums in three orders (rows in sequence,
    pairwise, four interleaved sequences) do equal the float64 sums"""
    for v in (x, x * x):
        if bool((_blocks(v.abs()).sum(1) / _units(v) >= 2 ** 24).any()):
            return False
        want = _blocks(v).sum(1)
        for order in ("seq", "tree", "strided"):
            if not torch.equal(block_sums32(v, order).double(), want):
                return False
    return True


def marker_variance_shift(P, C, G):
    """for each marker: |var without the row / var - 1| of its group (the divisor unchanged)"""
    x = gn_image("exact", P, C, G, False)
    cpg = C // G
    out = []
    for p, gi, _ in markers(P, C, G):
        xg = x[:, gi * cpg:(gi + 1) * cpg]
        n = float(P * cpg)
        var = (xg * xg).sum() / n - (xg.sum() / n) ** 2
        xs = torch.cat([xg[:p], xg[p + 1:]])
        var2 = (xs * xs).sum() / n - (xs.sum() / n) ** 2
        out.append(abs(float(var2 / var) - 1))
    return out


# ------------------------------------------------------------------------------------------------- B. the exact passes
def grid4(T, H, W, C, salt=0, scale=1.0):
    """float64 [T, H, W, C] on the grid_x grid (multiples of 2^-3 in [-4, 4]) times scale: one step along any axis changes the value"""
    base = grid_x(T * H * W, C, salt)
    t = torch.arange(T).view(T, 1, 1, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    x = base.view(T, H, W, C) * 8 + t * 3 + h * 9
    return ((x + 32) % 65 - 32) / 8 * scale


def guarded(n, dtype, fill=SENTINEL, guard=64):
    """a flat buffer of guard + n + guard elements filled with the sentinel"""
    return torch.full((guard + n + guard,), fill, dtype=dtype)


def expect_guarded(payload, dtype, fill=SENTINEL, guard=64):
    out = guarded(payload.numel(), dtype, fill, guard)
    out[guard:guard + payload.numel()] = payload.reshape(-1)
    return out


UPSAMPLE_CASES = [(T, H, W, C) for T, H, W in ((1, 3, 5), (3, 5, 7)) for C in (8, 16, 96)]


def upsample_ref(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


INTERLEAVE_CASES = [(T, H, W, C2, f32) for T, H, W in ((1, 3, 5), (3, 7, 5)) for C2 in (16, 32, 192) for f32 in (False, True)]


def interleave_ref(x):
    """[T, H, W, 2C] -> [2T, H, W, C]: channel half h of frame t becomes frame 2t + h"""
    T, H, W, C2 = x.shape
    return torch.stack((x[..., :C2 // 2], x[..., C2 // 2:]), dim=1).reshape(2 * T, H, W, C2 // 2)


LO, HI = -0.5, 0.75
# (T, H, W, C, r, extra guard channels)
SHUFFLE_SHAPES = ((3, 5, 7, 3, 2, 0), (3, 5, 7, 3, 2, 4), (2, 3, 5, 3, 1, 0), (2, 3, 5, 3, 1, 5), (3, 3, 5, 2, 2, 8))
SHUFFLE_CASES = [s + (t0, f32) for s in SHUFFLE_SHAPES for t0 in (0, s[0] - 1) for f32 in (False, True)]


def _neighbours(v, dtype):
    t = torch.tensor([v], dtype=dtype)
    if dtype == BF:
        i = t.view(torch.int16)
        return [float((i + k).view(BF)) for k in (-1, 1)]
    return [float(torch.nextafter(t, torch.tensor([s], dtype=dtype))) for s in (-10.0, 10.0)]


def shuffle_operand(T, H, W, C, r, extra, f32):
    """float64 [T, H, W, Cs]: grid values in [-1, 1], every 5th element one of lo, hi and their neighbours in the storage type,
    the guard channels [C r^2, Cs) values outside [lo, hi] and outside the grid's range"""
    Cs = C * r * r + extra
    x = grid4(T, H, W, Cs, salt=r, scale=0.25)
    dt = F32 if f32 else BF
    special = torch.tensor([LO, HI] + _neighbours(LO, dt) + _neighbours(HI, dt), dtype=F64)
    flat = x.reshape(-1)
    idx = torch.arange(0, flat.numel(), 5)
    flat[idx] = special[(idx // 5) % 6]
    x = flat.view(T, H, W, Cs)
    if extra:
        c = torch.arange(extra)
        x[..., C * r * r:] = torch.where(c % 2 == 0, 2.0 + c.double(), -3.0 - c.double())
    assert torch.equal(x.to(dt).double(), x)
    return x


def shuffle_ref(x, C, r, t0, lo=LO, hi=HI):
    """[T, H, W, Cs] -> [C, T - t0, H r, W r]"""
    img = x[..., :C * r * r].clamp(lo, hi).permute(0, 3, 1, 2)
    img = F.pixel_shuffle(img, r) if r > 1 else img
    return img[t0:].permute(1, 0, 2, 3).contiguous()


CROSSFADE_CASES = [(E, dim, f32) for E in (4, 8, 5, 6) for dim in (1, 2) for f32 in (False, True)]
CROSSFADE_SHAPE = (3, 11, 13, 8)      # [T, H, W, C] of both tensors


def crossfade_operands(E, dim):
    """(a_full, b_full) float64 [T, H, W, C] on the grid; a = the trailing E of a_full along dim, b = the leading E of b_full"""
    return grid4(*CROSSFADE_SHAPE, salt=1), grid4(*CROSSFADE_SHAPE, salt=4)


def crossfade_ref(a_full, b_full, E, dim, mut=None):
    """(expected b_full, env) float64.  mut: 'w_plus' (e + 1) / E | 'w_em1' e / (E - 1) | 'swap' | 'shift' (the band one row on)"""
    n = a_full.shape[dim]
    a, out = a_full.narrow(dim, n - E, E), b_full.clone()
    start = 1 if mut == "shift" else 0
    b = b_full.narrow(dim, start, E)
    e = torch.arange(E, dtype=F64)
    w = (e + 1) / E if mut == "w_plus" else e / (E - 1) if mut == "w_em1" else e / E
    w = w.view([-1 if k == dim else 1 for k in range(4)])
    if mut == "swap":
        a, b = b, a
    out.narrow(dim, start, E).copy_(a * (1 - w) + b * w)
    env = torch.zeros_like(out)
    env.narrow(dim, start, E).copy_(4 * U * ((a * (1 - w)).abs() + (b * w).abs()))
    return out, env


GROUP_MEAN_CASES = [(gs, C, f32) for gs, C in ((1, 24), (2, 9), (3, 7), (16, 5), (64, 3)) for f32 in (False, True)]
GROUP_MEAN_POS = (3, 5, 7)


def group_mean_ref(x, C, gs, dtype, mut=None):
    """x float64 [.., C gs] -> store(f32(sum) / f32(gs)).  mut: 'gs_m1' divides by gs - 1 | 'skip_last' leaves the last member out"""
    xs = x.view(*x.shape[:-1], C, gs)
    s = (xs[..., :-1] if mut == "skip_last" else xs).sum(-1)
    assert float(xs.abs().sum(-1).max()) <= 256 and torch.equal(xs * 8, (xs * 8).round())
    div = torch.tensor(float(gs - 1 if mut == "gs_m1" else gs), dtype=F32)
    return (s.float() / div).to(dtype)


def u8_codes():
    """every bf16 code point in [-2, 2] (both zeros included): bf16 [32770]"""
    v = all_bf16_codes()
    return v[v.float().abs() <= 2.0]


U8_SHAPE = (2, 145, 113)              # T, H, W: 32770 positions, all odd but T


def u8_video(C, f32):
    """a channels-last tile [T, H, W, 4] whose channel c holds u8_codes() rotated by 1237 c, channel 3 the sentinel; the operand is
    the strided view [C, T, H, W] of its first C channels"""
    codes = u8_codes()
    T, H, W = U8_SHAPE
    assert codes.numel() == T * H * W
    tile = torch.full((T, H, W, 4), SENTINEL, dtype=BF)
    for c in range(3):
        tile[..., c] = torch.roll(codes, 1237 * c).view(T, H, W)
    return tile.float() if f32 else tile


def finite_bf16_codes():
    v = all_bf16_codes()
    return v[torch.isfinite(v.float())]


def tanh_ref64(x, inv_scale):
    """3 tanh(x inv_scale / 3) in float64, inv_scale as the float the kernel receives"""
    return 3 * torch.tanh(x.double() * float(torch.tensor(inv_scale, dtype=F32)) / 3)


def tanh_properties(x, y):
    """None, or what fails: x the finite bf16 code points as the storage type, y the outputs.  Non-decreasing, odd bit for bit,
    |y| <= 3"""
    xs, order = torch.sort(x.double(), stable=True)
    ys = y.double()[order]
    if not bool(torch.isfinite(ys).all()):
        return "non-finite output of a finite input"
    if bool((ys[1:] < ys[:-1]).any()):
        i = int((ys[1:] < ys[:-1]).nonzero()[0])
        return f"decreasing at x = {float(xs[i])!r} -> {float(xs[i + 1])!r}: y {float(ys[i])!r} -> {float(ys[i + 1])!r}"
    if float(ys.abs().max()) > 3.0:
        return f"|y| = {float(ys.abs().max())!r} > 3"
    # pair x with -x through the sort: the finite code points are symmetric
    xp, yp = x[x.double() > 0], y[x.double() > 0]
    xn, yn = x[x.double() < 0], y[x.double() < 0]
    op, on = torch.argsort(xp.double()), torch.argsort(-xn.double())
    if not torch.equal(xp.double()[op], -xn.double()[on]):
        return "the inputs are not symmetric"
    bits = torch.int16 if y.dtype == BF else torch.int32
    if not torch.equal(yp[op].contiguous().view(bits), (-yn[on]).contiguous().view(bits)):
        i = int((yp[op].double() != -yn[on].double()).nonzero()[0]) if bool((yp[op].double() != -yn[on].double()).any()) else -1
        return f"y(-x) != -y(x) at x = {float(xp[op][i])!r}" if i >= 0 else "y(-x) and -y(x) differ in the sign of a zero"
    zero = x.double() == 0
    if not torch.equal(y[zero].contiguous().view(bits), x[zero].contiguous().view(bits)):
        return "a signed zero does not map to itself"
    return None
