"""Probe C of the attention kernels, "graded weights" (probes A and B: tests/attention_probes.py).  Pure torch on the CPU; the GPU
tests (tests/test_gpu_attention_weight_probes.py) feed the operands to the kernels, the host tests
(tests/test_attention_weight_probes_host.py) prove that the verdicts accept an f32 flash loop and reject single wrong decisions.

Operands.  "signs": q_i[c], k_j[c] = +-1 from a seed (exact in bf16 and f16).  Every score n_ij = q_i . k_j is an integer,
|n_ij| <= D: exact in an f32 accumulator whatever the summation order, and every column and every MFMA k-step contributes a full
unit.  At the default scale D^-0.5 the base-2 exponent n scale log2(e) has a standard deviation of 1.44 at every D: a row's weights
are graded over about a dozen binades and dozens of keys matter.  "staged": k_j agrees with a fixed sign vector g in a(j) columns,
a rising by a fixed step from one 64-key tile to the next, q_i = g with at most `flips` seeded flips: n_ij = 2 a(j) - D up to
+-2 flips, so every row's running maximum rises at EVERY tile by 2 step c -+ 4 flips c binades (c = scale log2 e; step and flips
are chosen so that this lies within 2 .. 4).  V = code_values(...) of probe A: non-negative, each output column the weight share
of one residue class of the key index, so rounding errors cannot cancel and the bars are relative.

Reference, float64, from the rule alone: x_ij = scale n_ij + ln w_ij with w = weights_of(...) of probe A, out = softmax(x) V,
lse = logsumexp(x); a row without keys gives 0 and -inf (attention_lse_ref.attention_ref, one (batch, head) at a time).

Conditions, asserted on the host for every case: every score is an integer; over the allowed keys of a row the base-2 exponents
x log2(e) lie within +-40 and spread over at most 40, so no weight underflows relative to the largest (2^-40 > 2^-126) and the
first-tile-maximum loop of the w64 kernel stays under its 2^60 threshold (Sk 2^40 < 2^60); SENTINEL lies outside the
reference's range [0, 1].

The output bar: |out - ref| <= (m u + e_s) ref elementwise, ref == 0 an exact zero, u = U[dtype] (2^-8 bf16, 2^-11 f16).
  m = 2 for the flash contract of csrc/attn_tile.h (l is summed in f32 from the unrounded p, P is rounded once for the P V MFMA,
    the quotient is rounded once at the store; every term is non-negative, so each rounding moves the result by at most u
    relative): ops.attention (every head dim: the generic kernel keeps P in f32 and rounds only at the store, which is less),
    attention_prepared, attention_masked, attention_window, attention_prepared_window, attention_band,
    attention_prepared_band, attention_wide, attention_varlen.
  m = 3 for attention_bias and attention_framecausal, which materialise the NORMALISED bf16(p / l) (csrc/attention.hip,
    softmax_rows_kernel / softmax_bias_rows_kernel): the weights that multiply V no longer sum to one, and the
    argument for a normaliser summed over rounded P applies: numerator u + normaliser u + store u.  The same m = 3 holds for
    attention_chunked and attention_merge: every partial is a stored result (2 u + e_s of its own reference), the merge is a
    convex combination of them in f32 and rounds once more at its store; its weights exp(lse_p - m) carry the partials' lse
    errors, hence + 2 e_l.
    attention_wide with key_splits > 1 keeps its partials in f32: m = 2, + 2 e_l for the merge weights.
  attention_prepared_dual stores bf16(bf16(o_t) + bf16(o_i)): each branch within (2 u + e_s) of its reference, the sum rounded
    once more: |out - (r_t + r_i)| <= ((2 u + e_s)(1 + u) + u)(r_t + r_i).
e_s, the score side (every bound in relative terms of one probability p = 2^(n c - M), A = 40 the asserted exponent range):
  c = f32(f32(scale) f32(log2 e)): three roundings, relative 3 2^-24; on the exponent differences within a row (<= A) that is
      A 3 2^-24 < 2^-17.8 binades;
  the exponent itself: fused kernels round fma(n, c, -M) once, |.| < 64: 2^-19; the masked kernels round n c, mask log2(e) (|.| < 4:
      2^-23), their sum and the difference to M: 3 2^-19 + 2^-23.  Together < 2^-17 binades;
  so p is off by ln 2 (2^-17 + 2^-17.8) < 2^-16.7 relative; hardware exp2 (1 ulp, 2^-23), the reciprocal of l and the product
      with it (2^-23 + 2^-24) add < 2^-21.  E_ARG = 2^-16 covers the sum;
  the f32 sums of Sk non-negative terms (l, and the P V accumulator): at most Sk - 1 roundings of 2^-24 on any term in ANY order,
      Sk 2^-24 each.  e_s = 2^-16 + Sk 2^-23.  (The depth of the flash loop's sums would give less than 2^-16; the order-free
      bound is kept instead, 2^-12 at Sk = 2048, 3 % of the bf16 bar.)
  ops.attention's generic kernel (head dims other than 128 below 256 x 256 scores) folds f32(scale) into q and sums D fma steps:
      step d rounds a partial sum of magnitude <= d scale, sum_d d scale 2^-24 = D^2 scale 2^-25 nats.  Added for those cases.
e_l, the LSE bar |lse - ref| <= e_l: the relative error of l (E_ARG + Sk 2^-24, where the absolute error of the exponents,
  A 3 2^-24 ln 2, is inside E_ARG as above), the hardware log2 (1 ulp of |log2 l| <= 17), the sum with M and the product with
  ln 2, each a rounding of a value below 64: 4 2^-20 together; + ln(1 + u) only where l sums rounded P (no such entry returns an
  lse today).  A merged lse carries the worst partial's error and its own: 2 e_l."""
import functools
import math

import torch

from tests import attention_probes as P
from tests.attention_lse_ref import attention_ref

U, BF, F16 = P.U, P.BF, P.F16
LOG2E = 1.4426950408889634
E_ARG = 2.0 ** -16
A_MAX = 40.0                 # asserted range and spread of the base-2 exponents of a row
SENTINEL = 2.0               # fills the output buffers: ref lies in [0, 1]
LSE_SENTINEL = 1.0e4         # |lse| <= 40 ln 2 + ln Sk


def e_s(p):
    e = E_ARG + p["Sk"] * 2.0 ** -23
    if p.get("generic"):
        e += p["D"] ** 2 * abs(scale_of(p)) * 2.0 ** -25
    return e


def e_l(p, rounded_dtype=None):
    e = E_ARG + p["Sk"] * 2.0 ** -24 + 4 * 2.0 ** -20
    return e + (math.log1p(U[rounded_dtype]) if rounded_dtype is not None else 0.0)


def out_bar(p, m=None, merged=None):
    """relative elementwise bar of problem p: (m u + e_s), + 2 e_l for a merged result"""
    m = p.get("m", 2) if m is None else m
    merged = p.get("merged", False) if merged is None else merged
    return m * U[p["dtype"]] + e_s(p) + (2 * e_l(p) if merged else 0.0)


def lse_bar(p, merged=None):
    merged = p.get("merged", False) if merged is None else merged
    return (2 if merged else 1) * e_l(p)


def scale_of(p):
    return p["D"] ** -0.5 if p["scale"] is None else p["scale"]


# ---------------------------------------------------------------------------------------------------------------- operands
def sign_inputs(B, Hq, Hkv, Sq, Sk, D, dtype, seed, period=0):
    """q [B, Hq, Sq, D], k [B, Hkv, Sk, D] of +-1.  period > 0 (Hq == Hkv only): head h repeats head h % period, so the float64
    softmax of a 33-head shape is computed for `period` heads; V still differs per head."""
    g = torch.Generator().manual_seed(seed)
    hq, hk = (min(Hq, period), min(Hkv, period)) if period else (Hq, Hkv)
    q = (torch.randint(0, 2, (B, hq, Sq, D), generator=g) * 2 - 1).to(dtype)
    k = (torch.randint(0, 2, (B, hk, Sk, D), generator=g) * 2 - 1).to(dtype)
    if period:
        q, k = q[:, torch.arange(Hq) % hq].contiguous(), k[:, torch.arange(Hkv) % hk].contiguous()
    return q, k


def staged_plan(Sk, D, scale):
    """(step, flips, a [tiles]): agreements per 64-key tile; the rise per tile 2 step c -+ 4 flips c lies within 2 .. 4 binades"""
    c = scale * LOG2E
    step = round(3.0 / (2 * c))
    flips = max(1, int(1.0 / (4 * c)))
    tiles = (Sk + 63) // 64
    a = [D - 2 - step * (tiles - 1 - t) for t in range(tiles)]
    assert a[0] >= 0 and 2.0 <= 2 * step * c - 4 * flips * c and 2 * step * c + 4 * flips * c <= 4.0, (step, flips, a)
    return step, flips, a


def staged_inputs(B, Hq, Hkv, Sq, Sk, D, dtype, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    step, flips, a = staged_plan(Sk, D, scale)
    g = (torch.randint(0, 2, (D,), generator=gen) * 2 - 1).float()
    q = g.expand(B, Hq, Sq, D).clone()
    k = g.expand(B, Hkv, Sk, D).clone()
    # key j disagrees with g in D - a(j) seeded columns
    order = torch.rand(B, Hkv, Sk, D, generator=gen).argsort(-1)
    ndis = D - torch.tensor(a)[torch.arange(Sk) // 64]
    k = torch.where(order < ndis[None, None, :, None], -k, k)
    # row i: 0 .. flips seeded flips
    order = torch.rand(B, Hq, Sq, D, generator=gen).argsort(-1)
    nfl = torch.randint(0, flips + 1, (B, Hq, Sq, 1), generator=gen)
    q = torch.where(order < nfl, -q, q)
    return q.to(dtype), k.to(dtype)


# ------------------------------------------------------------------------------------------------------------ the problems
def _band_mask(lo, hi, Sq, Sk):
    m = torch.zeros(Sq, Sk, dtype=torch.bool)
    for b, (a, e) in enumerate(zip(lo, hi)):
        m[256 * b:256 * b + 256, a:e] = True
    return m


BAND_PLANS = {"768x768": ([0, 128, 384], [512, 768, 768], 768, 768),           # the smallest plans of the band tests
              "700x1000 ragged": ([0, 512, 64], [1000, 1000, 128], 700, 1000)}
WIDE_SHAPE = (1, 2, 70, 333)
VARLEN_LENS = ((65, 200, 1), (1, 65, 200))          # query / key lengths of the three packed sequences
CHUNK_SHAPE = (2, 4, 2, 200, 333)                   # B, Hq, Hkv, Sq, Sk of the LSE tests
CUTS = ((0, 70), (70, 71), (71, 333))
EXPLICIT_SCALE = 0.125                              # exact in f32, sqrt(2) above 128^-0.5
RAGGED = (1, 2, 160, 200)


def _bias_values(shape, seed):
    return torch.randint(-2, 3, shape, generator=torch.Generator().manual_seed(seed)).float() * 0.5


def block_diagonal(ql, kl):
    m = torch.zeros(sum(ql), sum(kl), dtype=torch.bool)
    r = c = 0
    for a, b in zip(ql, kl):
        m[r:r + a, c:c + b] = True
        r, c = r + a, c + b
    return m


@functools.lru_cache(maxsize=None)
def problems():
    """name -> dict(family, B, Hq, Hkv, Sq, Sk, D, dtype, mask, causal, scale (None: D^-0.5), seed, and optionally period, m (3
    where the docstring says so), lse (an entry returns it), merged (the widest bar of the problem's entries is a merge's),
    generic (ops.attention's generic kernel), q_from (q shared with another problem).  The rule of a problem is
    weights_of(mask, ..., causal)."""
    c = {}

    def add(name, B, Hq, Sq, Sk, D=128, dtype=BF, Hkv=None, mask=None, causal=False, scale=None, family="signs", **kw):
        assert name not in c, name
        c[name] = dict(family=family, B=B, Hq=Hq, Hkv=Hkv or Hq, Sq=Sq, Sk=Sk, D=D, dtype=dtype, mask=mask, causal=causal,
                       scale=scale, seed=1000 + len(c), **kw)

    shapes = {s for group in P.UNMASKED_SHAPES.values() for s in group} | {RAGGED}
    for s in sorted(shapes):
        add("plain " + "x".join(map(str, s)), *s, period=3 if s[1] > 4 else 0)
    add("plain 1x3x129x65 scale 0.125", 1, 3, 129, 65, scale=EXPLICIT_SCALE)
    add("plain 2x2x333x1000 scale 0.125", 2, 2, 333, 1000, scale=EXPLICIT_SCALE)
    add("staged 1x2x200x333", 1, 2, 200, 333, family="staged")
    for D in (40, 64, 192, 320):
        for dt in (BF, F16):
            add(f"head dim {D} {_dt(dt)} 1x2x129x200", 1, 2, 129, 200, D=D, dtype=dt, generic=True)
    for name, m in P.masked_cases().items():
        add("masked " + name, m["B"], m["Hq"], m["Sq"], m["Sk"], D=m["D"], dtype=m["dtype"], Hkv=m["Hkv"], mask=m["mask"],
            causal=m["causal"], lse=True, case=name)
    for name in ("causal & bool 129x128 bf16 D128", "band 449x449 f16 D64", "additive f32 129x333 bf16 D128"):
        m = P.masked_cases()[name]
        add("masked negative scale " + name, m["B"], m["Hq"], m["Sq"], m["Sk"], D=m["D"], dtype=m["dtype"], Hkv=m["Hkv"],
            mask=m["mask"], causal=m["causal"], lse=True, case=name, scale=-m["D"] ** -0.5)
    add("masked staged causal 200x333 bf16 D128", 1, 2, 200, 333, causal=True, lse=True, family="staged")
    for name in P.WINDOW_CASES:
        allowed = P.window_case(name)[3]
        add(f"window {name} bf16 D128", 2, 2, *allowed.shape, mask=allowed, window=name)
        add(f"window {name} f16 D64", 2, 2, *allowed.shape, D=64, dtype=F16, mask=allowed, window=name)
        add(f"prepared window {name}", 1, 3, *allowed.shape, mask=allowed, window=name)
    for name, (lo, hi, Sq, Sk) in BAND_PLANS.items():
        add("band " + name, 1, 2, Sq, Sk, mask=_band_mask(lo, hi, Sq, Sk), band=name)
    for D, frames, per in P.FRAMECAUSAL_CASES:
        S = frames * per
        add(f"framecausal D{D} {frames}x{per}", 1, 1, S, S, D=D, mask=P.framecausal_allowed(frames, per), m=3)
    for n, (name, b) in enumerate(P.bias_cases().items()):
        mask, bias = b["allowed"], None
        if n == 3:                                                     # a non-zero bias (multiples of 0.5, f32 [H, S, S])
            bias = _bias_values((b["H"], b["S"], b["S"]), 70)
            mask = torch.where(b["allowed"], bias, torch.full((), float("-inf")))[None]
        add("bias " + name, 1, b["H"], b["S"], b["S"], D=b["D"], Hkv=b["Hkv"], mask=mask, scale=b["D"] ** -0.5, m=3, bias=name,
            bias_values=bias)
    add(f"dual text Sk={P.DUAL_SK_T}", 2, 2, 333, P.DUAL_SK_T, m=3)
    for sk in P.DUAL_SK_I:
        if sk:
            add(f"dual image Sk={sk}", 2, 2, 333, sk, m=3, q_from=f"dual text Sk={P.DUAL_SK_T}")      # one q for both branches
    for D in (256, 384, 512):
        add(f"wide D{D} bf16", *WIDE_SHAPE, D=D, lse=True, merged=True)
    add("wide D256 f16", *WIDE_SHAPE, D=256, dtype=F16, lse=True, merged=True)
    add("wide staged D512 bf16", *WIDE_SHAPE, D=512, lse=True, merged=True, family="staged")
    ql, kl = VARLEN_LENS
    for D, dt in ((128, BF), (64, F16)):
        add(f"varlen {_dt(dt)} D{D}", 1, 4, sum(ql), sum(kl), D=D, dtype=dt, Hkv=2, mask=block_diagonal(ql, kl), lse=True)
        B, Hq, Hkv, Sq, Sk = CHUNK_SHAPE
        add(f"chunked {_dt(dt)} D{D}", B, Hq, Sq, Sk, D=D, dtype=dt, Hkv=Hkv, lse=True, m=3, merged=True)
        add(f"chunked bool {_dt(dt)} D{D}", B, Hq, Sq, Sk, D=D, dtype=dt, Hkv=Hkv, mask=chunk_mask(), lse=True, m=3, merged=True)
    return c


def _dt(dtype):
    return "bf16" if dtype == BF else "f16"


@functools.lru_cache(maxsize=None)
def chunk_mask():
    """bool [B, 1, Sq, Sk] of the LSE tests: rows without a key, rows whose keys all lie in one chunk"""
    B, _, _, SQ, SK = CHUNK_SHAPE
    m = P._rand_bool((B, 1, SQ, SK), 21, 0.5)
    m[:, :, [0, 127, 128, 199]] = False
    for r in (5, 64, 131):
        m[:, :, r, 70:] = False
    for r in (6, 129, 198):
        m[:, :, r] = False
        m[:, :, r, 70] = True
    for r in (7, 63, 130):
        m[:, :, r, :71] = False
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(q, k, v) of problem `name` in its dtype"""
    p = problems()[name]
    args = (p["B"], p["Hq"], p["Hkv"], p["Sq"], p["Sk"], p["D"], p["dtype"], p["seed"])
    q, k = staged_inputs(*args, scale_of(p)) if p["family"] == "staged" else sign_inputs(*args, p.get("period", 0))
    if p.get("q_from"):
        q = inputs(p["q_from"])[0]
    v = P.code_values(p["B"], p["Hkv"], p["Sk"], p["D"], p["dtype"], levels=3 if p["Sk"] > 1024 else 2)
    return q, k, v


def head_weights(p, b, h):
    """w [Sq, Sk] float64 of one (batch, head) from the rule"""
    m = None if p["mask"] is None else p["mask"].expand(p["B"], p["Hq"], p["Sq"], p["Sk"])[b:b + 1, h:h + 1]
    return P.weights_of(m, 1, 1, p["Sq"], p["Sk"], p["causal"])[0, 0]


def head_scores(p, q, k, b, h):
    """n [Sq, Sk] float64: the integer scores of one (batch, head)"""
    return q[b, h].double() @ k[b, h // (p["Hq"] // p["Hkv"])].double().t()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(out [B, Hq, Sq, D], lse [B, Hq, Sq]) float64, one (batch, head) at a time; heads that repeat (period) share the softmax"""
    p = problems()[name]
    q, k, v = inputs(name)
    rep = p["Hq"] // p["Hkv"]
    out = torch.empty(p["B"], p["Hq"], p["Sq"], p["D"], dtype=torch.float64)
    lse = torch.empty(p["B"], p["Hq"], p["Sq"], dtype=torch.float64)
    period = p.get("period", 0)
    prob = {}
    for b in range(p["B"]):
        for h in range(p["Hq"]):
            w = head_weights(p, b, h)[None, None]
            sl = (slice(b, b + 1), slice(h, h + 1))
            kv = (slice(b, b + 1), slice(h // rep, h // rep + 1))
            if period:                     # softmax(x) once per distinct head, then times this head's V
                if (b, h % period) not in prob:
                    prob[(b, h % period)] = softmax_head(head_scores(p, q, k, b, h), torch.log(w[0, 0]), scale_of(p))
                pm, l = prob[(b, h % period)]
                out[b, h], lse[b, h] = pm @ v[b, h // rep].double(), l
            else:
                out[sl], lse[sl] = attention_ref(q[sl], k[kv], v[kv], w, scale_of(p))
    return out, lse


# ---------------------------------------------------------------------------------------------------------------- verdicts
def out_ratio(out, ref, bar):
    """(worst |out - ref| / (bar ref) over ref > 0, whether out == 0 exactly wherever ref == 0); inf for a non-finite output"""
    o = out.to(torch.float64)
    pos = ref > 0
    ratio = ((o - ref).abs()[pos] / (bar * ref[pos])).max().item() if pos.any() else 0.0
    if not torch.isfinite(o).all():
        ratio = math.inf
    return ratio, bool((o[~pos] == 0).all())


def lse_ratio(lse, ref_lse, bar):
    """worst |lse - ref| / bar over the live rows; inf unless the dead rows are exactly -inf and nothing is NaN"""
    l = lse.to(torch.float64)
    dead = torch.isinf(ref_lse)
    if torch.isnan(l).any() or not torch.equal(l[dead], ref_lse[dead]):
        return math.inf
    return ((l[~dead] - ref_lse[~dead]).abs().max().item() / bar) if bool((~dead).any()) else 0.0


def rows_rejected(out, ref, bar, lse=None, ref_lse=None, lbar=None):
    """bool [..., Sq]: the rows the verdicts reject (an element over the bar, a non-zero at an exact zero, the lse over its bar)"""
    o = out.to(torch.float64)
    bad = ((o - ref).abs() > bar * ref).any(-1) | ~torch.isfinite(o).all(-1)
    if lse is not None:
        l = lse.to(torch.float64)
        dead = torch.isinf(ref_lse)
        bad |= torch.where(dead, l != ref_lse, ~((l - ref_lse).abs() <= lbar))
    return bad


def old_bar_accepts(out, ref, lse=None, ref_lse=None):
    """the bars the random-input tests hold attention to: rel-L2 < 1e-2, max-abs within 3 bf16 ulps of the largest reference
    magnitude (tests/test_gpu_ops.py _check), and |lse - ref| <= 4e-3 (LSE_CEILING of tests/test_gpu_attention_lse.py)"""
    o = out.to(torch.float64)
    ok = float((o - ref).norm() / ref.norm().clamp_min(1e-300)) < 1e-2
    ok &= float((o - ref).abs().max()) <= 3.0 * 2.0 ** -8 * float(ref.abs().max()) + 1e-6
    if lse is not None:
        live = ~torch.isinf(ref_lse)
        ok &= bool(((lse.to(torch.float64) - ref_lse)[live].abs() <= 4e-3).all())
    return bool(ok)


# ----------------------------------------------------------------------------------- one head, exactly and as an f32 flash loop
def softmax_head(n, logw, scale):
    """float64 (softmax [Sq, Sk], lse [Sq]) of x = scale n + logw (logw = -inf: excluded); a row without keys gives 0 and -inf"""
    x = scale * n + logw
    m = x.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(x - m)
    l = e.sum(-1, keepdim=True)
    pm = torch.where(l > 0, e / l.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))
    return pm, (m + torch.log(l)).squeeze(-1)


def exact_head(n, logw, scale, v):
    """float64 (out [Sq, D], lse [Sq]) of one head from the definition"""
    pm, lse = softmax_head(n, logw, scale)
    return pm @ v.double(), lse


def truncate(x32, dtype):
    """MUTATION helper: the store by truncation instead of round-to-nearest-even"""
    drop = 16 if dtype == BF else 13
    bits = x32.contiguous().view(torch.int32) & (-1 << drop)
    return bits.view(torch.float32).to(dtype)


def flash_head(n, logw, scale, v, dtype, tile=64, l_rounded=False, skip_rescale=False, l_last_tile=False, trunc=False):
    """f32 emulation of the flash loop on one head: tiles of `tile` keys, integer running maximum, p = exp2(fma(n, c, mask) - M),
    P rounded to dtype for P V, f32 o and l, one store.  l_rounded: l sums the rounded P.  The last three are MUTATIONS: the
    rescale of o and l skipped when the maximum rises, l taken from the last tile alone, the store truncated.
    Returns (out [Sq, D] dtype, lse [Sq] f32)."""
    f32 = torch.float32
    c = (torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32))
    s = n.to(f32) * c + (logw.to(f32) * torch.tensor(LOG2E, dtype=f32))          # -inf stays -inf
    Sq, Sk = n.shape
    vf = v.to(f32)
    m_run = torch.full((Sq, 1), -1.0e30, dtype=f32)
    l_run = torch.zeros(Sq, 1, dtype=f32)
    o = torch.zeros(Sq, v.shape[1], dtype=f32)
    for j0 in range(0, Sk, tile):
        st = s[:, j0:j0 + tile]
        m_new = torch.maximum(m_run, torch.ceil(st.max(-1, keepdim=True).values))
        alpha = torch.ones_like(m_run) if skip_rescale else torch.exp2(m_run - m_new)
        p = torch.exp2(st - m_new)
        pr = p.to(dtype).to(f32)
        psum = (pr if l_rounded else p).sum(-1, keepdim=True)
        l_run = psum if l_last_tile else l_run * alpha + psum
        o = o * alpha + pr @ vf[j0:j0 + tile]
        m_run = m_new
    live = l_run > 0
    res = torch.where(live, o / l_run.clamp_min(1e-38), torch.zeros((), dtype=f32))
    lse = torch.where(live, (m_run + torch.log2(l_run.clamp_min(1e-38))) * math.log(2.0), torch.full((), float("-inf"), dtype=f32))
    return (truncate(res, dtype) if trunc else res.to(dtype)), lse.squeeze(-1)
