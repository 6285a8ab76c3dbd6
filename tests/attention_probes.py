"""Closed-form probes of the attention kernels: inputs whose correct output is known exactly, the expected outputs (float64, from
the mask RULE alone, never from a kernel) and elementwise comparisons with derived bars.  Pure torch on the CPU; the GPU tests feed
the inputs to the kernels, the host tests prove that the comparisons reject single wrong decisions.

Probe A, membership: q = 0 makes every score exactly 0, so a row's output is the (mask-weighted) mean of V over the keys it sees.
V >= 0 is a sum of one-hot codes of the key index, so every output column counts the allowed keys of one residue class: one key
added or dropped moves a column by >= 1 / 33 relative (Sk <= 1024), far above the bar of 2 u |ref| (u = 2^-8 bf16, 2^-11 f16;
all terms non-negative: the roundings of P and of the store cannot cancel).  ref == 0 must come back as an exact zero.

Probe B, selection: q_i = 8 e_a(i), k_j = 4 e_a'(j) with softmax_scale 1: the target key pi(i) scores 32 (46 binades), every other
allowed key 0, so out[i] = V[pi(i)] up to one rounding of P and one of the store: |out - V[pi]| <= 2^-7 |V[pi]| + Sk 2^-40 max|V|
(bf16; 2^-10 for f16).  Only a subset T of the keys (at most one per code) carries a code, the other keys are zero rows (score 0)
or DECOYS: keys that score 64 for the rows of one code and that the rule excludes for every such row.  A rule error that admits
a decoy, or a row that reads another K / V row, is visibly wrong.

Neither lets the VALUE of a score or of a probability matter (A: every score 0; B: one column of D, a 46-binade argmax).  Probe C,
graded weights, does: tests/attention_weight_probes.py (+-1 operands, integer scores over all D columns, weights graded over a
dozen binades, the same V codes, weights_of and case tables as here; the bar (2 u + e_s) |ref| and the LSE bar e_l are derived
there)."""
import functools
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
BF, F16 = torch.bfloat16, torch.float16


# ------------------------------------------------------------------------------------------------------------- rules -> weights
def causal_rule(Sq, Sk):
    """top-left aligned: key j <= query i (rows i >= Sk see every key)"""
    return torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None]


def band_rule(Sq, Sk, below, above):
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    return (j > i - below) & (j <= i + above)


def weights_of(mask, B, Hq, Sq, Sk, causal=False):
    """w [B, Hq, Sq, Sk] float64 of torch's sdpa rule: bool mask -> {0, 1}, additive mask -> exp(mask), AND-ed with causal"""
    if mask is None:
        w = torch.ones(B, Hq, Sq, Sk, dtype=torch.float64)
    elif mask.dtype == torch.bool:
        w = mask.expand(B, Hq, Sq, Sk).to(torch.float64)
    else:
        w = torch.exp(mask.to(torch.float64)).expand(B, Hq, Sq, Sk)
    if causal:
        w = w * causal_rule(Sq, Sk).to(torch.float64)
    return w.contiguous()


def block_map(allowed, dense=None):
    """CPU restatement of the kernels' block map over (128-row query block, 64-key tile): 0 SKIP (no allowed pair), 1 DENSE (all
    pairs allowed, additive value 0 where `dense` says so), 2 PARTIAL; rows / keys past the ends belong to no pair."""
    Sq, Sk = allowed.shape
    dense = allowed if dense is None else dense
    out = torch.empty((Sq + 127) // 128, (Sk + 63) // 64, dtype=torch.uint8)
    for i in range(out.shape[0]):
        for j in range(out.shape[1]):
            a, d = allowed[i * 128:(i + 1) * 128, j * 64:(j + 1) * 64], dense[i * 128:(i + 1) * 128, j * 64:(j + 1) * 64]
            out[i, j] = 0 if not a.any() else 1 if d.all() else 2
    return out


# ---------------------------------------------------------------------------------------------------------- probe A: membership
def code_values(B, Hkv, Sk, D, dtype, levels=2):
    """V [B, Hkv, Sk, D] >= 0: groups of 32 columns, each the one-hot of one base-32 digit of the key index (shifted per (batch,
    head) so that a wrong head is a wrong code): j % 32, (j // 32) % 32, then for D >= 128 the same two digits of j + 1 (levels=2)
    or (j // 1024) % 32 and (j + 1) % 32 (levels=3, Sk > 1024); D > 128 tiles the 128 columns."""
    v = torch.zeros(B, Hkv, Sk, D, dtype=torch.float64)
    for b in range(B):
        for h in range(Hkv):
            j = torch.arange(Sk) + 5 * (b * Hkv + h)
            digits = [j % 32, (j // 32) % 32]
            digits += [(j + 1) % 32, ((j + 1) // 32) % 32] if levels == 2 else [(j // 1024) % 32, (j + 1) % 32]
            for d0 in range(0, D, 32):
                v[b, h, torch.arange(Sk), d0 + digits[(d0 // 32) % 4]] = 1.0
    return v.to(dtype)


def membership_expected(w, v):
    """out[b, h, i, :] = sum_j w_ij V[j] / sum_j w_ij in float64 (grouped-query heads: query head h reads kv head h / group); a row
    without an allowed key is all zeros"""
    B, Hq = w.shape[:2]
    vv = v.to(torch.float64).repeat_interleave(Hq // v.shape[1], dim=1)
    den = w.sum(-1, keepdim=True)
    return torch.where(den > 0, (w @ vv) / den.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))


def membership_check(out, ref, dtype):
    """(worst |out - ref| / (2 u ref) over ref > 0, whether out == 0 exactly wherever ref == 0)"""
    o = out.to(torch.float64)
    pos = ref > 0
    ratio = ((o - ref).abs()[pos] / (2 * U[dtype] * ref[pos])).max().item() if pos.any() else 0.0
    if not torch.isfinite(o).all():
        ratio = math.inf
    return ratio, bool((o[~pos] == 0).all())


def membership_ok(out, ref, dtype):
    ratio, zeros = membership_check(out, ref, dtype)
    return ratio <= 1.0 and zeros


# ----------------------------------------------------------------------------------------------------------- probe B: selection
def _targets(Sk, ncodes, g):
    """key positions that carry a code for kv head number g: about every s-th key with a head-dependent jitter (all offsets inside a
    64-key tile occur), key 0 and the last key Sk - 1; at most `ncodes` of them, at least every second key stays free for decoys"""
    s = max(2, -(-Sk // (ncodes - 17)))
    pos = {0, Sk - 1}
    t = 1
    while len(pos) < ncodes - 16:                                       # 16 codes stay in reserve (selection_inputs)
        p = t * s + (t * (2 * g + 1)) % s
        if p >= Sk:
            break
        pos.add(p)
        t += 1
    return torch.tensor(sorted(pos))


def selection_inputs(allowed, Hkv, D, dtype, seed=0, neg=False, dims=None):
    """allowed bool [B, Hq, Sq, Sk] (the whole rule, causal included).  Returns dict(q, k, v, pi, has, expect, bound, decoys):
    q [B, Hq, Sq, D], k / v [B, Hkv, Sk, D] in `dtype`, pi [B, Hq, Sq] the target key of every row (has: rows with an allowed key),
    expect = V[pi] (zeros for rows without keys) and the derived elementwise bound, float64.  dims = (lo, hi): the code columns
    used (the dual kernel's two branches share q and take one half of the columns each).  neg: k negated (softmax_scale -1)."""
    B, Hq, Sq, Sk = allowed.shape
    lo, hi = dims or (0, D)
    ncodes, group = hi - lo, Hq // Hkv
    gen = torch.Generator().manual_seed(seed)
    q = torch.zeros(B, Hq, Sq, D)
    k = torch.zeros(B, Hkv, Sk, D)
    v = torch.randn(B, Hkv, Sk, D, generator=gen).to(dtype)
    pi = torch.zeros(B, Hq, Sq, dtype=torch.long)
    has = allowed.any(-1)
    rows = torch.arange(Sq)
    ndecoys = 0
    for b in range(B):
        for g in range(Hkv):
            T = _targets(Sk, ncodes, b * Hkv + g)
            extra = []                                                   # rows whose few keys hold no coded key: code their last key
            for h in range(g * group, (g + 1) * group):
                for i in (has[b, h] & ~allowed[b, h][:, T].any(1)).nonzero().flatten().tolist():
                    if not bool(allowed[b, h, i, extra].any()):
                        extra.append(int(allowed[b, h, i].nonzero()[-1]))
            T = torch.tensor(sorted(set(T.tolist()) | set(extra)))
            if len(T) > ncodes:
                raise ValueError("selection probe: more rows without a coded key than spare codes (badly designed case)")
            codes = (torch.arange(len(T)) + 5 * (b * Hkv + g)) % ncodes
            k[b, g, T, lo + codes] = 4.0
            tcode = torch.full((group, Sq), -1, dtype=torch.long)
            for hh in range(group):
                h = g * group + hh
                A = allowed[b, h][:, T]                                  # [Sq, |T|]
                n = A.sum(1)
                if bool(((n == 0) & has[b, h]).any()):
                    raise ValueError("selection probe: a row's allowed keys hold no coded key (badly designed case)")
                # even rows + head: the LAST coded key they may see (the rule's edge); the others: a spread choice
                r = torch.where((rows + h) % 2 == 0, n - 1, (7 * rows + 3 * h + b) % n.clamp_min(1))
                t_idx = ((A.cumsum(1) == (r + 1)[:, None]) & A).to(torch.int8).argmax(1)
                pi[b, h] = T[t_idx]
                tcode[hh] = torch.where(has[b, h], codes[t_idx], torch.full((), -1, dtype=torch.long))
                q[b, h, rows[has[b, h]], lo + codes[t_idx][has[b, h]]] = 8.0
            # decoys on the free keys: code c at key j only if NO row of code c may see j; prefer a row for which j lies just outside
            Ag = allowed[b, g * group:(g + 1) * group].reshape(group * Sq, Sk)
            tc = tcode.reshape(-1)
            blocked = torch.zeros(ncodes, Sk)
            blocked.index_add_(0, tc.clamp_min(0), (Ag & (tc >= 0)[:, None]).float())
            blocked = blocked > 0
            used = torch.zeros(ncodes, dtype=torch.bool)
            used[tc[tc >= 0]] = True
            left = torch.cat([torch.zeros(len(Ag), 1, dtype=torch.bool), Ag[:, :-1]], 1)
            right = torch.cat([Ag[:, 1:], torch.zeros(len(Ag), 1, dtype=torch.bool)], 1)
            edge = ~Ag & (left | right) & (tc >= 0)[:, None]             # [rows, Sk]: key j is just outside this row's keys
            free = torch.ones(Sk, dtype=torch.bool)
            free[T] = False
            if bool(Ag.all()):                                           # nothing excluded: no place for a decoy
                continue
            for j in free.nonzero().flatten().tolist():
                cand = tc[edge[:, j]]
                cand = cand[~blocked[cand, j]]
                if len(cand) == 0:
                    cand = (used & ~blocked[:, j]).nonzero().flatten()
                if len(cand):
                    k[b, g, j, lo + int(cand[(j + b + g) % len(cand)])] = 8.0
                    ndecoys += 1
    if neg:
        k = -k
    vv = v.to(torch.float64).repeat_interleave(group, dim=1)
    expect = torch.gather(vv, 2, pi[..., None].expand(B, Hq, Sq, D)) * has[..., None]
    tol = 2.0 ** -7 if dtype == BF else 2.0 ** -10
    bound = tol * expect.abs() + Sk * 2.0 ** -40 * float(v.abs().max())
    return dict(q=q.to(dtype), k=k.to(dtype), v=v, pi=pi, has=has, expect=expect, bound=bound, decoys=ndecoys)


def selection_ratio(out, expect, bound):
    """worst |out - expect| / bound (inf for a non-finite output)"""
    o = out.to(torch.float64)
    if not torch.isfinite(o).all():
        return math.inf
    return ((o - expect).abs() / bound).max().item()


def selection_reference(s, allowed, scale):
    """float64 softmax of the probe's own q, k, v under `allowed`: what the closed form claims to equal (host check); one
    (batch, head) at a time, so the 2048-key shapes stay small"""
    B, Hq = allowed.shape[:2]
    rep = Hq // s["k"].shape[1]
    out = torch.empty(s["q"].shape, dtype=torch.float64)
    for b in range(B):
        for h in range(Hq):
            sc = (s["q"][b, h].to(torch.float64) @ s["k"][b, h // rep].to(torch.float64).t()) * scale
            p = torch.softmax(sc.masked_fill(~allowed[b, h], float("-inf")), -1).nan_to_num(0.0)
            out[b, h] = p @ s["v"][b, h // rep].to(torch.float64)
    return out


# --------------------------------------------------------------------------------------------------------------- the case tables
SIZES = ((1, 1), (63, 64), (64, 63), (65, 127), (127, 65), (128, 129), (129, 128), (333, 333), (64, 333), (333, 63))
# Sq < Sk, Sq > Sk and Sq == Sk over {1, 63, 64, 65, 127, 128, 129, 333}


def _rand_bool(shape, seed, p=0.5):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < p


def _additive(shape, seed, dtype, dead_rows=()):
    """multiples of 0.5 in [-1, 1] (exact in bf16 / f16; the lightest key still weighs e^-2 of the heaviest, so dropping it moves
    its column by more than the bar) and -inf; `dead_rows`: all -inf"""
    g = torch.Generator().manual_seed(seed)
    m = (torch.randint(-2, 3, shape, generator=g).float() * 0.5)
    m[torch.rand(shape, generator=g) < 0.35] = float("-inf")
    for r in dead_rows:
        m[..., r, :] = float("-inf")
    return m.to(dtype)


@functools.lru_cache(maxsize=None)
def band_case_mask():
    """449 x 449 band (i - 200, i + 5]: both edges sweep every offset of a 64-key tile and of a 128-row block"""
    m = band_rule(449, 449, 200, 5)
    codes = set(block_map(m).flatten().tolist())
    assert codes == {0, 1, 2}, codes                                   # SKIP, DENSE and PARTIAL tiles all occur
    for mm, period in ((m, 64), (m.t(), 128)):                         # key edges inside a tile, row edges inside a block
        first, past = mm.to(torch.int8).argmax(1), 449 - mm.flip(1).to(torch.int8).argmax(1)
        for edge in (first, past):                                     # first allowed index / first index past the band
            assert {0, 1, 31, 32, 63, 64} <= set((edge % period).tolist()) | ({64} if period == 64 else set())
    return m


@functools.lru_cache(maxsize=None)
def masked_cases():
    """name -> dict(B, Hq, Hkv, Sq, Sk, D, dtype, mask, causal, gqa, layout): the ops.attention_masked / hip_mfma_sdpa probes.
    `mask` is what the kernel is given; the rule is weights_of(mask, ..., causal)."""
    c = {}

    def add(name, Sq, Sk, mask=None, causal=False, B=2, Hq=2, Hkv=None, wide=True, layout="bhsd"):
        D, dtype = (128, BF) if wide else (64, F16)
        c[f"{name} {Sq}x{Sk} {'bf16 D128' if wide else 'f16 D64'}"] = dict(
            B=B, Hq=Hq, Hkv=Hkv or Hq, Sq=Sq, Sk=Sk, D=D, dtype=dtype, mask=mask, causal=causal, gqa=Hkv is not None, layout=layout)

    for n, (Sq, Sk) in enumerate(SIZES):
        wide = n % 2 == 0
        add("causal", Sq, Sk, causal=True, wide=wide)
        add("bool [Sq,Sk]", Sq, Sk, _rand_bool((Sq, Sk), 10 + n), wide=not wide)
        add("causal & bool", Sq, Sk, _rand_bool((Sq, Sk), 30 + n, 0.7), causal=True, wide=wide)
    for wide in (True, False):
        add("no mask", 129, 65, wide=wide)
        add("bool [B,1,1,Sk]", 127, 333, _rand_bool((2, 1, 1, 333), 50, 0.6), wide=wide)
        add("bool [B,H,Sq,Sk]", 129, 127, _rand_bool((2, 2, 129, 127), 51), wide=wide)
        rows = _rand_bool((333, 1), 52, 0.7)
        rows[[0, 127, 128, 332]] = torch.tensor([False, True, False, True])[:, None]
        add("bool [Sq,1] over keys", 333, 129, rows, wide=wide)
        add("band", 449, 449, band_case_mask(), B=1, wide=wide)
        dt = BF if wide else F16
        add("additive f32", 129, 333, _additive((1, 2, 129, 333), 53, torch.float32, dead_rows=(0, 64, 128)), wide=wide)
        add("additive q dtype", 333, 129, _additive((2, 1, 333, 129), 54, dt, dead_rows=(5, 127, 332)), wide=wide)
        add("additive & causal", 128, 128, _additive((128, 128), 55, torch.float32), causal=True, wide=wide)
        add("gqa 4/2 causal & bool", 129, 333, _rand_bool((2, 4, 129, 333), 56, 0.6), causal=True, Hq=4, Hkv=2, wide=wide)
        add("gqa Hkv=1 bool", 65, 129, _rand_bool((65, 129), 57), Hq=4, Hkv=1, wide=wide)
        add("bshd views causal & bool", 333, 333, _rand_bool((333, 333), 58, 0.6), causal=True, Hq=4, wide=wide, layout="bshd")
    return c


def _in_two_layouts(rule):
    """(buf, wide): `rule` [Sq, Sk] as the leading columns buf[:, :Sk] of a buffer whose row stride is Sk rounded up to 16
    elements (offset 0: 16-byte rows for every mask dtype, the vector block-map pass, with a ragged last key tile when Sk % 64 != 0)
    and as the columns wide[:, 3:3 + Sk] of a buffer with an odd row stride (the element pass).  The views are cut on the device:
    moving a view would pack it."""
    Sq, Sk = rule.shape
    buf = torch.zeros(Sq, (Sk + 15) // 16 * 16, dtype=rule.dtype)
    buf[:, :Sk] = rule
    wide = torch.zeros(Sq, (Sk + 6) | 1, dtype=rule.dtype)
    wide[:, 3:3 + Sk] = rule
    return buf, wide


def aligned_and_sliced_mask(Sq, Sk, kind=torch.bool, seed=60):
    """(rule, buf, wide): one rule, bool or additive (`kind` a float dtype), in the two buffers of _in_two_layouts; among the PARTIAL
    tiles the first block row holds one DENSE and one SKIP tile"""
    if kind == torch.bool:
        rule = _rand_bool((Sq, Sk), seed, 0.6)
        rule[:128, 64:128] = True
        rule[:128, 128:192] = False
    else:
        rule = _additive((Sq, Sk), seed, kind)
        rule[:128, 64:128] = 0.0
        rule[:128, 128:192] = float("-inf")
    return (rule,) + _in_two_layouts(rule)


def case_weights(c):
    return weights_of(c["mask"], c["B"], c["Hq"], c["Sq"], c["Sk"], c["causal"])


def case_values(c):
    return code_values(c["B"], c["Hkv"], c["Sk"], c["D"], c["dtype"])


def selection_cases():
    """name -> (masked case name or dict, neg): the probe-B runs of ops.attention_masked.  The rule is the case's whole rule."""
    m = masked_cases()
    pick = ["causal 333x333 f16 D64", "causal 129x128 bf16 D128", "causal 128x129 f16 D64", "causal 333x63 f16 D64",
            "causal 64x333 bf16 D128", "causal & bool 333x333 f16 D64", "causal & bool 129x128 bf16 D128",
            "bool [Sq,Sk] 333x333 bf16 D128", "bool [Sq,Sk] 64x63 f16 D64", "band 449x449 bf16 D128", "band 449x449 f16 D64",
            "bool [B,1,1,Sk] 127x333 bf16 D128", "additive q dtype 333x129 f16 D64", "gqa 4/2 causal & bool 129x333 bf16 D128",
            "gqa Hkv=1 bool 65x129 f16 D64", "bshd views causal & bool 333x333 bf16 D128", "causal 1x1 bf16 D128",
            "no mask 129x65 bf16 D128", "no mask 129x65 f16 D64"]     # no mask: half the rows target key Sk - 1 = 64 (LAST_KEY_CASES)
    out = {n: (m[n], False) for n in pick}
    for n in ("causal & bool 129x128 bf16 D128", "band 449x449 f16 D64", "gqa 4/2 causal & bool 129x333 bf16 D128"):
        out["negative scale " + n] = (m[n], True)
    return out


def case_allowed(c):
    return case_weights(c) > 0


# Probe-B cases of attention_masked in which every second row targets the last key of a ragged key tail.  A padded key that the
# kernel lets through reads the clamped K row Sk - 1, so it TIES with that target, and carries V = 0 (the zero padding of V^T):
# the row comes out as V[Sk - 1] / 2 or less.  This is what sees the key-tail clamp in rows too wide for probe A.
LAST_KEY_CASES = ("no mask 129x65 bf16 D128", "no mask 129x65 f16 D64")


# ---- every other probe-B input set of the GPU tests, by the same builders (the host tests check each of them)
UNMASKED_SHAPES = {"default": ((2, 2, 333, 1000), (1, 3, 129, 65), (2, 4, 1, 1), (1, 2, 700, 63)),
                   "c4": ((2, 2, 700, 333), (1, 2, 260, 1000)),          # (ops.attention, ops.attention_prepared)
                   "w64": ((1, 3, 2048, 2048), (1, 3, 513, 2085)),
                   "tail": ((1, 33, 2048, 2048), (1, 33, 2048, 2085))}   # 33 heads x 8 query blocks = 256 + 8 workgroups
DUAL_SK_T, DUAL_SK_I = 512, (0, 1, 63, 257)


def unmasked_selection(B, H, Sq, Sk):
    return selection_inputs(torch.ones(B, H, Sq, Sk, dtype=torch.bool), H, 128, BF, seed=6)


def window_selection(name, D, dtype, prepared=False):
    """probe-B inputs of a window case: B, H = 2, 2 for attention_window, 1, 3 for attention_prepared_window"""
    allowed = window_case(name)[3]
    B, H = (1, 3) if prepared else (2, 2)
    return selection_inputs(allowed.expand(B, H, *allowed.shape), H, D, dtype, seed=5 if prepared else 4)


def dual_selection(Sk_i, B=2, H=2, Sq=333):
    """(text set, image set or None, shared q, expect, bound): the text branch's codes live in columns [0, 64), the image branch's
    in [64, 128).  out = bf16(bf16(V_t[pi_t]) + bf16(V_i[pi_i])): each branch within its probe-B bound, the sum within one further
    bf16 ulp (2^-7 relative)"""
    t = selection_inputs(torch.ones(B, H, Sq, DUAL_SK_T, dtype=torch.bool), H, 128, BF, seed=7, dims=(0, 64))
    if not Sk_i:
        return t, None, t["q"], t["expect"], t["bound"]
    i = selection_inputs(torch.ones(B, H, Sq, Sk_i, dtype=torch.bool), H, 128, BF, seed=8, dims=(64, 128))
    expect = t["expect"] + i["expect"]
    return t, i, t["q"] + i["q"], expect, t["bound"] + i["bound"] + 2.0 ** -7 * expect.abs()


# ---- coordinate windows
WINDOW_CASES = {
    "self (6,10,12) r(1,9,11)": ((6, 10, 12), None, (1, 9, 11), None),
    "self (5,9,13) r(1,8,12) ragged": ((5, 9, 13), None, (1, 8, 12), None),
    "self (3,7,11) r(0,2,3) ragged": ((3, 7, 11), None, (0, 2, 3), None),
    "cross (5,9,13)->(6,10,12) r(1,4,6) + a row without keys": ((5, 9, 13), (6, 10, 12), (1, 4, 6), 301),
}


def raster(grid):
    f, h, w = grid
    return torch.stack(torch.meshgrid(torch.arange(f), torch.arange(h), torch.arange(w), indexing="ij"), dim=-1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def window_case(name):
    """(q coords, k coords or None, radius, allowed [Sq, Sk] from the coordinate rule)"""
    gq, gk, radius, planted = WINDOW_CASES[name]
    cq = raster(gq).clone()
    ck = cq if gk is None else raster(gk)
    if planted is not None:
        cq[planted] = torch.tensor([100, 100, 100])                     # far from every key
    allowed = ((cq[:, None, :] - ck[None, :, :]).abs() <= torch.tensor(radius)).all(-1)
    assert (planted is None) == bool(allowed.any(1).all())
    assert {0, 2} <= set(block_map(allowed).flatten().tolist())
    return cq, (None if gk is None else ck), radius, allowed


# ---- text-encoder attention (keep / seg / causal / kv_heads) and the frame-causal VAE attention: probe A only
def bias_cases():
    """name -> dict(H, Hkv, S, D, keep, seg, causal, allowed [S, S])"""
    out = {}
    for name, H, Hkv, S, D, keep, seg, causal in (("keep holes", 4, 4, 77, 64, True, False, False),
                                                  ("causal keep", 4, 4, 77, 64, True, False, True),
                                                  ("causal gqa 4/2", 4, 2, 150, 64, False, False, True),
                                                  ("seg keep D128", 2, 2, 200, 128, True, True, False),
                                                  ("seg causal gqa 4/1 D128", 4, 1, 131, 128, False, True, True)):
        allowed = torch.ones(S, S, dtype=torch.bool)
        kp = sg = None
        if keep:
            kp = torch.ones(S, dtype=torch.uint8)
            kp[[3, 63, 64]] = 0
            kp[S - S // 3:] = 0
            allowed &= kp.bool()[None, :]
        if seg:
            cuts = torch.tensor([16, 17, 64, 129, S])
            sg = torch.bucketize(torch.arange(S), cuts, right=True).to(torch.int32)
            allowed &= sg[:, None] == sg[None, :]
        if causal:
            allowed &= causal_rule(S, S)
        out[name] = dict(H=H, Hkv=Hkv, S=S, D=D, keep=kp, seg=sg, causal=causal, allowed=allowed)
    return out


FRAMECAUSAL_CASES = ((128, 3, 80), (256, 5, 35), (128, 1, 64))          # (D, frames, tokens per frame): boundaries cross the tiles


def framecausal_allowed(frames, per):
    f = torch.arange(frames * per) // per
    return f[None, :] <= f[:, None]


# ------------------------------------------------------------------------------------------------- mutations (host tests)
def flip_positions(Sq, Sk, n_random=24, seed=0):
    """(row, key) decisions to flip: tile corners, the causal diagonal +-1, the last valid key, block-row boundaries, seeded
    random positions; at least 32 distinct ones whenever Sq x Sk allows"""
    rows = sorted({r for r in (0, 1, 31, 32, 63, 64, 126, 127, 128, 129, 255, 256, Sq - 2, Sq - 1) if 0 <= r < Sq})
    keys = sorted({k for k in (0, 1, 31, 32, 62, 63, 64, 65, 127, 128, Sk - 2, Sk - 1) if 0 <= k < Sk})
    pos = {(r, k) for r in rows for k in (0, 63, 64, Sk - 1) if k < Sk} | {(r, k) for r in (0, 127, 128, Sq - 1) if r < Sq for k in keys}
    for r in rows:
        pos |= {(r, k) for k in (r - 1, r, r + 1) if 0 <= k < Sk}
    g = torch.Generator().manual_seed(seed)
    for _ in range(n_random):
        pos.add((int(torch.randint(Sq, (1,), generator=g)), int(torch.randint(Sk, (1,), generator=g))))
    return sorted(pos)


def membership_mutants(w, v, ref, dtype, positions, bh):
    """for every (row, key) flip of the rule at (batch, head) bh: does membership_ok reject the output a kernel with that one wrong
    decision would store (the mutated row, rounded to dtype)?  Returns the positions that were NOT rejected."""
    b, h = bh
    vv = v[b, h // (w.shape[1] // v.shape[1])].to(torch.float64)
    missed = []
    for (i, j) in positions:
        row = w[b, h, i].clone()
        row[j] = 0.0 if row[j] > 0 else 1.0
        den = row.sum()
        mut = (row @ vv) / den if den > 0 else torch.zeros_like(vv[0])
        if membership_ok(mut.to(dtype), ref[b, h, i], dtype):
            missed.append((i, j))
    return missed
