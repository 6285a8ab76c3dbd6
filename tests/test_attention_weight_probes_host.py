"""Host proofs of probe C (tests/attention_weight_probes.py), for every case the GPU file runs and on one (batch, head) of it:
(a) an f32 emulation of the flash loop is accepted (64-key tiles, 32-key tiles, and l summed from the rounded P under the bar of
    that arithmetic);
(b) single wrong decisions, evaluated exactly in float64 (the loop mutations in the f32 emulation), are rejected;
(c) the conditions the derivation of the bars leans on hold.
No GPU.

What the older bars make of the same mutants (old_bar_accepts: rel-L2 < 1e-2, 3 bf16 ulps of the largest magnitude, |lse - ref| <=
4e-3), counted over the cases by test_what_the_old_bars_let_through: see the table at the end of this file."""
import math

import pytest
import torch

from tests import attention_probes as P
from tests import attention_weight_probes as W

NAMES = list(W.problems())
LN2 = math.log(2.0)


def _head(name):
    """(p, n, logw, v, ref, ref_lse, allowed) of the last (batch, head) of the problem"""
    p = W.problems()[name]
    q, k, v = W.inputs(name)
    b, h = p["B"] - 1, p["Hq"] - 1
    w = W.head_weights(p, b, h)
    ref, ref_lse = W.reference(name)
    return p, W.head_scores(p, q, k, b, h), torch.log(w), v[b, h // (p["Hq"] // p["Hkv"])], ref[b, h], ref_lse[b, h], w > 0


def _changed_rows(dn, allowed):
    """rows whose softmax a score change dn moves at all: dn is not constant over the row's allowed keys"""
    hi = torch.where(allowed, dn, torch.full((), -math.inf, dtype=dn.dtype)).max(-1).values
    lo = torch.where(allowed, dn, torch.full((), math.inf, dtype=dn.dtype)).min(-1).values
    return allowed.any(-1) & (hi > lo)


def exact_mutants(name):
    """label -> (out, lse, rows that must be rejected through the output alone, rows that must be rejected once the lse counts)"""
    p, n, logw, v, ref, ref_lse, allowed = _head(name)
    q, k, _ = W.inputs(name)
    b, h = p["B"] - 1, p["Hq"] - 1
    qh, kh = q[b, h].double(), k[b, h // (p["Hq"] // p["Hkv"])].double()
    D, scale = p["D"], W.scale_of(p)
    many = _changed_rows(scale * n, allowed)          # a change of the scale moves a row iff its scores are not all equal
    out = {}

    def add(label, n2, scale2=scale, logw2=logw, rows=None):
        o, l = W.exact_head(n2, logw2, scale2, v)
        touched = ((scale2 * n2 + logw2 != scale * n + logw) & allowed).any(-1)      # the lse moves with any exponent of the row
        out[label] = (o, l, _changed_rows(n2 - n, allowed) if rows is None else rows, touched)

    for label, cols in (("column 0 dropped", [0]), (f"column D-1 dropped", [D - 1]), ("an interior column dropped", [D // 2 - 3]),
                        ("columns 8..15 dropped", list(range(8, 16)))):
        add(label, n - qh[:, cols] @ kh[:, cols].t())
    ks = kh.clone()
    ks[:, [10, 11]] = kh[:, [11, 10]]
    add("k columns 10 and 11 swapped", qh @ ks.t())
    add("scale times 1 + 2^-6", n, scale * (1 + 2.0 ** -6), rows=many)
    add("natural exp for exp2 (log2 e missing)", n, scale * LN2, logw * LN2, rows=many)
    if p["scale"] is not None and abs(p["scale"]) != D ** -0.5:
        add("D^-0.5 for the explicit scale", n, D ** -0.5, rows=many)
    x = scale * n + logw
    top = x.argmax(-1)
    bump = torch.zeros_like(n)
    bump[torch.arange(n.shape[0]), top] = 1.0 if scale > 0 else -1.0
    add("the strongest key's score one unit up", n + bump)
    return out


def loop_mutants(name):
    """label -> (out, lse) of the f32 flash loop with one wrong step"""
    p, n, logw, v, ref, ref_lse, allowed = _head(name)
    args = (n, logw, W.scale_of(p), v, p["dtype"])
    return {"rescale skipped on a raised maximum": W.flash_head(*args, skip_rescale=True),
            "l from the last tile only": W.flash_head(*args, l_last_tile=True),
            "store truncated": W.flash_head(*args, trunc=True)}


def _verdict(p, out, lse, ref, ref_lse, m=None, rounded=None):
    """rows rejected through the output, and through output or lse"""
    bar = W.out_bar(p, m)
    rows = W.rows_rejected(out, ref, bar)
    return rows, W.rows_rejected(out, ref, bar, lse, ref_lse, W.e_l(p, rounded) * (2 if p.get("merged") else 1))


# ------------------------------------------------------------------------------------------------------------- (c) conditions
@pytest.mark.parametrize("name", NAMES)
def test_conditions(name):
    p = W.problems()[name]
    q, k, v = W.inputs(name)
    assert q.dtype == k.dtype == v.dtype == p["dtype"]
    assert bool((q.double().abs() == 1).all()) and bool((k.double().abs() == 1).all())        # +-1: every score is an integer
    ref, ref_lse = W.reference(name)
    assert 0.0 <= float(ref.min()) and float(ref.max()) <= 1.0 + 1e-12 < W.SENTINEL
    live = ~torch.isinf(ref_lse)
    assert not torch.isnan(ref_lse).any() and (not bool(live.any()) or float(ref_lse[live].abs().max()) < 100 < W.LSE_SENTINEL)
    assert bool((ref[~live] == 0).all()) and bool((ref_lse[~live] == -math.inf).all())
    heads = range(min(p["Hq"], p.get("period") or p["Hq"]))
    for b in range(p["B"]):
        for h in heads:
            n = W.head_scores(p, q, k, b, h)
            assert bool((n == n.round()).all()) and float(n.abs().max()) <= p["D"]
            w = W.head_weights(p, b, h)
            ex = (W.scale_of(p) * n + torch.log(w)) * W.LOG2E
            hi = ex.max(-1).values
            lo = torch.where(w > 0, ex, torch.full((), math.inf, dtype=torch.float64)).min(-1).values
            rows = (w > 0).any(-1)
            if bool(rows.any()):
                assert float(hi[rows].max()) <= W.A_MAX and float(lo[rows].min()) >= -W.A_MAX
                assert float((hi - lo)[rows].max()) <= W.A_MAX
            if p["family"] == "staged":      # every tile that holds an allowed key raises the row's maximum by 2 .. 4 binades
                tmax = torch.stack([ex[:, j:j + 64].max(-1).values for j in range(0, p["Sk"], 64)], 1)
                low = torch.where(w > 0, ex, torch.full((), math.inf, dtype=torch.float64))
                tmin = torch.stack([low[:, j:j + 64].min(-1).values for j in range(0, p["Sk"], 64)], 1)
                both = torch.isfinite(tmax[:, 1:]) & torch.isfinite(tmax[:, :-1])
                assert bool(both.any())
                rise = (tmax[:, 1:] - tmax[:, :-1])[both]
                assert 2.0 <= float(rise.min()) and float(rise.max()) <= 4.0, (float(rise.min()), float(rise.max()))
                assert bool((tmin[:, 1:] > tmax[:, :-1])[both].all())       # every key of a tile beats every key before it


def test_the_case_table_covers_every_entry_and_launch_variant():
    names = " | ".join(NAMES)
    for s in (x for g in P.UNMASKED_SHAPES.values() for x in g):
        assert "plain " + "x".join(map(str, s)) in W.problems()
    for D in (40, 64, 192, 320, 256, 384, 512):
        assert f"D{D}" in names or f"head dim {D}" in names
    for case in P.masked_cases():
        assert "masked " + case in W.problems()
    assert sum(p["family"] == "staged" for p in W.problems().values()) >= 3
    assert any(p["scale"] is not None and p["scale"] < 0 for p in W.problems().values())


# ------------------------------------------------------------------------------------------- (a) the f32 flash loop is accepted
@pytest.mark.parametrize("name", NAMES)
def test_f32_flash_loop_is_accepted(name):
    p, n, logw, v, ref, ref_lse, allowed = _head(name)
    args = (n, logw, W.scale_of(p), v, p["dtype"])
    for label, kw, m, rounded in (("tile 64", dict(tile=64), 2, None), ("tile 32", dict(tile=32), 2, None),
                                  ("l from rounded P", dict(l_rounded=True), 3, p["dtype"])):
        out, lse = W.flash_head(*args, **kw)
        ratio, zeros = W.out_ratio(out, ref, m * W.U[p["dtype"]] + W.e_s(p))
        lr = W.lse_ratio(lse, ref_lse, W.e_l(p, rounded))
        assert zeros and ratio <= 1.0 and lr <= 1.0, (name, label, ratio, lr)


# --------------------------------------------------------------------------------------- (b) single wrong decisions are rejected
@pytest.mark.parametrize("name", NAMES)
def test_exact_mutants_are_rejected(name):
    p, n, logw, v, ref, ref_lse, allowed = _head(name)
    for label, (out, lse, rows_out, rows_lse) in exact_mutants(name).items():
        got_out, got_all = _verdict(p, out, lse, ref, ref_lse)
        if not bool(rows_out.any()):
            continue
        frac = float(got_out[rows_out].float().mean())
        # A scale off by 2^-6 moves every weight of a row by a few per cent in both directions, and a column is the share of a
        # whole residue class: the shares of some rows stay within the bar (one row in a hundred below 500 keys, one in six at
        # 2048).  Most rows are still rejected, and every row by its lse.
        soft = label == "scale times 1 + 2^-6"
        assert frac > 0.5 if soft else frac == 1.0, (name, label, frac, int(rows_out.sum()))
        if p.get("lse"):
            assert bool(got_all[rows_lse].all()), (name, label, "lse")


def test_swapped_columns_are_rejected_in_the_rows_they_touch():
    """q_i[10] == q_i[11]: the swap leaves row i alone; otherwise every score of the row moves by 0 or +-2"""
    for name in ("plain 2x2x333x1000", "masked causal 333x333 f16 D64", "wide D384 bf16"):
        p, n, logw, v, ref, ref_lse, allowed = _head(name)
        out, lse, rows, _ = exact_mutants(name)["k columns 10 and 11 swapped"]
        got, _ = _verdict(p, out, lse, ref, ref_lse)
        assert 0.3 < float(rows.float().mean()) < 0.7 and bool(got[rows].all()) and not bool(got[~rows].any())


@pytest.mark.parametrize("name", NAMES)
def test_loop_mutants_are_rejected(name):
    p, n, logw, v, ref, ref_lse, allowed = _head(name)
    x = (W.scale_of(p) * n + logw) * W.LOG2E
    tmax = torch.stack([x[:, j:j + 64].max(-1).values for j in range(0, p["Sk"], 64)], 1).ceil()
    run = torch.cummax(tmax, 1).values
    # a row is touched by a skipped rescale iff its integer running maximum rises after a tile that held keys
    raised = (torch.isfinite(run[:, :-1]) & (run[:, 1:] > run[:, :-1])).any(-1)
    # ... and by l from the last tile iff an earlier tile held keys as well
    early = torch.isfinite(tmax[:, :-1]).any(-1) & allowed.any(-1)
    mut = loop_mutants(name)
    for label, rows in (("rescale skipped on a raised maximum", raised), ("l from the last tile only", early)):
        out, lse = mut[label]
        got, _ = _verdict(p, out, lse, ref, ref_lse)
        assert bool(got[rows].all()), (name, label, int((~got[rows]).sum()), int(rows.sum()))
    if p["family"] == "staged":
        assert bool(raised[allowed[:, 64:].any(-1)].all())          # every row with keys past the first tile


def test_a_truncating_store_is_rejected_in_most_cases():
    """Truncation stays below one ulp, which is 2 u at the bottom of a binade: alone it is the size of the bar.  On top of the
    rounding of P it crosses the bar in some element of most cases, but not of every case (one-key rows come out exact)."""
    hit = 0
    for name in NAMES:
        p, n, logw, v, ref, ref_lse, allowed = _head(name)
        out, lse = loop_mutants(name)["store truncated"]
        hit += W.out_ratio(out, ref, W.out_bar(p))[0] > 1.0
    assert hit >= 0.75 * len(NAMES), (hit, len(NAMES))


OLD_BAR_GAPS = {"column 0 dropped": ("plain 1x3x513x2085", "plain 1x33x2048x2048"),
                "an interior column dropped": ("plain 1x3x2048x2048", "staged 1x2x200x333"),
                "scale times 1 + 2^-6": ("plain 1x33x2048x2085", "window self (3,7,11) r(0,2,3) ragged bf16 D128",
                                         "framecausal D256 5x35", "bias causal keep"),
                "the strongest key's score one unit up": ("plain 1x3x513x2085", "staged 1x2x200x333", "wide staged D512 bf16")}


@pytest.mark.parametrize("label", list(OLD_BAR_GAPS))
def test_what_the_old_bars_let_through(label):
    """mutants that pass rel-L2 < 1e-2, 3 bf16 ulps and the 4e-3 lse ceiling, and that probe C rejects"""
    for name in OLD_BAR_GAPS[label]:
        p, n, logw, v, ref, ref_lse, allowed = _head(name)
        out, lse, rows, _ = exact_mutants(name)[label]
        assert W.old_bar_accepts(out, ref, lse if p.get("lse") else None, ref_lse), (name, label)
        got, _ = _verdict(p, out, lse, ref, ref_lse)
        assert float(got[rows].float().mean()) > 0.5 and W.out_ratio(out, ref, W.out_bar(p))[0] > 3.0, (name, label)


# What the older bars make of each mutant, over the 115 cases (one head each; 110 hold a row with more than one key), against
# probe C:
#   mutant                                   probe C: every touched row rejected      old bars accept the whole output in
#   column 0 / D-1 / interior dropped        all cases                                4 / 5 / 5 cases (the 2048-key shapes, staged)
#   columns 8..15 dropped                    all cases                                none
#   k columns 10 and 11 swapped              all cases (the rows with q10 != q11)     none
#   scale times 1 + 2^-6                     89 cases; > 2/3 of the rows elsewhere,   13 cases (2048 keys, narrow windows,
#                                            every row once the lse counts            framecausal D256, attention_bias)
#   natural exp for exp2                     all cases                                none
#   D^-0.5 for the explicit scale            both explicit-scale cases                none
#   the strongest key's score one unit up    all cases                                6 cases (2048 keys, the staged family)
#   rescale skipped on a raised maximum      all cases (every row whose max rises)    none
#   l from the last tile only                all cases                                none
#   store truncated                          some element in 92 cases, never all      all cases
