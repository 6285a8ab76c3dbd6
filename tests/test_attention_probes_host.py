"""The attention probes can fail (tests/attention_probes.py): on the CPU, every case's comparison accepts its own expectation and
rejects the expectation of a rule with ONE decision flipped (probe A) or of a row that reads another key (probe B), and the
closed forms agree with F.scaled_dot_product_attention in float64."""
import pytest
import torch
import torch.nn.functional as F

from tests import attention_probes as P


def _mutate_all(w, v, dtype, Sq, Sk, name):
    ref = P.membership_expected(w, v)
    assert P.membership_ok(ref.to(dtype), ref, dtype), name             # the rounded expectation passes its own bar
    pos = P.flip_positions(Sq, Sk)
    assert len(pos) >= min(32, Sq * Sk), (name, len(pos))
    B, Hq = w.shape[:2]
    for bh in {(0, 0), (B - 1, Hq - 1)}:
        missed = P.membership_mutants(w, v, ref, dtype, pos, bh)
        assert not missed, f"{name}: flipped decisions the probe does not see at (batch, head) {bh}: {missed[:8]}"
    return ref


@pytest.mark.parametrize("name", list(P.masked_cases()))
def test_membership_probe_rejects_every_flipped_decision(name):
    c = P.masked_cases()[name]
    w, v = P.case_weights(c), P.case_values(c)
    ref = _mutate_all(w, v, c["dtype"], c["Sq"], c["Sk"], name)
    # the closed form is torch's sdpa of q = 0 under the same mask, in float64
    q = torch.zeros(c["B"], c["Hq"], c["Sq"], c["D"], dtype=torch.float64)
    k = torch.randn(c["B"], c["Hkv"], c["Sk"], c["D"], dtype=torch.float64)
    m = c["mask"]
    if m is not None and m.dtype != torch.bool:
        m = m.to(torch.float64)
    if c["causal"] and m is not None:                                   # torch takes one of the two: fold causal into the mask
        cz = P.causal_rule(c["Sq"], c["Sk"])
        m = (m & cz) if m.dtype == torch.bool else m.masked_fill(~cz, float("-inf"))
    rep = c["Hq"] // c["Hkv"]
    sd = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1), attn_mask=m,
                                        is_causal=c["causal"] and m is None and c["Sq"] <= c["Sk"])
    if c["causal"] and m is None and c["Sq"] > c["Sk"]:
        sd = F.scaled_dot_product_attention(q, k.repeat_interleave(rep, 1), v.double().repeat_interleave(rep, 1),
                                            attn_mask=P.causal_rule(c["Sq"], c["Sk"]))
    live = w.sum(-1) > 0                                                # torch gives NaN or a mean for rows without keys
    assert torch.allclose(sd[live], ref[live], rtol=1e-12, atol=1e-15), name


def test_a_padded_key_let_through_is_seen_in_narrow_rows():
    """A key past Sk that a kernel lets through carries V = 0 (the zero padding of V^T) and a score of 0: a row of n keys comes out
    as ref n / (n + 1).  Stored, that is at least ref / (n + 1) - u ref away from ref, which is over the bar of 2 u ref whenever
    1 / (n + 1) > 3 u: rows of up to 84 keys in bf16, 681 in f16.  What probe A does NOT see: a padded key in a wider row.  Those
    rows are covered by probe B, not here: the masked cases of P.LAST_KEY_CASES (test_last_key_cases_see_a_padded_key_that_ties)
    and, in the prepared layouts, the value planted in the V^T columns past Sk on the GPU."""
    seen = []
    for name, c in P.masked_cases().items():
        w, v = P.case_weights(c), P.case_values(c)
        ref = P.membership_expected(w, v)
        den = w.sum(-1, keepdim=True)
        u = P.U[c["dtype"]]
        narrow = ((den > 0) & (den + 1 < 1 / (3 * u))).expand_as(ref)
        if c["Sk"] % 64 == 0 or not narrow.any():                       # no padded key in the last tile / no narrow row: nothing to see
            continue
        seen.append(name)
        mut = ref * den / (den + 1)
        bad = ((mut.to(c["dtype"]).double() - ref).abs() > 2 * u * ref) & (ref > 0)
        assert bool(bad.any(-1)[narrow[..., 0]].all()), name
    assert len(seen) >= 30, seen                                        # most cases have ragged key tails and narrow rows


def test_last_key_cases_see_a_padded_key_that_ties():
    for name in P.LAST_KEY_CASES:
        c, neg, allowed, s = _selection(name)
        Sk = c["Sk"]
        assert Sk % 64 not in (0, 63)                                   # at least two padded keys in the last tile
        last = s["pi"] == Sk - 1
        assert int(last[0, 0].sum()) >= c["Sq"] // 2                    # every second row targets the last key
        for npad in (1, 64 - Sk % 64):                                  # the tying padded keys halve the row, or worse
            mut = s["expect"] / (1 + npad)
            bad = ((mut.to(c["dtype"]).double() - s["expect"]).abs() > s["bound"]).any(-1)
            assert bool(bad[last].all()), name


@pytest.mark.parametrize("kind", [torch.bool, torch.float32, torch.bfloat16])
def test_aligned_and_sliced_masks_state_one_rule(kind):
    rule, buf, wide = P.aligned_and_sliced_mask(333, 333, kind)
    aligned, sliced = buf[:, :333], wide[:, 3:336]
    assert torch.equal(rule, aligned) and torch.equal(rule, sliced)
    assert aligned.stride() == (336, 1) and aligned.storage_offset() == 0          # 16-element rows: the vector block-map pass
    assert sliced.stride() == (339, 1) and sliced.storage_offset() == 3            # odd stride and offset: the element pass
    w = P.weights_of(rule, 1, 2, 333, 333)
    dense = rule if kind == torch.bool else rule == 0
    assert {0, 1, 2} <= set(P.block_map(w[0, 0] > 0, dense).flatten().tolist())
    _mutate_all(w, P.code_values(1, 2, 333, 128, P.BF), P.BF, 333, 333, f"aligned / sliced {kind}")


@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
def test_window_rule_probe_rejects_every_flipped_decision(name):
    _, _, _, allowed = P.window_case(name)
    Sq, Sk = allowed.shape
    for D, dtype in ((128, P.BF), (64, P.F16)):
        _mutate_all(P.weights_of(allowed, 2, 2, Sq, Sk), P.code_values(2, 2, Sk, D, dtype), dtype, Sq, Sk, name)


@pytest.mark.parametrize("name", list(P.bias_cases()))
def test_bias_rule_probe_rejects_every_flipped_decision(name):
    c = P.bias_cases()[name]
    S = c["S"]
    _mutate_all(P.weights_of(c["allowed"], 1, c["H"], S, S), P.code_values(1, c["Hkv"], S, c["D"], P.BF), P.BF, S, S, name)


@pytest.mark.parametrize("D,frames,per", P.FRAMECAUSAL_CASES)
def test_framecausal_rule_probe_rejects_every_flipped_decision(D, frames, per):
    S = frames * per
    _mutate_all(P.weights_of(P.framecausal_allowed(frames, per), 1, 1, S, S), P.code_values(1, 1, S, D, P.BF), P.BF, S, S, "fc")


@pytest.mark.parametrize("Sk,levels", [(65, 2), (1000, 2), (2048, 3), (2085, 3)])
def test_unmasked_probe_sees_the_key_tail(Sk, levels):
    """no mask: the mean over exactly Sk keys; one key more or fewer at the tail must be rejected (three-level codes above 1024)"""
    v = P.code_values(1, 2, Sk + 1, 128, P.BF, levels)
    ref = P.membership_expected(torch.ones(1, 2, 1, Sk, dtype=torch.float64), v[:, :, :Sk])
    assert P.membership_ok(ref.to(P.BF), ref, P.BF)
    for n in (Sk - 1, Sk + 1):
        wrong = v[:, :, :n].double().mean(2, keepdim=True)
        assert not P.membership_ok(wrong.to(P.BF), ref, P.BF), (Sk, n)
    dropped = (v[:, :, :Sk].double().sum(2, keepdim=True) - v[:, :, 64:65].double()) / (Sk - 1)       # a key in the middle
    assert not P.membership_ok(dropped.to(P.BF), ref, P.BF)


def _selection(name):
    c, neg = P.selection_cases()[name]
    allowed = P.case_allowed(c)
    return c, neg, allowed, P.selection_inputs(allowed, c["Hkv"], c["D"], c["dtype"], seed=3, neg=neg)


def _check_selection(name, s, allowed, Hq, Hkv, dtype, scale=1.0):
    """one probe-B input set: its closed form against the float64 softmax, decoys wherever the rule excludes keys, the loosened
    rule rejected, and a row that reads a neighbouring key, a key 64 away, or its key in another head / batch rejected"""
    Sk = allowed.shape[-1]
    exp, bound = s["expect"], s["bound"]
    assert P.selection_ratio(exp.to(dtype), exp, bound) <= 1.0
    ref = P.selection_reference(s, allowed, scale)
    assert ((ref - exp).abs() <= Sk * 2.0 ** -40 * float(s["v"].abs().max())).all(), name
    assert bool(torch.gather(allowed, 3, s["pi"][..., None])[s["has"]].all())          # every target is an allowed key
    if not bool(allowed.all()):
        if Sk > 2:
            assert s["decoys"] > 0, name
        if s["decoys"]:                                                  # with every excluded key admitted the decoys win
            loose = P.selection_reference(s, torch.ones_like(allowed), scale)
            assert P.selection_ratio(loose, exp, bound) > 1.0, name
    vv = s["v"].double().repeat_interleave(Hq // Hkv, 1)
    B, _, Sq, D = exp.shape

    def rejected(pi2, src=None):
        src = vv if src is None else src
        mut = torch.gather(src, 2, pi2[..., None].expand(B, Hq, Sq, D)) * s["has"][..., None]
        bad = ((mut.to(dtype).double() - exp).abs() > bound).any(-1)
        return bool(bad[s["has"] & (pi2 != s["pi"])].all()) if src is vv else bool(bad[s["has"]].all())

    for shift in (1, -1, 64, -64):
        if Sk > abs(shift):
            assert rejected((s["pi"] + shift) % Sk), (name, shift)
    if Hkv > 1:
        assert rejected(s["pi"], vv.roll(Hq // Hkv, 1)), name
    if B > 1:
        assert rejected(s["pi"], vv.roll(1, 0)), name


@pytest.mark.parametrize("name", list(P.selection_cases()))
def test_selection_probe_closed_form_and_mutants(name):
    c, neg, allowed, s = _selection(name)
    _check_selection(name, s, allowed, c["Hq"], c["Hkv"], c["dtype"], -1.0 if neg else 1.0)


@pytest.mark.parametrize("name", list(P.WINDOW_CASES))
@pytest.mark.parametrize("D,dtype,prepared", [(128, P.BF, False), (64, P.F16, False), (128, P.BF, True)])
def test_window_selection_inputs(name, D, dtype, prepared):
    s = P.window_selection(name, D, dtype, prepared)
    B, H = s["q"].shape[:2]
    allowed = P.window_case(name)[3]
    _check_selection(name, s, allowed.expand(B, H, *allowed.shape), H, H, dtype)


@pytest.mark.parametrize("shape", sorted({sh for group in P.UNMASKED_SHAPES.values() for sh in group}))
def test_unmasked_selection_inputs(shape):
    B, H, Sq, Sk = shape
    s = P.unmasked_selection(*shape)
    assert bool((s["pi"] >= Sk - 64).any()) and bool((s["pi"] < 64).any())             # targets in the last tile and in the first
    _check_selection(str(shape), s, torch.ones(B, H, Sq, Sk, dtype=torch.bool), H, H, P.BF)


@pytest.mark.parametrize("Sk_i", P.DUAL_SK_I)
def test_dual_selection_inputs(Sk_i):
    """each branch of the dual probe on its own key set, under the SHARED q (the other branch's half of q must score nothing)"""
    t, i, q, expect, bound = P.dual_selection(Sk_i)
    for s in (t, i) if i else (t,):
        B, H, Sq = s["has"].shape
        _check_selection(f"dual {Sk_i}", dict(s, q=q), torch.ones(B, H, Sq, s["k"].shape[2], dtype=torch.bool), H, H, P.BF)
    # the sum of the two branches, stored with the kernel's three roundings, passes; one branch reading a neighbouring key does not
    both = t["expect"].to(P.BF).double() + (i["expect"].to(P.BF).double() if i else 0)
    assert P.selection_ratio(both.to(P.BF), expect, bound) <= 1.0
    wrong = torch.gather(t["v"].double(), 2, ((t["pi"] + 1) % P.DUAL_SK_T)[..., None].expand_as(expect)) + (i["expect"] if i else 0)
    assert bool((((wrong.to(P.BF).double() - expect).abs() > bound).any(-1)).all())


def test_selection_targets_reach_late_tiles_and_every_tile_offset():
    c, _, allowed, s = _selection("bshd views causal & bool 333x333 bf16 D128")
    pi = s["pi"]
    assert bool((pi >= 64).any()) and bool((pi[:, :, 200:] < 64).any())                 # late targets and first-tile targets
    assert len(set((pi % 64).flatten().tolist())) == 64
    pi = _selection("causal 129x128 bf16 D128")[3]["pi"]                                # even rows: the coded key next to the diagonal
    assert bool((pi[0, 0, 0:128:2] >= torch.arange(0, 128, 2) - 3).all()) and bool((pi[0, 0, 0:128:2] <= torch.arange(0, 128, 2)).all())
