"""No GPU: the conditions under which tests/norm_rope_probes.py may judge a kernel, for every case tests/test_gpu_norm_rope_probes.py
runs (the same case tables), the single wrong decisions its verdicts reject and the older two-number bar accepts, and the shapes
apexmi_qk_rms_rope_rows must refuse because its V^T tiles would leave their rows."""
import pytest
import torch

from tests import norm_rope_probes as N
from tests.norm_rope_probes import BF, F32


def _accepts(out, ref, env, what):
    v = N.verdict(out, ref, env)
    assert v.passed, f"{what}: {N.describe(v, out, ref, env)}"
    return v


# ------------------------------------------------------------------------------------------------------------------ conditions
def test_constants_match_the_library_and_the_sentinel_is_bf16_exact():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    assert (N.ROPE_INTERLEAVED, N.ROPE_COMPLEX, N.ROPE_NONE) == (lib.ROPE_INTERLEAVED, lib.ROPE_COMPLEX, lib.ROPE_NONE)
    assert float(torch.tensor(N.SENTINEL).to(BF)) == N.SENTINEL
    assert N.EPS == float(torch.tensor(1e-6, dtype=F32))


def test_exact_operands_sit_on_their_grids_and_tell_neighbours_apart():
    for mode in (N.ROPE_INTERLEAVED, N.ROPE_COMPLEX):
        t = N.rope_table(207, mode)
        N.check_grid(table=t)
        planes = (t[0], t[1]) if mode == N.ROPE_INTERLEAVED else (t[..., 0], t[..., 1])
        for p in planes:                                   # one step along either axis changes the value
            assert bool((p[1:] != p[:-1]).all()) and bool((p[:, 1:] != p[:, :-1]).all())
    t = N.rope_table(207, N.ROPE_INTERLEAVED)
    assert bool((t[:, :, 0::2] != t[:, :, 1::2]).all()), "interleaved mode: the two entries of a pair must differ"
    for Dh in (80, 128):
        cos, sin = N.half_tables(N.ROPE_HALF_ROWS, Dh)
        N.check_grid(table=cos), N.check_grid(table=sin)
        assert bool((cos[:, :Dh // 2] != cos[:, Dh // 2:]).all()) and bool((sin[:, :Dh // 2] != sin[:, Dh // 2:]).all())
    x = N.grid_x(131, 8 * 128, 1)
    N.check_grid(x64=x)
    assert bool((x[1:] != x[:-1]).all()) and bool((x[:, 1:] != x[:, :-1]).all())
    assert not torch.equal(N.grid_x(5, 128, 1), N.grid_x(5, 128, 2))


@pytest.mark.parametrize("H", N.QKV_H)
def test_qkv_cases_conditions(H):
    cases = N.qkv_cases(H)
    # the rotation of the k / v presence and of the spare V^T tiles reaches every S and every rope mode
    for key in ("S", "mode", "row0"):
        for val in {getattr(c, key) for c in cases}:
            sub = [c for c in cases if getattr(c, key) == val]
            assert {c.kv for c in sub} == set(N._KVS) and {c.skp_extra for c in sub} == {0, 64}, (key, val)
    for case in cases:
        o, want = N.qkv_operands(case), N.qkv_expected(case)
        dt = F32 if case.f32 else BF
        assert N.vt_call_fits(case.S, case.Skp, case.row0) and case.S_out > case.row0 + case.S
        for name, x, w, w2 in (("q", o["q"], o["wq"], o["wq2"]), ("k", o["k"], o["wk"], o["wk2"])):
            if x is None:
                continue
            ref, env = want[name]
            assert float(ref.abs().max()) < N.SENTINEL / 4
            for order in N.ORDERS if case.norm != "none" else ("torch",):
                emu = N.qk_emulate(x, H, w, w2, case.split, o["table"], case.mode, case.row0, order, dt)
                if case.norm == "none":                   # the claim of the exact probes: plain f32 arithmetic is exact on the grid
                    N.check_grid(x64=x)
                    assert torch.equal(emu, N.store(ref, dt)) and float(env.max()) <= 2 * N.U * 8, case.id
                else:
                    v = _accepts(emu, ref, env, f"{case.id} {name} {order}")
                    assert v.undecided <= N.UNDECIDED_CAP, (case.id, v.undecided)
        if o["v"] is not None:
            N.check_grid(x64=o["v"])


def test_rope_half_and_v_transpose_cases_conditions():
    for Dh, heads, f32 in N.ROPE_HALF_CASES:
        buf, cos, sin, want = N.rope_half_case(Dh, heads)
        keep = buf == N.SENTINEL
        N.check_grid(x64=buf[~keep])
        assert torch.equal(want[keep], buf[keep]) and float(want[~keep].abs().max()) <= 8 and int(keep.sum()) == N.ROPE_HALF_ROWS * (heads * (128 - Dh) + 8)
        a = buf.float()                                    # plain f32 arithmetic is exact on the grid
        for hd in range(heads):
            lo, hi = a[:, hd * 128: hd * 128 + Dh // 2].clone(), a[:, hd * 128 + Dh // 2: hd * 128 + Dh].clone()
            a[:, hd * 128: hd * 128 + Dh // 2] = lo * cos[:, :Dh // 2] - hi * sin[:, :Dh // 2]
            a[:, hd * 128 + Dh // 2: hd * 128 + Dh] = hi * cos[:, Dh // 2:] + lo * sin[:, Dh // 2:]
        assert torch.equal(a.double(), want)
    for S, H in N.V_TRANSPOSE_CASES:
        assert N.vt_call_fits(S, N.round_up(S, 64) + 64, 0)


@pytest.mark.parametrize("C", N.BLOCK_C + N.WAVE_C)
def test_ln_cases_conditions(C):
    """(1) undecided share <= 3 %, (2) the reference in f32, three summation orders, accepted everywhere: every case of the width"""
    worst_u, worst_r = 0.0, 0.0
    for case in N.ln_cases(C):
        ref, env = N.ln_case_ref(case)
        for order in N.ORDERS:
            v = _accepts(N.ln_emulate(case, order), ref, env, f"{case.id} {order}")
            worst_r = max(worst_r, v.ratio)
        if N.storage_dtypes(case.storage)[1] == BF:
            assert v.undecided <= N.UNDECIDED_CAP, (case.id, v.undecided)
            worst_u = max(worst_u, v.undecided)
    print(f"C = {C}: largest undecided share {worst_u:.4f}, worst |err| / env of the f32 evaluations {worst_r:.3f}")


def test_ln_rows_hold_the_decisions_they_are_built_for():
    for C in (256, 5120):
        x = N.ln_rows(C, False)
        ms = x.pow(2).mean(-1)
        assert 0.5 * N.EPS < float(ms[N.ROW_TINY]) < 2 * N.EPS, "row 1: mean square about eps"
        assert float(x[N.ROW_ZERO].abs().max()) == 0.0
        off = x[N.ROW_OFFSET]
        assert float(off.mean()) > 8 * float(off.std()), "row 5: mean >> spread"
        mv = N.mod_vectors(C)
        for k, t in mv.items():                            # a neighbour's column or chunk is a different value
            t = t.float()
            assert bool((t[1:] != t[:-1]).all()) and bool((t[8:] != t[:-8]).all()), k
        assert float((mv["scale"] != mv["scale2"]).float().mean()) > 0.9 and float((mv["shift"] != mv["shift2"]).float().mean()) > 0.9
    case = N.LnCase(256, 13, "bf16", "affine_mod")
    ref, _ = N.ln_case_ref(case)
    mv = N.mod_vectors(256)
    assert torch.equal(ref[N.ROW_ZERO], mv["beta"].double() * (1 + mv["scale"].double()) + mv["shift"].double())
    assert bool(torch.isfinite(ref).all())


@pytest.mark.parametrize("case", N.rows_cases(), ids=lambda c: c.id)
def test_rows_cases_conditions(case):
    """qk_rms_rope_rows is judged through the three passes it is documented to equal: the whole-row RMSNorm under the ln_modulate
    verdict, then the RoPE + layout pass on the stored norm (operands without error of their own)."""
    o = N.rows_operands(case.H, case.S, case.f32)
    C, dt = case.H * 128, F32 if case.f32 else BF
    table = N.rope_table(case.S_out, case.mode)
    assert N.vt_call_fits(case.S, case.Skp, case.row0)
    for x, w in ((o["q"], o["wq"]),) + (((o["k"], o["wk"]),) if case.kv == "qkv" else ()):
        ref, env = N.ln_ref(x, C, rms=True, gamma=w)
        for order in N.ORDERS:
            mean, rstd = N.ln_stats32(x.float(), True, order)
            stored = (x.float() * rstd * w.float()).to(dt)
            v = _accepts(stored, ref, env, f"{case.id} norm {order}")
            assert v.undecided <= N.UNDECIDED_CAP
        ref2, env2 = N.rope_only_expected(stored.double(), case.H, table, case.mode, case.row0)
        emu = N.qk_emulate(stored.double(), case.H, None, None, 0, table, case.mode, case.row0, "torch", dt)
        if case.f32:
            _accepts(emu, ref2, env2, f"{case.id} rope")
        else:                                              # 13-bit products, one rounding of their sum: exact, no envelope
            assert torch.equal(emu, N.store(ref2, BF)), case.id


def test_cast_probe_inputs_cover_every_normal_code_point_and_no_subnormal_result():
    x = N.cast_probe_inputs()
    assert x.numel() == 3 * 65024 + 8 and not bool(torch.isnan(x).any())
    want = x.to(BF)
    tiny = float(torch.finfo(BF).tiny)
    assert bool(((want.float().abs() >= tiny) | (want.float() == 0)).all()), "no subnormal result"
    codes = N.normal_bf16_codes().numel()
    mid = x[codes:2 * codes]                               # exact ties: half of them round up, half down (to even)
    up = (mid.to(BF).float().abs() > mid.abs()).float().mean()
    assert abs(float(up) - 0.5) < 1e-3
    top = float(torch.finfo(BF).max)                       # the largest float overflows; the first float above the largest bf16 does not
    assert bool(torch.isinf(want[-6:-2].float()).all()) and want[-2:].float().tolist() == [top, -top]
    assert bool(torch.isinf(x[codes:2 * codes].to(BF).float()).sum() == 2), "the midpoint above the largest code point goes to inf"
    assert bool(torch.isnan(N.cast_nan_inputs()).all())
    allc = N.all_bf16_codes()
    assert allc.numel() == 65536 and allc.view(torch.int16).unique().numel() == 65536


# -------------------------------------------------------------------------------------------------------------------- mutations
def _mutant(case, mut, order="chunk8", x=None, old_bar=None):
    """the verdict accepts the f32 evaluation and rejects the mutated one on a DECIDED element; old_bar: what the two-number bar says"""
    ref, env = N.ln_case_ref(case, x)
    _accepts(N.ln_emulate(case, order, x=x), ref, env, case.id)
    bad = N.ln_emulate(case, order, mut, x=x)
    v = N.verdict(bad, ref, env)
    assert v.rejects_decided(), f"{case.id}: '{mut}' slips through the verdict"
    if old_bar is not None:
        assert N.old_bar_accepts(bad, ref) == old_bar, f"{case.id}: '{mut}' against the two-number bar"
    return v


def test_mutation_variance_over_c_minus_1():
    _mutant(N.LnCase(5120, 13, "bf16", "plain"), "cm1", old_bar=True)         # relative error 1e-4
    _mutant(N.LnCase(4096, 5, "f32", "mod"), "cm1")


def test_mutation_eps_dropped():
    # rows 0, 3, 4: on the row scaled by 2^-7 eps is a 1e-3 effect, which the two-number bar accepts ...
    x = N.ln_rows(2048, False)[[0, N.ROW_SMALL, 4]]
    _mutant(N.LnCase(2048, 3, "bf16", "plain"), "noeps", x=x, old_bar=True)
    _mutant(N.LnCase(2048, 3, "bf16", "mod"), "noeps", x=x, old_bar=True)
    # ... and on the row whose mean square is about eps it moves the result by tens of percent (and the all-zero row to NaN)
    case = N.LnCase(2048, 2, "bf16", "plain")
    ref, _ = N.ln_case_ref(case)
    bad = N.ln_emulate(case, "chunk8", "noeps").double()
    assert float(((bad[N.ROW_TINY] - ref[N.ROW_TINY]).abs() / ref[N.ROW_TINY].abs().clamp_min(0.1)).median()) > 0.2
    _mutant(N.LnCase(2048, 13, "bf16", "mod"), "noeps")


def test_mutation_second_bf16_rounding_before_the_modulation():
    _mutant(N.LnCase(2048, 13, "bf16", "mod"), "round_twice", old_bar=True)
    _mutant(N.LnCase(3072, 13, "f32in", "affine_mod"), "round_twice", old_bar=True)   # the f32-in form documents ONE rounding


def test_mutation_one_pass_variance_on_the_offset_row():
    """E[x^2] - mean^2 loses mean^2 / var in relative accuracy.  On bf16 rows 8 + k / 16 the squares are 16-bit numbers and their
    f32 sums nearly exact, so the offset row of this proof carries float detail (the f32-in form) at mean / spread = 157."""
    C = 256
    c = torch.arange(C)
    x = N.ln_rows(C, True).clone()
    x[N.ROW_OFFSET] = (N.offset_row(C, 1) + (((c * 37) % 101).double() / 101 - 0.5) / 16).float().double()
    for order in N.ORDERS:
        v = _mutant(N.LnCase(C, 13, "f32in", "mod"), "onepass", order, x=x, old_bar=True)
        assert not bool((~v.ok)[torch.arange(13) != N.ROW_OFFSET].any()), "only the offset row is affected"


def test_mutation_modulation_read_one_chunk_off():
    for form in ("scale", "shift", "mod"):
        _mutant(N.LnCase(2048, 5, "bf16", form), "chunk_off")


def test_mutation_split_off_by_one_row():
    for M, split in ((13, 3), (13, 12), (5, 0), (5, 4)):
        v = _mutant(N.LnCase(3072, M, "bf16", "split", split), "split_off")
        assert not bool((~v.ok)[torch.arange(M) != split].any()), "exactly the row at the boundary"


def test_mutation_last_row_of_an_odd_m_from_the_previous_rows_data():
    for M in (5, 13):
        v = _mutant(N.LnCase(3072, M, "bf16", "mod"), "prev_row")
        assert not bool((~v.ok)[:M - 1].any())


def _exact_case(mode, row0=64):
    return N.QkvCase(4, 100, row0, mode, "none", "qkv")


def test_mutation_rope_entry_of_the_pairs_other_element():
    case = _exact_case(N.ROPE_INTERLEAVED)
    good, bad = N.qkv_expected(case), N.qkv_expected(case, mut="other_entry")
    for name in ("q", "k"):
        a, b = N.store(good[name][0], BF), N.store(bad[name][0], BF)
        assert float((a != b).float().mean()) > 0.9, "nearly every element tells the two entries apart"


def test_mutation_rope_row_s_instead_of_row0_plus_s():
    for mode in (N.ROPE_INTERLEAVED, N.ROPE_COMPLEX):
        case = _exact_case(mode)
        good, bad = N.qkv_expected(case), N.qkv_expected(case, mut="row_s")
        assert float((N.store(good["q"][0], BF) != N.store(bad["q"][0], BF)).float().mean()) > 0.9
        zero = _exact_case(mode, row0=0)                   # (with row0 = 0 the two readings coincide: why the GPU cases use 64)
        assert torch.equal(N.qkv_expected(zero)["q"][0], N.qkv_expected(zero, mut="row_s")["q"][0])


def test_mutation_vt_pad_left_non_zero_and_stores_outside_the_tiles():
    case = _exact_case(N.ROPE_NONE)
    v = N.qkv_operands(case)["v"]
    want = N.qkv_expected(case)["vt"]
    assert N.mismatches(N.vt_expected(v, case.H, case.Skp, case.row0, BF, pad=N.SENTINEL), want)      # pad never written
    assert N.mismatches(N.vt_expected(v, case.H, case.Skp, case.row0, BF, pad=0.125), want)
    lo, hi = N.vt_written_columns(case.S, case.row0)
    assert (lo, hi) == (64, 192) and bool((want[:, :, :lo] == N.SENTINEL).all()) and bool((want[:, :, hi:] == N.SENTINEL).all())
    assert bool((want[:, :, lo + case.S:hi] == 0).all())
    assert torch.equal(want[1, 5, lo:lo + case.S].double(), v[:, 128 + 5])


def test_mutation_truncation_at_the_store():
    # exact probes: the reference lands between code points on a share of the elements, ties included
    case = _exact_case(N.ROPE_COMPLEX)
    ref = N.qkv_expected(case)["q"][0]
    rne, cut = N.store(ref, BF), N.truncate_bf16(ref.float())
    inexact = rne.double() != ref
    assert float(inexact.float().mean()) > 0.1 and bool((rne != cut)[inexact].any())
    ties = ((ref * 2 ** 7) % 1 == 0) & inexact             # not all exact references are ties; those that are go to even
    assert bool(ties.any())
    # the casts: truncation is wrong on every midpoint-or-above input
    x = N.cast_probe_inputs()[:3 * 65024]
    assert float((N.truncate_bf16(x) != x.to(BF)).float().mean()) > 0.4
    # the norms
    _mutant(N.LnCase(3072, 13, "bf16", "mod"), "trunc")
    _mutant(N.LnCase(256, 5, "f32in", "plain"), "trunc")


def test_verdict_rejects_non_finite_and_reports_the_margin():
    case = N.LnCase(256, 5, "bf16", "mod")
    ref, env = N.ln_case_ref(case)
    out = N.ln_emulate(case)
    v = N.verdict(out, ref, env)
    assert v.passed and 0 <= v.ratio < 1
    for bad in (float("nan"), float("inf")):
        o = out.clone()
        o[2, 7] = bad
        vb = N.verdict(o, ref, env)
        assert not vb.passed and not bool(vb.ok[2, 7]) and int((~vb.ok).sum()) == 1
    f = N.LnCase(256, 5, "f32", "mod")
    ref, env = N.ln_case_ref(f)
    o = N.ln_emulate(f).clone()
    o[1, 3] += 2 * float(env[1, 3]) + 1e-7
    assert not bool(N.verdict(o, ref, env).ok[1, 3])


# --------------------------------------------------------------------------------------------------------------------- refusals
LISTED = [(100, 104, 0), (100, 128, 8), (64, 64, 64), (1, 8, 0)]


def _overrunning_triples():
    """(S, Skp, row0) with 8-aligned Skp and row0 (what the 16-byte stores need) and Skp >= row0 + S (the data fits) or not, whose
    whole-tile writes, by the model of the documented tiling, leave their row of V^T or start off a tile"""
    out = []
    for S in (1, 5, 63, 64, 65, 100, 128, 131):
        for row0 in (0, 8, 64, 72):
            for Skp in sorted({N.round_up(row0 + S, 8), N.round_up(row0 + S, 8) + 8, N.round_up(S, 64), row0 + N.round_up(S, 64) - 8,
                               row0 + N.round_up(S, 64), row0 + N.round_up(S, 64) + 8, row0 + N.round_up(S, 64) + 64}):
                if Skp > 0 and not N.vt_call_fits(S, Skp, row0):
                    out.append((S, Skp, row0))
    return out


def test_rows_entry_points_refuse_v_transposes_that_leave_their_rows():
    """Only refused calls reach the C entry points here (dummy, never dereferenced pointers); accepted shapes run on the GPU."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000
    bad = _overrunning_triples()
    for t in LISTED:
        S, Skp, row0 = t
        lo, hi = N.vt_written_columns(S, row0)
        assert t in bad and (hi > Skp or lo % 64), t
    assert (100, 104, 0) in bad and N.vt_written_columns(100, 0) == (0, 128)      # 24 columns into the next row, 48 bytes past the end
    assert len(bad) > 60
    for fn in (L.apexmi_qk_rms_rope_rows, L.apexmi_qk_rms_rope_rows_f32):
        for S, Skp, row0 in bad:
            for H in (24, 40):
                rc = fn(P, P, P, 3 * H * 128, S, H, P, P, 1e-6, None, lib.ROPE_NONE, P, P, P, row0 + S, Skp, row0, None)
                msg = L.apexmi_last_error().decode()
                assert rc != 0 and "not tile aligned" in msg and f"Skp={Skp}" in msg, ((S, Skp, row0), rc, msg)
    # what every in-tree caller allocates fits
    assert all(N.vt_call_fits(S, N.round_up(S, 64) + r0, r0) for S in (1, 100, 131) for r0 in (0, 64))
