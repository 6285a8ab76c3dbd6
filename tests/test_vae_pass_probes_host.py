"""No GPU.  The conditions of tests/vae_pass_probes.py for every case tests/test_gpu_vae_pass_probes.py runs, from the same case
tables, and the mutations: single wrong decisions the verdict must reject, with whether the older bar (rel-L2 < 4e-3) lets each
through (run with -s for the table)."""
import pytest
import torch

from tests import vae_pass_probes as V
from tests.vae_pass_probes import BF, F32, F64


def _id(cg):
    return f"C{cg[0]}G{cg[1]}"


# ------------------------------------------------------------------------------------------------------------- case tables
def test_groupnorm_case_tables_cover_what_the_kernel_decides():
    assert set(V.GN_CG) == {(32, 32), (64, 32), (128, 32), (256, 32), (512, 32), (512, 64), (16, 2), (8, 1)}
    for C, G in V.GN_CG:
        cases = V.gn_cases(C, G)
        assert len({c.id for c in cases}) == len(cases)
        r = V.rows_per_pass(C)
        for f32 in (False, True):
            ps = {c.P for c in cases if c.image == "exact" and c.f32 == f32}
            assert {1, V.BLOCK_ROWS, V.BLOCK_ROWS + 1, V.FOUR_BLOCKS} <= ps and any(1 < p < r for p in ps), (C, G, ps)
            for silu in (False, True):
                assert any(c.image == "exact" and c.f32 == f32 and c.silu == silu and c.P == V.BLOCK_ROWS + 1 for c in cases)
                assert any(c.image == "const" and c.f32 == f32 and c.silu == silu for c in cases)
            for image in ("plain", "tiny", "offset", "groups"):
                assert {c.silu for c in cases if c.image == image} == {False, True}
                assert any(c.image == image and c.f32 == f32 for c in cases)
        gamma, beta = (t.double() for t in V.gn_affine(C))
        for step in {1, 8, C // G} - {C}:
            assert bool((gamma[step:] != gamma[:-step]).all()) and bool((beta[step:] != beta[:-step]).all()), (C, step)
        assert bool((beta != 0).all()) and bool((gamma != beta).all())
    assert V.rows_per_pass(8) == 256 and V.rows_per_pass(512) == 4 and V.gn_affine(32)[0].dtype == BF


@pytest.mark.parametrize("cg", V.GN_CG, ids=_id)
def test_groupnorm_family_one_operands(cg):
    """bf16-exact, exact f32 sums in three orders, every marker moves its group's variance by more than ten percent, adjacent
    groups and the two halves of a group have different statistics"""
    C, G = cg
    cpg = C // G
    for P in V.gn_positions(C):
        x = V.gn_image("exact", P, C, G, False)
        assert torch.equal(x.to(BF).double(), x) and float(x.abs().max()) <= V.MARKER
        assert V.exact_sums_hold(x), (C, G, P)
        shift = V.marker_variance_shift(P, C, G)
        if P > 1:
            assert len(shift) >= 2 and min(shift) > 0.10, (C, G, P, shift)
        if P >= 61:
            rows = V.marker_rows(P, C)
            assert rows == sorted({p for p in (0, V.rows_per_pass(C) - 1, V.rows_per_pass(C), 1023, 1024, P - 1) if p < P})
            if G >= 12:
                assert len({g for _, g, _ in V.markers(P, C, G)}) == len(rows)      # a different group per marker
            mean, var, _ = V.gn_stats64(x, G)
            m, v = mean.view(G), var.view(G)
            for a, b in zip(range(G - 1), range(1, G)):
                assert abs(float(m[a] - m[b])) > 1e-3 or abs(float(v[a] / v[b]) - 1) > 1e-2, (C, G, P, a)
            if cpg > 1:
                xg = x.view(P, G, cpg)
                lo, hi = xg[..., :cpg // 2].mean((0, 2)), xg[..., cpg // 2:].mean((0, 2))
                assert bool(((lo - hi).abs() > 1e-2).all())


# -------------------------------------------------------------------------------------------------------- the two conditions
@pytest.mark.parametrize("cg", V.GN_CG, ids=_id)
def test_groupnorm_conditions_hold_for_every_gpu_case(cg):
    worst = {}
    for case in V.gn_cases(*cg):
        x = V.case_image(case)
        assert torch.equal(x.to(case.dtype).double(), x)
        ref, env = V.gn_case_ref(case)
        assert float(ref.abs().max()) < V.SENTINEL / 4 and bool((env >= 0).all())
        # (1) the reference alone, under the envelope the GPU output is judged by
        doc = V.gn_documented(case)
        v = V.verdict(doc, ref, env)
        assert v.passed, f"{case.id}: the documented route: {V.describe(v, doc, ref, env)}"
        assert v.undecided <= V.UNDECIDED_CAP, f"{case.id}: {v.undecided:.4f} undecided"
        if case.f32:
            assert v.undecided == 0.0
        w = worst.setdefault((case.image, case.f32), [0.0, 0.0])
        w[0] = max(w[0], v.undecided)
        if case.image in ("const", "bigconst") or (case.P == 1 and case.C == case.G):        # variance exactly 0: beta or silu(beta)
            beta = V.gn_affine(case.C)[1].double().view(1, -1).expand_as(ref)
            assert torch.equal(ref, V.silu64(beta) if case.silu else beta)
            if not case.f32:
                assert bool(v.decided.all()) and torch.equal(doc, V.store(ref, BF))
        # (2) three f32 evaluations under the contract
        cref, cenv = V.gn_case_ref(case, False)
        assert bool((cenv >= env * 0.999).all()) or case.image not in V.EXACT_IMAGES, case.id
        for order in V.ORDERS:
            out = V.gn_emulate(case, order)
            vv = V.verdict(out, cref, cenv)
            assert vv.passed, f"{case.id}: f32 evaluation '{order}': {V.describe(vv, out, cref, cenv)}"
            w[1] = max(w[1], vv.ratio)
            if case.image not in V.EXACT_IMAGES:
                assert vv.undecided <= V.UNDECIDED_CAP
    print(f"[conditions] {_id(cg)}: " + ", ".join(f"{k[0]}.{'f32' if k[1] else 'bf16'} undecided {a:.4f} worst f32 evaluation {b:.3f}"
                                                  for k, (a, b) in sorted(worst.items())))


def test_silu_envelope_admits_an_f32_evaluation_with_one_ulp_primitives():
    """silu_env against x * rcp(1 + exp2(-log2e x)) evaluated in f32 with exp2 and rcp each moved one ulp either way"""
    r = torch.linspace(-20, 20, 20001, dtype=F32)
    env = V.silu_env(r.double(), torch.zeros_like(r).double(), store_u=0.0)
    ref = V.silu64(r.double())
    z = r * torch.tensor(1.4426950408889634, dtype=F32)
    for de in (-1, 0, 1):
        for dr in (-1, 0, 1):
            e = torch.exp2(-z.double()).float()
            e = (e.view(torch.int32) + de).view(F32)
            q = (1.0 / (1.0 + e).double()).float()
            q = (q.view(torch.int32) + dr).view(F32)
            out = (r * q).double()
            assert bool(((out - ref).abs() <= env).all()), (de, dr, float(((out - ref).abs() / env).max()))


# ------------------------------------------------------------------------------------------------------------------ mutations
def _judge(case, out):
    """(rejected by the verdict under the contract, rejected at a decided element, accepted by the old bar)"""
    ref, env = V.gn_case_ref(case, False)
    v = V.verdict(out, ref, env)
    return (not v.passed), v.rejects_decided(), V.old_bar_accepts(out, ref)


def _exact(C, G, P, f32=False, silu=False):
    return V.GnCase(C, G, P, "exact", f32, silu)


def test_groupnorm_mutations_are_rejected():
    table = {}

    def check(name, case, out, must=True):
        rej, dec, old = _judge(case, out)
        t = table.setdefault(name, [0, 0, 0])
        t[0] += 1
        t[1] += int(rej)
        t[2] += int(rej and old)
        if must:
            assert rej, f"{name} on {case.id} is accepted"
        return rej

    for C, G in V.GN_CG:
        cpg = C // G
        for f32 in (False, True):
            for P in (61, V.BLOCK_ROWS + 1, V.FOUR_BLOCKS):
                case = _exact(C, G, P, f32, silu=bool(P % 2) and f32)
                base = V.gn_emulate(case)
                assert not _judge(case, base)[0]
                for p, g, _ in V.markers(P, C, G):
                    check("marker row left out", case, V.gn_emulate(case, mut=("drop_row", p)))
                check("divisor nblk * 1024", case, V.gn_emulate(case, mut="div_nblk"))
                if G >= 2:
                    check("group c // (2 cpg)", case, V.gn_emulate(case, mut="map_pair"))
                    check("group (c // cpg + 1) % G", case, V.gn_emulate(case, mut="map_next"))
                if cpg >= 2:
                    check("halves of a group swapped", case, V.gn_emulate(case, mut="swap_halves"))
                check("gamma and beta swapped", case, V.gn_emulate(case, mut="swap_affine"))
                check("SiLU flipped", case, V.gn_emulate(case, mut="silu_flip"))
                if not f32:
                    check("bf16 store by truncation", case, V.gn_emulate(case, mut="trunc"))
            # the tail row of an ordinary image, no marker in it: a 1e-3 effect on the statistics
            case = V.GnCase(C, G, V.BLOCK_ROWS + 1, "plain", f32, False)
            check("tail row of the plain 1025-row image left out", case, V.gn_emulate(case, mut=("drop_row", case.P - 1)), must=f32)
            for image in ("tiny", "exact"):
                case = V.GnCase(C, G, V.BLOCK_ROWS + 1, image, f32, False)
                must = image == "tiny" or f32        # a 1e-4 effect on family 1: below the resolution of a bf16 output
                check("eps dropped", case, V.gn_emulate(case, mut="noeps"), must)
                check("eps doubled", case, V.gn_emulate(case, mut="eps2"), must)
        # the parent's one-pass f32 order: the f32 offset and groups images (the bf16 offset image holds integers, whose squares
        # sum exactly in f32 in chains of 260: nothing to see there)
        for image in ("offset", "groups"):
            for P in (61, V.BLOCK_ROWS + 1, V.FOUR_BLOCKS):
                case = V.GnCase(C, G, P, image, True, False)
                check(f"one-pass f32 sums, f32 {image} image", case, V.gn_emulate(case, mut="onepass"),
                      must=image == "offset" or P == V.BLOCK_ROWS + 1)
        case = V.GnCase(C, G, V.BLOCK_ROWS + 1, "offset", False, False)
        check("one-pass f32 sums, bf16 offset image", case, V.gn_emulate(case, mut="onepass"), must=False)
        # the clamp: a constant image whose float64 sums are inexact (the constant 1.5 sums exactly: var = 0 without a clamp)
        case = V.GnCase(C, G, V.BLOCK_ROWS + 1, "bigconst", True, False)
        assert not _judge(case, V.gn_documented(case))[0]
        check("variance not clamped (constant 99999.9)", case, V.gn_emulate(case, mut="noclamp"), must=False)
        case = V.GnCase(C, G, V.BLOCK_ROWS + 1, "const", True, False)
        assert not _judge(case, V.gn_emulate(case, mut="noclamp"))[0]
    for name, (n, rej, old) in table.items():
        print(f"[mutation] {name:55s} rejected on {rej:3d} of {n:3d} cases; the old bar accepts {old:3d} of those")
    assert table["variance not clamped (constant 99999.9)"][1] >= 4, "the unclamped variance is hardly ever rejected"


# ------------------------------------------------------------------------------------------------------------ B. exact passes
def test_exact_pass_operands_and_references():
    for T, H, W, C in V.UPSAMPLE_CASES:
        x = V.grid4(T, H, W, C)
        V.check_grid(x.reshape(-1, C))
        assert (T * 2 * H * 2 * W * C // 8) % 256 != 0 and H % 2 == 1 and W % 2 == 1
        for ax in range(4):
            if x.shape[ax] > 1:
                assert bool((x.narrow(ax, 1, x.shape[ax] - 1) != x.narrow(ax, 0, x.shape[ax] - 1)).all()), (ax, x.shape)
        y = V.upsample_ref(x)
        assert y.shape == (T, 2 * H, 2 * W, C) and torch.equal(y[:, 1::2, 0::2], x) and torch.equal(y[:, 0::2, 1::2], x)
    assert {c[3] for c in V.UPSAMPLE_CASES} == {8, 16, 96} and {c[0] for c in V.UPSAMPLE_CASES} == {1, 3}
    for T, H, W, C2, f32 in V.INTERLEAVE_CASES:
        x = V.grid4(T, H, W, C2, salt=2)
        y = V.interleave_ref(x)
        assert (H * W) % 2 == 1 and y.shape == (2 * T, H, W, C2 // 2)
        assert torch.equal(y[0], x[0, ..., :C2 // 2]) and torch.equal(y[1], x[0, ..., C2 // 2:])
        assert not torch.equal(y[0], y[1])
    assert {c[3] for c in V.INTERLEAVE_CASES} == {16, 32, 192}
    for T, H, W, C, r, extra, t0, f32 in V.SHUFFLE_CASES:
        x = V.shuffle_operand(T, H, W, C, r, extra, f32)
        y = V.shuffle_ref(x, C, r, t0)
        assert y.shape == (C, T - t0, H * r, W * r) and float(y.min()) == V.LO and float(y.max()) == V.HI
        live = x[..., :C * r * r]
        dt = F32 if f32 else BF
        for val in [V.LO, V.HI] + V._neighbours(V.LO, dt) + V._neighbours(V.HI, dt):
            assert bool((live == val).any()), (val, f32)
        if extra:
            guard = x[..., C * r * r:]
            assert bool(((guard > 1.5) | (guard < -2.5)).all())
            assert not bool(torch.isin(y, guard.unique()).any())
        # one pixel by hand: channel c r^2 + i r + j -> pixel (h r + i, w r + j) of image channel c
        c, i, j, h, w = C - 1, r - 1, 0, H - 1, 1
        assert float(y[c, 0, h * r + i, w * r + j]) == float(x[t0, h, w, c * r * r + i * r + j].clamp(V.LO, V.HI))
    assert {(c[4], c[5] > 0) for c in V.SHUFFLE_CASES} == {(1, False), (1, True), (2, False), (2, True)}


def test_crossfade_conditions_and_mutations():
    for E, dim, f32 in V.CROSSFADE_CASES:
        dt = F32 if f32 else BF
        a, b = V.crossfade_operands(E, dim)
        V.check_grid(a.reshape(-1, 8))
        V.check_grid(b.reshape(-1, 8))
        ref, env = V.crossfade_ref(a, b, E, dim)
        n = b.shape[dim]
        assert torch.equal(ref.narrow(dim, E, n - E), b.narrow(dim, E, n - E))
        assert torch.equal(ref.narrow(dim, 0, 1), a.narrow(dim, n - E, 1))              # weight 0: a
        if E in (4, 8):      # exact: multiples of 2^-6, one f32 evaluation in either association equals the float64 value
            assert torch.equal(ref * 64, (ref * 64).round())
            want = V.store(ref, dt)
        w = (torch.arange(E, dtype=F32) / E).view([-1 if k == dim else 1 for k in range(4)])
        av, bv = a.float().narrow(dim, n - E, E), b.float().narrow(dim, 0, E)
        emu = b.float().clone()
        emu.narrow(dim, 0, E).copy_(av * (1.0 - w) + bv * w)
        emu = emu.to(dt)
        if E in (4, 8):
            assert torch.equal(emu, want)
        else:
            v = V.verdict(emu, ref, env)
            assert v.passed and v.undecided <= V.UNDECIDED_CAP, (E, dim, f32, v.undecided)
        for mut in ("w_plus", "w_em1", "swap", "shift"):
            bad, _ = V.crossfade_ref(a, b, E, dim, mut=mut)
            bad = V.store(bad, dt)
            if E in (4, 8):
                assert not torch.equal(bad, want), (E, dim, mut)
            else:
                vb = V.verdict(bad, ref, env)
                assert vb.rejects_decided(), (E, dim, mut)


def test_group_mean_reference_and_mutations():
    for gs, C, f32 in V.GROUP_MEAN_CASES:
        dt = F32 if f32 else BF
        x = V.grid4(*V.GROUP_MEAN_POS, C * gs, salt=gs)
        V.check_grid(x.reshape(-1, C * gs))
        ref = V.group_mean_ref(x, C, gs, dt)
        assert (x.numel() // gs) % 256 != 0
        # the sequential f32 sum is exact
        xs = x.float().view(*x.shape[:-1], C, gs)
        acc = torch.zeros(xs.shape[:-1])
        for g in range(gs):
            acc = acc + xs[..., g]
        assert torch.equal(acc.double(), x.view(*x.shape[:-1], C, gs).sum(-1))
        assert torch.equal((acc / torch.tensor(float(gs))).to(dt), ref)
        if gs > 1:
            for mut in ("gs_m1", "skip_last"):
                assert not torch.equal(V.group_mean_ref(x, C, gs, dt, mut=mut), ref), (gs, mut)
    assert {c[0] for c in V.GROUP_MEAN_CASES} == {1, 2, 3, 16, 64}


def test_u8_and_tanh_operands():
    codes = V.u8_codes()
    assert codes.numel() == 32770 == V.U8_SHAPE[0] * V.U8_SHAPE[1] * V.U8_SHAPE[2]
    assert float(codes.float().min()) == -2.0 and float(codes.float().max()) == 2.0
    for f32 in (False, True):
        tile = V.u8_video(3, f32)
        assert tile.shape == V.U8_SHAPE + (4,) and bool((tile[..., 3] == V.SENTINEL).all())
        assert not torch.equal(tile[..., 0], tile[..., 1])
    fin = V.finite_bf16_codes()
    assert fin.numel() == 65536 - 2 * 128 and fin.numel() % 8 == 0
    for inv in (1.0, 1.0 / 1.03682):
        ref = V.tanh_ref64(fin, inv)
        for dt in (BF, F32):
            assert V.tanh_properties(fin.to(dt), ref.to(dt)) is None
    # the properties reject: a dip, a broken symmetry, an overshoot
    y = V.tanh_ref64(fin, 1.0).to(BF)
    i = int((fin.float() == 1.0).nonzero()[0])
    for k, delta in ((i, -0.5), (i, 0.25)):
        bad = y.clone()
        bad[k] = bad[k] + delta
        assert V.tanh_properties(fin, bad) is not None
    bad = y.clone()
    bad[fin.float() > 100] = 3.015625
    assert "> 3" in V.tanh_properties(fin, bad)
