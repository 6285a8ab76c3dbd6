"""The GEMM probes have teeth (no GPU): every case the GPU file runs meets the conditions that make its expected output exact;
the exact comparison rejects every single wrong decision planted into the reference path and names a coordinate; the two-number
bar of the older GEMM tests (rel-L2 < 3e-3, max-abs within 2 bf16 ulps of the largest magnitude) accepts a wrong rounding rule."""
import pytest
import torch

from tests import gemm_probes as G
from tests.gemm_probes import BF

GAP_SHAPES = [(300, 520, 64), (300, 520, 320), (300, 520, 1024), (385, 264, 4096)]


def _rejected(mutant, want, tile=(256, 256), prob=None):
    """the exact comparison rejects the mutant and names a coordinate and a tile"""
    msg = G.mismatches(mutant, want, tile=tile, prob=prob)
    assert not torch.equal(mutant, want) and "got" in msg and "want" in msg and "tiles (m // 256, n // 256)" in msg, msg
    return msg


# ---- the store: wrong rounding rules on the exact float32 value
def _bits(f):
    return f.contiguous().view(torch.int32)


def round_half_up(f):
    """float32 -> bf16, ties away from zero (add half a step to the magnitude, cut)"""
    return ((_bits(f) + 0x8000) & ~0xFFFF).view(torch.float32).to(BF)


def truncate(f):
    return (_bits(f) & ~0xFFFF).view(torch.float32).to(BF)


# ------------------------------------------------------------------------------------------------ conditions of every case
@pytest.mark.parametrize("case", G.all_exact_cases(), ids=G.case_id)
def test_every_gpu_case_meets_the_exactness_conditions(case):
    family, M, N, K, salt = case
    op = G.operands(family, M, N, K, salt)           # the constructor asserts the bf16 round trip and the grids
    for epilogue in ("bias", "gate_res"):
        for bias in (True, False):
            assert G.span_log2(op, epilogue, bias) < G.SPAN_BITS
            ref = G.gemm_ref(op, epilogue, bias)
            y = op.a.double() @ op.w.double().T + (op.bias.double() if bias else 0)
            assert torch.equal(ref, y if epilogue == "bias" else op.res.double() + op.gate.double() * y)
            assert float(ref.abs().max()) < G.SENTINEL / 4
            # float32 arithmetic in torch's own order reproduces it exactly
            y32 = op.a @ op.w.T + (op.bias if bias else 0)
            assert torch.equal((y32 if epilogue == "bias" else op.res + op.gate * y32).double(), ref)
            assert torch.equal(G.expected(ref, torch.float32).double(), ref)
            if family == "fixed" and ref.numel() >= 4096:      # (1, 8) and (1, 72) are addressing edges: too few elements to count
                assert G.tie_fraction(ref) >= 0.01, G.tie_fraction(ref)
    if family == "selector":
        assert float(G.gemm_ref(op, "gate_res").abs().max()) <= 256 and float(op.a.abs().max()) <= 4


@pytest.mark.parametrize("case", [c for c in G.all_exact_cases() if c[0] == "selector"], ids=G.case_id)
def test_selector_reaches_every_tile_and_position(case):
    """Over the columns of a case every K-tile is hit, and from three K-tiles on every one of the 64 positions of a tile.  The
    position formula (11 n + 23 t + 3 (n // 7)) % 64 = (16 (n // 7) + 11 (n % 7) + 23 t) % 64 takes 28 values per K-tile, so
    one K-tile reaches 28 positions and two reach 48; every 16-byte chunk of a tile row is reached in every case."""
    _, M, N, K, _ = case
    T = K // G.BK
    chosen = G.selector_tiles(N, T)
    pos, coef = G.selector_positions(N, T)
    w = G.selector(M, N, K).w.view(N, T, G.BK)
    assert torch.equal((w != 0), torch.zeros_like(w, dtype=torch.bool).scatter_(2, pos.unsqueeze(2), chosen.unsqueeze(2)))
    assert int((w != 0).sum(2).max()) == 1 and int(chosen.sum(1).max()) <= 12 and bool(chosen[:, 0].all()) and bool(chosen[:, -1].all())
    if N < 64:
        return
    assert bool(chosen.any(0).all()), "a K-tile no column reads"
    hit = set(pos[chosen].tolist())
    assert len(hit) == (64 if T >= 3 else 28 if T == 1 else 48), len(hit)
    assert {p // 8 for p in hit} == set(range(8))
    assert set(coef.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}


def test_formula_input_has_no_tile_period():
    a = G.int_a(300, 640)
    assert float(a.min()) == -4 and float(a.max()) == 4 and not torch.equal(a[:300, :300], a[:300, :300].T)
    for d in range(2):
        assert not torch.equal(a, a.flip(d))
        for p in (1, 2, 4, 8, 16, 32, 64, 128, 256):
            assert not torch.equal(a.narrow(d, 0, a.shape[d] - p), a.narrow(d, p, a.shape[d] - p)), (d, p)


def test_activation_and_verification_operands():
    for M, N, K in [(165, 136, 64), (165, 136, 320), (421, 264, 320), (80, 136, G.GROUP_K)]:
        op = G.act_operands(M, N, K)
        x = G.pre_activation(op)
        assert 2.0 < float(x.abs().max()) <= G.ACT_RANGE and G.span_log2(op) < G.SPAN_BITS
        for epi in ("gelu", "gelu_erf", "silu", "quick_gelu"):
            assert torch.isfinite(G.act_ref(op, epi)).all()
    tg = torch.nn.functional.gelu(x, approximate="tanh")
    assert float((G.act_ref(op, "gelu") - tg).abs().max()) < 1e-12
    assert float((G.act_ref(op, "gelu_erf") - torch.nn.functional.gelu(x)).abs().max()) < 1e-12
    assert float((G.act_ref(op, "silu") - torch.nn.functional.silu(x)).abs().max()) < 1e-12
    for M, N, K in [(165, 136, 64), (293, 264, 256), (421, 264, 256)]:
        op = G.verify_operands(M, N, K)
        # the kernel sums the split parts: |hi| + |mid| <= |a| (1 + 2^-7), i.e. at most log2(1 + 2^-7) < 0.012 more
        assert G.span_log2(op, "gate_res") + 0.012 < G.SPAN_BITS
        ref = G.gemm_ref(op, "gate_res")
        assert torch.equal(G.expected(ref, torch.float32).double(), ref)


def test_gemv_operands_are_exact_in_float32():
    for M, N, K in G.GEMV:
        op = G.gemv_operands(M, N, K)
        assert G.span_log2(op) < G.SPAN_BITS, (K, G.span_log2(op))
        y = G.gemm_ref(op)
        assert torch.equal(G.expected(y, torch.float32).double(), y)
        assert torch.equal(G.expected(y + op.res.double(), torch.float32).double(), y + op.res.double())
    assert G.w_grid(16384) == (8, 2.0 ** -5) and G.w_grid(4096) == (16, 2.0 ** -6)


def test_tie_and_rounding_helpers():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0, 1.0 + 2.0 ** -9, -(2.0 + 2.0 ** -7), 0.0], dtype=torch.float64)
    assert G.tie_fraction(v) == 3 / 6 and G.exact_fraction(v) == 2 / 6
    f = v.float()
    assert f.to(BF).tolist() == [1.0, 1.015625, 1.0, 1.0, -2.0, 0.0]                       # nearest even
    assert round_half_up(f).tolist() == [1.0078125, 1.015625, 1.0, 1.0, -2.015625, 0.0]
    assert truncate(f).tolist() == [1.0, 1.0078125, 1.0, 1.0, -2.0, 0.0]
    got = torch.tensor([[1.0, 1.0078125]]).to(BF)
    assert G.ulp_worst(got, torch.tensor([[1.0, 1.0]], dtype=torch.float64)) == (1, (0, 1))


# --------------------------------------------------------------------------------------------------------------- the mutants
@pytest.mark.parametrize("M,N,K", GAP_SHAPES)
def test_wrong_rounding_rules_pass_the_old_bar_and_fail_the_exact_comparison(M, N, K):
    op = G.fixed_point(M, N, K)
    # 1 round-half-up, 2 truncation: on the bias epilogue
    ref = G.gemm_ref(op)
    want = G.expected(ref)
    assert G.old_bar_accepts(want, ref)
    up, cut = round_half_up(ref.float()), truncate(ref.float())
    _rejected(up, want)
    _rejected(cut, want)
    assert G.old_bar_accepts(up, ref), "the gap: the two-number bar accepts round-half-up"
    frac = float((up != want).float().mean())
    assert 0.01 < frac < 0.2, frac
    # 3 double rounding: y rounded to bf16 before r + gate * y
    refg = G.gemm_ref(op, "gate_res")
    wantg = G.expected(refg)
    y16 = G.pre_activation(op).float().to(BF).float()
    twice = (op.res + op.gate * y16).to(BF)
    _rejected(twice, wantg)
    assert G.old_bar_accepts(wantg, refg) and G.old_bar_accepts(twice, refg), "the gap: the two-number bar accepts double rounding"
    # 4 bias outside the gate
    acc = op.a.double() @ op.w.double().T
    _rejected((op.res.double() + op.gate.double() * acc + op.bias.double()).float().to(BF), wantg)
    # 5 one k dropped for the last row
    a2 = op.a.clone()
    k0 = K - 5
    assert a2[M - 1, k0] != 0
    a2[M - 1, k0] = 0
    drop = (a2.double() @ op.w.double().T + op.bias.double()).float().to(BF)
    msg = _rejected(drop, want)
    assert f"({M - 1}, " in msg and f"({(M - 1) // 256}, " in msg
    if K == 4096:
        # for the committed seed the old bar accepts the dropped element at K = 4096: the max-abs part is set by the largest |ref|
        assert G.old_bar_accepts(drop, ref), "the gap: one dropped k of one row at K = 4096"
    elif K <= 320:
        assert not G.old_bar_accepts(drop, ref)


def test_addressing_mutants_are_rejected():
    M, N, K = 293, 264, 320
    op = G.fixed_point(M, N, K)
    want, wantg = G.want("fixed", M, N, K), G.want("fixed", M, N, K, "gate_res")
    y = G.pre_activation(op, bias=False)
    # 6 bias shifted by one inside the last 8-column group
    b2 = op.bias.clone()
    b2[N - 8:] = op.bias[N - 8:].roll(1)
    msg = _rejected((y + b2.double()).float().to(BF), want)
    assert "(0, 256)" in msg and "[(0, 1), (1, 1)]" in msg
    # 7 gate taken from the neighbouring column
    _rejected((op.res.double() + op.gate.roll(1).double() * (y + op.bias.double())).float().to(BF), wantg)
    # 8 residual read with ldc in place of ldr: R lives in a buffer with ldr = N + 24, C is contiguous (ldc = N)
    ldr = N + 24
    rbuf = torch.zeros(M, ldr)
    rbuf[:, :N] = op.res
    wrong_r = rbuf.flatten()[: M * N].view(M, N)                     # R[m * ldc + n]
    _rejected((wrong_r.double() + op.gate.double() * (y + op.bias.double())).float().to(BF), wantg)
    # 9 row M - 1 computed from the clamped row M - 2
    clamped = want.clone()
    clamped[M - 1] = want[M - 2]
    msg = _rejected(clamped, want)
    assert f"({M - 1}, 0)" in msg
    # 12 one 8-column group of one row of a tile left at the sentinel
    left = want.clone()
    left[M - 1, 256:264] = G.SENTINEL
    msg = _rejected(left, want)
    assert msg.startswith("8 of") and "[(1, 1)]" in msg


def test_group_and_batch_mutants_are_rejected():
    BM, BN = 256, 256
    (M0, N0), (M1, N1) = G.group_shapes(BM, BN)[0], G.group_shapes(BM, BN)[2]
    p0, p1 = G.fixed_point(M0, N0, G.GROUP_K, 0), G.fixed_point(M1, N1, G.GROUP_K, 2)
    want0 = G.want("fixed", M0, N0, G.GROUP_K)
    # 10 one K-tile taken from the other problem of the group
    a2 = p0.a.clone()
    a2[:, 64:128] = p1.a[:M0, 64:128]
    _rejected((a2.double() @ p0.w.double().T + p0.bias.double()).float().to(BF), want0, prob=0)
    # 11 batch element z reading z - 1's weight
    M, N, K = G.BATCHED[1]
    ops_ = [G.fixed_point(M, N, K, z) for z in range(G.BATCH)]
    wants = torch.stack([G.want("fixed", M, N, K, bias=False, salt=z) for z in range(G.BATCH)])
    assert not torch.equal(wants[0], wants[1]) and not torch.equal(wants[1], wants[2])
    stale = torch.stack([(ops_[z].a.double() @ ops_[max(z - 1, 0)].w.double().T).float().to(BF) for z in range(G.BATCH)])
    msg = G.mismatches(stale, wants, tile=(256, 256))
    assert "(1, 0, 0)" in msg and torch.equal(stale[0], wants[0])
    for z in (1, 2):
        assert "problem / batch" in _rejected(stale[z], wants[z], prob=z)
