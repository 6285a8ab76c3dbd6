"""The grouped fp8 GEMM (`apexmi_gemm_fp8_grouped`) and its fused q/k/v epilogue (`apexmi_gemm_fp8_grouped_qkv`) on the GPU.

  1. exact: two `gemm_fp8_probes.Fixed` problems in one launch against that module's fixed-point references (whole
     sentinel-filled buffers, torch.equal; the tanh GELU under the module's own bars, as in tests/test_gpu_gemm_fp8_probes.py);
  2. grouped == single: on random codes and scales every problem of a grouped launch leaves the bits `ops.gemm_fp8` leaves for it
     alone, up to the Flux single-block shape (M 4608, N 9216 + 12288, K 3072);
  3. fused q/k/v == two-pass: `gemm_fp8_grouped_qkv` against `gemm_fp8_grouped` -> `ops.qkv_prepare` on the same codes, bit for bit,
     for aligned and unaligned joint streams, the single block's QKV + MLP-up launch and the Flux shape (H 24, K 3072, M 4608);
  4. refusals raise with a message and write nothing.

No bar in this file is a measurement: every comparison is torch.equal except the GELU one, whose bars are gemm_fp8_probes'."""
import pytest
import torch

from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF, F8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _padded_codes(codes, extra=128):
    """the codes [M, K] as a view of a wider byte buffer: lda = K + extra, the padding holds a NaN code"""
    M, K = codes.shape
    buf = torch.full((M, K + extra), P.SENTINEL_CODE, dtype=U8, device=DEV)
    buf[:, :K] = codes.to(DEV)
    return buf[:, :K]


class Dev:
    """the operands of one fixed-point case on the device"""

    def __init__(self, op, per_row):
        ops = _ops()
        self.op, self.per_row = op, per_row
        self.qa = _padded_codes(P.codes_of(op.qa))
        self.w = ops.Fp8Weight(P.codes_of(op.qw).view(F8).to(DEV), (op.sw if per_row else op.sw_one).to(DEV))
        assert self.w.scale.numel() == (op.N if per_row else 1)
        self.sa, self.bias, self.gate = op.sa.to(DEV), op.bias.to(BF).to(DEV), op.gate.to(DEV)
        self.res = op.res.to(BF).to(DEV)


def _check_exact(buf, want, what):
    msg = P.buffer_mismatches(buf.cpu(), want)
    assert not msg, f"{what}: {msg}"


def _check_gelu(buf, x, what):
    """the view under gemm_fp8_probes' GELU bars, everything around it still the sentinel"""
    host = buf.cpu()
    M, N = x.shape
    got = host[1:M + 1, P.GUARD:P.GUARD + N]
    full = torch.full_like(host, P.SENTINEL)
    full[1:M + 1, P.GUARD:P.GUARD + N] = got
    assert torch.equal(host, full), f"{what}: store outside the output view"
    assert not bool((got == P.SENTINEL).any()), f"{what}: elements left at the sentinel"
    worst, equal = P.gelu_judge(got, x)
    print(f"[{what}] worst {worst} bf16 ulp from the float64 definition, {100 * equal:.3f} % equal")
    assert worst <= P.GELU_MAX_ULP and equal > P.GELU_MIN_EQUAL, (what, worst, equal)


# ------------------------------------------------------------------------------------------------------------- 1. exact
EXACT_LAUNCHES = [([(200, 144), (72, 144)], 128), ([(200, 144), (72, 144)], 256), ([(1160, 256), (1160, 384)], 256)]
EXACT_EPILOGUES = [("bias", "gelu"), ("gate_res", "gate_res"), ("bias", "gate_res")]


@pytest.mark.parametrize("shapes,K", EXACT_LAUNCHES, ids=lambda v: str(v).replace(" ", ""))
def test_grouped_launch_against_the_fixed_point_references(shapes, K):
    """sw per row in problem 0, the single value in problem 1; gate_res runs in place (C == R)"""
    ops = _ops()
    devs = [Dev(P.fixed_point(M, N, K), per_row=(i == 0)) for i, (M, N) in enumerate(shapes)]
    for epis in EXACT_EPILOGUES:
        bufs, views = zip(*[P.sentinel_buffer(M, N, DEV) for M, N in shapes])
        for d, v, e in zip(devs, views, epis):
            if e == "gate_res":
                v.copy_(d.res)
        ops.gemm_fp8_grouped([d.qa for d in devs], [d.sa for d in devs], [d.w for d in devs], [d.bias for d in devs], list(views),
                             epilogue=list(epis), gate_list=[d.gate for d in devs],
                             residual_list=[v if e == "gate_res" else None for v, e in zip(views, epis)])
        torch.cuda.synchronize()
        for i, (d, buf, e, (M, N)) in enumerate(zip(devs, bufs, epis, shapes)):
            what = f"gemm_fp8_grouped {shapes} K={K} {epis} problem {i}"
            if e == "gelu":
                assert P.span_log2(d.op, "bias", d.per_row, True) < P.SPAN_BITS
                _check_gelu(buf, P.pre_activation(d.op, d.per_row, True), what)
            else:
                _check_exact(buf, P.want(M, N, K, e, d.per_row, True), what)


# ------------------------------------------------------------------------------------------------- 2. grouped == single
def _random_codes(shape, gen):
    """random e4m3 codes with the top exponent bit clear: both signs, |value| < 2 spread over the exponents, subnormals and zeros
    included, no NaN code; made on the device from random bytes"""
    return torch.randint(0, 256, shape, generator=gen, device=DEV, dtype=torch.int32).to(U8) & 0xBF


def _random_problem(M, N, K, seed, per_row):
    """random codes, positive activation scales, weight scales of both signs, bias, gate and residual on the device"""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)          # noqa: E731
    qa = _padded_codes(_random_codes((M, K), g))
    w = ops.Fp8Weight(_random_codes((N, K), g).view(F8), (r(N) * 0.1 if per_row else r(1) * 0.1))
    return dict(qa=qa, sa=(r(M).abs() * 0.2 + 1e-2), w=w, bias=r(N).to(BF), gate=r(N), res=r(M, N).to(BF), M=M, N=N)


def _grouped_equals_single(shapes, K, epis, seed):
    ops = _ops()
    ps = [_random_problem(M, N, K, seed + i, per_row=(i == 0)) for i, (M, N) in enumerate(shapes)]
    gb, gv = zip(*[P.sentinel_buffer(M, N, DEV) for M, N in shapes])
    sb, sv = zip(*[P.sentinel_buffer(M, N, DEV) for M, N in shapes])
    for p, a, b, e in zip(ps, gv, sv, epis):
        if e == "gate_res":
            a.copy_(p["res"])
            b.copy_(p["res"])
    ops.gemm_fp8_grouped([p["qa"] for p in ps], [p["sa"] for p in ps], [p["w"] for p in ps], [p["bias"] for p in ps], list(gv),
                         epilogue=list(epis), gate_list=[p["gate"] for p in ps],
                         residual_list=[v if e == "gate_res" else None for v, e in zip(gv, epis)])
    for p, v, e in zip(ps, sv, epis):
        kw = dict(gate=p["gate"], residual=v) if e == "gate_res" else {}
        ops.gemm_fp8(p["qa"], p["sa"], p["w"], p["bias"], out=v, epilogue=e, **kw)
    torch.cuda.synchronize()
    for i, (a, b, v) in enumerate(zip(gb, sb, sv)):
        assert torch.isfinite(v.float()).all() and float(v.float().abs().max()) > 0
        assert torch.equal(a, b), (shapes, K, epis, i, int((a != b).sum()))


@pytest.mark.parametrize("shapes,K", EXACT_LAUNCHES, ids=lambda v: str(v).replace(" ", ""))
def test_each_problem_of_a_grouped_launch_equals_its_single_launch(shapes, K):
    for n, epis in enumerate(EXACT_EPILOGUES):
        _grouped_equals_single(shapes, K, epis, 100 + 10 * n)


def test_three_and_four_problems_in_one_launch():
    _grouped_equals_single([(200, 144), (72, 144), (129, 272)], 256, ("gelu", "gate_res", "bias"), 300)
    _grouped_equals_single([(1, 16), (200, 144), (72, 144), (129, 272)], 128, ("bias", "gelu", "gate_res", "bias"), 310)


def test_flux_single_block_shape_equals_the_single_launches():
    _grouped_equals_single([(4608, 9216), (4608, 12288)], 3072, ("bias", "gelu"), 400)


# ------------------------------------------------------------------------------------------- 3. fused q/k/v == two-pass
def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(BF)


def _rope(S, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ang = torch.rand(S, 64, generator=g, device=DEV) * 6.283
    return torch.stack([ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)]).contiguous().float()


def _fp8_weight(N, K, seed):
    """random codes (|value| < 2) with a per-ROW `sw` of both signs, sized so that the projection is of order 1"""
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(seed)
    sw = (torch.rand(N, generator=g, device=DEV) + 0.5) * torch.where(torch.rand(N, generator=g, device=DEV) < 0.5, -1.0, 1.0)
    return ops.Fp8Weight(_random_codes((N, K), g).view(F8), sw * 2.0 * K ** -0.5)


def _guarded(shape):
    """(flat buffer, contiguous view of `shape`) with 128 sentinel elements in front and behind"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 256,), P.SENTINEL, dtype=BF, device=DEV)
    return buf, buf[128:128 + n].view(*shape)


def _check_qkv(ref, got, S):
    (q0, k0, vt0), ((qb, q1), (kb, k1), (vb, vt1)) = ref, got
    torch.cuda.synchronize()
    assert torch.isfinite(q0.float()).all() and float(q0.float().abs().max()) > 0 and float(vt0.float().abs().max()) > 0
    assert torch.equal(q1, q0), int((q1 != q0).sum())
    assert torch.equal(k1, k0), int((k1 != k0).sum())
    assert torch.equal(vt1[:, :, :S], vt0[:, :, :S]), int((vt1[:, :, :S] != vt0[:, :, :S]).sum())
    assert bool((vt1[:, :, S:] == P.SENTINEL).all()), "columns >= S_out of V^T are not written"
    for b in (qb, kb, vb):
        assert bool((b[:128] == P.SENTINEL).all()) and bool((b[-128:] == P.SENTINEL).all()), "store outside the outputs"


def _joint_streams(H, K, m_img, m_txt):
    from apex_studio_amd import lib as _l
    ops = _ops()
    inner, S = H * 128, m_img + m_txt
    skp0 = (S + 63) // 64 * 64          # the two-pass V^T pass writes whole 64-key tiles
    skp = skp0 + 8                      # the fused launch: columns >= S must stay as they are
    n = 2 if m_txt else 1
    xs = [_rand((m_img, K), 1), _rand((max(m_txt, 1), K), 2)][:n]
    qs = [ops.quant_rows_fp8(x) for x in xs]
    codes, scales = [q[0] for q in qs], [q[1] for q in qs]
    ws = [_fp8_weight(3 * inner, K, 3), _fp8_weight(3 * inner, K, 4)][:n]
    bs = [_rand((3 * inner,), 5, 0.1), _rand((3 * inner,), 6, 0.1)][:n]
    nq = [_rand((128,), 7) * 0.2 + 1, _rand((128,), 8) * 0.2 + 1]
    nk = [_rand((128,), 9) * 0.2 + 1, _rand((128,), 10) * 0.2 + 1]
    rope = _rope(S, 11)
    row0 = [m_txt, 0][:n]
    # two-pass reference on the same codes
    qkv = torch.empty(S, 3 * inner, device=DEV, dtype=BF)
    ops.gemm_fp8_grouped(codes, scales, ws, bs, [qkv[m_txt:], qkv[:m_txt]][:n])
    q0, k0 = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    vt0 = torch.zeros(H, 128, skp0, device=DEV, dtype=BF)
    ops.qkv_prepare(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], H, q0, k0, vt0, wq=nq[0], wk=nk[0],
                    wq2=nq[1] if m_txt else None, wk2=nk[1] if m_txt else None, split=m_txt, eps=1e-6, rope=rope,
                    rope_mode=_l.ROPE_INTERLEAVED)
    # fused
    got = [_guarded((H, S, 128)), _guarded((H, S, 128)), _guarded((H, 128, skp))]
    ops.gemm_fp8_grouped_qkv(codes, scales, ws, bs, [None] * n, "bias", [1] * n, nq[:n], nk[:n], row0, H, 1e-6, rope,
                             got[0][1], got[1][1], got[2][1])
    _check_qkv((q0, k0, vt0), got, S)


@pytest.mark.parametrize("m_img,m_txt", [(200, 72), (203, 77), (1100, 3), (256, 0)])
def test_joint_streams_bit_identical_to_two_pass(m_img, m_txt):
    """(203, 77): an unaligned row0 and M, the element-wise V^T store; distinct norm weights per stream, per-row sw"""
    _joint_streams(2, 256, m_img, m_txt)


def _single_block(H, K, S, mlp):
    from apex_studio_amd import lib as _l
    ops = _ops()
    inner = H * 128
    skp0 = (S + 63) // 64 * 64          # the two-pass V^T pass writes whole 64-key tiles
    skp = skp0 + 8                      # the fused launch: columns >= S must stay as they are
    codes, scales = ops.quant_rows_fp8(_rand((S, K), 21))
    wqkv, wmlp = _fp8_weight(3 * inner, K, 22), _fp8_weight(mlp, K, 23)
    bqkv, bmlp = _rand((3 * inner,), 24, 0.1), _rand((mlp,), 25, 0.1)
    nq, nk = _rand((128,), 26) * 0.2 + 1, _rand((128,), 27) * 0.2 + 1
    rope = _rope(S, 28)
    qkv = torch.empty(S, 3 * inner, device=DEV, dtype=BF)
    ub0, up0 = P.sentinel_buffer(S, mlp, DEV)
    ops.gemm_fp8_grouped([codes, codes], [scales, scales], [wqkv, wmlp], [bqkv, bmlp], [qkv, up0], epilogue=["bias", "gelu"])
    q0, k0 = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    vt0 = torch.zeros(H, 128, skp0, device=DEV, dtype=BF)
    ops.qkv_prepare(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], H, q0, k0, vt0, wq=nq, wk=nk, split=0, eps=1e-6,
                    rope=rope, rope_mode=_l.ROPE_INTERLEAVED)
    got = [_guarded((H, S, 128)), _guarded((H, S, 128)), _guarded((H, 128, skp))]
    ub1, up1 = P.sentinel_buffer(S, mlp, DEV)
    ops.gemm_fp8_grouped_qkv([codes, codes], [scales, scales], [wqkv, wmlp], [bqkv, bmlp], [None, up1], ["bias", "gelu"], [1, 0],
                             [nq, None], [nk, None], [0, 0], H, 1e-6, rope, got[0][1], got[1][1], got[2][1])
    _check_qkv((q0, k0, vt0), got, S)
    assert float(up0.float().abs().max()) > 0 and torch.equal(ub1, ub0), "the ride-along MLP-up output, guards included"


def test_single_block_launch_with_mlp_up_bit_identical():
    _single_block(4, 512, 1160, 1024)


def test_flux_shape_bit_identical_to_two_pass():
    _joint_streams(24, 3072, 4608, 0)


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def _refusal_operands(K=256, n=1):
    ops = _ops()
    d = [Dev(P.Fixed(72, 144, K, salt=i), per_row=True) for i in range(n)]
    bufs, views = zip(*[P.sentinel_buffer(72, 144, DEV) for _ in range(n)])
    return ops, d, bufs, list(views)


def _untouched(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == P.SENTINEL).all()), "a refused launch wrote something"


def test_refuses_e5m2():
    ops, d, bufs, views = _refusal_operands(n=2)
    w5 = ops.Fp8Weight(d[1].w.q.view(torch.float8_e5m2), d[1].w.scale)
    with pytest.raises(RuntimeError, match="e5m2"):
        ops.gemm_fp8_grouped([x.qa for x in d], [x.sa for x in d], [d[0].w, w5], [x.bias for x in d], views)
    _untouched(bufs)


def test_refuses_a_float_output():
    ops, d, bufs, views = _refusal_operands(n=2)
    fbuf = torch.full((72, 144), P.SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="f32 output"):
        ops.gemm_fp8_grouped([x.qa for x in d], [x.sa for x in d], [x.w for x in d], [x.bias for x in d], [views[0], fbuf])
    _untouched(list(bufs) + [fbuf])


def test_refuses_k_192():
    ops, d, bufs, views = _refusal_operands(K=192, n=2)
    with pytest.raises(RuntimeError, match="multiple of 128"):
        ops.gemm_fp8_grouped([x.qa for x in d], [x.sa for x in d], [x.w for x in d], [x.bias for x in d], views)
    _untouched(bufs)


def test_refuses_more_than_four_problems():
    ops, d, bufs, views = _refusal_operands(K=128, n=5)
    with pytest.raises(RuntimeError, match="count=5"):
        ops.gemm_fp8_grouped([x.qa for x in d], [x.sa for x in d], [x.w for x in d], [x.bias for x in d], views)
    _untouched(bufs)


def test_refuses_a_fused_problem_whose_n_is_not_3_h_128():
    ops, d, bufs, views = _refusal_operands(n=1)              # N = 144, H = 2 wants 768
    got = [_guarded((2, 72, 128)), _guarded((2, 72, 128)), _guarded((2, 128, 72))]
    with pytest.raises(RuntimeError, match="3 H 128"):
        ops.gemm_fp8_grouped_qkv([d[0].qa], [d[0].sa], [d[0].w], [d[0].bias], [None], "bias", [1], [None], [None], [0], 2, 1e-6,
                                 _rope(72, 1), got[0][1], got[1][1], got[2][1])
    _untouched(list(bufs) + [g[0] for g in got])
