"""The grouped MXFP4 GEMM (`apexmi_gemm_mxfp4_grouped`) and its fused q/k/v epilogue (`apexmi_gemm_mxfp4_grouped_qkv`) on the GPU.

  1. exact: the fixed-point problems of tests/mxfp4_ref.py in ONE launch against that module's references, on whole sentinel-filled
     buffers; GELU under the bars of the single-kernel test;
  2. grouped == single: on random codes and scale bytes every problem leaves the bits `ops.gemm_mxfp4` leaves for it alone — the
     XCD remainder, unequal tile counts, problems that are row slices of one buffer;
  3. fused q/k/v == two-pass: `gemm_mxfp4_grouped_qkv` against `gemm_mxfp4_grouped` -> `ops.qkv_prepare` on the same codes, bit for
     bit, the joint streams of a double block and the single block's launch with its ride-along MLP-up;
  4. refusals leave the outputs untouched.
The grouped kernel is the single kernel's K-loop behind another problem lookup, so (2) carries (1)'s exactness to every shape."""
import pytest
import torch

from tests import gemm_fp8_probes as P
from tests import mxfp4_ref as R
from tests.test_gpu_gemm_fp8_grouped import _check_qkv, _guarded, _rand, _rope

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U8 = torch.uint8


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _mismatch(host_buf, want):
    """'' if the whole sentinel buffer holds `want` in its view and the sentinel elsewhere"""
    M, N = want.shape
    full = torch.full_like(host_buf, R.SENTINEL)
    full[1:M + 1, R.GUARD:R.GUARD + N] = want
    if torch.equal(host_buf, full):
        return ""
    return P.mismatches(host_buf[1:M + 1, R.GUARD:R.GUARD + N], want) or "store outside the output view"


# ------------------------------------------------------------------------------------------------------------------ 1. exact
LAUNCHES = [([(200, 144), (72, 144)], 256), ([(200, 144), (72, 144)], 768), ([(1160, 256), (1160, 384)], 256)]
EPI_SETS = [("bias", "gelu"), ("gate_res", "gate_res"), ("bias", "gate_res")]


@pytest.fixture(scope="module")
def fixed_on_device():
    """the fixed-point problems, made once: {(M, N, K): (op, codes, scales, Mxfp4Weight, bias, gate, residual)} with wide strides"""
    ops = _ops()
    out = {}
    for shapes, K in LAUNCHES:
        for M, N in shapes:
            op = R.fixed_point(M, N, K)
            out[(M, N, K)] = (op, R.wide(op.qa.to(DEV), 32), R.wide(op.sa.to(DEV), 8),
                              ops.Mxfp4Weight(R.wide(op.qw.to(DEV), 16), R.wide(op.sw.to(DEV), 4)), op.bias.to(BF).to(DEV),
                              op.gate.to(DEV), op.res.to(BF).to(DEV))
    return out


@pytest.mark.parametrize("epis", EPI_SETS, ids=lambda e: "+".join(e))
@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda l: "_".join(f"{m}x{n}" for m, n in l[0]) + f"_k{l[1]}")
def test_fixed_point_problems_of_one_launch_are_exact(fixed_on_device, launch, epis):
    ops = _ops()
    shapes, K = launch
    ps = [fixed_on_device[(M, N, K)] for M, N in shapes]
    in_place = epis == ("gate_res", "gate_res")
    bufs, outs, res = [], [], []
    for (op, *_rest), e in zip(ps, epis):
        buf, out = R.sentinel_buffer(op.M, op.N, DEV)
        r = None
        if e == "gate_res":
            r = _rest[5].clone()
            if in_place:
                out.copy_(r)
                r = out
        bufs.append(buf), outs.append(out), res.append(r)
    ops.gemm_mxfp4_grouped([p[1] for p in ps], [p[2] for p in ps], [p[3] for p in ps], [p[4] for p in ps], outs, epilogue=list(epis),
                           gate_list=[p[5] if e == "gate_res" else None for p, e in zip(ps, epis)], residual_list=res)
    torch.cuda.synchronize()
    for i, ((op, *_), e, buf) in enumerate(zip(ps, epis, bufs)):
        host = buf.cpu()
        if e != "gelu":
            assert _mismatch(host, op.want(e)) == "", f"problem {i} ({e}, in place: {in_place})"
            continue
        # gelu: the activation is not exact arithmetic; the bars of the single-kernel test (tests/test_gpu_mxfp4.py)
        got = host[1:op.M + 1, R.GUARD:R.GUARD + op.N]
        worst, equal = P.gelu_judge(got, op.ref("bias"))
        assert worst <= P.GELU_MAX_ULP and equal >= P.GELU_MIN_EQUAL, (worst, equal)
        full = torch.full_like(host, R.SENTINEL)
        full[1:op.M + 1, R.GUARD:R.GUARD + op.N] = got
        assert torch.equal(host, full), f"problem {i}: store outside the output view"


# ------------------------------------------------------------------------------------------------------- 2. grouped == single
def _random_pair(rows, K, gen):
    """random e2m1 codes (every byte value) and scale bytes 2^-7 .. 2^7 per block, with strides wider than the rows"""
    q = torch.randint(0, 256, (rows, K // 2), generator=gen, device=DEV, dtype=torch.int32).to(U8)
    s = torch.randint(120, 135, (rows, K // 32), generator=gen, device=DEV, dtype=torch.int32).to(U8)
    return R.wide(q, 32), R.wide(s, 8)


def _random_problem(M, N, K, seed, act=None):
    ops = _ops()
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)          # noqa: E731
    qa, sa = _random_pair(M, K, g) if act is None else act
    w = ops.Mxfp4Weight(*_random_pair(N, K, g))
    return dict(qa=qa, sa=sa, w=w, bias=r(N).to(BF), gate=r(N), res=r(M, N).to(BF), M=M, N=N)


def _grouped_equals_single(ps, epis):
    ops = _ops()
    singles, grouped, outs, res = [], [], [], []
    for p, e in zip(ps, epis):
        kw = dict(gate=p["gate"], residual=p["res"]) if e == "gate_res" else {}
        buf, out = R.sentinel_buffer(p["M"], p["N"], DEV)
        ops.gemm_mxfp4(p["qa"], p["sa"], p["w"], p["bias"], out=out, epilogue=e, **kw)
        singles.append(buf)
        buf, out = R.sentinel_buffer(p["M"], p["N"], DEV)
        grouped.append(buf), outs.append(out), res.append(p["res"] if e == "gate_res" else None)
    ops.gemm_mxfp4_grouped([p["qa"] for p in ps], [p["sa"] for p in ps], [p["w"] for p in ps], [p["bias"] for p in ps], outs,
                           epilogue=list(epis), gate_list=[p["gate"] if e == "gate_res" else None for p, e in zip(ps, epis)],
                           residual_list=res)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(singles, grouped)):
        view = a[1:-1, R.GUARD:-R.GUARD].float()
        assert torch.isfinite(view).all() and float(view.abs().max()) > 0
        assert torch.equal(a, b), f"problem {i} ({epis[i]}): {int((a != b).sum())} elements differ from the single launch"


GROUPS = [([(200, 144), (72, 144)], 256), ([(200, 144), (72, 144)], 768), ([(1160, 256), (1160, 384)], 256),
          ([(130, 144), (72, 272), (300, 128)], 512), ([(130, 144), (72, 272), (300, 128), (1, 16)], 512)]


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "_".join(f"{m}x{n}" for m, n in g[0]) + f"_k{g[1]}")
def test_every_problem_of_a_launch_leaves_its_single_launch(group):
    shapes, K = group
    tiles = sum(((M + 127) // 128) * ((N + 127) // 128) for M, N in shapes)
    if len(shapes) > 2:
        assert tiles % 8 != 0, "the XCD remainder"
    ps = [_random_problem(M, N, K, 100 + 7 * i + K, None) for i, (M, N) in enumerate(shapes)]
    _grouped_equals_single(ps, ["bias", "gelu", "gate_res", "bias"][:len(shapes)])
    _grouped_equals_single(ps, ["gate_res", "bias", "gelu", "gelu"][:len(shapes)])


def test_problems_that_are_row_slices_of_one_buffer():
    K, s_txt, s_img = 512, 72, 200
    g = torch.Generator(device=DEV).manual_seed(77)
    q, s = _random_pair(s_txt + s_img, K, g)
    ps = [_random_problem(s_img, 144, K, 78, act=(q[s_txt:], s[s_txt:])), _random_problem(s_txt, 272, K, 79, act=(q[:s_txt], s[:s_txt])),
          _random_problem(s_txt + s_img, 128, K, 80, act=(q, s))]
    _grouped_equals_single(ps, ["gelu", "gate_res", "bias"])


# --------------------------------------------------------------------------------------------------- 3. fused q/k/v == two-pass
def _fp4_weight(N, K, seed):
    """the MXFP4 record of a random bf16 weight sized so that the projection is of order 1"""
    return _ops().Mxfp4Weight.from_bf16(_rand((N, K), seed, 2.0 * K ** -0.5))


def _joint_streams(H, K, m_img, m_txt, norms):
    from apex_studio_amd import lib as _l
    ops = _ops()
    inner, S = H * 128, m_img + m_txt
    skp0 = (S + 63) // 64 * 64          # the two-pass V^T pass writes whole 64-key tiles
    skp = skp0 + 8                      # the fused launch: columns >= S must stay as they are
    q, s = ops.quant_blocks_mxfp4(_rand((S, K), 1))       # ONE joint buffer, text rows first: the streams are row slices
    codes, scales = [q[m_txt:], q[:m_txt]], [s[m_txt:], s[:m_txt]]
    ws = [_fp4_weight(3 * inner, K, 3), _fp4_weight(3 * inner, K, 4)]
    bs = [_rand((3 * inner,), 5, 0.1), _rand((3 * inner,), 6, 0.1)]
    nq = [_rand((128,), 7) * 0.2 + 1, _rand((128,), 8) * 0.2 + 1] if norms else [None, None]
    nk = [_rand((128,), 9) * 0.2 + 1, _rand((128,), 10) * 0.2 + 1] if norms else [None, None]
    rope = _rope(S, 11)
    qkv = torch.empty(S, 3 * inner, device=DEV, dtype=BF)
    ops.gemm_mxfp4_grouped(codes, scales, ws, bs, [qkv[m_txt:], qkv[:m_txt]])
    q0, k0 = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    vt0 = torch.zeros(H, 128, skp0, device=DEV, dtype=BF)
    ops.qkv_prepare(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], H, q0, k0, vt0, wq=nq[0], wk=nk[0], wq2=nq[1], wk2=nk[1],
                    split=m_txt, eps=1e-6, rope=rope, rope_mode=_l.ROPE_INTERLEAVED)
    got = [_guarded((H, S, 128)), _guarded((H, S, 128)), _guarded((H, 128, skp))]
    ops.gemm_mxfp4_grouped_qkv(codes, scales, ws, bs, [None, None], "bias", [1, 1], nq, nk, [m_txt, 0], H, 1e-6, rope,
                               got[0][1], got[1][1], got[2][1])
    _check_qkv((q0, k0, vt0), got, S)


@pytest.mark.parametrize("norms", [True, False], ids=["norm", "no_norm"])
@pytest.mark.parametrize("K", [256, 768])
@pytest.mark.parametrize("m_img,m_txt", [(200, 72), (200, 77)])
def test_joint_streams_bit_identical_to_two_pass(m_img, m_txt, K, norms):
    """(200, 77): an unaligned row0 and M, the element-wise V^T store"""
    _joint_streams(2, K, m_img, m_txt, norms)


@pytest.mark.parametrize("K", [256, 768])
def test_single_block_launch_with_mlp_up_bit_identical(K):
    from apex_studio_amd import lib as _l
    ops = _ops()
    H, S, mlp = 2, 272, 1024
    inner = H * 128
    skp0 = (S + 63) // 64 * 64
    skp = skp0 + 8
    codes, scales = ops.quant_blocks_mxfp4(_rand((S, K), 21))
    wqkv, wmlp = _fp4_weight(3 * inner, K, 22), _fp4_weight(mlp, K, 23)
    bqkv, bmlp = _rand((3 * inner,), 24, 0.1), _rand((mlp,), 25, 0.1)
    nq, nk = _rand((128,), 26) * 0.2 + 1, _rand((128,), 27) * 0.2 + 1
    rope = _rope(S, 28)
    qkv = torch.empty(S, 3 * inner, device=DEV, dtype=BF)
    ub0, up0 = R.sentinel_buffer(S, mlp, DEV)
    ops.gemm_mxfp4_grouped([codes, codes], [scales, scales], [wqkv, wmlp], [bqkv, bmlp], [qkv, up0], epilogue=["bias", "gelu"])
    q0, k0 = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    vt0 = torch.zeros(H, 128, skp0, device=DEV, dtype=BF)
    ops.qkv_prepare(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], H, q0, k0, vt0, wq=nq, wk=nk, split=0, eps=1e-6,
                    rope=rope, rope_mode=_l.ROPE_INTERLEAVED)
    got = [_guarded((H, S, 128)), _guarded((H, S, 128)), _guarded((H, 128, skp))]
    ub1, up1 = R.sentinel_buffer(S, mlp, DEV)
    ops.gemm_mxfp4_grouped_qkv([codes, codes], [scales, scales], [wqkv, wmlp], [bqkv, bmlp], [None, up1], ["bias", "gelu"], [1, 0],
                               [nq, None], [nk, None], [0, 0], H, 1e-6, rope, got[0][1], got[1][1], got[2][1])
    _check_qkv((q0, k0, vt0), got, S)
    assert float(up0.float().abs().max()) > 0 and torch.equal(ub1, ub0), "the ride-along MLP-up output, guards included"


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_write_nothing():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError

    def problems(n, K=256, N=144, M=72):
        ps = [_random_problem(M, N, K, 300 + i) for i in range(n)]
        bufs, views = zip(*[R.sentinel_buffer(M, N, DEV) for _ in range(n)])
        return ps, list(bufs), list(views)

    def call(ps, views, **kw):
        return ops.gemm_mxfp4_grouped([p["qa"] for p in ps], [p["sa"] for p in ps], [p["w"] for p in ps], [p["bias"] for p in ps], views, **kw)

    def untouched(bufs):
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b == R.SENTINEL).all()), "a refused launch wrote something"

    ps, bufs, views = problems(5)
    with pytest.raises(ApexMIError, match="1 to 4 problems"):
        call(ps, views)
    untouched(bufs)
    ps, bufs, views = problems(2)
    other = _random_problem(72, 144, 512, 310)
    with pytest.raises(ApexMIError, match="share K"):
        call([ps[0], other], views)
    fbuf = torch.full((72, 144), R.SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(ApexMIError, match="f32 output"):
        call(ps, [views[0], fbuf])
    with pytest.raises(ApexMIError, match="gate_res epilogue needs"):
        call(ps, views, epilogue=["bias", "gate_res"])
    with pytest.raises(ApexMIError, match="epilogue 'silu'"):
        call(ps, views, epilogue=["bias", "silu"])
    with pytest.raises(ApexMIError, match=r"scales must be \[72, 8\]"):
        ops.gemm_mxfp4_grouped([p["qa"] for p in ps], [ps[0]["sa"], ps[1]["sa"][:, :7]], [p["w"] for p in ps], None, views)
    with pytest.raises(ApexMIError, match=r"out: expected \[72, 144\]"):
        call(ps, [views[0], views[1][:, :128]])
    untouched(bufs + [fbuf])
    # the fused form: N = 144 is not 3 H 128; a missing rope table; a missing output
    got = [_guarded((2, 72, 128)), _guarded((2, 72, 128)), _guarded((2, 128, 72))]
    one = ([ps[0]["qa"]], [ps[0]["sa"]], [ps[0]["w"]], [ps[0]["bias"]], [None], "bias", [1], [None], [None], [0], 2, 1e-6)
    with pytest.raises(ApexMIError, match="3 H 128"):
        ops.gemm_mxfp4_grouped_qkv(*one, _rope(72, 1), got[0][1], got[1][1], got[2][1])
    wq = _fp4_weight(768, 256, 311)
    fused = ([ps[0]["qa"]], [ps[0]["sa"]], [wq], [None], [None], "bias", [1], [None], [None], [0], 2, 1e-6)
    with pytest.raises(ApexMIError, match="rope"):
        ops.gemm_mxfp4_grouped_qkv(*fused, None, got[0][1], got[1][1], got[2][1])
    with pytest.raises(ApexMIError, match="output"):
        ops.gemm_mxfp4_grouped_qkv(*fused, _rope(72, 1), got[0][1], None, got[2][1])
    with pytest.raises(ApexMIError, match="must lie inside S_out"):
        ops.gemm_mxfp4_grouped_qkv(*fused[:9], [8], 2, 1e-6, _rope(72, 1), got[0][1], got[1][1], got[2][1])
    torch.cuda.synchronize()
    for b, _ in got:
        assert bool((b == P.SENTINEL).all()), "a refused launch wrote something"
    untouched(bufs)
