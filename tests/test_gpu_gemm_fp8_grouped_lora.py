"""The grouped run-time LoRA form of the FP8 GEMM on the GPU: `ops.gemm_fp8_grouped(lora_t_list=, lora_B_list=)`
and `ops.gemm_fp8_grouped_qkv(lora_t_list=, lora_B_list=)`.

Exact probes (cases and references: tests/gemm_fp8_grouped_lora_probes.py on top of gemm_fp8_probes / gemm_fp8_lora_probes; their
conditions and what the comparison rejects: tests/test_fp8_grouped_lora_host.py): whole sentinel-filled buffers compared with
torch.equal, against the exact reference AND against each problem's own single launch.  The fused q/k/v form is compared with the
grouped LoRA launch followed by `ops.qkv_prepare`.  Measured values (profiles/flux_fp8_lora_measured.jsonl) stand beside the calls."""
import pytest
import torch

from tests import gemm_fp8_grouped_lora_probes as GL
from tests import gemm_fp8_probes as P
from tests.conftest import measured
from tests.gemm_fp8_probes import BF, F8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _codes(codes):
    """codes [M, K] with a padded row stride"""
    M, K = codes.shape
    qbuf = torch.full((M, K + 128), P.SENTINEL_CODE, dtype=U8, device=DEV)
    qbuf[:, :K] = codes.to(DEV)
    return qbuf[:, :K]


def _padded(x, extra=64):
    """a bf16 [rows, Rp] operand in a tensor of its own with a row stride > Rp (a multiple of 8)"""
    n, Rp = x.shape
    buf = torch.full((n, Rp + extra), P.SENTINEL, dtype=BF, device=DEV)
    buf[:, :Rp] = x.to(BF).to(DEV)
    return buf[:, :Rp]


def _check_exact(buf, want, what):
    msg = P.buffer_mismatches(buf.cpu(), want)
    assert not msg, f"{what}: {msg}"


def _check_gelu(buf, x, what):
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


class _Dev:
    """the device operands of one probe problem"""

    def __init__(self, ops, p):
        op = p.op
        self.p = p
        self.qa = _codes(P.codes_of(op.qa))
        qw = P.codes_of(op.qw).view(F8).to(DEV)
        self.w = {True: ops.Fp8Weight(qw, op.sw.to(DEV)), False: ops.Fp8Weight(qw, op.sw_one.to(DEV))}
        self.sa, self.bias, self.gate, self.res = op.sa.to(DEV), op.bias.to(BF).to(DEV), op.gate.to(DEV), op.res.to(BF).to(DEV)
        self.t = None if p.lo is None else _padded(p.lo.t)
        self.lb = None if p.lo is None else _padded(p.lo.lb)


# ------------------------------------------------------------------------------------------------------------ fixed point
@pytest.mark.parametrize("name", sorted(GL.GROUPS))
def test_every_problem_leaves_the_bits_of_its_own_single_launch(name):
    """MIXED: three problems sharing K = 256, the middle one without an adapter; TWIN: nk = 1 into two rank tiles, the same shape
    twice with different t / B'.  Epilogues and scale kinds mixed across the problems of a launch."""
    ops = _ops()
    devs = [_Dev(ops, p) for p in GL.group(name)]
    for launch in GL.LAUNCHES[name]:
        bufs, views, singles = [], [], []
        for d, (epi, per_row, bias) in zip(devs, launch):
            buf, view = P.sentinel_buffer(d.p.M, d.p.N, DEV)
            sbuf, sview = P.sentinel_buffer(d.p.M, d.p.N, DEV)
            if epi == "gate_res":            # in place in the grouped launch, separate in the single one
                view.copy_(d.res)
            bufs.append(buf), views.append(view), singles.append((sbuf, sview))
        ops.gemm_fp8_grouped([d.qa for d in devs], [d.sa for d in devs], [d.w[v[1]] for d, v in zip(devs, launch)],
                             [d.bias if v[2] else None for d, v in zip(devs, launch)], views, [v[0] for v in launch],
                             gate_list=[d.gate for d in devs], residual_list=[vw if v[0] == "gate_res" else None for vw, v in zip(views, launch)],
                             lora_t_list=[d.t for d in devs], lora_B_list=[d.lb for d in devs])
        for d, (epi, per_row, bias), (sbuf, sview) in zip(devs, launch, singles):
            kw = dict(gate=d.gate, residual=d.res) if epi == "gate_res" else {}
            if d.t is not None:
                kw.update(lora_t=d.t, lora_B=d.lb)
            ops.gemm_fp8(d.qa, d.sa, d.w[per_row], d.bias if bias else None, out=sview, epilogue=epi, **kw)
        torch.cuda.synchronize()
        for i, (d, (epi, per_row, bias)) in enumerate(zip(devs, launch)):
            what = f"{name} problem {i} ({d.p.M}x{d.p.N} Rp {d.p.Rp}) {epi} sw={'row' if per_row else 'one'} bias={bias}"
            assert torch.equal(bufs[i], singles[i][0]), f"{what}: differs from its own single launch"
            if epi == "gelu":
                _check_gelu(bufs[i], d.p.pre_activation(per_row, bias), what)
            else:
                _check_exact(bufs[i], d.p.want(epi, per_row, bias), what)


def test_one_hot_rank_on_two_problems_with_different_rank_counts():
    """all codes zero, one product per output: each problem reads its own t / B' and its own rank count"""
    ops = _ops()
    ohs = GL.one_hot_group()
    K = GL.ONE_HOT_K
    out = [P.sentinel_buffer(oh.M, oh.N, DEV) for oh in ohs]
    ops.gemm_fp8_grouped([_codes(torch.zeros(oh.M, K, dtype=U8)) for oh in ohs], [oh.sa.to(DEV) for oh in ohs],
                         [ops.Fp8Weight(torch.zeros(oh.N, K, dtype=U8, device=DEV).view(F8), oh.sw.to(DEV)) for oh in ohs],
                         [None, None], [v for _, v in out], "bias",
                         lora_t_list=[_padded(oh.t) for oh in ohs], lora_B_list=[_padded(oh.lb) for oh in ohs])
    torch.cuda.synchronize()
    for i, (oh, (buf, _)) in enumerate(zip(ohs, out)):
        _check_exact(buf, P.expected(oh.ref()), f"one-hot rank, problem {i} (Rp {oh.Rp})")


# --------------------------------------------------------------------------------------------------------- fused q/k/v
H, QK, S_OUT = 2, 256, 277
STREAMS = ((200, 77), (77, 0))         # (M, row0): an unaligned stream (element-wise V^T store) and a part-filled last tile


def _stream(ops, M, seed, Rp, N=3 * H * 128):
    """one QKV problem on random codes: (codes, scales, weight, bias, t or None, B' or None)"""
    c = GL.random_case(M, N, QK, max(Rp, 64))
    w = ops.Fp8Weight(c["qw"].view(F8).to(DEV), c["sw"].to(DEV))
    t = _padded(c["t"][:, :Rp]) if Rp else None
    lb = _padded(c["lb"][:, :Rp]) if Rp else None
    return _codes(c["qa"]), c["sa"].to(DEV), w, c["bias"].to(DEV), t, lb


def _qkv_outputs():
    Skp = (S_OUT + 63) // 64 * 64          # the two-pass V^T pass writes whole 64-key tiles
    return (torch.full((H, S_OUT, 128), 3.0, dtype=BF, device=DEV), torch.full((H, S_OUT, 128), 3.0, dtype=BF, device=DEV),
            torch.zeros((H, 128, Skp), dtype=BF, device=DEV))


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "no-norm"])
@pytest.mark.parametrize("ranks", [(64, 64), (128, 128), (64, 0), (0, 128)], ids=lambda r: f"r{r[0]}-{r[1]}")
def test_fused_qkv_is_the_grouped_lora_launch_followed_by_qkv_prepare(ranks, norm):
    ops = _ops()
    from apex_studio_amd import lib
    probs = [_stream(ops, M, i, Rp) for i, ((M, _), Rp) in enumerate(zip(STREAMS, ranks))]
    g = torch.Generator().manual_seed(9)
    nw = [(1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV) for _ in range(4)] if norm else [None] * 4
    ang = torch.rand(S_OUT, 64, generator=g) * 6.28
    rope = torch.stack([ang.cos().repeat_interleave(2, 1), ang.sin().repeat_interleave(2, 1)]).float().contiguous().to(DEV)
    row0 = [r for _, r in STREAMS]
    lists = ([p[0] for p in probs], [p[1] for p in probs], [p[2] for p in probs], [p[3] for p in probs])
    lora = dict(lora_t_list=[p[4] for p in probs], lora_B_list=[p[5] for p in probs])
    q1, k1, v1 = _qkv_outputs()
    ops.gemm_fp8_grouped_qkv(*lists, [None, None], "bias", [1, 1], [nw[0], nw[1]], [nw[2], nw[3]], row0, H, 1e-6, rope, q1, k1, v1, **lora)
    # two-pass: the grouped LoRA launch into the joint [S, 3 inner] buffer, then qkv_prepare (text rows first: split = 77)
    QKV = torch.zeros(S_OUT, 3 * H * 128, dtype=BF, device=DEV)
    ops.gemm_fp8_grouped(*lists, [QKV[r:r + M] for M, r in STREAMS], "bias", **lora)
    q2, k2, v2 = _qkv_outputs()
    inner = H * 128
    ops.qkv_prepare(QKV[:, :inner], QKV[:, inner:2 * inner], QKV[:, 2 * inner:], H, q2, k2, v2, wq=nw[0], wk=nw[2], wq2=nw[1], wk2=nw[3],
                    split=77, eps=1e-6, rope=rope, rope_mode=lib.ROPE_INTERLEAVED)
    torch.cuda.synchronize()
    assert torch.isfinite(q1.float()).all() and float(q1.float().std()) > 0
    assert torch.equal(q1, q2) and torch.equal(k1, k2), "q / k"
    assert torch.equal(v1[:, :, :S_OUT], v2[:, :, :S_OUT]), "V^T"


def test_single_block_shape_qkv_plus_gelu_problem_sharing_the_codes():
    ops = _ops()
    from apex_studio_amd import lib
    M = 200
    qa, sa, w, b, t, lb = _stream(ops, M, 0, 64)
    c2 = GL.random_case(M, 272, QK, 128)
    w2, b2 = ops.Fp8Weight(c2["qw"].view(F8).to(DEV), c2["sw"].to(DEV)), c2["bias"].to(DEV)
    t2, lb2 = _padded(c2["t"]), _padded(c2["lb"])
    g = torch.Generator().manual_seed(10)
    nq, nk = [(1 + 0.1 * torch.randn(128, generator=g)).to(BF).to(DEV) for _ in range(2)]
    ang = torch.rand(M, 64, generator=g) * 6.28
    rope = torch.stack([ang.cos().repeat_interleave(2, 1), ang.sin().repeat_interleave(2, 1)]).float().contiguous().to(DEV)
    lists = ([qa, qa], [sa, sa], [w, w2], [b, b2])
    lora = dict(lora_t_list=[t, t2], lora_B_list=[lb, lb2])
    mk = lambda: (torch.zeros(H, M, 128, dtype=BF, device=DEV), torch.zeros(H, M, 128, dtype=BF, device=DEV),  # noqa: E731
                  torch.zeros(H, 128, 256, dtype=BF, device=DEV))
    q1, k1, v1 = mk()
    mlp1 = torch.zeros(M, 272, dtype=BF, device=DEV)
    ops.gemm_fp8_grouped_qkv(*lists, [None, mlp1], ["bias", "gelu"], [1, 0], [nq, None], [nk, None], [0, 0], H, 1e-6, rope, q1, k1, v1, **lora)
    QKV, mlp2 = torch.zeros(M, 3 * H * 128, dtype=BF, device=DEV), torch.zeros(M, 272, dtype=BF, device=DEV)
    ops.gemm_fp8_grouped(*lists, [QKV, mlp2], ["bias", "gelu"], **lora)
    q2, k2, v2 = mk()
    inner = H * 128
    ops.qkv_prepare(QKV[:, :inner], QKV[:, inner:2 * inner], QKV[:, 2 * inner:], H, q2, k2, v2, wq=nq, wk=nk, split=0, eps=1e-6, rope=rope,
                    rope_mode=lib.ROPE_INTERLEAVED)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(k1, k2) and torch.equal(v1[:, :, :M], v2[:, :, :M]) and torch.equal(mlp1, mlp2)
    assert float(mlp1.float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_launch():
    ops = _ops()
    from apex_studio_amd import lib
    devs = [_Dev(ops, p) for p in GL.group("twin")]
    outs = [P.sentinel_buffer(d.p.M, d.p.N, DEV) for d in devs]

    def launch(n=2, **kw):
        ds = (devs * 3)[:n]
        args = dict(lora_t_list=[d.t for d in ds], lora_B_list=[d.lb for d in ds])
        args.update(kw)
        ops.gemm_fp8_grouped([d.qa for d in ds], [d.sa for d in ds], [d.w[True] for d in ds], [d.bias for d in ds],
                             [(outs * 3)[i][1] for i in range(n)], "bias", **args)

    t, lb = devs[0].t, devs[0].lb
    wide = torch.zeros(devs[0].p.M, 136, dtype=BF, device=DEV)
    cases = (("no problem carries an adapter", dict(lora_t_list=[None, None], lora_B_list=[None, None])),
             ("Rp=32", dict(lora_t_list=[t[:, :32], t], lora_B_list=[lb[:, :32], lb])),
             ("at least Rp=128 wide", dict(lora_t_list=[t, wide.as_strided((devs[0].p.M, 128), (120, 1))])),
             ("16-byte aligned", dict(lora_t_list=[t, wide[:, 4:132]])),
             ("block_scales_list / out_mx_list", dict(out_mx_list=[None, None])),
             ("count=5", dict(n=5)))
    for needle, kw in cases:
        with pytest.raises(lib.ApexMIError, match=needle):
            launch(**kw)
    torch.cuda.synchronize()
    for buf, _ in outs:
        assert bool((buf == P.SENTINEL).all()), "a refused launch wrote something"


# -------------------------------------------------------------------------------------------------------- random operands
# The grouped form is the arithmetic of the single-problem kernel, which sits at 1.65e-3 .. 1.70e-3 (tests/test_gpu_gemm_fp8_lora.py);
# measured on the MI355X (profiles/flux_fp8_lora_measured.jsonl): see the values beside the calls; the bars are 2x those
# measured: 200x272 1.665e-3, 77x272 1.659e-3
_BARS = {"200x272": 3.33e-3, "77x272": 3.32e-3}


def test_random_operands_against_the_float64_contract():
    ops = _ops()
    shapes, K = GL.RANDOM
    cs = [GL.random_case(M, N, K, Rp) for M, N, Rp in shapes]
    ws = [ops.Fp8Weight(c["qw"].view(F8).to(DEV), c["sw"].to(DEV)) for c in cs]
    qa, sa, bias = [_codes(c["qa"]) for c in cs], [c["sa"].to(DEV) for c in cs], [c["bias"].to(DEV) for c in cs]
    ts, lbs = [_padded(c["t"]) for c in cs], [_padded(c["lb"]) for c in cs]
    outs = [torch.zeros(M, N, dtype=BF, device=DEV) for M, N, _ in shapes]
    ops.gemm_fp8_grouped(qa, sa, ws, bias, outs, "bias", lora_t_list=ts, lora_B_list=lbs)
    # the second problem WITHOUT its adapter, next to the first with it: the bits of the plain single launch (the SCALED
    # epilogue's order, not the in-place order of the adapter form; tests/test_fp8_grouped_lora_host.py shows they differ here)
    mixed = [torch.zeros(M, N, dtype=BF, device=DEV) for M, N, _ in shapes]
    ops.gemm_fp8_grouped(qa, sa, ws, bias, mixed, "bias", lora_t_list=[ts[0], None], lora_B_list=[lbs[0], None])
    plain = ops.gemm_fp8(qa[1], sa[1], ws[1], bias[1])
    single = ops.gemm_fp8(qa[0], sa[0], ws[0], bias[0], lora_t=ts[0], lora_B=lbs[0])
    torch.cuda.synchronize()
    assert torch.equal(mixed[1], plain), "a problem without an adapter leaves the bits of apexmi_gemm_fp8"
    assert torch.equal(mixed[0], single) and torch.equal(outs[0], single)
    for (M, N, _), c, o in zip(shapes, cs, outs):
        rel = float((o.cpu().double() - c["ref"]).norm() / c["ref"].norm())
        print(f"[gemm_fp8 grouped lora {M}x{N}x{K} r64] rel-L2 against the float64 contract {rel:.3e}")
        measured(f"gemm_fp8_grouped_lora.bias.{M}x{N}x{K}.r64", rel, _BARS[f"{M}x{N}"])
