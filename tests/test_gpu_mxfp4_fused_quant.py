"""The two fusions of the MXFP4 mode that remove a `quant_blocks_mxfp4` launch: the norm that writes MXFP4
(`ops.ln_modulate_quant_mxfp4`) and the MXFP4 output of the fp4 GEMM (`ops.gemm_mxfp4(out_mx=)` and the grouped forms).  Both are
defined as BIT-IDENTICAL to the launches they replace, so every check here is `torch.equal` against those launches on the same
operands: `ops.ln_modulate` -> `ops.quant_blocks_mxfp4`, and `ops.gemm_mxfp4` -> `ops.quant_blocks_mxfp4`.  The quantiser itself
is pinned against the CPU restatement of the format in tests/test_gpu_mxfp4.py."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
U8 = torch.uint8
SENT = 0x5A


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


@contextlib.contextmanager
def ln_wave(v):
    from apex_studio_amd import lib
    try:
        lib.tune_set("ln.wave", v)
        yield
    finally:
        lib.tune_set("ln.wave", 1)


def _rand(shape, seed, dtype=BF, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


# ------------------------------------------------------------------------------------------------------------------- 1. the norm
# every operand form of the norm: (rms, gamma, beta, modulation, split: 0 none | 1 in the middle | 2 at M)
FORMS = [(False, False, False, False, 0), (False, True, True, True, 0), (False, False, False, True, 1), (False, True, False, True, 2),
         (True, True, False, False, 0), (True, False, False, False, 0), (True, True, False, True, 1)]


def _norm_operands(C, form, seed):
    rms, has_g, has_b, has_mod, _ = form
    kw = {"rms": rms, "eps": 1e-6}
    if has_g:
        g = _rand((C,), seed + 1) + 1.0
        # planted: gamma zero over one aligned block (a zero block: scale byte 127, the sign of -0 kept) and powers of two over
        # another, so that the exponents of neighbouring blocks differ by more than the data would make them
        g[32:64] = 0.0
        g[64:96] = 2.0 ** 9
        if C >= 256:
            g[C - 64:C - 32] = 2.0 ** -11
        kw["gamma"] = g
    if has_b:
        b = _rand((C,), seed + 2, scale=0.25)
        b[32:64] = 0.0
        kw["beta"] = b
    if has_mod:
        kw["scale"], kw["shift"] = _rand((C,), seed + 3, torch.float32, 0.3), _rand((C,), seed + 4, torch.float32, 0.3)
        kw["scale2"], kw["shift2"] = _rand((C,), seed + 5, torch.float32, 0.3), _rand((C,), seed + 6, torch.float32, 0.3)
        if has_g and not rms:
            for k in ("shift", "shift2"):
                kw[k][32:64] = 0.0          # keep the planted zero block zero through the modulation
    return kw


@pytest.mark.parametrize("xdt", [BF, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("wave", [0, 1, 2])
@pytest.mark.parametrize("C", [128, 256, 1536, 3072, 3584, 5120, 8192])
def test_norm_writes_the_bits_of_norm_then_quantise(C, wave, xdt):
    ops = _ops()
    with ln_wave(wave):
        for M in (1, 5, 67):
            x = _rand((M, C + 8), 100 + M, xdt)[:, :C]         # a row stride wider than the row
            for fi, form in enumerate(FORMS):
                kw = _norm_operands(C, form, 7 * fi)
                kw["split"] = (0, M // 2, M)[form[4]]
                if form[4] == 0:
                    kw.pop("scale2", None), kw.pop("shift2", None)
                xn = ops.ln_modulate(x, out=torch.empty(M, C, dtype=BF, device=DEV), **kw)
                wq, ws = ops.quant_blocks_mxfp4(xn)
                # wider rows than needed, sentinel-filled; `out` given on every other form
                qbuf = torch.full((M, C // 2 + 16), SENT, dtype=U8, device=DEV)
                sbuf = torch.full((M, C // 32 + 3), SENT, dtype=U8, device=DEV)
                obuf = torch.full((M, C + 8), 3.0, dtype=BF, device=DEV) if fi % 2 else None
                q, s = ops.ln_modulate_quant_mxfp4(x, codes=qbuf[:, :C // 2], scale_out=sbuf[:, :C // 32],
                                                   out=None if obuf is None else obuf[:, :C], **kw)
                what = f"C {C} wave {wave} M {M} form {form}"
                assert torch.equal(s, ws), f"scale bytes, {what}: {int((s != ws).sum())} differ"
                assert torch.equal(q, wq), f"codes, {what}: {int((q != wq).sum())} bytes differ"
                assert bool((qbuf[:, C // 2:] == SENT).all()) and bool((sbuf[:, C // 32:] == SENT).all()), f"padding written, {what}"
                if obuf is not None:
                    assert torch.equal(obuf[:, :C], xn) and bool((obuf[:, C:] == 3.0).all()), f"out, {what}"
                if form[1] and not form[0]:
                    assert bool((s[:, 1] == 127).all()), f"the zero block's scale byte, {what}"
                    assert bool(((q[:, 16:32] & 0x77) == 0).all()), f"the zero block's magnitudes, {what}"


def test_norm_keeps_the_sign_of_minus_zero_and_defaults_to_the_scratch():
    ops = _ops()
    M, C = 5, 256
    x = _rand((M, C), 3)
    g = torch.ones(C, dtype=BF, device=DEV)
    g[32:64] = 0.0
    xn = ops.ln_modulate(x, gamma=g)
    assert bool((xn[:, 32:64] == 0).all()) and bool((xn[:, 32:64].view(torch.int16) != 0).any()), "the planted block holds -0"
    wq, ws = ops.quant_blocks_mxfp4(xn)
    q, s = ops.ln_modulate_quant_mxfp4(x, gamma=g)                # the per-stream scratch of the fp4 route
    assert torch.equal(q, wq) and torch.equal(s, ws)
    assert bool((q[:, 16:32] & 0x88).any()), "sign bits of -0 are kept"
    assert q.stride(0) % 16 == 0


# --------------------------------------------------------------------------------------------------------- 2. the GEMM's MX output
def _weight(N, K, seed, zero_rows=None):
    ops = _ops()
    w = _rand((N, K), seed, scale=0.5)
    if zero_rows is not None:
        w[zero_rows[0]:zero_rows[1]] = 0.0
    return ops.Mxfp4Weight.from_bf16(w)


def _acts(M, K, seed):
    return _ops().quant_blocks_mxfp4(_rand((M, K), seed))


def _mx_buffers(M, N, extra_rows=0):
    qbuf = torch.full((M + extra_rows, N // 2 + 16), SENT, dtype=U8, device=DEV)
    sbuf = torch.full((M + extra_rows, N // 32 + 4), SENT, dtype=U8, device=DEV)
    return qbuf, sbuf


@pytest.mark.parametrize("epilogue", ["bias", "gelu"])
@pytest.mark.parametrize("K", [256, 512])
@pytest.mark.parametrize("N", [128, 256, 512])
@pytest.mark.parametrize("M", [1, 127, 129, 200])
def test_gemm_mx_output_is_the_bf16_launch_then_quantise(M, N, K, epilogue):
    ops = _ops()
    qa, sa = _acts(M, K, 11 + M)
    w = _weight(N, K, 13 + N, zero_rows=(32, 64))                 # 32 zero weight rows: with a zero bias a zero output block
    for has_bias in (False, True):
        bias = None
        if has_bias:
            bias = _rand((N,), 17, scale=0.5)
            bias[32:64] = 0.0
        ref = ops.gemm_mxfp4(qa, sa, w, bias, epilogue=epilogue)
        wq, ws = ops.quant_blocks_mxfp4(ref)
        qbuf, sbuf = _mx_buffers(M, N, extra_rows=3)               # a taller and wider buffer: rows >= M and the padding stay
        q, s = ops.gemm_mxfp4(qa, sa, w, bias, epilogue=epilogue, out_mx=(qbuf[:M, :N // 2], sbuf[:M, :N // 32]))
        what = f"M {M} N {N} K {K} {epilogue} bias {has_bias}"
        # the entry point with a C that must not be written (the wrapper passes none)
        from apex_studio_amd import lib
        cbuf = torch.full((M, N), 9.0, dtype=BF, device=DEV)
        q2, s2 = torch.empty_like(wq), torch.empty_like(ws)
        rc = lib.load().apexmi_gemm_mxfp4_mx(qa.data_ptr(), qa.stride(0), sa.data_ptr(), sa.stride(0), w.q.data_ptr(), w.q.stride(0),
                                             w.s.data_ptr(), w.s.stride(0), None if bias is None else bias.data_ptr(), cbuf.data_ptr(),
                                             cbuf.stride(0), q2.data_ptr(), q2.stride(0), s2.data_ptr(), s2.stride(0), M, N, K,
                                             lib.EPI_BIAS_GELU if epilogue == "gelu" else lib.EPI_BIAS, None, None, 0, ops._stream())
        assert rc == 0 and torch.equal(q2, wq) and torch.equal(s2, ws), what
        assert torch.equal(s, ws), f"scale bytes, {what}: {int((s != ws).sum())} differ"
        assert torch.equal(q, wq), f"codes, {what}: {int((q != wq).sum())} bytes differ"
        assert bool((s[:, 1] == 127).all()) and bool(((q[:, 16:32] & 0x77) == 0).all()), f"the planted zero block, {what}"
        assert bool((qbuf[M:] == SENT).all()) and bool((sbuf[M:] == SENT).all()), f"rows >= M written, {what}"
        assert bool((qbuf[:, N // 2:] == SENT).all()) and bool((sbuf[:, N // 32:] == SENT).all()), f"padding written, {what}"
        assert bool((cbuf == 9.0).all()), f"C written, {what}"


def test_gemm_mx_chain_equals_the_three_launches():
    ops = _ops()
    M, K, H, N = 200, 256, 512, 256
    qa, sa = _acts(M, K, 21)
    w_up, w_down = _weight(H, K, 22), _weight(N, H, 23)
    b_up, b_down = _rand((H,), 24, scale=0.5), _rand((N,), 25, scale=0.5)
    h = ops.gemm_mxfp4(qa, sa, w_up, b_up, epilogue="gelu")
    want = ops.gemm_mxfp4(*ops.quant_blocks_mxfp4(h), w_down, b_down)
    hq = torch.empty((M, H // 2), dtype=U8, device=DEV)
    hs = torch.empty((M, H // 32), dtype=U8, device=DEV)
    pair = ops.gemm_mxfp4(qa, sa, w_up, b_up, epilogue="gelu", out_mx=(hq, hs))
    assert pair[0] is hq and pair[1] is hs
    assert torch.equal(ops.gemm_mxfp4(hq, hs, w_down, b_down), want)


def test_gemm_route_keywords():
    ops = _ops()
    M, K, H = 67, 256, 512
    a = _rand((M, K), 31)
    w = torch.nn.Parameter(_rand((H, K), 32, scale=0.5), requires_grad=False)
    w._fp4 = ops.Mxfp4Weight.from_bf16(w.data)
    want = ops.gemm(a, w, epilogue="gelu")
    pair = ops.quant_blocks_mxfp4(a)
    never = torch.empty_like(a)                                    # only its shape is read
    assert torch.equal(ops.gemm(never, w, epilogue="gelu", quantised_mxfp4=pair), want)
    hq, hs = ops.gemm(never, w, epilogue="gelu", quantised_mxfp4=pair,
                      out_mxfp4=(torch.empty((M, H // 2), dtype=U8, device=DEV), torch.empty((M, H // 32), dtype=U8, device=DEV)))
    wq, ws = ops.quant_blocks_mxfp4(want)
    assert torch.equal(hq, wq) and torch.equal(hs, ws)
    plain = _rand((H, K), 33)
    with pytest.raises(Exception, match="does not take the MXFP4 route"):
        ops.gemm(a, plain, quantised_mxfp4=pair)
    with pytest.raises(Exception, match="does not take the MXFP4 route"):
        ops.gemm(a, plain, out_mxfp4=(hq, hs))


# ---------------------------------------------------------------------------------------------------------------- 3. grouped forms
def test_grouped_mx_outputs_as_row_slices_of_one_buffer():
    ops = _ops()
    Ms, K, N = (200, 77), 256, 512
    S = sum(Ms)
    qa, sa = _acts(S, K, 41)
    rows = [(0, Ms[0]), (Ms[0], S)]
    ws_ = [_weight(N, K, 42), _weight(N, K, 43)]
    bs = [_rand((N,), 44, scale=0.5), None]
    qbuf = torch.full((S, N // 2), SENT, dtype=U8, device=DEV)
    sbuf = torch.full((S, N // 32), SENT, dtype=U8, device=DEV)
    ops.gemm_mxfp4_grouped([qa[a:b] for a, b in rows], [sa[a:b] for a, b in rows], ws_, bs, [None, None], "gelu",
                           out_mx_list=[(qbuf[a:b], sbuf[a:b]) for a, b in rows])
    for (a, b), w, bias in zip(rows, ws_, bs):
        wq, wsc = ops.gemm_mxfp4(qa[a:b], sa[a:b], w, bias, epilogue="gelu",
                                 out_mx=(torch.empty((b - a, N // 2), dtype=U8, device=DEV), torch.empty((b - a, N // 32), dtype=U8, device=DEV)))
        assert torch.equal(qbuf[a:b], wq) and torch.equal(sbuf[a:b], wsc)


def test_grouped_launch_mixes_mx_and_bf16_outputs():
    ops = _ops()
    Ms, K, Ns = (200, 77), 256, (256, 48)
    acts = [_acts(m, K, 51 + i) for i, m in enumerate(Ms)]
    ws_ = [_weight(n, K, 53 + i) for i, n in enumerate(Ns)]
    bs = [_rand((n,), 55 + i, scale=0.5) for i, n in enumerate(Ns)]
    res = _rand((Ms[1], Ns[1]), 57)
    gate = _rand((Ns[1],), 58, torch.float32)
    want0 = ops.quant_blocks_mxfp4(ops.gemm_mxfp4(*acts[0], ws_[0], bs[0]))
    want1 = ops.gemm_mxfp4(*acts[1], ws_[1], bs[1], epilogue="gate_res", gate=gate, residual=res)
    q0 = torch.empty((Ms[0], Ns[0] // 2), dtype=U8, device=DEV)
    s0 = torch.empty((Ms[0], Ns[0] // 32), dtype=U8, device=DEV)
    out1 = torch.empty((Ms[1], Ns[1]), dtype=BF, device=DEV)
    ops.gemm_mxfp4_grouped([a[0] for a in acts], [a[1] for a in acts], ws_, bs, [None, out1], ["bias", "gate_res"],
                           gate_list=[None, gate], residual_list=[None, res], out_mx_list=[(q0, s0), None])
    assert torch.equal(q0, want0[0]) and torch.equal(s0, want0[1]) and torch.equal(out1, want1)
    # a launch whose list holds no pair is the plain grouped launch
    out0 = torch.empty((Ms[0], Ns[0]), dtype=BF, device=DEV)
    ops.gemm_mxfp4_grouped([acts[0][0]], [acts[0][1]], ws_[:1], bs[:1], [out0], "bias", out_mx_list=[None])
    assert torch.equal(out0, ops.gemm_mxfp4(*acts[0], ws_[0], bs[0]))


def test_fused_qkv_launch_with_a_gelu_mx_problem():
    ops = _ops()
    H, S, K, NM = 2, 200, 256, 512
    qa, sa = _acts(S, K, 61)
    w_qkv, w_mlp = _weight(3 * H * 128, K, 62), _weight(NM, K, 63)
    b_qkv, b_mlp = _rand((3 * H * 128,), 64, scale=0.5), _rand((NM,), 65, scale=0.5)
    nq, nk = _rand((128,), 66) + 1.0, _rand((128,), 67) + 1.0
    g = torch.Generator().manual_seed(68)
    ang = torch.rand((S, 64), generator=g) * 6.28
    rope = torch.stack([torch.cos(ang).repeat_interleave(2, 1), torch.sin(ang).repeat_interleave(2, 1)]).float().contiguous().to(DEV)
    Skp = (S + 7) // 8 * 8

    def outputs():
        return [torch.zeros((H, S, 128), dtype=BF, device=DEV), torch.zeros((H, S, 128), dtype=BF, device=DEV),
                torch.zeros((H, 128, Skp), dtype=BF, device=DEV)]
    want = outputs()
    mlp = torch.empty((S, NM), dtype=BF, device=DEV)
    ops.gemm_mxfp4_grouped_qkv([qa, qa], [sa, sa], [w_qkv, w_mlp], [b_qkv, b_mlp], [None, mlp], ["bias", "gelu"], [1, 0], [nq, None],
                               [nk, None], [0, 0], H, 1e-6, rope, *want)
    wq, ws = ops.quant_blocks_mxfp4(mlp)
    got = outputs()
    mq = torch.empty((S, NM // 2), dtype=U8, device=DEV)
    ms = torch.empty((S, NM // 32), dtype=U8, device=DEV)
    ops.gemm_mxfp4_grouped_qkv([qa, qa], [sa, sa], [w_qkv, w_mlp], [b_qkv, b_mlp], [None, None], ["bias", "gelu"], [1, 0], [nq, None],
                               [nk, None], [0, 0], H, 1e-6, rope, *got, out_mx_list=[None, (mq, ms)])
    assert torch.equal(mq, wq) and torch.equal(ms, ws)
    for a, b, name in zip(got, want, ("q", "k", "V^T")):
        assert torch.equal(a, b), name
    with pytest.raises(Exception, match="fused q/k/v"):
        ops.gemm_mxfp4_grouped_qkv([qa, qa], [sa, sa], [w_qkv, w_mlp], [b_qkv, b_mlp], [None, None], ["bias", "gelu"], [1, 0],
                                   [nq, None], [nk, None], [0, 0], H, 1e-6, rope, *got,
                                   out_mx_list=[(torch.empty((S, 3 * H * 64), dtype=U8, device=DEV),
                                                 torch.empty((S, 3 * H * 4), dtype=U8, device=DEV)), None])
