"""Per-element probes of ln_modulate (block kernel, wave kernel under ln.wave 0 / 1 / 2, every operand form and storage),
qkv_prepare (qk.group 0 / 2 / 1), qk_rms_rope_rows, v_transpose, rope_half_ and the casts.  Operands, float64 references, the
envelope and the verdict: tests/norm_rope_probes.py; what the verdict rejects and the older two-number bar accepts, and the two
conditions of the envelope for every case below: tests/test_norm_rope_probes_host.py.

Everything without a reciprocal square root is compared with torch.equal on WHOLE sentinel-filled buffers; the norms must lie in
the a-priori envelope, bit for bit where the envelope holds one bf16 value.  Every tune key is restored in a `finally`.

MEASURED MARGIN of the envelope (worst over all cases of the variant; float outputs: |out - ref| / env, bf16 outputs: the least
pre-rounding error consistent with the output, max(0, |out - ref| - half an ulp) / env; MI355X):
  ln_modulate, block kernel (10 widths)               bf16 out 0.016   f32 out 0.085
  ln_modulate, wave kernel, ln.wave 1 and 2           bf16 out 0.020   f32 out 0.044
  ln_modulate, block kernel at 3072 / 3584 / 5120     bf16 out 0.027   f32 out 0.044
  qkv_prepare, per-head norm + RoPE, three launches   bf16 out 0.065   f32 out 0.125
  whole-row RMSNorm pass of the qk_rms_rope_rows path bf16 out 0.020   f32 out 0.046
  RoPE of a stored float norm (no norm in the call)                    f32 out 0.974   (the bound of one fma is attained)
The kernels use about a tenth of the envelope or less; it is not asserted beyond the verdict itself.

Found by these probes: apexmi_qk_rms_rope_rows_f32 was not bit-identical to the three passes (case H24.S5.r0.inter.qkv.f32 and 13
more float cases: one ulp of rstd on a few rows in a hundred).  The compiler had fused the squares of the one-pass kernel into
fmas and left those of ln_modulate_wave_kernel unfused; a float squares inexactly, a bf16 value exactly, so only the float form
showed it.  Both kernels now square float rows through add_square_unfused (csrc/elementwise.hip)."""
import contextlib
import functools

import pytest
import torch

from tests import norm_rope_probes as N
from tests.norm_rope_probes import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = {"ln.wave": 1, "qk.group": 1}


@contextlib.contextmanager
def tuned():
    """yields lib.tune_set; the shipped values come back whatever happens"""
    from apex_studio_amd import lib
    try:
        yield lib.tune_set
    finally:
        for key, v in DEFAULTS.items():
            lib.tune_set(key, v)


def _ops():
    from apex_studio_amd import ops
    return ops


class Margin:
    """largest |err| / env seen, per output type"""

    def __init__(self, what):
        self.what, self.worst = what, {}

    def add(self, v, out):
        k = "bf16" if out.dtype == BF else "f32"
        self.worst[k] = max(self.worst.get(k, 0.0), v.ratio)

    def report(self):
        print(f"[margin] {self.what}: " + ", ".join(f"{k} out {r:.3f}" for k, r in sorted(self.worst.items())))


def _judge(out, ref, env, what, margin):
    v = N.verdict(out, ref, env)
    assert v.passed, f"{what}: {N.describe(v, out, ref, env)}"
    margin.add(v, out)


def _same(got, want, what):
    msg = N.mismatches(got, want)
    assert not msg, f"{what}: {msg}"


# ---------------------------------------------------------------------------------------------------------------- ln_modulate
@functools.lru_cache(maxsize=None)
def _mods_dev(C):
    return {k: t.to(DEV) for k, t in N.mod_vectors(C).items()}


def _ln_run(case):
    """the case on the device -> (out rows [M, C] on the host, None or a message about a store outside them)"""
    ops = _ops()
    x64, mods = N.ln_operands(case)
    M, C = x64.shape
    xd, od = N.storage_dtypes(case.storage)
    px, po = N.ln_pad(case.storage) if case.layout == "strided" else (0, 0)
    xbuf = torch.full((M, C + px), N.SENTINEL, dtype=xd)
    xbuf[:, :C] = x64.to(xd)
    xbuf = xbuf.to(DEV)
    x = xbuf[:, :C]
    if case.layout == "inplace":
        obuf, out = None, x
    else:                                   # one guard row above and below, guard columns when strided
        obuf = torch.full((M + 2, C + po), N.SENTINEL, dtype=od, device=DEV)
        out = obuf[1:M + 1, :C]
    kw = {k: _mods_dev(C)[k] for k in mods}
    got = ops.ln_modulate(x, out=out, eps=N.EPS, rms="rms" in N.FORMS[case.form], split=case.split, **kw)
    assert got.data_ptr() == out.data_ptr()
    rows = out.cpu()
    if obuf is not None:
        whole = obuf.cpu()
        want = torch.full_like(whole, N.SENTINEL)
        want[1:M + 1, :C] = rows
        _same(whole, want, f"{case.id}: store outside the output rows (guards included)")
        assert torch.equal(xbuf.cpu()[:, :C], x64.to(xd)), f"{case.id}: x changed"
    assert torch.equal(xbuf.cpu()[:, C:], torch.full((M, px), N.SENTINEL, dtype=xd)), f"{case.id}: store into the pad columns of x"
    return rows


def _ln_check(case, rows, margin):
    ref, env = N.ln_case_ref(case)
    _judge(rows, ref, env, case.id, margin)


@pytest.mark.parametrize("C", N.BLOCK_C)
def test_ln_modulate_block_kernel(C):
    margin = Margin(f"ln_modulate block kernel C = {C}")
    for case in N.ln_cases(C):
        _ln_check(case, _ln_run(case), margin)
    margin.report()


@pytest.mark.parametrize("C", N.WAVE_C)
def test_ln_modulate_wave_kernel_one_and_two_rows_per_wave(C):
    """ln.wave = 1 under the verdict; ln.wave = 2 (two rows per wave, bf16 x) must give the same bits at every case"""
    margin = Margin(f"ln_modulate wave kernel (ln.wave 1 = 2) C = {C}")
    with tuned() as tune:
        for case in N.ln_cases(C):
            tune("ln.wave", 1)
            one = _ln_run(case)
            _ln_check(case, one, margin)
            tune("ln.wave", 2)
            _same(_ln_run(case), one, f"{case.id}: ln.wave = 2 against ln.wave = 1")
    margin.report()


@pytest.mark.parametrize("C", N.WAVE_C)
def test_ln_modulate_block_kernel_at_the_wave_widths(C):
    """ln.wave = 0: the sums differ in shape from the wave kernel's, so this run stands under the verdict, not under torch.equal"""
    margin = Margin(f"ln_modulate block kernel (ln.wave 0) C = {C}")
    with tuned() as tune:
        tune("ln.wave", 0)
        for case in N.ln_cases(C):
            _ln_check(case, _ln_run(case), margin)
    margin.report()


# ---------------------------------------------------------------------------------------------------------------- qkv_prepare
def _proj(q, k, v, dt):
    """[S, 3 W + 8] device buffer with q | k | v side by side (absent ones left at the sentinel) and its three row views"""
    S, W = q.shape
    buf = torch.full((S, 3 * W + 8), N.SENTINEL, dtype=dt)
    for i, t in enumerate((q, k, v)):
        if t is not None:
            buf[:, i * W:(i + 1) * W] = t.to(dt)
    buf = buf.to(DEV)
    return [buf[:, i * W:(i + 1) * W] if t is not None else None for i, t in enumerate((q, k, v))]


def _dev(t):
    return None if t is None else t.to(DEV)


def _qk_check(got, want, case, name, exact, margin):
    """got: the whole [H, S_out, 128] buffer on the host; want = (ref, env) of the rows [row0, row0 + S)"""
    ref, env = want
    if exact:
        _same(got, N.placed(N.store(ref, got.dtype), case.S_out, case.row0), f"{case.id} {name}")
        return
    rows = got[:, case.row0:case.row0 + case.S]
    _judge(rows, ref, env, f"{case.id} {name}", margin)
    _same(got, N.placed(rows, case.S_out, case.row0), f"{case.id} {name}: rows of another stream")


@pytest.mark.parametrize("H", N.QKV_H)
def test_qkv_prepare_three_launches(H):
    """qk.group 0 / 2 / 1 (H = 3 takes the one-head kernel under any setting): identical bits, and the first under the verdicts"""
    ops = _ops()
    margin = Margin(f"qkv_prepare H = {H}")
    with tuned() as tune:
        for case in N.qkv_cases(H):
            o, want = N.qkv_operands(case), N.qkv_expected(case)
            dt = F32 if case.f32 else BF
            q, k, v = _proj(o["q"], o["k"], o["v"], dt)
            table = _dev(o["table"])
            outs = []
            for grp in (0, 2, 1):
                tune("qk.group", grp)
                qo = torch.full((H, case.S_out, 128), N.SENTINEL, dtype=dt, device=DEV)
                ko = torch.full_like(qo, N.SENTINEL) if k is not None else None
                vt = torch.full((H, 128, case.Skp), N.SENTINEL, dtype=dt, device=DEV) if v is not None else None
                ops.qkv_prepare(q, k, v, H, qo, ko, vt, wq=_dev(o["wq"]), wk=_dev(o["wk"]), wq2=_dev(o["wq2"]), wk2=_dev(o["wk2"]),
                                split=case.split, eps=N.EPS, rope=table, rope_mode=case.mode, row0=case.row0)
                outs.append([None if t is None else t.cpu() for t in (qo, ko, vt)])
            for grp, other in zip((2, 1), outs[1:]):
                for name, a, b in zip("qkv", outs[0], other):
                    if a is not None:
                        _same(b, a, f"{case.id} {name}: qk.group = {grp} against 0")
            qo, ko, vt = outs[0]
            _qk_check(qo, want["q"], case, "q", case.norm == "none", margin)
            if ko is not None:
                _qk_check(ko, want["k"], case, "k", case.norm == "none", margin)
            if vt is not None:
                _same(vt, want["vt"], f"{case.id} V^T (transpose, zero pad, sentinel outside the tiles)")
    margin.report()


# ----------------------------------------------------------------------------------------------------------- qk_rms_rope_rows
@pytest.mark.parametrize("case", N.rows_cases(), ids=lambda c: c.id)
def test_qk_rms_rope_rows_equals_the_three_passes(case):
    """The three passes (whole-row RMSNorm on q, on k, then qkv_prepare without norm weights) each under their verdict, and the
    one-pass kernel bit-identical to them on whole sentinel-filled buffers."""
    ops = _ops()
    margin, margin_rope = Margin(f"whole-row RMSNorm of {case.id}"), Margin(f"RoPE of the stored norm of {case.id}")
    H, S, C, dt = case.H, case.S, case.H * 128, F32 if case.f32 else BF
    o = N.rows_operands(H, S, case.f32)
    full = case.kv == "qkv"
    q, k, v = _proj(o["q"], o["k"] if full else None, o["v"] if full else None, dt)
    wq, wk, table = _dev(o["wq"]), _dev(o["wk"]), _dev(N.rope_table(case.S_out, case.mode))

    def buffers():
        qo = torch.full((H, case.S_out, 128), N.SENTINEL, dtype=dt, device=DEV)
        return qo, (torch.full_like(qo, N.SENTINEL) if full else None), \
            (torch.full((H, 128, case.Skp), N.SENTINEL, dtype=dt, device=DEV) if full else None)

    # pass 1 and 2: the norms, into a second projection buffer with the same row stride
    nq, nk, nv = _proj(o["q"], o["k"] if full else None, o["v"] if full else None, dt)
    stored = {}
    for name, x, n, w, x64 in (("q", q, nq, wq, o["q"]), ("k", k, nk, wk, o["k"])):
        if x is None:
            continue
        ops.ln_modulate(x, out=n, gamma=w, eps=N.EPS, rms=True)
        stored[name] = n.cpu()
        ref, env = N.ln_ref(x64, C, rms=True, gamma=o["w" + name])
        _judge(stored[name], ref, env, f"{case.id} norm of {name}", margin)
    # pass 3: RoPE + layout + V^T
    q3, k3, vt3 = buffers()
    ops.qkv_prepare(nq, nk, nv, H, q3, k3, vt3, eps=N.EPS, rope=table, rope_mode=case.mode, row0=case.row0)
    for name, got in (("q", q3), ("k", k3)):
        if got is None:
            continue
        want = N.rope_only_expected(stored[name].double(), H, N.rope_table(case.S_out, case.mode), case.mode, case.row0)
        _qk_check(got.cpu(), want, case, f"RoPE of the stored {name}", not case.f32, margin_rope)
    if full:
        _same(vt3.cpu(), N.vt_expected(o["v"], H, case.Skp, case.row0, dt), f"{case.id} V^T")
    # the one-pass kernel
    q1, k1, vt1 = buffers()
    ops.qk_rms_rope_rows(q, k, v, H, q1, k1, vt1, wq=wq, wk=wk if full else None, eps=N.EPS, rope=table, rope_mode=case.mode,
                         row0=case.row0)
    for name, a, b in (("q", q1, q3), ("k", k1, k3), ("V^T", vt1, vt3)):
        if a is not None:
            _same(a.cpu(), b.cpu(), f"{case.id} {name}: one pass against three")
    margin.report()
    if case.f32:
        margin_rope.report()


# ------------------------------------------------------------------------------------------------- v_transpose, rope_half, casts
@pytest.mark.parametrize("S,H", N.V_TRANSPOSE_CASES)
def test_v_transpose_strided_view(S, H):
    ops = _ops()
    v64 = N.grid_x(S, H * 128, 4)
    _, _, v = _proj(v64, None, v64, BF)                # the third slice of a [S, 3 W + 8] buffer
    Skp = N.round_up(S, 64) + 64
    vt = torch.full((H, 128, Skp), N.SENTINEL, dtype=BF, device=DEV)
    ops.v_transpose(v.unflatten(1, (H, 128)), vt)
    _same(vt.cpu(), N.vt_expected(v64, H, Skp, 0, BF), f"v_transpose S = {S}")


@pytest.mark.parametrize("Dh,heads,f32", N.ROPE_HALF_CASES)
def test_rope_half_exact(Dh, heads, f32):
    ops = _ops()
    dt = F32 if f32 else BF
    buf64, cos, sin, want = N.rope_half_case(Dh, heads)
    buf = buf64.to(dt).to(DEV)
    ops.rope_half_(buf[:, :heads * 128], heads, 128, cos.to(DEV), sin.to(DEV))
    _same(buf.cpu(), N.store(want, dt), f"rope_half D = {Dh} heads = {heads}")


def test_cast_f32_to_bf16_rounds_to_nearest_even_at_every_code_point():
    ops = _ops()
    x = N.cast_probe_inputs()
    got = ops.to_bf16(x.to(DEV)).cpu()
    bad = (got.view(torch.int16) != x.to(BF).view(torch.int16)).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} differ; first f32 bits {[hex(int(x.view(torch.int32)[i]) & 0xFFFFFFFF) for i in bad[:6]]}"
    nan = ops.to_bf16(N.cast_nan_inputs().to(DEV)).cpu()
    assert bool(torch.isnan(nan.float()).all())


def test_cast_bf16_to_f32_on_all_code_points():
    ops = _ops()
    x = N.all_bf16_codes()
    got, want = ops.to_f32(x.to(DEV)).cpu(), x.float()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32)), "bit for bit, the sign of zero included"
