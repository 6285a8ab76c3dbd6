"""`ops.ln_modulate_quant_fp8`: the norm that writes the e4m3 codes and row scales itself, held bit for bit to
the two launches it replaces (`ops.ln_modulate` into bf16, then `ops.quant_rows_fp8`) and to the quantiser's CPU restatement
(`tests.gemm_fp8_probes.quant_ref`) on the GPU's bf16 norm output.  Every comparison is torch.equal.

Widths: 128 / 256 / 1152 / 2176 / 8192 run the row-per-workgroup kernel with 1 / 1 / 1 / 2 / 4 chunks per thread, the last one part
filled except at 8192; 3072 / 3584 / 5120 run the wave-per-row kernel (and, at `ln.wave` = 0 / 2, the workgroup kernel and the
two-rows-per-wave form).  M = 1, 2, 3, 9: odd M, and a second workgroup of the wave kernel with a single live row."""
import functools

import pytest
import torch

from tests import gemm_fp8_probes as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
BLOCK_CS = (128, 256, 1152, 2176, 8192)
WAVE_CS = (3072, 3584, 5120)
MS = (1, 2, 3, 9)
PLANT_COLS = (0, 7, 8, 511, 512, -1)


@functools.lru_cache(maxsize=None)
def _vectors(C):
    """the modulation and affine vectors of width C (CPU): scale, shift, scale2, shift2 float32; gamma, beta bf16"""
    g = torch.Generator().manual_seed(4100 + C)
    f = lambda s: (torch.randn(C, generator=g) * s)  # noqa: E731
    return dict(scale=f(0.3), shift=f(0.2), scale2=f(0.3), shift2=f(0.2), gamma=(1.0 + f(0.2)).to(BF), beta=f(0.1).to(BF))


@functools.lru_cache(maxsize=None)
def _rows(M, C):
    g = torch.Generator().manual_seed(7 * C + M)
    x = torch.randn(M, C, generator=g) * 2.0 + 0.5
    x = x * torch.tensor([30.0 if r % 2 else 0.05 for r in range(M)]).view(-1, 1)      # adjacent rows far apart in size
    return x.to(BF)


def _variants(M):
    v = [("ln scale/shift", dict(scale=1, shift=1)), ("ln plain", dict()), ("affine", dict(gamma=1, beta=1)),
         ("affine + modulation", dict(gamma=1, beta=1, scale=1, shift=1)), ("rms gamma", dict(gamma=1, rms=True))]
    for split in sorted({0, M // 2, M}):
        v.append((f"split {split} of {M}", dict(scale=1, shift=1, scale2=1, shift2=1, split=split)))
    return v


def _kwargs(C, spec):
    vec = _vectors(C)
    kw = {k: vec[k].to(DEV) for k in ("scale", "shift", "scale2", "shift2", "gamma", "beta") if spec.get(k)}
    kw.update(rms=bool(spec.get("rms")), split=int(spec.get("split", 0)), eps=1e-6)
    return kw


def _check(x, kw, what):
    """the fused op on x (device, bf16 or float32) against the two launches and the CPU restatement; strided outputs in guarded
    buffers"""
    from apex_studio_amd import ops
    M, C = x.shape
    ref_out = torch.empty(M, C, dtype=BF, device=DEV)
    ops.ln_modulate(x, out=ref_out, **kw)
    ref_codes, ref_scales = ops.quant_rows_fp8(ref_out)
    cpu_codes, cpu_scales = P.quant_ref(ref_out.cpu())

    # (1) with the bf16 row: codes in a view of a wider byte buffer (ldq > C) with guard rows and columns, out in a guarded view
    cbuf, _ = P.byte_buffer(M + 2, C + 16, DEV)
    codes = cbuf[1:M + 1, 16:16 + C]
    obuf, out = P.sentinel_buffer(M, C, DEV)
    scales = torch.full((M + 2,), -1.0, device=DEV)
    got_codes, got_scales = ops.ln_modulate_quant_fp8(x, codes=codes, scale_out=scales[1:M + 1], out=out, **kw)
    assert got_codes.data_ptr() == codes.data_ptr() and got_scales.data_ptr() == scales[1:M + 1].data_ptr()
    assert torch.equal(codes, ref_codes), f"{what}: codes differ from ln_modulate -> quant_rows_fp8: " + P.mismatches(codes.cpu(), ref_codes.cpu())
    assert torch.equal(scales[1:M + 1], ref_scales), f"{what}: scales {scales[1:M + 1].tolist()} != {ref_scales.tolist()}"
    assert torch.equal(out, ref_out), f"{what}: the bf16 row differs from ln_modulate: " + P.mismatches(out.cpu(), ref_out.cpu())
    assert torch.equal(codes.cpu(), cpu_codes) and torch.equal(scales[1:M + 1].cpu(), cpu_scales), f"{what}: not the documented formula"
    assert P.buffer_mismatches(obuf.cpu(), ref_out.cpu()) == "", f"{what}: a bf16 store left the output view"
    host = cbuf.cpu()
    full = torch.full_like(host, P.SENTINEL_CODE)
    full[1:M + 1, 16:16 + C] = ref_codes.cpu()
    assert torch.equal(host, full), f"{what}: a code store left the output view"
    assert not bool(((codes & 0x7F) == 0x7F).any()), f"{what}: a NaN code"
    assert float(scales[0]) == -1.0 and float(scales[M + 1]) == -1.0, f"{what}: a scale store left its rows"

    # (2) without it: the same codes and scales, and a bf16 buffer that is passed nowhere stays what it was
    bystander = torch.full((M, C), P.SENTINEL, dtype=BF, device=DEV)
    c2, s2 = ops.ln_modulate_quant_fp8(x, out=None, **kw)
    assert torch.equal(c2, ref_codes) and torch.equal(s2, ref_scales), f"{what}: out=None changes the codes or scales"
    assert bool((bystander == P.SENTINEL).all())


@pytest.mark.parametrize("C", BLOCK_CS + WAVE_CS)
def test_fused_norm_quant_equals_the_two_launches(C):
    import apex_studio_amd  # noqa: F401
    for M in MS:
        x = _rows(M, C).to(DEV)
        for name, spec in _variants(M):
            _check(x, _kwargs(C, spec), f"C {C} M {M} {name}")
        # float x (the f32 residual stream): values that are no bf16
        xf = (_rows(M, C).float() * 1.001 + 1e-3).to(DEV)
        _check(xf, _kwargs(C, dict(scale=1, shift=1)), f"C {C} M {M} float x")
        _check(xf, _kwargs(C, dict(gamma=1, beta=1)), f"C {C} M {M} float x affine")


@pytest.mark.parametrize("wave", (0, 2))
def test_fused_norm_quant_follows_the_ln_wave_tune_value(wave):
    """`ln.wave` = 0 sends a wave width to the row-per-workgroup kernel and 2 to two rows per wave: the fused entry runs the twin of
    whatever the norm alone runs, so it equals the two launches under every value"""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    C = 5120
    assert L.apexmi_tune_set(b"ln.wave", wave) == 0
    try:
        for M in MS:
            x = _rows(M, C).to(DEV)
            _check(x, _kwargs(C, dict(scale=1, shift=1)), f"ln.wave {wave} C {C} M {M}")
            _check(x, _kwargs(C, dict(scale=1, shift=1, scale2=1, shift2=1, split=M // 2)), f"ln.wave {wave} C {C} M {M} split")
            _check(x.float(), _kwargs(C, dict(scale=1, shift=1)), f"ln.wave {wave} C {C} M {M} float x")
    finally:
        assert L.apexmi_tune_set(b"ln.wave", 1) == 0


@pytest.mark.parametrize("C", BLOCK_CS + WAVE_CS)
def test_planted_rows_give_the_exact_scale(C):
    """row 0 constant: LayerNorm gives zeros, so with no shift the scale is 1 and every code 0.  Then one row per planted column
    (0, 7, 8, 511, 512, C - 1: the first and last lane and chunk) whose single dominant element decides the scale: scale =
    |y[col]| / 448 exactly and the code there is +-448's; odd rows carry a NEGATIVE maximum."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    cols = sorted({c % C for c in PLANT_COLS if c < C})
    M = 1 + len(cols)
    g = torch.Generator().manual_seed(99 + C)
    x = torch.randn(M, C, generator=g)
    x[0] = 3.0
    for r, c in enumerate(cols, start=1):
        x[r, c] = (-1.0 if r % 2 else 1.0) * 4000.0
    x = x.to(BF).to(DEV)
    vec = _vectors(C)
    # a modulation near one keeps the planted element dominant; no shift, so the constant row stays zero
    kw = dict(scale=(vec["scale"] * 0.1).to(DEV), eps=1e-6)
    ref_out = ops.ln_modulate(x, out=torch.empty(M, C, dtype=BF, device=DEV), **kw)
    codes, scales = ops.ln_modulate_quant_fp8(x, codes=torch.empty(M, C, dtype=torch.uint8, device=DEV),
                                              scale_out=torch.empty(M, device=DEV), **kw)
    y = ref_out.float().cpu()
    codes, scales = codes.cpu(), scales.cpu()
    assert bool((y[0] == 0).all()) and float(scales[0]) == 1.0 and bool((codes[0] & 0x7F == 0).all())
    for r, c in enumerate(cols, start=1):
        assert int(y[r].abs().argmax()) == c and float(y[r, c]) * (-1.0 if r % 2 else 1.0) > 4 * float(y[r].abs().sort().values[-2])
        want = y[r, c].abs() / torch.tensor(448.0)
        assert float(scales[r]) == float(want), (C, r, c, float(scales[r]), float(want))
        assert int(codes[r, c]) == (0xFE if r % 2 else 0x7E), (C, r, c, hex(int(codes[r, c])))
    ref_codes, ref_scales = P.quant_ref(ref_out.cpu())
    assert torch.equal(codes, ref_codes) and torch.equal(scales, ref_scales)


def test_gemm_takes_the_norm_s_codes_and_refuses_them_off_the_fp8_route():
    """`ops.gemm(quantised=)`: on the fp8 route the result is the one with the GEMM's own quantise launch, which is then not made;
    a call that takes neither fp8 route raises instead of dropping the codes"""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib, ops
    M, K, N = 9, 256, 32
    g = torch.Generator().manual_seed(5)
    w = ops.Fp8Weight((torch.randn(N, K, generator=g) * 20).to(torch.float8_e4m3fn).to(DEV), torch.full((N,), 0.01, device=DEV))
    w.compute = "fp8"
    x = _rows(M, K).to(DEV)
    kw = _kwargs(K, dict(scale=1, shift=1))
    xn = ops.ln_modulate(x, out=torch.empty(M, K, dtype=BF, device=DEV), **kw)
    want = ops.gemm(xn, w, epilogue="gelu")
    assert ops.fp8_norm_quant_route(x, xn, w, None, "gelu") == (True, False)
    calls = []
    real = ops.quant_rows_fp8
    ops.quant_rows_fp8 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        q = ops.ln_modulate_quant_fp8(x, **kw)
        never_written = torch.full((M, K), P.SENTINEL, dtype=BF, device=DEV)      # the route reads its shape and dtype only
        got = ops.gemm(never_written, w, epilogue="gelu", quantised=q)
    finally:
        ops.quant_rows_fp8 = real
    assert torch.equal(got, want) and calls == []
    w.compute = "bf16"
    with pytest.raises(lib.ApexMIError, match="fp8_norm_quant_route"):
        ops.gemm(xn, w, quantised=q)
    with pytest.raises(lib.ApexMIError, match="fp8_norm_quant_route"):
        ops.gemm(xn, torch.zeros(N, K, dtype=BF, device=DEV), quantised=q)
