"""Per-element probes of the channels-last VAE passes on the GPU: groupnorm_cl under the a-priori envelope (bit for bit where it
holds one bf16 value), upsample2x_cl, time_interleave_cl, pixel_shuffle_clamp, crossfade_, group_mean and frames_to_u8 with
torch.equal on WHOLE sentinel-filled buffers, tanh_clamp by its properties over every bf16 code point.  Operands, float64
references, envelopes: tests/vae_pass_probes.py; the conditions of the envelope for every case below and what the verdict rejects:
tests/test_vae_pass_probes_host.py.  Entry points whose Python wrapper allocates the output are called through lib.load() with a
larger sentinel-filled buffer (64 guard elements either side).

MEASURED on the MI355X (profiles/vae_pass_probes_measured.jsonl), worst |err| / env over the eight (C, G); bf16 outputs: the least
pre-rounding error consistent with the output:
  family 1 and the constant images (exact statistics)   bf16 out 0.627   f32 out 0.998   (the KNOWN rounding of the mean to f32 is
                                                                                         the whole envelope where d is small: attained)
  plain 3 N + 0.5                                       bf16 out 0.078   f32 out 0.319
  2^-10 N                                               bf16 out 0.051   f32 out 0.363
  offset (128 + 4 k | 64 + 0.125 N)                     bf16 out 0.138   f32 out 0.370
  groups (means -6 .. 6, spreads 0.25 .. 1.75)          bf16 out 0.062   f32 out 0.374
  tanh_clamp, bf16: every output of every finite code point equals bf16(ref64); f32: worst 2.23 (inv_scale 1) and 2.40
  (1 / 1.03682) f32 ulps against float64.  The two bars below are those figures plus one unit, as SILU_ULP_BAR was set.

Found by these probes: groupnorm_cl summed x and x^2 in f32 (chains of up to 260 terms) and formed E[x^2] - mean^2 from those sums.
On the MI355X that kernel failed 57 of the cases above, all of family 2 and the clamp's image, none of family 1:
  f32 offset image, 24 of 24 cases, 9 to 3672 envelopes out, rel-L2 up to 3.6e-2 (C32.G32.P61.offset.f32.silu, element (46, 19): got
    -0.273858, reference -0.278274);
  f32 groups image, 23 of 24, up to 37 envelopes (C32.G32.P61.groups.f32.lin, element (1, 16): -3.282912 for -3.283530), rel-L2 4e-5:
    invisible to the older bar; bf16 groups image, 2 cases, one flipped rounding each (C128.G32.P1025.groups.bf16.lin, element
    (1000, 121): 2.5625 for 2.5547);
  the constant 99999.9 image, 8 of 8: the f32 mean was off by up to 0.17, so the output was -171.9 where it is beta = -0.03125
    (C256.G32.P1025.bigconst.f32.lin, element (0, 11)).
The sums are float64 now (csrc/conv.hip, gn_partial_kernel)."""
import functools

import numpy as np
import pytest
import torch

from tests import vae_pass_probes as V
from tests.conftest import measured
from tests.vae_pass_probes import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
TANH_F32_ULP_BAR = 3.4              # measured 2.40 f32 ulps (inv_scale 1 / 1.03682) + 1
TANH_BF16_OFF_BAR = 1               # measured 0 outputs off bf16(ref64) + 1


def _ops():
    from apex_studio_amd import ops
    return ops


def _lib():
    from apex_studio_amd import lib
    return lib


def _same(got, want, what):
    msg = V.mismatches(got, want)
    assert not msg, f"{what}: {msg}"


def _entry(name, f32):
    return getattr(_lib().load(), name + ("_f32" if f32 else ""))


def _guarded_call(call, n_out, dtype, fill=V.SENTINEL):
    """runs call(pointer to n_out elements inside a sentinel-filled buffer) -> the whole buffer on the host"""
    buf = V.guarded(n_out, dtype, fill, GUARD).to(DEV)
    _lib().check(call(buf[GUARD:].data_ptr()), "probe call")
    torch.cuda.synchronize()
    return buf.cpu()


# ------------------------------------------------------------------------------------------------------------- A. GroupNorm
@functools.lru_cache(maxsize=None)
def _affine_dev(C):
    return tuple(t.to(DEV) for t in V.gn_affine(C))


def _gn_run(case):
    """the case on the device: the output rows on the host; one guard row above and below and x itself are checked"""
    x64 = V.case_image(case)
    P, C = x64.shape
    x = x64.to(case.dtype).to(DEV)
    gamma, beta = _affine_dev(C)
    obuf = torch.full((P + 2, C), V.SENTINEL, dtype=case.dtype, device=DEV)
    out = obuf[1:P + 1]
    got = _ops().groupnorm_cl(x, gamma, beta, groups=case.G, eps=V.EPS, silu=case.silu, out=out)
    assert got.data_ptr() == out.data_ptr()
    whole = obuf.cpu()
    guard = torch.full((C,), V.SENTINEL, dtype=case.dtype)
    assert torch.equal(whole[0], guard) and torch.equal(whole[P + 1], guard), f"{case.id}: store outside the output rows"
    assert torch.equal(x.cpu(), x64.to(case.dtype)), f"{case.id}: x changed"
    return whole[1:P + 1]


@pytest.mark.parametrize("cg", V.GN_CG, ids=lambda cg: f"C{cg[0]}G{cg[1]}")
def test_groupnorm_cl_under_the_envelope(cg):
    worst = {}
    for case in V.gn_cases(*cg):
        rows = _gn_run(case)
        ref, env = V.gn_case_ref(case)
        v = V.verdict(rows, ref, env)
        assert v.passed, f"{case.id}: {V.describe(v, rows, ref, env)}"
        key = ("family1" if case.image in V.EXACT_IMAGES else case.image) + (".f32" if case.f32 else ".bf16")
        worst[key] = max(worst.get(key, 0.0), v.ratio)
    for key, r in sorted(worst.items()):
        print(f"[margin] groupnorm_cl C{cg[0]} G{cg[1]} {key}: |err| / env = {r:.3f}")
        measured(f"groupnorm_cl.C{cg[0]}.G{cg[1]}.{key}.err_over_env", r, 1.0 + 1e-9)      # <= 1 is the verdict itself


def test_groupnorm_cl_is_run_to_run_bit_identical():
    for case in (V.GnCase(128, 32, V.FOUR_BLOCKS, "groups", False, True), V.GnCase(512, 32, V.FOUR_BLOCKS, "offset", True, False)):
        a = _gn_run(case)
        for _ in range(2):
            assert torch.equal(_gn_run(case), a), case.id


def test_norm_operators_refuse_wrong_affine_operands():
    """refused in Python before any launch: a float beta (it would be read as bf16), a short gamma or beta (read past its end),
    an operand on the host; rmsnorm_cl's float gamma"""
    ops, lib = _ops(), _lib()
    x = torch.zeros(4, 64, dtype=BF, device=DEV)
    g, b = torch.ones(64, dtype=BF, device=DEV), torch.zeros(64, dtype=BF, device=DEV)
    with pytest.raises(lib.ApexMIError, match="beta"):
        ops.groupnorm_cl(x, g, b.float())
    with pytest.raises(lib.ApexMIError, match="gamma"):
        ops.groupnorm_cl(x, g.float(), b)
    with pytest.raises(lib.ApexMIError, match="gamma"):
        ops.groupnorm_cl(x, g[:32], b)
    with pytest.raises(lib.ApexMIError, match="beta"):
        ops.groupnorm_cl(x, g, b[:56])
    with pytest.raises(lib.ApexMIError, match="beta"):
        ops.groupnorm_cl(x, g, b.cpu())
    with pytest.raises(lib.ApexMIError, match="gamma"):
        ops.groupnorm_cl(x, g.cpu(), b)
    with pytest.raises(lib.ApexMIError, match="gamma"):
        ops.rmsnorm_cl(x, g.float())


def test_flux_vae_decode_of_a_batch_equals_the_single_decodes():
    """every leading dimension of groupnorm_cl's operand is a position of ONE sample: the decoder normalises sample by sample"""
    from apex_studio_amd.vae_flux import AutoencoderKL
    from oracle.vae_flux import AutoencoderKLDecoder
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    cfg = dict(latent_channels=16, block_out_channels=(32, 64, 128, 128), layers_per_block=1)
    sd = vae_synthetic_state_dict(AutoencoderKLDecoder(**cfg).eval(), 19)
    vae = AutoencoderKL(**cfg, device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in sd.items()}, strict=True)
    z = seeded((2, 16, 12, 10), 64).to(BF).to(DEV)
    z[1] = z[1] * 0.5 + 0.25                     # different statistics in the two samples
    both = vae.decode(z, return_dict=False)[0]
    assert both.shape == (2, 3, 96, 80)
    for i in range(2):
        assert torch.equal(both[i:i + 1], vae.decode(z[i:i + 1], return_dict=False)[0]), i
    assert not torch.equal(both[0], both[1])


# -------------------------------------------------------------------------------------------------------- B. the exact passes
@pytest.mark.parametrize("T,H,W,C", V.UPSAMPLE_CASES)
def test_upsample2x_cl_whole_buffer(T, H, W, C):
    x64 = V.grid4(T, H, W, C)
    x = V.store(x64, BF).to(DEV)
    fn = _lib().load().apexmi_upsample2x_cl
    want = V.store(V.upsample_ref(x64), BF)
    whole = _guarded_call(lambda y: fn(x.data_ptr(), y, T, H, W, C, _ops()._stream()), want.numel(), BF)
    _same(whole, V.expect_guarded(want, BF, guard=GUARD), f"upsample2x_cl {(T, H, W, C)}")
    assert torch.equal(_ops().upsample2x_cl(x).cpu(), want)


@pytest.mark.parametrize("T,H,W,C2,f32", V.INTERLEAVE_CASES)
def test_time_interleave_cl_whole_buffer(T, H, W, C2, f32):
    dt = F32 if f32 else BF
    x64 = V.grid4(T, H, W, C2, salt=2)
    x = V.store(x64, dt).to(DEV)
    fn = _entry("apexmi_time_interleave_cl", f32)
    want = V.store(V.interleave_ref(x64), dt)
    whole = _guarded_call(lambda y: fn(x.data_ptr(), y, T, H * W, C2 // 2, _ops()._stream()), want.numel(), dt)
    _same(whole, V.expect_guarded(want, dt, guard=GUARD), f"time_interleave_cl {(T, H, W, C2, f32)}")
    assert torch.equal(_ops().time_interleave_cl(x).cpu(), want)


@pytest.mark.parametrize("T,H,W,C,r,extra,t0,f32", V.SHUFFLE_CASES)
def test_pixel_shuffle_clamp_whole_buffer(T, H, W, C, r, extra, t0, f32):
    dt = F32 if f32 else BF
    x64 = V.shuffle_operand(T, H, W, C, r, extra, f32)
    x = V.store(x64, dt).to(DEV)
    Cs = x.shape[-1]
    fn = _entry("apexmi_pixel_shuffle_clamp", f32)
    want = V.store(V.shuffle_ref(x64, C, r, t0), dt)
    whole = _guarded_call(lambda y: fn(x.data_ptr(), y, T, H, W, Cs, C, r, t0, V.LO, V.HI, _ops()._stream()), want.numel(), dt)
    _same(whole, V.expect_guarded(want, dt, guard=GUARD), f"pixel_shuffle_clamp {(T, H, W, C, r, extra, t0, f32)}")
    assert torch.equal(_ops().pixel_shuffle_clamp(x, C, r, trim=t0, lo=V.LO, hi=V.HI).cpu(), want)
    assert torch.equal(x.cpu(), V.store(x64, dt))


def test_pixel_shuffle_clamp_refusals_stay():
    x = torch.zeros(2, 3, 5, 8, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        _ops().pixel_shuffle_clamp(x, 3, 3)                      # r = 3 (Cs = 8 < 27 as well)
    with pytest.raises(RuntimeError):
        _ops().pixel_shuffle_clamp(torch.zeros(2, 3, 5, 32, dtype=BF, device=DEV), 3, 3)      # r = 3 alone
    with pytest.raises(RuntimeError):
        _ops().pixel_shuffle_clamp(x, 3, 2)                      # Cs = 8 < C r^2 = 12


@pytest.mark.parametrize("E,dim,f32", V.CROSSFADE_CASES)
def test_crossfade_whole_tensors(E, dim, f32):
    dt = F32 if f32 else BF
    a64, b64 = V.crossfade_operands(E, dim)
    a_full, b_full = V.store(a64, dt).to(DEV), V.store(b64, dt).to(DEV)
    n = a_full.shape[dim]
    got = _ops().crossfade_(a_full.narrow(dim, n - E, E), b_full.narrow(dim, 0, E), dim=dim)
    assert got.data_ptr() == b_full.narrow(dim, 0, E).data_ptr()
    ref, env = V.crossfade_ref(a64, b64, E, dim)
    out = b_full.cpu()
    assert torch.equal(a_full.cpu(), V.store(a64, dt)), "a changed"
    if E in (4, 8):
        _same(out, V.store(ref, dt), f"crossfade E = {E} dim = {dim} f32 = {f32}")
    else:
        v = V.verdict(out, ref, env)
        assert v.passed, f"crossfade E = {E} dim = {dim} f32 = {f32}: {V.describe(v, out, ref, env)}"
        rest = torch.ones_like(out, dtype=torch.bool)
        rest.narrow(dim, 0, E).fill_(False)
        assert torch.equal(out[rest], V.store(b64, dt)[rest]), "b changed outside the band"


@pytest.mark.parametrize("gs,C,f32", V.GROUP_MEAN_CASES)
def test_group_mean_whole_buffer(gs, C, f32):
    dt = F32 if f32 else BF
    x64 = V.grid4(*V.GROUP_MEAN_POS, C * gs, salt=gs)
    x = V.store(x64, dt).to(DEV)
    P = x64.numel() // (C * gs)
    fn = getattr(_lib().load(), "apexmi_group_mean_f32" if f32 else "apexmi_group_mean_bf16")
    want = V.group_mean_ref(x64, C, gs, dt)
    whole = _guarded_call(lambda y: fn(x.data_ptr(), y, P, C, gs, _ops()._stream()), want.numel(), dt)
    _same(whole, V.expect_guarded(want, dt, guard=GUARD), f"group_mean gs = {gs} C = {C} f32 = {f32}")
    assert torch.equal(_ops().group_mean(x, C).cpu(), want)


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("f32", (False, True), ids=("bf16", "f32"))
def test_frames_to_u8_every_code_point_whole_buffer(C, f32):
    from oracle.postprocess import video_to_uint8_frames
    tile = V.u8_video(C, f32).to(DEV)
    view = tile[..., :C].permute(3, 0, 1, 2)
    T, H, W = V.U8_SHAPE
    want = torch.from_numpy(video_to_uint8_frames(view.cpu()[None])[0])
    assert want.shape == (T, H, W, C) and want.dtype == torch.uint8
    fn = _entry("apexmi_frames_to_u8", f32)
    whole = _guarded_call(lambda y: fn(view.data_ptr(), view.stride(0), view.stride(1), view.stride(2), view.stride(3), C, T, H, W,
                                       y, _ops()._stream()), want.numel(), torch.uint8, fill=165)
    exp = V.expect_guarded(want, torch.uint8, fill=165, guard=GUARD)
    assert torch.equal(whole, exp), f"{int((whole != exp).sum())} bytes differ"
    assert np.array_equal(_ops().frames_to_u8(view).cpu().numpy(), want.numpy())


@pytest.mark.parametrize("inv", (1.0, 1.0 / 1.03682), ids=("inv1", "inv1.03682"))
@pytest.mark.parametrize("f32", (False, True), ids=("bf16", "f32"))
def test_tanh_clamp_properties_over_every_code_point(inv, f32):
    dt = F32 if f32 else BF
    fin = V.finite_bf16_codes()
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1.0, -1.0, 2.0], dtype=BF)
    x = torch.cat([fin, special]).to(dt)
    fn = _entry("apexmi_tanh_clamp", f32)
    xd = x.to(DEV)
    whole = _guarded_call(lambda y: fn(xd.data_ptr(), y, x.numel(), float(inv), _ops()._stream()), x.numel(), dt)
    sent = torch.full((GUARD,), V.SENTINEL, dtype=dt)
    assert torch.equal(whole[:GUARD], sent) and torch.equal(whole[GUARD + x.numel():], sent), "store outside the output"
    y = whole[GUARD:GUARD + x.numel()]
    yf, ys = y[:fin.numel()], y[fin.numel():]
    assert float(ys[0]) == 3.0 and float(ys[1]) == -3.0 and bool(torch.isnan(ys[2])), ys[:3]
    why = V.tanh_properties(x[:fin.numel()], yf)
    assert why is None, why
    ref = V.tanh_ref64(fin, inv)
    name = f"tanh_clamp.{'f32' if f32 else 'bf16'}.inv{inv:.5f}"
    if f32:
        ulp = torch.ldexp(torch.ones_like(ref), torch.frexp(ref.abs().clamp_min(2.0 ** -126))[1] - 24)
        err = float(((yf.double() - ref).abs() / ulp).max())
        print(f"[measured] {name}: worst error {err:.2f} f32 ulps against float64")
        measured(name + ".worst_f32_ulps", err, TANH_F32_ULP_BAR)
        assert V.ulp_distance(yf.to(BF), ref) <= 1
    else:
        assert V.ulp_distance(yf, ref) <= 1
        off = int((yf != V.store(ref, BF)).sum())
        print(f"[measured] {name}: {1 - off / yf.numel():.6f} of the outputs equal bf16(ref64)")
        measured(name + ".outputs_not_equal_bf16_ref64", off, TANH_BF16_OFF_BAR + 1)      # off <= TANH_BF16_OFF_BAR
