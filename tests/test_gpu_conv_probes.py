"""Exact integer probes of every convolution tile family, padding mode and edge (operands and references: tests/conv_probes.py).
Every output element of every kernel must equal the integer reference bit for bit: torch.equal, no bar, no fraction allowed to
differ.  Each case asserts, through ops.conv3d_cl_family, the tile family it means to test: a shape that falls under a dispatch
threshold would silently test the 128x128 kernel again.  (What the comparison rejects: tests/test_conv_probes_host.py.)"""
import contextlib
import functools

import pytest
import torch

from tests import conv_probes as P
from tests.conftest import measured
from tests.conv_probes import BF, Mode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = {"conv.v2": 1, "conv.slab": 2, "conv.pp": 1, "conv.torder": 1}
K133, K233, K333 = (1, 3, 3), (2, 3, 3), (3, 3, 3)
# fused RMS norm + SiLU against the float64 reference, in bf16 code points.  Measured on the MI355X: 1 on every shape below
# (profiles/conv_probes_measured.jsonl); the bar is that plus 1 code point of margin for other seeds.
SILU_ULP_BAR = 2


@contextlib.contextmanager
def tuned(**kv):
    from apex_studio_amd import lib
    try:
        for key, v in kv.items():
            lib.tune_set("conv." + key, v)
        yield
    finally:
        for key, v in DEFAULTS.items():
            lib.tune_set(key, v)


def _family(x, wp, k, mode, norm=False):
    from apex_studio_amd import ops
    return ops.conv3d_cl_family(tuple(x.shape), tuple(wp.shape), k, replicate=mode.replicate, independent_frames=mode.independent,
                                upsample2x=mode.up, norm=norm, clip_frames=mode.clip, stride=mode.stride,
                                pad=mode.pad or (-1, -1), out_hw=mode.out_hw or (0, 0), tstride=mode.tstride or (1, 0, 0))


def _exact(got, want, what):
    torch.cuda.synchronize()
    msg = P.mismatches(got.float().cpu(), want.float())
    assert not msg, f"{what}: {msg}"


class Case:
    """operands of one probe on the device, its exact reference on the host"""

    def __init__(self, x, w, k, mode, bias, res, ref, dt=BF):
        from apex_studio_amd import ops
        self.k, self.mode, self.ref = k, mode, ref
        self.x = x.to(dt).to(DEV)
        self.wp = ops.pack_conv_weight(w.to(BF).to(DEV))
        c4 = self.wp.shape[0]
        self.bias = None if bias is None else P.pad_channels(bias, c4).to(BF).to(DEV)
        self.res = None if res is None else P.pad_channels(res, c4).to(dt).to(DEV)

    def family(self, norm=False):
        return _family(self.x, self.wp, self.k, self.mode, norm)

    def run(self, slope=False):
        from apex_studio_amd import ops
        m, k = self.mode, self.k
        if slope is not False:
            return ops.conv3d_cl_act(self.x, self.wp, self.bias, k, residual=self.res, slope=slope, upsample2x=m.up,
                                     independent_frames=m.independent)
        if m.tstride is not None:
            return ops.conv3d_cl_tstrided(self.x, self.wp, self.bias, k, *m.tstride)
        if m.stride != (1, 1):
            assert m.stride[0] == m.stride[1] and m.pad[0] == m.pad[1]
            return ops.conv2d_cl_strided(self.x, self.wp, self.bias, stride=m.stride[0], pad=m.pad[0])
        return ops.conv3d_cl(self.x, self.wp, self.bias, k, residual=self.res, replicate=m.replicate,
                             independent_frames=m.independent, upsample2x=m.up, clip_frames=m.clip)


def selector_host(T, H, W, cin, cout, k, mode=Mode(), extras=True):
    """selector weights over the formula input, with (extras) or without bias and residual (the strided entry points take no
    residual): (x, dense w, bias, residual, exact reference)"""
    x = P.int_input(T, H, W, cin)
    ci, coef = P.selector(cout, cin, k)
    To, Ho, Wo, _ = P.tap_sources(T, H, W, k, mode)
    bias = P.int_bias(cout) if extras else None
    res = P.int_residual(To, Ho, Wo, cout) if extras and mode.stride == (1, 1) and mode.tstride is None else None
    ref = P.check_bf16_exact(P.conv_ref(x, (ci, coef), k, mode, bias, res))
    return x, P.selector_dense(ci, coef, cin, k), bias, res, ref


@functools.lru_cache(maxsize=None)
def selector_case(T, H, W, cin, cout, k, mode=Mode(), extras=True):
    """the reference is computed once and shared by every test of the shape"""
    x, w, bias, res, ref = selector_host(T, H, W, cin, cout, k, mode, extras)
    return Case(x, w, k, mode, bias, res, ref)


@functools.lru_cache(maxsize=None)
def dense_case(name):
    T, H, W, cin, cout, k, mk, seed = P.DENSE_CASES[name]
    x, w, bias, res, ref = P.dense_case(name)
    return Case(x, w, k, Mode(**mk), bias, res, ref)


# ------------------------------------------------------------------------------------------------- 128x128 implicit GEMM
GEMM128 = [   # T, H, W, cin, cout, k, mode: odd H, W; M = T * 561 is no multiple of 128; T = 1 takes the single-frame tap skip
    (2, 33, 17, 16, 3, (1, 1, 1), {}),
    (3, 33, 17, 16, 16, (3, 1, 1), {}),
    (1, 33, 17, 96, 96, K133, {}),
    (2, 33, 17, 96, 160, K333, {}),
    (1, 33, 17, 128, 384, K333, {}),
    (3, 33, 17, 128, 16, K233, {}),
    (2, 33, 17, 16, 3, K333, {"replicate": True}),
    (3, 33, 17, 128, 96, K333, {"replicate": True}),
    (1, 33, 17, 96, 160, K333, {"replicate": True}),
    (3, 33, 17, 96, 16, K333, {"independent": True}),
    (2, 17, 9, 96, 16, K333, {"up": True}),
    (3, 17, 9, 16, 3, K133, {"up": True, "independent": True}),
]


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk", GEMM128)
def test_gemm128_selector(T, H, W, cin, cout, k, mk):
    for extras in (True, False):
        c = selector_case(T, H, W, cin, cout, k, Mode(**mk), extras)
        assert c.family() == ("128x128", 0)
        _exact(c.run(), c.ref, f"128x128 {T}x{H}x{W} {cin}->{cout} k={k} {mk} extras={extras}")
    assert c.ref.shape[-1] == c.wp.shape[0] and not c.ref[..., cout:].any()      # padded channels: exact zeros expected


@pytest.mark.parametrize("name", ["gemm128.3x3x3", "gemm128.repl", "gemm128.up"])
def test_gemm128_dense(name):
    c = dense_case(name)
    assert c.family() == ("128x128", 0)
    _exact(c.run(), c.ref, name)


def test_gemm128_on_a_large_shape_with_the_other_families_off():
    c = selector_case(3, 131, 173, 96, 96, K333)
    with tuned(v2=0, slab=0):
        assert c.family() == ("128x128", 0)
        _exact(c.run(), c.ref, "128x128 3x131x173 96->96")


# ------------------------------------------------------------------------------------------------------ conv-shaped v2 tiles
V2 = [   # one shape per N extent (M = 66013 / 66246 / 66528 >= 65536; 251 = 15 * 16 + 11, 263 = 8 * 32 + 7)
    (1, 251, 263, 48, 24, K133, {}, 32),
    (2, 181, 183, 16, 48, K333, {}, 64),
    (1, 251, 263, 48, 96, K133, {}, 96),
    (1, 251, 263, 16, 640, K133, {}, 128),
    (1, 251, 263, 48, 192, K133, {}, 192),
    (1, 251, 263, 16, 256, K133, {}, 256),
    (1, 251, 263, 144, 160, K133, {}, 192),            # masked columns: 160 of the 192
    (1, 126, 132, 48, 96, K133, {"up": True}, 96),
    (1, 251, 263, 48, 192, K133, {"replicate": True}, 192),
    (1, 251, 263, 48, 96, K333, {"replicate": True}, 96),   # T = 1 under replicate: the earlier temporal taps read frame 0
]


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk,bn", V2)
def test_v2_tiles_selector(T, H, W, cin, cout, k, mk, bn):
    c = selector_case(T, H, W, cin, cout, k, Mode(**mk))
    with tuned(slab=0):
        assert c.family() == ("v2", bn)
        y = c.run()
        _exact(y, c.ref, f"v2 N={bn} {T}x{H}x{W} {cin}->{cout} k={k} {mk}")
        assert torch.equal(c.run(), y)


def test_v2_tiles_dense():
    c = dense_case("v2.n192")
    with tuned(slab=0):
        assert c.family() == ("v2", 192)
        _exact(c.run(), c.ref, "v2.n192")


# ------------------------------------------------------------------------------------------------------------- slab kernels
SLAB48 = [   # 48-channel slices; pp values that select another kernel for the shape
    (1, 251, 263, 48, 32, K133, {}, (0, 1, 2)),          # nt = 1, kT = 1
    (1, 251, 263, 96, 64, K133, {}, (0, 1, 2)),          # nt = 2
    (3, 131, 173, 96, 96, K333, {}, (0, 1, 2, 3)),       # nt = 3, kT = 3
    (1, 251, 263, 96, 192, K133, {}, (0, 1, 2, 3)),
    (2, 67, 250, 48, 384, K233, {}, (0, 1, 2, 3)),       # two N groups, kT = 2, 288 workgroups under 65536 positions
    (3, 131, 173, 96, 96, K333, {"independent": True}, (0, 1, 2, 3)),
    (1, 126, 132, 48, 96, K133, {"up": True}, (0, 1, 2, 3)),
]
SLAB64 = [   # 64-channel slices (pp = 3 has no kernel of its own here)
    (4, 67, 250, 128, 128, K333, {}, (0, 1, 2)),
    (4, 67, 250, 256, 128, K333, {"replicate": True}, (0, 1, 2)),
    (1, 27, 250, 512, 1024, K333, {}, (0, 1, 2)),        # 256 workgroups of 8 N groups; T = 1: tap skip
]


def _slab_sweep(c, family, pps, what):
    first = None
    for pp in pps:
        for torder in (1, 0):
            with tuned(pp=pp, torder=torder):
                assert c.family() == (family, 0)
                y = c.run()
                _exact(y, c.ref, f"{what} pp={pp} torder={torder}")
                if first is None:
                    first = y          # pp 1, torder 1 = the shipped default
    with tuned():
        assert torch.equal(c.run(), first)       # a second call returns the same bits


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk,pps", SLAB48)
def test_slab48_selector(T, H, W, cin, cout, k, mk, pps):
    c = selector_case(T, H, W, cin, cout, k, Mode(**mk))
    _slab_sweep(c, "slab48", (1,) + tuple(p for p in pps if p != 1), f"slab48 {T}x{H}x{W} {cin}->{cout} k={k} {mk}")


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk,pps", SLAB64)
def test_slab64_selector(T, H, W, cin, cout, k, mk, pps):
    c = selector_case(T, H, W, cin, cout, k, Mode(**mk))
    _slab_sweep(c, "slab64", (1,) + tuple(p for p in pps if p != 1), f"slab64 {T}x{H}x{W} {cin}->{cout} k={k} {mk}")


@pytest.mark.parametrize("name,family", [("slab48.nt3", "slab48"), ("slab48.192", "slab48"), ("slab64.128", "slab64")])
def test_slab_dense(name, family):
    _slab_sweep(dense_case(name), family, (1, 0, 2), name)


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk", [(1, 251, 263, 96, 64, K133, {}), (3, 131, 173, 96, 96, K333, {}),
                                                  (3, 131, 173, 96, 96, K333, {"independent": True})])
def test_slab96_order_preserving_form(T, H, W, cin, cout, k, mk):
    c = selector_case(T, H, W, cin, cout, k, Mode(**mk))
    with tuned(slab=1):
        assert c.family() == ("slab96", 0)
        _exact(c.run(), c.ref, f"slab96 {T}x{H}x{W} {cin}->{cout} {mk}")
    d = dense_case("slab48.nt3")
    with tuned(slab=1):
        assert d.family() == ("slab96", 0)
        _exact(d.run(), d.ref, "slab96 dense")


# ---------------------------------------------------------------------------------------------------------------- fused norm
def _norm_check(got, raw_ref, gamma, silu, name):
    torch.cuda.synchronize()
    d = P.ulp_distance(got.cpu(), P.rmsnorm_ref(raw_ref, gamma, silu))
    if silu:
        measured(name, d, SILU_ULP_BAR + 1)      # d <= SILU_ULP_BAR
    else:
        # the f32 sum of squares and scale carry ~1e-6 relative error, far below 2^-9: only a tie of the final rounding moves
        assert d <= 1, f"{name}: {d} bf16 code points from the float64 RMS norm"


@pytest.mark.parametrize("T,H,W,cin,cout,k,mk,slab,family", [
    (1, 251, 263, 48, 96, K133, {}, 0, ("v2", 96)),
    (1, 251, 263, 48, 192, K133, {}, 0, ("v2", 192)),
    (1, 126, 132, 48, 96, K133, {"up": True}, 0, ("v2", 96)),
    (3, 131, 173, 96, 96, K333, {}, 2, ("slab48", 0)),
    (1, 251, 263, 96, 192, K133, {}, 2, ("slab48", 0)),
    (3, 131, 173, 96, 96, K333, {}, 1, ("slab96", 0)),
])
def test_fused_norm_raw_exact_and_normed_within_one_step(T, H, W, cin, cout, k, mk, slab, family):
    from apex_studio_amd import ops
    c = selector_case(T, H, W, cin, cout, k, Mode(**mk))
    gamma = P.gamma_of(cout)
    g = gamma.to(BF).to(DEV)
    for pp in ((1,) if slab != 2 else (1, 0, 2)):
        for silu in (False, True):
            with tuned(slab=slab, pp=pp):
                assert ops.conv3d_cl_norm_fusable(c.x, cout, c.mode.up) and c.family(norm=True) == family
                y, yn = ops.conv3d_cl_norm(c.x, c.wp, c.bias, k, g, silu=silu, residual=c.res, upsample2x=c.mode.up,
                                           independent_frames=c.mode.independent)
            what = f"conv_norm.{family[0]}{family[1] or ''}.{cin}x{cout}.pp{pp}" + (".up" if c.mode.up else "") + (".silu" if silu else "")
            _exact(y, c.ref, what + " raw")
            _norm_check(yn, c.ref, gamma, silu, what)


@pytest.mark.parametrize("C", [96, 192, 384, 1024])
def test_rmsnorm_cl_on_integer_rows(C):
    """the three lane widths (16, 32, 64 lanes per position) and the wide kernel, alone, under the same comparison"""
    from apex_studio_amd import ops
    raw = P.int_residual(3, 37, 21, C) * 9 + P.int_input(3, 37, 21, C)          # integers in [-148, 148], exact in bf16
    raw[1, 5, 7] = 0                                                              # an all-zero position
    gamma = P.gamma_of(C)
    x, g = raw.to(BF).to(DEV), gamma.to(BF).to(DEV)
    assert torch.equal(x.float().cpu(), raw)
    for silu in (False, True):
        _norm_check(ops.rmsnorm_cl(x, g, silu=silu), raw, gamma, silu, f"rmsnorm_cl.{C}" + (".silu" if silu else ""))


# ------------------------------------------------------------------------------------------------------------- stacked clips
@pytest.mark.parametrize("replicate", [False, True])
@pytest.mark.parametrize("k", [K333, (3, 1, 1)])
@pytest.mark.parametrize("clip", [1, 2, 3])
def test_stacked_clips(clip, k, replicate):
    """T / clip clips, each causal on its own: the first frames of a clip must not read the previous clip (consecutive frames of
    the formula input differ everywhere, so a leak changes the result)"""
    from apex_studio_amd import ops
    T, H, W, cin, cout = 6, 19, 13, 16, 16
    c = selector_case(T, H, W, cin, cout, k, Mode(replicate=replicate, clip=clip))
    assert not torch.equal(c.ref, selector_case(T, H, W, cin, cout, k, Mode(replicate=replicate)).ref)
    assert c.family() == ("128x128", 0)
    y = c.run()
    _exact(y, c.ref, f"clips of {clip} k={k} replicate={replicate}")
    per_clip = torch.cat([ops.conv3d_cl(c.x[i:i + clip].contiguous(), c.wp, c.bias, k, residual=c.res[i:i + clip].contiguous(),
                                        replicate=replicate) for i in range(0, T, clip)])
    assert torch.equal(y, per_clip)


def test_stacked_clips_on_a_slab_sized_shape_stay_on_the_128x128_kernel():
    c = selector_case(6, 67, 173, 96, 96, K333, Mode(clip=3))
    assert _family(c.x, c.wp, K333, Mode()) == ("slab48", 0) and c.family() == ("128x128", 0)
    _exact(c.run(), c.ref, "clips of 3, 6x67x173 96->96")


# -------------------------------------------------------------------------------------------------------------------- strides
@pytest.mark.parametrize("H,W", [(34, 18), (33, 17)])
def test_conv2d_down2(H, W):
    """ZeroPad2d((0, 1, 0, 1)) + 3x3 stride 2: the last output row / column of an even image reads the zero line"""
    from apex_studio_amd import ops
    Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
    for cin, cout in ((16, 16), (96, 160)):
        c = selector_case(2, H, W, cin, cout, K133, Mode(stride=(2, 2), pad=(0, 0), out_hw=(Ho, Wo)))
        assert c.family() == ("128x128", 0)
        _exact(ops.conv2d_cl_down2(c.x, c.wp, c.bias), c.ref, f"down2 {H}x{W} {cin}->{cout}")


@pytest.mark.parametrize("pad", [1, 0])
@pytest.mark.parametrize("H,W", [(34, 18), (33, 17)])
def test_conv2d_strided(H, W, pad):
    Ho, Wo = (H + 2 * pad - 3) // 2 + 1, (W + 2 * pad - 3) // 2 + 1
    for cin, cout in ((16, 16), (96, 160)):
        c = selector_case(2, H, W, cin, cout, K133, Mode(stride=(2, 2), pad=(pad, pad), out_hw=(Ho, Wo)))
        assert c.family() == ("128x128", 0)
        _exact(c.run(), c.ref, f"strided(2, {pad}) {H}x{W} {cin}->{cout}")


@pytest.mark.parametrize("k", [(3, 1, 1), K333])
@pytest.mark.parametrize("st,t0,To", [(2, 2, 3), (2, 1, 3)])
def test_temporal_stride(st, t0, To, k):
    c = selector_case(7, 33, 17, 16, 16, k, Mode(tstride=(st, t0, To)))
    assert c.family() == ("128x128", 0)
    _exact(c.run(), c.ref, f"tstrided({st}, {t0}, {To}) k={k}")


# ----------------------------------------------------------------------------------------------------------------- activation
@pytest.mark.parametrize("T,H,W,cin,cout,k,mk,family", [
    (2, 33, 17, 16, 16, K333, {}, "128x128"),
    (3, 33, 17, 96, 160, K233, {}, "128x128"),             # MemBlock's kT = 2
    (2, 17, 9, 96, 16, K333, {"up": True}, "128x128"),
    (3, 33, 17, 96, 16, K333, {"independent": True}, "128x128"),
    (3, 131, 173, 96, 96, K333, {}, "slab48"),
    (4, 67, 250, 128, 128, K333, {}, "slab64"),
])
def test_leaky_relu_epilogue(T, H, W, cin, cout, k, mk, family):
    for extras in (True, False):
        c = selector_case(T, H, W, cin, cout, k, Mode(**mk), extras)
        assert c.family()[0] == family
        for slope in (None, 0.5, 0.25):
            # slope a power of two: slope * y is exact in f32, the kernel's ONE bf16 rounding is the reference's
            _exact(c.run(slope=slope), P.leaky(c.ref, slope), f"act slope={slope} {T}x{H}x{W} {cin}->{cout} {mk} extras={extras}")


# ------------------------------------------------------------------------------------------------------------ f32-storage form
@functools.lru_cache(maxsize=None)
def f32_case(T, H, W, cin, cout, k, mode):
    """float activations holding integers: the three-way bf16 split is exact (mid and lo parts zero); the float output has no
    256 limit: dense integer weights in [-2, 2], sums in the thousands"""
    x, w = P.int_input(T, H, W, cin), P.int_weight(cout, cin, k)
    To, Ho, Wo, _ = P.tap_sources(T, H, W, k, mode)
    bias = P.int_bias(cout)
    res = P.int_residual(To, Ho, Wo, cout) * 64 if mode.stride == (1, 1) and mode.tstride is None else None
    return Case(x, w, k, mode, bias, res, P.conv_ref(x, w, k, mode, bias, res), dt=torch.float32)


@pytest.mark.parametrize("k,mk", [
    (K333, {}), (K333, {"replicate": True}), (K333, {"up": True}), (K333, {"independent": True}),
    (K133, {"stride": (2, 2), "pad": (1, 1), "out_hw": (17, 9)}), (K133, {"stride": (2, 2), "pad": (0, 0), "out_hw": (16, 8)}),
    ((3, 1, 1), {"tstride": (2, 2, 2)}), (K333, {"tstride": (2, 1, 2)}),
])
def test_f32_storage_form(k, mk):
    from apex_studio_amd import ops
    assert not ops.shipped_verification()
    c = f32_case(5, 33, 17, 96, 16, k, Mode(**mk))
    assert c.x.dtype == torch.float32 and (k != K333 or float(c.ref.abs().max()) > 1000)
    y = c.run()
    assert y.dtype == torch.float32
    _exact(y, c.ref, f"f32 k={k} {mk}")
    if mk.get("pad") == (0, 0):
        _exact(ops.conv2d_cl_down2(c.x, c.wp, c.bias), c.ref, "f32 down2")
