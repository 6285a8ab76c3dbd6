"""Exact integer probes of the convolution family: operands whose correct output is an exactly representable integer, and the
references, written from the documented semantics of ops.conv3d_cl* (the docstrings), never from a kernel.  Pure torch on the
CPU; the GPU tests feed the operands to the kernels and compare with torch.equal, the host tests prove that the comparison rejects
single wrong decisions the whole-tensor rel-L2 bar lets through.

Why no tolerance: bf16 holds every integer up to 256; with |x| <= 4 and |w| <= 2 every product and every f32 partial sum is an
integer far below 2^24, so the f32 accumulation is exact in ANY order (the implicit GEMM's K order, the slab kernels' temporal-tap /
slice / spatial-tap order, conv.torder 0 / 1).  If |sum + bias + residual| <= 256 the bf16 store is exact too.

Selector weights: for each (output channel, tap) exactly one input channel carries a coefficient from {-2, -1, 1, 2}, so every tap
is told apart by channel and by sign / magnitude; |out| <= 27 * 2 * 4 = 216 for any channel count and the reference is 27 shifted
gathers.  Dense ternary weights: x, w in {-1, 0, 1} with the density of w chosen so that the reference stays <= 256 (asserted)."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

BF = torch.bfloat16
LIMIT = 256          # largest magnitude up to which bf16 holds every integer


class Mode(NamedTuple):
    """How a call reads its input (ops.conv3d_cl / conv3d_cl_act / conv2d_cl_strided / conv2d_cl_down2 / conv3d_cl_tstrided)."""
    replicate: bool = False            # clamp (t, y, x) instead of reading zeros
    independent: bool = False          # every frame is a one-frame clip
    up: bool = False                   # read through a nearest 2x spatial upsample
    clip: int = 0                      # T / clip clips stacked along T, each causal on its own (0: one clip)
    stride: Tuple[int, int] = (1, 1)   # spatial stride
    pad: Optional[Tuple[int, int]] = None          # (top, left) zero padding; None = "same"
    out_hw: Optional[Tuple[int, int]] = None       # output extents of a strided call
    tstride: Optional[Tuple[int, int, int]] = None  # (stride_t, t_first, out_frames)


# ------------------------------------------------------------------------------------------------------------------ operands
def int_input(T, H, W, C, salt=0):
    """x[t, h, w, c] in [-4, 4] from all four coordinates: one step along any axis changes the value (4, 7, 2, 5 are units mod 9),
    h and w enter differently (no h <-> w symmetry), nothing is symmetric under a reflection, and the period along every axis is 9
    or a multiple of it, which divides no tile extent (8, 16, 32, 48, 64, 128)."""
    t = torch.arange(T).view(T, 1, 1, 1) + salt
    h, w, c = torch.arange(H).view(1, H, 1, 1), torch.arange(W).view(1, 1, W, 1), torch.arange(C).view(1, 1, 1, C)
    return ((t * 4 + h * 7 + w * 2 + c * 5 + (h * w) % 5 + (w * c) % 7 + (t * c) % 3) % 9 - 4).float()


def selector(cout, cin, k):
    """(ci [cout, taps] long, coef [cout, taps] float): the one input channel and the coefficient of each (output channel, tap).
    As co runs, ci = (5 co + 19 tap + 3 (co // 7)) % cin walks through every 48- and 64-channel slice and every 8-channel chunk of
    a slice (checked by the host tests for the shapes the GPU probes use)."""
    taps = k[0] * k[1] * k[2]
    co, tap = torch.arange(cout).view(-1, 1), torch.arange(taps).view(1, -1)
    ci = (co * 5 + tap * 19 + 3 * (co // 7)) % cin
    coef = torch.tensor([1.0, -2.0, 2.0, -1.0])[(co * 3 + tap * 5 + (co * tap) % 7) % 4]
    return ci, coef


def selector_dense(ci, coef, cin, k):
    """the selector as a dense [cout, cin, kT, kH, kW] weight (what pack_conv_weight takes)"""
    cout, taps = ci.shape
    w = torch.zeros(cout, taps, cin)
    w.scatter_(2, ci.unsqueeze(2), coef.unsqueeze(2))
    return w.view(cout, k[0], k[1], k[2], cin).permute(0, 4, 1, 2, 3).contiguous()


def ternary(shape, seed, density):
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return sign * (torch.rand(shape, generator=g) < density).float()


def ternary_density(K):
    """density of non-zeros in w for x of density 2/3: the sum of K products has sigma = sqrt(K * 2/3 * d); d = min(4/9, 1500 / K)
    keeps sigma <= 31.7, so 7 sigma + |bias| + |residual| <= 222 + 24 < 256 (4/9 at K = 2592: sigma 27.7)."""
    return min(4.0 / 9.0, 1500.0 / K)


def ternary_operands(T, H, W, cin, cout, k, seed):
    """(x [T, H, W, cin], w [cout, cin, kT, kH, kW]) in {-1, 0, 1}"""
    K = k[0] * k[1] * k[2] * cin
    return ternary((T, H, W, cin), seed, 2.0 / 3.0), ternary((cout, cin) + tuple(k), seed + 1, ternary_density(K))


def int_weight(cout, cin, k):
    """dense integers in [-2, 2] for the float-storage form (no 256 limit there)"""
    taps = k[0] * k[1] * k[2]
    co, ci, tap = torch.arange(cout).view(-1, 1, 1), torch.arange(cin).view(1, -1, 1), torch.arange(taps).view(1, 1, -1)
    w = ((co * 3 + ci * 7 + tap * 2 + (co * tap) % 5 + (ci * tap) % 3) % 5 - 2).float()
    return w.view(cout, cin, *k).contiguous()


def int_bias(cout):
    """[-8, 8] over the real channels; the caller pads to the packed channel count with zeros"""
    return ((torch.arange(cout) * 5 + 3) % 17 - 8).float()


def int_residual(T, H, W, cout):
    """[-16, 16], position- and channel-dependent"""
    t, h = torch.arange(T).view(T, 1, 1, 1), torch.arange(H).view(1, H, 1, 1)
    w, c = torch.arange(W).view(1, 1, W, 1), torch.arange(cout).view(1, 1, 1, cout)
    return ((t * 5 + h * 3 + w * 11 + c * 7 + (h * c) % 5 + (w * t) % 3) % 33 - 16).float()


def pad_channels(v, cout4):
    """zero-extend the last axis to the packed channel count"""
    if v.shape[-1] == cout4:
        return v
    out = torch.zeros(v.shape[:-1] + (cout4,), dtype=v.dtype)
    out[..., :v.shape[-1]] = v
    return out


# ---------------------------------------------------------------------------------------------------------------- references
def _axis(n_out, n_in, stride, offset, clamp, up=False):
    """source index and validity of one tap along one spatial axis: output i reads coordinate i * stride + offset of the
    (upsampled, if up) image of extent n_in; outside: zeros, or the clamped coordinate"""
    pos = torch.arange(n_out) * stride + offset
    ok = (pos >= 0) & (pos < n_in)
    pos = pos.clamp(0, n_in - 1)
    if clamp:
        ok = torch.ones_like(ok)
    return (pos // 2 if up else pos), ok


def tap_sources(T, H, W, k, mode=Mode()):
    """The documented read rule.  Returns (To, Ho, Wo, taps) with taps[i] = ((kt, ky, kx), (ti, tok), (yi, yok), (xi, xok)) in
    weight order: output (t, y, x) reads stored x[ti[t], yi[y], xi[x]] where all three ok flags hold, zero otherwise."""
    kT, kH, kW = k
    He, We = (2 * H, 2 * W) if mode.up else (H, W)           # extents the convolution runs over
    pt, pl = mode.pad if mode.pad is not None else ((kH - 1) // 2, (kW - 1) // 2)
    Ho, Wo = mode.out_hw if mode.out_hw is not None else (He, We)
    st, t0, To = mode.tstride if mode.tstride is not None else (1, 0, T)
    clip = 1 if mode.independent else (mode.clip or T)
    taps = []
    for kt in range(kT):
        t_end = torch.arange(To) * st + t0                    # the frame the causal window of output t ends at
        pos = t_end + kt - (kT - 1)
        first = (t_end // clip) * clip                        # first frame of that frame's clip
        tok = pos >= first
        pos = torch.maximum(pos, first)
        if mode.replicate:
            tok = torch.ones_like(tok)
        for ky in range(kH):
            ysrc = _axis(Ho, He, mode.stride[0], ky - pt, mode.replicate, mode.up)
            for kx in range(kW):
                taps.append(((kt, ky, kx), (pos, tok), ysrc, _axis(Wo, We, mode.stride[1], kx - pl, mode.replicate, mode.up)))
    return To, Ho, Wo, taps


def shifted(x, src):
    """x [T, H, W, C] as one tap sees it: [To, Ho, Wo, C]"""
    _, (ti, tok), (yi, yok), (xi, xok) = src
    s = x[ti.view(-1, 1, 1), yi.view(1, -1, 1), xi.view(1, 1, -1)]        # one gather
    if bool(tok.all()) and bool(yok.all()) and bool(xok.all()):
        return s
    ok = tok.view(-1, 1, 1, 1) & yok.view(1, -1, 1, 1) & xok.view(1, 1, -1, 1)
    return s * ok.to(s.dtype)


def conv_ref(x, w, k, mode=Mode(), bias=None, residual=None, cout4=None, hook=None):
    """The exact result [To, Ho, Wo, cout4] (float32 integers; padded channels zero) of x [T, H, W, cin] with w either a dense
    [cout, cin, kT, kH, kW] tensor (one matmul per tap) or a selector (ci, coef) (one gather per tap); bias [cout], residual
    [To, Ho, Wo, cout].  Every partial sum is an integer below 2^24, so float32 is exact.  hook(tap_index, (kt, ky, kx), s) -> s
    lets the host tests plant one wrong decision into what a tap reads."""
    T, H, W, _ = x.shape
    To, Ho, Wo, taps = tap_sources(T, H, W, k, mode)
    sel = isinstance(w, tuple)
    cout = w[0].shape[0] if sel else w.shape[0]
    out = torch.zeros(To, Ho, Wo, cout)
    for i, src in enumerate(taps):
        s = shifted(x, src)
        if hook is not None:
            s = hook(i, src[0], s)
        if sel:
            out += s[..., w[0][:, i]] * w[1][:, i]
        else:
            kt, ky, kx = src[0]
            out += s @ w[:, :, kt, ky, kx].t()
    if bias is not None:
        out += bias
    if residual is not None:
        out += residual
    assert float(out.abs().max()) < 2 ** 24
    return pad_channels(out, cout4 or (cout + 3) // 4 * 4)


def check_bf16_exact(ref):
    """the condition of a bf16 probe (not a measurement): the reference is integer and no larger than 256"""
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) <= LIMIT, float(ref.abs().max())
    return ref


def leaky(y, slope):
    """leaky ReLU of the exact integers, ONE bf16 rounding (slope a power of two: y * slope is exact in float32)"""
    return (y if slope is None else torch.where(y < 0, y * slope, y)).to(BF)


def gamma_of(C):
    """bf16-exact norm weights in [0.5, 2]"""
    return 0.5 + ((torch.arange(C) * 7) % 13).float() / 8


def rmsnorm_ref(y, gamma, silu):
    """float64 WanRMS_norm (+ SiLU) per position over the last axis: y / max(||y||_2, 1e-12) * sqrt(C) * gamma"""
    y = y.double()
    n = y.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    r = y / n * (y.shape[-1] ** 0.5) * gamma.double()
    return r * torch.sigmoid(r) if silu else r


# --------------------------------------------------------------------------------------------------------------- comparisons
def _ordered(v):
    """bf16 -> int32 that counts code points monotonically (-0 and +0 both 0)"""
    i = v.contiguous().view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_distance(got, want64):
    """largest distance, in bf16 code points, between got (bf16) and the float64 reference rounded to bf16"""
    assert got.dtype == BF
    return int((_ordered(got) - _ordered(want64.to(BF))).abs().max())


def mismatches(got, want, n=6):
    """'count: (t, h, w, co) got g want v; ...' for the first n differing elements, '' when equal bit for bit"""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return ""
    bad = (got != want).nonzero()
    items = [f"{tuple(int(v) for v in ix)} got {float(got[tuple(ix)])} want {float(want[tuple(ix)])}" for ix in bad[:n]]
    return f"{bad.shape[0]} of {got.numel()} differ; first (t, h, w, co): " + "; ".join(items)


def rel_l2(a, b):
    """the whole-tensor bar of the older conv tests (test_conv3d_cl: < 4e-3)"""
    return float((a.double() - b.double()).norm() / b.double().norm())


REL_L2_BAR = 4e-3


# ----------------------------------------------------------------------------------------------- the dense cases of the GPU suite
# (T, H, W, cin, cout, k, mode-kwargs, seed): every dense ternary case the GPU probes run; the host tests evaluate each reference
# and its <= 256 condition without a GPU.  H, W ragged against 8, 16 and 32.
DENSE_CASES = {
    "gemm128.3x3x3": (2, 33, 17, 96, 160, (3, 3, 3), {}, 11),
    "gemm128.repl": (3, 33, 17, 128, 96, (3, 3, 3), {"replicate": True}, 12),
    "gemm128.up": (2, 17, 9, 96, 16, (3, 3, 3), {"up": True}, 13),
    "v2.n192": (1, 251, 263, 48, 192, (1, 3, 3), {}, 14),
    "slab48.nt3": (3, 131, 173, 96, 96, (3, 3, 3), {}, 15),
    "slab48.192": (1, 251, 263, 96, 192, (1, 3, 3), {}, 16),
    "slab64.128": (4, 67, 250, 128, 128, (3, 3, 3), {}, 17),
}


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(x, w, bias, residual, ref) of one DENSE_CASES entry, computed once"""
    T, H, W, cin, cout, k, mk, seed = DENSE_CASES[name]
    mode = Mode(**mk)
    x, w = ternary_operands(T, H, W, cin, cout, k, seed)
    To, Ho, Wo, _ = tap_sources(T, H, W, k, mode)
    bias, res = int_bias(cout), int_residual(To, Ho, Wo, cout)
    return x, w, bias, res, check_bf16_exact(conv_ref(x, w, k, mode, bias, res))
