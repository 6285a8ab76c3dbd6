"""The convolution probes have teeth (no GPU): the exact comparison rejects every single wrong decision planted into the
reference, the whole-tensor rel-L2 < 4e-3 bar of the older tests accepts some of them; the references agree with torch's own
convolutions on small cases; every probe's reference is exactly representable in bf16."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_probes as P
from tests.conv_probes import Mode

K333 = (3, 3, 3)


def _selector_case(T, H, W, cin, cout, k=K333, mode=Mode(), x=None, w=None, hook=None):
    x = P.int_input(T, H, W, cin) if x is None else x
    return P.conv_ref(x, P.selector(cout, cin, k) if w is None else w, k, mode, hook=hook)


def _rejected(mutant, ref):
    """the exact comparison rejects the mutant and names a coordinate"""
    msg = P.mismatches(mutant, ref)
    assert not torch.equal(mutant, ref) and "got" in msg and "want" in msg
    return P.rel_l2(mutant, ref)


# ------------------------------------------------------------------------------------------------------------------- mutations
def test_one_tap_dropped_at_one_corner_pixel_passes_the_rel_l2_bar_and_fails_the_exact_comparison():
    T, H, W = 2, 67, 93
    ref = _selector_case(T, H, W, 16, 16)

    def drop(i, tap, s):      # tap (kt 2, ky 0, kx 0) reads (y - 1, x - 1): inside the image at the bottom-right corner
        if tap == (2, 0, 0):
            s = s.clone()
            s[T - 1, H - 1, W - 1] = 0
        return s
    rel = _rejected(_selector_case(T, H, W, 16, 16, hook=drop), ref)
    assert rel < P.REL_L2_BAR, rel          # the gap: the older bar accepts a missed tap


def test_one_column_over_on_the_last_ragged_tile():
    T, H, W = 1, 17, 75            # the last 32-wide tile holds columns 64..74
    ref = _selector_case(T, H, W, 16, 16)

    def over(i, tap, s):
        s = s.clone()
        s[:, :, 64:W - 1] = s[:, :, 65:W].clone()
        return s
    _rejected(_selector_case(T, H, W, 16, 16, hook=over), ref)


def test_zero_padding_instead_of_the_clamp_on_the_top_row():
    T, H, W = 2, 131, 37
    ref = _selector_case(T, H, W, 16, 16, mode=Mode(replicate=True))

    def zero_top(i, tap, s):
        if tap[1] == 0:
            s = s.clone()
            s[:, 0] = 0
        return s
    _rejected(_selector_case(T, H, W, 16, 16, mode=Mode(replicate=True), hook=zero_top), ref)


@pytest.mark.parametrize("replicate", [False, True])
def test_first_frame_of_a_clip_sees_the_previous_clip(replicate):
    T, H, W = 4, 11, 13
    ref = _selector_case(T, H, W, 16, 16, mode=Mode(replicate=replicate, clip=2))
    leak = ref.clone()
    leak[2] = _selector_case(T, H, W, 16, 16, mode=Mode(replicate=replicate))[2]     # frame 0 of clip 1 as one long clip reads it
    _rejected(leak, ref)
    # and the rule itself: stacked clips == one call per clip
    x = P.int_input(T, H, W, 16)
    per_clip = torch.cat([_selector_case(2, H, W, 16, 16, mode=Mode(replicate=replicate), x=x[i:i + 2]) for i in (0, 2)])
    assert torch.equal(per_clip, ref)


def test_two_spatial_taps_swapped():
    ci, coef = P.selector(16, 16, K333)
    ci2, coef2 = ci.clone(), coef.clone()
    a, b = (2 * 3 + 0) * 3 + 1, (2 * 3 + 1) * 3 + 0          # (ky, kx) = (0, 1) <-> (1, 0) of the last temporal tap
    ci2[:, [a, b]], coef2[:, [a, b]] = ci[:, [b, a]], coef[:, [b, a]]
    _rejected(_selector_case(2, 33, 17, 16, 16, w=(ci2, coef2)), _selector_case(2, 33, 17, 16, 16))


def test_one_48_channel_slice_dropped():
    x = P.int_input(1, 33, 17, 96)
    x2 = x.clone()
    x2[..., 48:] = 0
    _rejected(_selector_case(1, 33, 17, 96, 96, x=x2), _selector_case(1, 33, 17, 96, 96, x=x))


def test_non_zero_in_the_padded_channel():
    ref = _selector_case(2, 33, 17, 16, 3)
    assert ref.shape[-1] == 4 and not ref[..., 3].any()
    bad = ref.clone()
    bad[1, 5, 7, 3] = 1
    assert _rejected(bad, ref) < P.REL_L2_BAR


def test_upsample_read_shifted_by_one_source_pixel():
    x = P.int_input(2, 17, 9, 16)
    ref = _selector_case(2, 17, 9, 16, 16, mode=Mode(up=True), x=x)
    assert ref.shape[:3] == (2, 34, 18)
    _rejected(_selector_case(2, 17, 9, 16, 16, mode=Mode(up=True), x=x.roll(1, dims=2)), ref)


# ---------------------------------------------------------------------------------------------------- the references themselves
def _torch_conv(x, w, k, mode):
    """torch's own convolution of the same semantics, float64: explicit padding, F.conv3d"""
    kT, kH, kW = k
    v = x.permute(3, 0, 1, 2).unsqueeze(0).double()                     # [1, C, T, H, W]
    if mode.up:
        v = F.interpolate(v, scale_factor=(1, 2, 2), mode="nearest")
    pt, pl = mode.pad if mode.pad is not None else ((kH - 1) // 2, (kW - 1) // 2)
    pads = (pl, kW, pt, kH, kT - 1, 0)                                   # generous right / bottom: cropped below
    v = F.pad(v, pads, mode="replicate") if mode.replicate else F.pad(v, pads)
    y = F.conv3d(v, w.double(), stride=(1,) + tuple(mode.stride))
    if mode.tstride is not None:
        st, t0, To = mode.tstride
        y = y[:, :, t0::st][:, :, :To]
    To, Ho, Wo, _ = P.tap_sources(x.shape[0], x.shape[1], x.shape[2], k, mode)
    return P.pad_channels(y[0, :, :, :Ho, :Wo].permute(1, 2, 3, 0).float().contiguous(), (w.shape[0] + 3) // 4 * 4)


@pytest.mark.parametrize("k,mk", [
    (K333, {}), ((2, 3, 3), {}), ((3, 1, 1), {}), ((1, 1, 1), {}), (K333, {"replicate": True}), ((1, 3, 3), {"up": True}),
    (K333, {"up": True}),
    ((1, 3, 3), {"stride": (2, 2), "pad": (1, 1), "out_hw": (6, 5)}),     # conv2d_cl_strided(2, 1) on 11 x 9
    ((1, 3, 3), {"stride": (2, 2), "pad": (0, 0), "out_hw": (5, 4)}),     # conv2d_cl_strided(2, 0) and conv2d_cl_down2
    ((3, 1, 1), {"tstride": (2, 2, 2)}), ((3, 3, 3), {"tstride": (2, 1, 2)}),
])
def test_references_agree_with_torch_conv3d(k, mk):
    mode = Mode(**mk)
    x = P.int_input(5, 11, 9, 16)
    ci, coef = P.selector(7, 16, k)
    w = P.selector_dense(ci, coef, 16, k)
    want = _torch_conv(x, w, k, mode)
    assert torch.equal(P.conv_ref(x, (ci, coef), k, mode), want)          # the 27 gathers
    assert torch.equal(P.conv_ref(x, w, k, mode), want)                   # the same weight through the dense path
    xd, wd = P.ternary_operands(5, 11, 9, 16, 7, k, 3)
    assert torch.equal(P.conv_ref(xd, wd, k, mode), _torch_conv(xd, wd, k, mode))


def test_down2_reads_the_zero_row_below_an_even_image():
    """ZeroPad2d((0, 1, 0, 1)) + Conv2d(3, stride 2): Ho = (H - 2) // 2 + 1 for even and odd H"""
    for H, W in ((12, 10), (11, 9)):
        x = P.int_input(2, H, W, 16)
        w = P.int_weight(8, 16, (1, 3, 3))
        Ho, Wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
        v = F.pad(x.permute(0, 3, 1, 2).double(), (0, 1, 0, 1))
        want = F.conv2d(v, w[:, :, 0].double(), stride=2).permute(0, 2, 3, 1).float()
        got = P.conv_ref(x, w, (1, 3, 3), Mode(stride=(2, 2), pad=(0, 0), out_hw=(Ho, Wo)))
        assert want.shape[1:3] == (Ho, Wo) and torch.equal(got, want)


def test_independent_frames_are_one_frame_clips():
    x = P.int_input(3, 11, 9, 16)
    w = P.selector(16, 16, K333)
    per_frame = torch.cat([P.conv_ref(x[i:i + 1], w, K333) for i in range(3)])
    assert torch.equal(P.conv_ref(x, w, K333, Mode(independent=True)), per_frame)
    assert torch.equal(P.conv_ref(x, w, K333, Mode(clip=1)), per_frame)


# --------------------------------------------------------------------------------------------------- conditions of the probes
def test_input_has_no_symmetry_and_no_tile_period():
    x = P.int_input(4, 64, 64, 16)
    assert float(x.min()) == -4 and float(x.max()) == 4
    assert not torch.equal(x, x.transpose(1, 2))
    for d in range(4):
        assert not torch.equal(x, x.flip(d))
        for p in (1, 2, 4, 8, 16, 32):
            if p < x.shape[d]:
                assert not torch.equal(x.narrow(d, 0, x.shape[d] - p), x.narrow(d, p, x.shape[d] - p)), (d, p)


@pytest.mark.parametrize("cin,cout", [(48, 32), (96, 96), (96, 192), (48, 384), (128, 128), (256, 128), (512, 1024), (144, 160)])
def test_selector_reaches_every_chunk_of_every_slice(cin, cout):
    ci, coef = P.selector(cout, cin, K333)
    assert set(coef.unique().tolist()) == {-2.0, -1.0, 1.0, 2.0}
    assert (ci // 8).unique().numel() == cin // 8                          # every 8-channel chunk, hence every slice
    for tap in range(27):                                                  # neighbouring taps never look alike
        same = (ci[:, tap] == ci[:, (tap + 1) % 27]) & (coef[:, tap] == coef[:, (tap + 1) % 27])
        assert not same.any()


def test_selector_bound_holds_for_any_channel_count():
    # |x| <= 4, one coefficient of magnitude <= 2 per tap, bias <= 8, residual <= 16: 27 * 8 + 24 = 240 <= 256
    assert 27 * 2 * 4 + 8 + 16 <= P.LIMIT
    assert float(P.int_bias(1024).abs().max()) <= 8 and float(P.int_residual(3, 33, 17, 160).abs().max()) <= 16
    x = P.int_input(2, 33, 17, 96)
    ref = P.conv_ref(x, P.selector(160, 96, K333), K333, Mode(), P.int_bias(160), P.int_residual(2, 33, 17, 160))
    P.check_bf16_exact(ref)


@pytest.mark.parametrize("name", sorted(P.DENSE_CASES))
def test_dense_ternary_references_stay_exact_in_bf16(name):
    x, w, bias, res, ref = P.dense_case(name)            # the builder asserts |ref| <= 256 and integrality
    assert float(ref.abs().max()) <= P.LIMIT and float(ref.abs().max()) > 64, float(ref.abs().max())


def test_ulp_distance_counts_code_points():
    a = torch.tensor([1.0, -1.0, 0.0, 256.0]).to(P.BF)
    assert P.ulp_distance(a, a.double()) == 0
    assert P.ulp_distance(a, torch.tensor([1.0 + 2.0 ** -7, -1.0, 0.0, 256.0]).double()) == 1
    assert P.ulp_distance(a, torch.tensor([1.0, -1.0 + 2.0 ** -8, 0.0, 256.0]).double()) == 1
    assert P.ulp_distance(a, torch.tensor([1.0, -1.0, 0.0, 260.0]).double()) == 2


# ------------------------------------------------------------------------------------------------- the family query (no launch)
def test_family_query_reports_the_launch_rule():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib, ops

    def fam(T, H, W, cin, cout, k, **kw):
        wp = ops.pack_conv_weight(torch.zeros(cout, cin, *k, dtype=P.BF))
        return ops.conv3d_cl_family((T, H, W, cin), wp.shape, k, **kw)
    try:
        assert fam(2, 33, 17, 96, 160, K333) == ("128x128", 0)
        assert fam(3, 131, 173, 96, 96, K333) == ("slab48", 0)
        assert fam(4, 67, 250, 128, 128, K333) == ("slab64", 0)
        assert fam(4, 67, 250, 256, 128, K333, replicate=True) == ("slab64", 0)
        assert fam(1, 67, 250, 128, 128, K333) == ("128x128", 0)           # 72 workgroups: under the slab threshold
        assert fam(6, 131, 173, 96, 96, K333, clip_frames=2) == ("128x128", 0)
        assert fam(1, 300, 300, 96, 96, (1, 3, 3), stride=(2, 2), pad=(0, 0), out_hw=(150, 150)) == ("128x128", 0)
        lib.tune_set("conv.slab", 1)
        assert fam(3, 131, 173, 96, 96, K333) == ("slab96", 0)
        lib.tune_set("conv.slab", 0)
        assert fam(3, 131, 173, 96, 96, K333) == ("v2", 96)
        assert fam(1, 251, 263, 144, 160, (1, 3, 3)) == ("v2", 192)
        assert fam(1, 251, 263, 48, 128, (1, 3, 3)) == ("128x128", 0)      # 256 x 128 measured slower: stays on 128x128
        lib.tune_set("conv.v2", 0)
        assert fam(3, 131, 173, 96, 96, K333) == ("128x128", 0)
    finally:
        lib.tune_set("conv.v2", 1)
        lib.tune_set("conv.slab", 2)
    with pytest.raises(lib.ApexMIError):
        fam(2, 4, 4, 12, 8, K333)
