"""The refusals of the convolution front end, string for string (no GPU, nothing is launched): one row or more per rule of the
shared check routine (csrc/conv.hip, conv_fill) and per extra rule of an entry point, with the complete apexmi_last_error()
text, and rows with two faults that pin which of the two is reported, i.e. the order of the checks.  A rule the family query
(apexmi_conv3d_cl_family) can trigger is reached through it; the others (operands, the activation code, an entry point's own
rule) through the entry point, with fake non-null addresses: every such row returns before anything is launched or read.  The
literals are what the library printed before the entry points shared one front end: they are the reference, not the code
under test."""
import ctypes

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import lib, ops

P = 0x100000                       # a 16-byte aligned non-null "device address"

# argument name -> default, in the order of the C signature (include/apexmi.h); a row overrides some of them
_SHAPE = dict(T=2, H=33, W=17, Cin=16, Cout=16, Kpad=512, kT=3, kH=3, kW=3)
_OPERANDS = dict(x=P, w=P, bias=None, residual=None, out=P, zeros=P)
_QUERY = dict(_SHAPE, replicate=0, independent=0, up=0, norm=0, clip_frames=0, stride_h=1, stride_w=1, pad_top=-1, pad_left=-1,
              Ho=0, Wo=0, stride_t=1, t_first=0, To=0)
ENTRIES = {
    "apexmi_conv3d_cl_family": _QUERY,
    "apexmi_conv3d_cl": dict(_OPERANDS, **_SHAPE, stream=None),
    "apexmi_conv3d_cl_frames": dict(_OPERANDS, **_SHAPE, stream=None),
    "apexmi_conv3d_cl_act": dict(_OPERANDS, **_SHAPE, independent=0, up=0, act=1, slope=0.25, stream=None),
    "apexmi_conv3d_cl_norm": dict(x=P, w=P, bias=None, residual=None, out=P, out_norm=P, gamma=P, silu=1, zeros=P, **_SHAPE,
                                  independent=0, up=0, stream=None),
    "apexmi_conv3d_cl_strided": dict(_OPERANDS, **_SHAPE, stride_h=2, stride_w=2, pad_top=1, pad_left=1, Ho=17, Wo=9, stream=None),
    "apexmi_conv3d_cl_tstrided": dict(_OPERANDS, **_SHAPE, stride_t=2, t_first=0, To=1, stream=None),
}


def call(L, entry: str, overrides: dict):
    """(return value, N extent or None, apexmi_last_error()) of one call of `entry` on the library handle L"""
    args = dict(ENTRIES[entry], **overrides)
    assert set(args) == set(ENTRIES[entry]), sorted(set(overrides) - set(ENTRIES[entry]))
    packed = list(args.values())                     # dicts keep the signature's order
    n = None
    if entry == "apexmi_conv3d_cl_family":
        n = ctypes.c_int(-7)
        packed.append(ctypes.addressof(n))
    rc = getattr(L, entry)(*packed)
    return rc, None if n is None else n.value, L.apexmi_last_error().decode()


Q = "apexmi_conv3d_cl_family"
TSTRIDE_EXCLUDES = "conv3d_cl: a temporal stride excludes the upsample / independent-frame / fused-norm modes"
FRAMES_ROOM = ("conv3d_cl_frames: Kpad=448 leaves no room to address the last temporal slice (need >= 480; pack the weight with "
               "apexmi's packing rule)")
ROWS = [
    # ---- the shared rules, in the order of the checks
    ("empty volume", Q, dict(T=0), "conv3d_cl: empty volume"),
    ("Cin % 8", Q, dict(Cin=12), "conv3d_cl: Cin=12 must be a multiple of 8, Cout=16 of 4"),
    ("Cout % 4", Q, dict(Cout=6), "conv3d_cl: Cin=16 must be a multiple of 8, Cout=6 of 4"),
    ("even kernel height", Q, dict(kH=2), "conv3d_cl: kernel 3x2x3 unsupported"),
    ("even kernel width", Q, dict(kW=4), "conv3d_cl: kernel 3x3x4 unsupported"),
    ("more than MAX_TAPS taps", Q, dict(kT=4, Kpad=1024), "conv3d_cl: kernel 4x3x3 unsupported"),
    ("no taps", Q, dict(kT=0), "conv3d_cl: kernel 0x3x3 unsupported"),
    ("stride 0", Q, dict(stride_h=0), "conv3d_cl: stride 0x1 / pad 1,1 / output 33x17 do not fit the 33x17 input"),
    ("pad >= kernel", Q, dict(pad_left=3), "conv3d_cl: stride 1x1 / pad 1,3 / output 33x17 do not fit the 33x17 input"),
    ("output past the input", Q, dict(stride_h=2, stride_w=2, pad_top=0, pad_left=0, Ho=18, Wo=9),
     "conv3d_cl: stride 2x2 / pad 0,0 / output 18x9 do not fit the 33x17 input"),
    ("output past the upsampled input", Q, dict(up=1, Ho=68), "conv3d_cl: stride 1x1 / pad 1,1 / output 68x34 do not fit the 66x34 input"),
    ("Kpad not a multiple of 64", Q, dict(Kpad=500), "conv3d_cl: Kpad=500 must be >= taps*Cin rounded up to 64"),
    ("Kpad below taps * Cin", Q, dict(Kpad=384), "conv3d_cl: Kpad=384 must be >= taps*Cin rounded up to 64"),
    ("volume", Q, dict(T=32768, H=256, W=256), "conv3d_cl: volume too large for one call"),
    ("upsampled volume", Q, dict(T=8192, H=256, W=256, up=1), "conv3d_cl: volume too large for one call"),
    ("frames: no room for the last slice", Q, dict(independent=1, Kpad=448), FRAMES_ROOM),
    ("frames: no room, entry point", "apexmi_conv3d_cl_frames", dict(Kpad=448), FRAMES_ROOM),
    ("frames: replicate", Q, dict(independent=1, replicate=1),
     "conv3d_cl_frames: Kpad=512 leaves no room to address the last temporal slice (need >= 480; pack the weight with apexmi's "
     "packing rule)"),
    ("activation code", "apexmi_conv3d_cl_act", dict(act=2),
     "conv3d_cl: activation 2 unsupported (0 none, 1 leaky ReLU; not together with the fused norm)"),
    ("temporal stride past the input", Q, dict(T=3, stride_t=2, t_first=1, To=2),
     "conv3d_cl: temporal stride 2 / first frame 1 / 2 output frames do not fit 3 input frames"),
    ("temporal stride 0", Q, dict(stride_t=0), "conv3d_cl: temporal stride 0 / first frame 0 / 2 output frames do not fit 2 input frames"),
    ("first frame < 0", Q, dict(t_first=-1), "conv3d_cl: temporal stride 1 / first frame -1 / 2 output frames do not fit 2 input frames"),
    ("temporal stride + upsample", Q, dict(T=3, stride_t=2, To=1, up=1), TSTRIDE_EXCLUDES),
    ("temporal stride + independent frames", Q, dict(T=3, stride_t=2, To=1, independent=1), TSTRIDE_EXCLUDES),
    ("temporal stride + norm", Q, dict(T=3, stride_t=2, To=1, norm=1), TSTRIDE_EXCLUDES),
    ("fewer output frames + norm", Q, dict(T=3, To=2, norm=1), TSTRIDE_EXCLUDES),
    ("clip_frames does not divide T", Q, dict(T=4, clip_frames=3), "conv3d_cl: clip_frames=3 must divide T=4 (stride-1 plain convolutions only)"),
    ("clip_frames < 0", Q, dict(clip_frames=-1), "conv3d_cl: clip_frames=-1 must divide T=2 (stride-1 plain convolutions only)"),
    ("clips + upsample", Q, dict(T=4, clip_frames=2, up=1), "conv3d_cl: clip_frames=2 must divide T=4 (stride-1 plain convolutions only)"),
    ("clips + norm", Q, dict(T=4, clip_frames=2, norm=1), "conv3d_cl: clip_frames=2 must divide T=4 (stride-1 plain convolutions only)"),
    ("clips + temporal stride", Q, dict(T=4, clip_frames=2, stride_t=2, To=2),
     "conv3d_cl: clip_frames=2 must divide T=4 (stride-1 plain convolutions only)"),
    # ---- operands: the entry points only (the query has none)
    ("null in", "apexmi_conv3d_cl", dict(x=None), "conv3d_cl: null operand"),
    ("null w", "apexmi_conv3d_cl", dict(w=None), "conv3d_cl: null operand"),
    ("null out", "apexmi_conv3d_cl", dict(out=None), "conv3d_cl: null operand"),
    ("null zeros", "apexmi_conv3d_cl", dict(zeros=None), "conv3d_cl: null operand"),
    ("misaligned in", "apexmi_conv3d_cl", dict(x=P + 8), "conv3d_cl: operands must be 16-byte aligned"),
    ("misaligned w", "apexmi_conv3d_cl", dict(w=P + 2), "conv3d_cl: operands must be 16-byte aligned"),
    ("misaligned out", "apexmi_conv3d_cl", dict(out=P + 4), "conv3d_cl: operands must be 16-byte aligned"),
    ("misaligned zeros", "apexmi_conv3d_cl", dict(zeros=P + 8), "conv3d_cl: operands must be 16-byte aligned"),
    # ---- the entry points' own rules, in front of the shared ones
    ("norm: no out_norm", "apexmi_conv3d_cl_norm", dict(out_norm=None), "conv3d_cl_norm: out_norm and gamma are required"),
    ("norm: no gamma", "apexmi_conv3d_cl_norm", dict(gamma=None), "conv3d_cl_norm: out_norm and gamma are required"),
    ("norm: Cout % 8", "apexmi_conv3d_cl_norm", dict(Cout=12), "conv3d_cl_norm: Cout=12 must be a multiple of 8"),
    ("strided: empty output", "apexmi_conv3d_cl_strided", dict(Ho=0), "conv3d_cl_strided: empty output 0x9"),
    ("strided: negative output", "apexmi_conv3d_cl_strided", dict(Wo=-1), "conv3d_cl_strided: empty output 17x-1"),
    ("tstrided: empty output", "apexmi_conv3d_cl_tstrided", dict(To=0), "conv3d_cl_tstrided: empty output"),
    # ---- two faults: the earlier check reports
    ("null operand before the shape", "apexmi_conv3d_cl", dict(x=None, Cin=12), "conv3d_cl: null operand"),
    ("empty volume before Cin", Q, dict(T=0, Cin=12), "conv3d_cl: empty volume"),
    ("Cin before the kernel", Q, dict(Cin=12, kH=2), "conv3d_cl: Cin=12 must be a multiple of 8, Cout=16 of 4"),
    ("kernel before stride", Q, dict(kH=2, stride_h=0), "conv3d_cl: kernel 3x2x3 unsupported"),
    ("stride before Kpad", Q, dict(stride_h=0, Kpad=500), "conv3d_cl: stride 0x1 / pad 1,1 / output 33x17 do not fit the 33x17 input"),
    ("Kpad before the volume", Q, dict(T=32768, H=256, W=256, Kpad=500), "conv3d_cl: Kpad=500 must be >= taps*Cin rounded up to 64"),
    ("shape before alignment", "apexmi_conv3d_cl", dict(x=P + 8, Kpad=500), "conv3d_cl: Kpad=500 must be >= taps*Cin rounded up to 64"),
    ("alignment before the frames rule", "apexmi_conv3d_cl_frames", dict(x=P + 8, Kpad=448), "conv3d_cl: operands must be 16-byte aligned"),
    ("frames rule before the temporal stride", Q, dict(independent=1, Kpad=448, stride_t=0), FRAMES_ROOM),
    ("alignment before the activation code", "apexmi_conv3d_cl_act", dict(w=P + 8, act=3), "conv3d_cl: operands must be 16-byte aligned"),
    ("temporal fit before its exclusions", Q, dict(T=3, stride_t=2, t_first=1, To=2, up=1),
     "conv3d_cl: temporal stride 2 / first frame 1 / 2 output frames do not fit 3 input frames"),
    ("temporal exclusions before the clips", Q, dict(T=4, stride_t=2, To=2, up=1, clip_frames=3), TSTRIDE_EXCLUDES),
    ("norm: its operands before its Cout", "apexmi_conv3d_cl_norm", dict(gamma=None, Cout=12), "conv3d_cl_norm: out_norm and gamma are required"),
    ("norm: its Cout before the shared rules", "apexmi_conv3d_cl_norm", dict(Cout=12, x=None), "conv3d_cl_norm: Cout=12 must be a multiple of 8"),
    ("norm: a null out alone is no null operand", "apexmi_conv3d_cl_norm", dict(out=None, Kpad=500),
     "conv3d_cl: Kpad=500 must be >= taps*Cin rounded up to 64"),
    ("strided: empty output before the shared rules", "apexmi_conv3d_cl_strided", dict(Ho=0, x=None), "conv3d_cl_strided: empty output 0x9"),
    ("tstrided: empty output before the shared rules", "apexmi_conv3d_cl_tstrided", dict(To=-2, Cin=12), "conv3d_cl_tstrided: empty output"),
]


@pytest.mark.parametrize("fault,entry,overrides,text", ROWS, ids=[r[0] for r in ROWS])
def test_refusal_text(fault, entry, overrides, text):
    rc, n, msg = call(lib.load(), entry, overrides)
    if entry == Q:
        assert (rc, n) == (-1, 0), (rc, n)
    else:
        assert rc == 1, rc
    assert msg == text


def test_one_row_or_more_per_rule():
    """every message family of the front end has a row"""
    texts = " | ".join(r[3] for r in ROWS)
    for stem in ("null operand", "empty volume", "must be a multiple of 8, Cout", "unsupported", "do not fit the", "rounded up to 64",
                 "volume too large", "leaves no room", "activation", "output frames do not fit", "a temporal stride excludes",
                 "must divide T", "out_norm and gamma are required", "Cout=12 must be a multiple of 8", "conv3d_cl_strided: empty output",
                 "conv3d_cl_tstrided: empty output", "16-byte aligned"):
        assert stem in texts, stem


# (overrides of the query, (family, N extent)) under the shipped conv.* settings
ACCEPTED = [
    (dict(), (0, 0)),                                                                       # the defaults: 128x128
    (dict(T=3, H=131, W=173, Cin=96, Cout=96, Kpad=2624), (2, 0)),                          # slab48
    (dict(T=3, H=131, W=173, Cin=96, Cout=96, Kpad=2624, norm=1), (2, 0)),                  # ... with the fused norm
    (dict(T=3, H=131, W=173, Cin=96, Cout=384, Kpad=2624, norm=1), (1, 192)),               # no slab tile holds 384 channels: v2
    (dict(T=4, H=67, W=250, Cin=128, Cout=128, Kpad=3456), (3, 0)),                         # slab64
    (dict(T=1, H=251, W=263, Cin=136, Cout=160, Kpad=1280, kT=1, norm=1), (1, 192)),        # v2, one N tile
    (dict(T=6, H=131, W=173, Cin=96, Cout=96, Kpad=2624, clip_frames=2), (0, 0)),           # stacked clips: 128x128
]


@pytest.mark.parametrize("overrides,want", ACCEPTED)
def test_query_needs_no_operands(overrides, want):
    """the query has no operand at all (none is passed: every pointer of the shared record stays null), with and without the
    fused norm, and reports the family the launch would take"""
    rc, n, _ = call(lib.load(), Q, overrides)
    assert (rc, n) == want


# ------------------------------------------------------------------------------------------------- the ops.py wrappers
@pytest.mark.parametrize("who,run", [
    ("conv3d_cl", lambda x, w: ops.conv3d_cl(x, w, None, (1, 3, 3))),
    ("conv3d_cl_act", lambda x, w: ops.conv3d_cl_act(x, w, None, (1, 3, 3), slope=0.2)),
    ("conv3d_cl_norm", lambda x, w: ops.conv3d_cl_norm(x, w, None, (1, 3, 3), torch.ones(8, dtype=torch.bfloat16))),
    ("conv3d_cl_tstrided", lambda x, w: ops.conv3d_cl_tstrided(x, w, None, (1, 3, 3), 2, 0, 1)),
    ("conv2d_cl_down2", lambda x, w: ops.conv2d_cl_down2(x, w, None)),
    ("conv2d_cl_strided", lambda x, w: ops.conv2d_cl_strided(x, w, None)),
])
def test_wrappers_refuse_under_their_own_name(who, run):
    """the shared operand helper words its refusals with the calling wrapper's name, as each wrapper did itself"""
    x, w = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16), torch.zeros(8, 128, dtype=torch.bfloat16)
    with pytest.raises(lib.ApexMIError) as e:
        run(x, w)
    assert str(e.value) == f"{who}.x: expected a ROCm device tensor, got cpu (no CPU fallback)"
