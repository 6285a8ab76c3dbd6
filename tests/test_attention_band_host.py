"""Per-block key bands on the large-attention kernel, the parts that need no GPU: the arithmetic of ops.frame_band_plan against a
brute-force loop (tests/attention_band_ref.py), the plan's dense mask against the exact +-radius frame mask and the stated slack,
every refusal of ops.band_plan with its exact text, every refusal of apexmi_attn_fwd_prepared_band / apexmi_attn_fwd_band that is
reachable before a launch (fake addresses, nothing is read), the header / binding / export agreement, the backend key and the Wan
and engine switches."""
import os
import re
import shutil
import subprocess

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError
from tests import attention_band_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("apexmi_attn_fwd_prepared_band", "apexmi_attn_fwd_band", "apexmi_attn_band_workspace_bytes")

# (frames, tokens per frame, radius): tokens per frame below / above / no multiple of 64 and 256, radius 0 and >= frames
GRIDS = [(7, 100, 0), (7, 100, 1), (7, 100, 2), (7, 100, 7), (7, 100, 50), (6, 64, 1), (5, 117, 1), (3, 300, 0), (3, 300, 1),
         (4, 256, 1), (9, 40, 2), (1, 70, 0), (2, 1000, 0)]


class _Plan(ops.BandPlan):
    """a BandPlan without a device copy: the host half is all these tests read"""

    def __init__(self, lo, hi, Sq, Sk):
        self.lo, self.hi, self.Sq, self.Sk, self.bands = [list(lo)], [list(hi)], Sq, Sk, None
        self.Hb, self.nqb = 1, len(lo)


@pytest.mark.parametrize("frames,tpf,radius", GRIDS)
def test_frame_bands_equal_the_brute_force_loop(frames, tpf, radius):
    lo, hi = ops.frame_bands(frames, tpf, radius)
    assert (lo, hi) == R.brute_frame_bands(frames, tpf, radius)
    S = frames * tpf
    assert len(lo) == (S + 255) // 256
    for a, e in zip(lo, hi):                               # the rules band_plan checks
        assert 0 <= a < e <= S and a % 64 == 0 and (e % 64 == 0 or e == S)


@pytest.mark.parametrize("frames,tpf,radius", GRIDS)
def test_dense_mask_holds_the_exact_window_within_the_stated_slack(frames, tpf, radius):
    S = frames * tpf
    lo, hi = ops.frame_bands(frames, tpf, radius)
    plan = _Plan(lo, hi, S, S)
    m = plan.dense_mask()
    assert m.shape == (1, S, S) and m.dtype == torch.bool
    exact, slack = R.exact_frame_mask(frames, tpf, radius), R.slack_frame_mask(frames, tpf, radius)
    assert bool((m[0] | ~exact).all())                    # a superset of the exact window
    assert bool((slack | ~m[0]).all())                    # never beyond the slack
    assert plan.kept_fraction == int(m.sum()) / m.numel()
    if radius >= frames:
        assert bool(m.all()) and plan.kept_fraction == 1.0


def test_frame_band_plan_refuses_bad_arguments():
    for args, msg in (((0, 100, 1), "frame_band_plan: frames=0 and tokens_per_frame=100 must be at least 1"),
                      ((3, 0, 1), "frame_band_plan: frames=3 and tokens_per_frame=0 must be at least 1"),
                      ((3, 100, -1), "frame_band_plan: radius=-1 must not be negative")):
        with pytest.raises(ApexMIError) as e:
            ops.frame_band_plan(*args, device="cuda:0")
        assert str(e.value) == msg
    assert "SUPERSET" in ops.frame_band_plan.__doc__ and "straddles" in ops.frame_band_plan.__doc__


BAND_ROWS = [
    ("unaligned lo", ([0, 100], [256, 512], 512, 512), "band_plan: lo=100 of block 1 (head row 0) is not a multiple of 64"),
    ("hi neither aligned nor Sk", ([0, 0], [256, 500], 512, 512),
     "band_plan: hi=500 of block 1 (head row 0) is neither a multiple of 64 nor Sk=512"),
    ("hi = ragged Sk is fine, another ragged hi is not", ([0, 0], [1000, 999], 512, 1000),
     "band_plan: hi=999 of block 1 (head row 0) is neither a multiple of 64 nor Sk=1000"),
    ("empty band", ([0, 128], [256, 128], 512, 512), "band_plan: band [128, 128) of block 1 (head row 0) is empty or outside [0, 512)"),
    ("lo above hi", ([0, 256], [256, 128], 512, 512), "band_plan: band [256, 128) of block 1 (head row 0) is empty or outside [0, 512)"),
    ("hi above Sk", ([0, 0], [256, 576], 512, 512), "band_plan: band [0, 576) of block 1 (head row 0) is empty or outside [0, 512)"),
    ("negative lo", ([-64, 0], [256, 512], 512, 512), "band_plan: band [-64, 256) of block 0 (head row 0) is empty or outside [0, 512)"),
    ("one band too few", ([0], [256], 512, 512), "band_plan: 1 bands for 2 query blocks of 256 rows (Sq=512)"),
    ("one band too many", ([0, 0, 0], [64, 64, 64], 512, 512), "band_plan: 3 bands for 2 query blocks of 256 rows (Sq=512)"),
    ("per-head rows, second head wrong", ([[0, 0], [0, 64]], [[64, 64], [64, 64]], 512, 512),
     "band_plan: band [64, 64) of block 1 (head row 1) is empty or outside [0, 512)"),
    ("lo and hi of different shapes", ([0, 0], [[64, 64], [64, 64]], 512, 512),
     "band_plan: lo and hi differ in shape (1 x [2] against 2 x [2, 2])"),
    ("not integers", ([0.0, 0.0], [64, 64], 512, 512), "band_plan: lo must be [nqb] or [H, nqb] integers, got [0.0, 0.0]"),
    ("empty problem", ([0], [64], 0, 512), "band_plan: empty problem (Sq=0 Sk=512)"),
    # two faults: the alignment of lo, then of hi, then the range
    ("unaligned lo, then empty", ([0, 100], [256, 100], 512, 512), "band_plan: lo=100 of block 1 (head row 0) is not a multiple of 64"),
    ("valid plan, not a ROCm device", ([0, 64], [256, 512], 512, 512), "band_plan: expected a ROCm device, got cpu (no CPU fallback)"),
]


@pytest.mark.parametrize("fault,args,message", BAND_ROWS, ids=[r[0] for r in BAND_ROWS])
def test_band_plan_refuses_with_the_exact_message(fault, args, message):
    with pytest.raises(ApexMIError) as e:
        ops.band_plan(*args, device="cpu")
    assert str(e.value) == message


def test_band_plan_takes_tensors_and_arrays_on_the_host_only():
    import numpy as np
    for lo, hi in ((torch.tensor([0, 64]), torch.tensor([256, 512])), (np.array([0, 64]), np.array([256, 512]))):
        with pytest.raises(ApexMIError, match="expected a ROCm device"):       # past every rule: only the device is missing
            ops.band_plan(lo, hi, 512, 512, device="cpu")
    with pytest.raises(ApexMIError) as e:
        ops.band_plan(torch.tensor([0.0, 64.0]), [256, 512], 512, 512, device="cpu")
    assert str(e.value) == "band_plan: lo must hold integers, got torch.float32"


def test_plan_check_refuses_a_mismatch():
    plan = _Plan([0, 64], [256, 512], 512, 512)
    plan.bands = torch.zeros(1, 2, 2, dtype=torch.int32)
    plan.check(512, 512, 5, torch.device("cpu"), "op")
    with pytest.raises(ApexMIError) as e:
        plan.check(512, 500, 5, torch.device("cpu"), "attention_band")
    assert str(e.value) == "attention_band: the band plan is for (Sq, Sk) = (512, 512), the operands have (512, 500)"
    plan.Hb = 3
    with pytest.raises(ApexMIError) as e:
        plan.check(512, 512, 5, torch.device("cpu"), "attention_band")
    assert str(e.value) == "attention_band: the band plan has bands for 3 heads, the operands have 5 (1 or H)"
    plan.check(512, 512, 3, torch.device("cpu"), "op")
    with pytest.raises(ApexMIError) as e:
        plan.check(512, 512, 3, torch.device("meta"), "attention_band")
    assert str(e.value) == "attention_band: the band plan is on cpu, the operands on meta"


def test_ops_refuse_cpu_tensors_and_foreign_plans():
    q = torch.zeros(1, 2, 512, 128, dtype=torch.bfloat16)
    with pytest.raises(ApexMIError, match="no CPU fallback"):
        ops.attention_band(q, q, q, None)
    with pytest.raises(ApexMIError, match="no CPU fallback"):
        ops.attention_prepared_band(q, q, q, q, 512, None)


# ---- the C entries ---------------------------------------------------------------------------------------------------------------
P = 0x100000
BIG = 1 << 30
O3 = (4096, 256, 128)
S3 = (1 << 20, 1 << 18, 128)
_PREPARED = dict(q=P, k=P, vt=P, out=P, B=1, H=2, Sq=8, Sk=8, Skp=64, os=O3, bands=P, Hb=1, scale=0.125, stream=None)
_STRIDED = dict(q=P, k=P, v=P, out=P, B=1, H=2, Sq=8, Sk=8, D=128, qs=S3, ks=S3, vs=S3, os=O3, bands=P, Hb=1, scale=0.125,
                dtype=lib.BF16, ws=P, wsb=BIG, stream=None)
ENTRIES = {"apexmi_attn_fwd_prepared_band": _PREPARED, "apexmi_attn_fwd_band": _STRIDED}
NEED = 2 * 128 * 64 * 2 + 2 * (8 + 8) * 128 * 2          # V^T + packed q and k of the default problem
_MANY = dict(B=1 << 16, H=1 << 15, Sq=128)
_PLAN_P = "attn_fwd_prepared_band: null or misaligned band plan (int32 pairs, 8-byte aligned)"
_PLAN_S = "attn_fwd_band: null or misaligned band plan (int32 pairs, 8-byte aligned)"
_OUT_S = "attn_fwd_band: out must be 16-byte aligned with strides multiples of 8 elements"

ROWS = [("apexmi_attn_fwd_prepared_band",) + r for r in [
    ("null q", dict(q=None), "attn_fwd_prepared_band: null operand"),
    ("null k", dict(k=None), "attn_fwd_prepared_band: null operand"),
    ("null vt", dict(vt=None), "attn_fwd_prepared_band: null operand"),
    ("null out", dict(out=None), "attn_fwd_prepared_band: null operand"),
    ("null out strides", dict(os=None), "attn_fwd_prepared_band: null operand"),
    ("B = 0", dict(B=0), "attn_fwd_prepared_band: empty problem"),
    ("H = 0", dict(H=0), "attn_fwd_prepared_band: empty problem"),
    ("Sq = 0", dict(Sq=0), "attn_fwd_prepared_band: empty problem"),
    ("Sk = -1", dict(Sk=-1), "attn_fwd_prepared_band: empty problem"),
    ("Skp = 100", dict(Skp=100), "attn_fwd_prepared_band: Skp=100 must be Sk=8 rounded up to 64"),
    ("Skp below Sk", dict(Sk=128, Skp=64), "attn_fwd_prepared_band: Skp=64 must be Sk=128 rounded up to 64"),
    ("q off by 8 bytes", dict(q=P + 8), "attn_fwd_prepared_band: operands must be 16-byte aligned"),
    ("k off by 8 bytes", dict(k=P + 8), "attn_fwd_prepared_band: operands must be 16-byte aligned"),
    ("vt off by 2 bytes", dict(vt=P + 2), "attn_fwd_prepared_band: operands must be 16-byte aligned"),
    ("out off by 8 bytes", dict(out=P + 8), "attn_fwd_prepared_band: operands must be 16-byte aligned"),
    ("out stride 68", dict(os=(4096, 256, 68)), "attn_fwd_prepared_band: output strides must be multiples of 8 elements"),
    ("out stride 4", dict(os=(4, 256, 128)), "attn_fwd_prepared_band: output strides must be multiples of 8 elements"),
    ("Sk above 2^20", dict(Sk=(1 << 20) + 1, Skp=(1 << 20) + 64), "attn_fwd_prepared_band: Sk=1048577 above 1048576 keys"),
    ("2^31 query blocks", _MANY, "attn_fwd_prepared_band: too many query blocks"),
    ("null plan", dict(bands=None), _PLAN_P),
    ("plan off by 4 bytes", dict(bands=P + 4), _PLAN_P),
    ("plan of 3 heads for 2", dict(Hb=3), "attn_fwd_prepared_band: plan of 3 heads for 2 heads (1 or H)"),
    ("plan of 0 heads", dict(Hb=0), "attn_fwd_prepared_band: plan of 0 heads for 2 heads (1 or H)"),
    ("null q, then B = 0", dict(q=None, B=0), "attn_fwd_prepared_band: null operand"),
    ("B = 0, then Skp = 100", dict(B=0, Skp=100), "attn_fwd_prepared_band: empty problem"),
    ("Skp = 100, then q off", dict(Skp=100, q=P + 8), "attn_fwd_prepared_band: Skp=100 must be Sk=8 rounded up to 64"),
    ("q off, then out stride 68", dict(q=P + 8, os=(4096, 256, 68)), "attn_fwd_prepared_band: operands must be 16-byte aligned"),
    ("2^31 query blocks, then null plan", dict(_MANY, bands=None), "attn_fwd_prepared_band: too many query blocks"),
    ("plan off, then plan of 3 heads", dict(bands=P + 4, Hb=3), _PLAN_P),
]] + [("apexmi_attn_fwd_band",) + r for r in [
    ("null q", dict(q=None), "attn_fwd_band: null operand"),
    ("null k", dict(k=None), "attn_fwd_band: null operand"),
    ("null v", dict(v=None), "attn_fwd_band: null operand"),
    ("null out", dict(out=None), "attn_fwd_band: null operand"),
    ("null q strides", dict(qs=None), "attn_fwd_band: null operand"),
    ("null k strides", dict(ks=None), "attn_fwd_band: null operand"),
    ("null v strides", dict(vs=None), "attn_fwd_band: null operand"),
    ("null out strides", dict(os=None), "attn_fwd_band: null operand"),
    ("B = 0", dict(B=0), "attn_fwd_band: empty problem (B=0 H=2 Sq=8 Sk=8)"),
    ("Sk = 0", dict(Sk=0), "attn_fwd_band: empty problem (B=1 H=2 Sq=8 Sk=0)"),
    ("D = 64", dict(D=64), "attn_fwd_band: head dim 64 unsupported (128 only: the band kernel is the D = 128 flash kernel)"),
    ("D = 256", dict(D=256), "attn_fwd_band: head dim 256 unsupported (128 only: the band kernel is the D = 128 flash kernel)"),
    ("dtype f16", dict(dtype=lib.F16), "attn_fwd_band: dtype 1 unsupported (bf16 only)"),
    ("dtype f32", dict(dtype=lib.F32), "attn_fwd_band: dtype 2 unsupported (bf16 only)"),
    ("key row stride 64", dict(ks=(1 << 20, 1 << 18, 64)), "attn_fwd_band: row strides below the head dim 128 (rows must not overlap)"),
    ("null workspace", dict(ws=None), f"attn_fwd_band: workspace too small or misaligned (1073741824 < {NEED})"),
    ("workspace of 16 bytes", dict(wsb=16), f"attn_fwd_band: workspace too small or misaligned (16 < {NEED})"),
    ("workspace off by 8 bytes", dict(ws=P + 8), f"attn_fwd_band: workspace too small or misaligned (1073741824 < {NEED})"),
    ("null plan", dict(bands=None), _PLAN_S),
    ("plan off by 4 bytes", dict(bands=P + 4), _PLAN_S),
    ("plan of 3 heads for 2", dict(Hb=3), "attn_fwd_band: plan of 3 heads for 2 heads (1 or H)"),
    ("out off by 8 bytes", dict(out=P + 8), _OUT_S),
    ("out stride 68", dict(os=(4096, 256, 68)), _OUT_S),
    ("Sk above 2^20", dict(Sk=(1 << 20) + 1, wsb=1 << 40), "attn_fwd_band: Sk=1048577 above 1048576 keys"),
    ("2^31 query blocks", dict(_MANY, wsb=1 << 62), "attn_fwd_band: too many query blocks"),
    ("null q, then B = 0", dict(q=None, B=0), "attn_fwd_band: null operand"),
    ("B = 0, then D = 64", dict(B=0, D=64), "attn_fwd_band: empty problem (B=0 H=2 Sq=8 Sk=8)"),
    ("D = 64, then dtype f32", dict(D=64, dtype=lib.F32), "attn_fwd_band: head dim 64 unsupported (128 only: the band kernel is the D = 128 flash kernel)"),
    ("dtype f32, then null workspace", dict(dtype=lib.F32, ws=None), "attn_fwd_band: dtype 2 unsupported (bf16 only)"),
    ("null workspace, then null plan", dict(ws=None, bands=None), f"attn_fwd_band: workspace too small or misaligned (1073741824 < {NEED})"),
    ("null plan, then out off", dict(bands=None, out=P + 8), _PLAN_S),
]]
_STRIDE_ARGS = ("qs", "ks", "vs", "os")


def _call(entry: str, overrides: dict):
    L = lib.load()
    args = dict(ENTRIES[entry], **overrides)
    assert set(args) == set(ENTRIES[entry])
    packed = [(lib.c_i64p._type_ * 3)(*v) if n in _STRIDE_ARGS and v is not None else v for n, v in args.items()]
    rc = getattr(L, entry)(*packed)
    return rc, L.apexmi_last_error().decode()


@pytest.mark.parametrize("entry,fault,overrides,message", ROWS, ids=[f"{r[0][12:]}: {r[1]}" for r in ROWS])
def test_entry_point_refuses_with_the_exact_message(entry, fault, overrides, message):
    rc, msg = _call(entry, overrides)
    assert rc != 0, fault
    assert msg == message


def test_workspace_bytes():
    L = lib.load()
    assert L.apexmi_attn_band_workspace_bytes(1, 2, 8, 8) == NEED
    assert L.apexmi_attn_band_workspace_bytes(2, 3, 700, 1000) == 2 * 3 * 128 * 1024 * 2 + 2 * 3 * 1700 * 128 * 2
    for args in ((0, 2, 8, 8), (1, 0, 8, 8), (1, 2, 0, 8), (1, 2, 8, -1)):
        assert L.apexmi_attn_band_workspace_bytes(*args) == 0


def test_header_signatures_and_exports_agree():
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES, name
    # the prepared entry: the arguments of apexmi_attn_fwd_prepared with (bands, Hb) between o_strides and the scale
    base, band = lib.SIGNATURES["apexmi_attn_fwd_prepared"][1], lib.SIGNATURES["apexmi_attn_fwd_prepared_band"][1]
    assert len(band) == len(base) + 2 == 14 and band[:10] == base[:10] and band[12:] == base[10:]
    # q, k, v, out | B, H, Sq, Sk, D | four stride triples | bands, Hb | scale, dtype | workspace, bytes, stream
    assert len(lib.SIGNATURES["apexmi_attn_fwd_band"][1]) == 4 + 5 + 4 + 2 + 2 + 3
    assert len(lib.SIGNATURES["apexmi_attn_band_workspace_bytes"][1]) == 4
    L = lib.load()
    assert all(hasattr(L, n) for n in SYMBOLS)
    nm = shutil.which("nm")
    if nm:
        exported = subprocess.run([nm, "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in SYMBOLS:
            assert re.search(r"\bT %s$" % name, exported, re.M), name


def test_build_refuses_a_band_kernel_that_spills_or_has_no_remark():
    from apex_studio_amd import build
    assert "attn_fwd_d128_w64_band_kernel" in build.NO_SPILL["attention.hip"]
    assert not any(s in "attn_fwd_d128_w64_band_kernel" for s in ("attn_fwd_d128_w64_kernel", "attn_fwd_d128_w64r_kernel"))

    def remark(name, scratch=0):
        loc = "./attn_w64_kernel.h:26:1: remark:"
        return (f"{loc} Function Name: _ZN12_GLOBAL__N_1{len(name)}{name}EPKtS1_S1_Ptiiiiiilllf [-Rpass-analysis=kernel-resource-usage]\n"
                + "".join(f"{loc}     {field}: {val} [-Rpass-analysis=kernel-resource-usage]\n" for field, val in
                          (("VGPRs", 256), ("AGPRs", 224), ("ScratchSize [bytes/lane]", scratch), ("SGPRs Spill", 0), ("VGPRs Spill", 0))))

    two = remark("attn_fwd_d128_w64_kernel") + remark("attn_fwd_d128_w64r_kernel")
    build.check_no_spill("attention.hip", two + remark("attn_fwd_d128_w64_band_kernel"), complete=True)
    with pytest.raises(RuntimeError, match="attn_fwd_d128_w64_band_kernel.*must not spill"):
        build.check_no_spill("attention.hip", two + remark("attn_fwd_d128_w64_band_kernel", scratch=16), complete=True)
    with pytest.raises(RuntimeError, match="must not spill"):
        build.check_no_spill("attention.hip", two + remark("attn_fwd_d128_w64_band_kernel", scratch=16))
    # a build hands over the remarks of the whole translation unit: a listed kernel without one is refused
    with pytest.raises(RuntimeError, match="no resource remark for kernel 'attn_fwd_d128_w64_band_kernel'"):
        build.check_no_spill("attention.hip", two, complete=True)
    with pytest.raises(RuntimeError, match="no resource remark"):
        build.check_no_spill("attention.hip", "")


# ---- backend key, Wan and engine switches ------------------------------------------------------------------------------------------
def test_the_key_is_registered_on_request_and_disturbs_nothing():
    from apex_studio_amd.register import FunctionRegister
    reg = FunctionRegister()
    ab.register(reg, set_default=True, band=True)
    assert ab.KEY_BAND == "hip_mfma_band" and reg.get(ab.KEY_BAND) is ab.hip_mfma_band
    assert reg.get_default() == ab.KEY and reg.is_available(ab.KEY_BAND) == reg.is_available(ab.KEY)
    assert sorted(reg) == sorted((ab.KEY, ab.KEY_SDPA, ab.KEY_WINDOW, ab.KEY_BAND))
    reg2 = FunctionRegister()
    ab.register(reg2)
    assert sorted(reg2) == sorted((ab.KEY, ab.KEY_SDPA, ab.KEY_WINDOW))
    reg3 = FunctionRegister()
    ab.register(reg3, varlen=True, band=True)
    assert sorted(reg3) == sorted((ab.KEY, ab.KEY_SDPA, ab.KEY_WINDOW, ab.KEY_VARLEN, ab.KEY_BAND))


def test_backend_refuses_what_it_does_not_do():
    q = torch.zeros(1, 2, 512, 128, dtype=torch.bfloat16)
    plan = object()
    for kw, msg in ((dict(dropout_p=0.1, band_plan=plan), "hip_mfma_band: dropout is not supported (inference only)"),
                    (dict(is_causal=True, band_plan=plan), "hip_mfma_band: causal attention is not supported (use hip_mfma_sdpa)"),
                    (dict(attn_mask=torch.ones(512, 512, dtype=torch.bool), band_plan=plan),
                     "hip_mfma_band: attn_mask is not supported next to a band plan (use hip_mfma_sdpa with a mask)"),
                    (dict(), "hip_mfma_band: band_plan= (ops.band_plan(...) / ops.frame_band_plan(...)) is required; there is no "
                             "dense fallback")):
        with pytest.raises(ApexMIError) as e:
            ab.hip_mfma_band(q, q, q, **kw)
        assert str(e.value) == msg


WAN = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=512, num_layers=1, cross_attn_norm=True, eps=1e-6)


def test_wan_switch_validates_caches_and_excludes_the_window(monkeypatch):
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**WAN, device="meta")
    assert m._attention_band is None and m._band_plans == {}
    for bad in (-1, 1.5, (1, 2, 3), True):
        with pytest.raises(ValueError, match="band radius"):
            m.set_attention_band(bad)
    built = []

    def fake_plan(frames, tokens_per_frame, radius, device=None):
        built.append((frames, tokens_per_frame, radius))
        return ("plan", len(built))

    monkeypatch.setattr(ops, "frame_band_plan", fake_plan)
    assert m.set_attention_band(2) is m and m._attention_band == 2
    p = m._band_plan((3, 4, 5))
    assert m._band_plan((3, 4, 5)) is p and built == [(3, 20, 2)]              # cached per (grid, radius); frame-major grid
    assert m._band_plan((3, 4, 6)) is not p and built[-1] == (3, 24, 2)
    m.set_attention_band(0)
    assert m._band_plans == {} and m._attention_band == 0                       # radius 0 is a band, not "off"
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.set_attention_window((1, 2, 3))
    assert m._attention_window is None
    m.set_attention_band(None)
    m.set_attention_window((1, 2, 3))
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.set_attention_band(1)
    assert m._attention_band is None
    m.set_attention_band(None)                                                  # clearing is always allowed
    m.set_attention_window(None)
    m._band_plans = {"k": 1}
    m._invalidate("moved")
    assert m._band_plans == {}


class _Tr:
    def __init__(self):
        self.config = type("C", (), {"out_channels": 16, "in_channels": 16})()
        self.band = "unset"

    def set_attention_band(self, frames):
        self.band = frames


@pytest.mark.parametrize("engine", ["t2v", "i2v"])
def test_engines_forward_the_band_to_both_experts(engine):
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    cls = WanT2VEngine if engine == "t2v" else WanI2VEngine
    hi, lo = _Tr(), _Tr()
    e = cls(hi, lo, attention_band=2)
    assert e.attention_band == 2 and hi.band == 2 and lo.band == 2
    hi, lo = _Tr(), _Tr()
    e = cls(hi, lo)
    assert e.attention_band is None and hi.band == "unset" and lo.band == "unset"
    one = _Tr()
    e = cls(one, attention_band=0)
    assert one.band == 0 and e.low_noise_transformer is one
