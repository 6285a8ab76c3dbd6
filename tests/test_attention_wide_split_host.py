"""Host side of the wide-head attention's key splits and log-sum-exp (apexmi_attn_fwd_wide_split, ops.attention_wide's
key_splits / return_lse, the VAEs' set_mid_attention(mode, key_splits)): no GPU.  The header, the ctypes table and the built
library agree, the pure split rule holds its properties, the workspace grows by the partials and nothing else, the wrappers
refuse before any device work, and the tile-range formulas of the kernel have one float64-free restatement here: over the
frame cases of the GPU test, the splits of every query block partition exactly the keys the rule allows."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.test_attention_wide_host import _FakeCuda, frame_allowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("apexmi_attn_wide_auto_splits", "apexmi_attn_wide_split_workspace_bytes", "apexmi_attn_fwd_wide_split")
QB, KV = 128, 64
# (name, Sq, Sk, frame_tokens): the cases of tests/test_gpu_attention_wide_split.py
CASES = (("plain 1021", 129, 1021, 0), ("plain 7", 33, 7, 0), ("frames 48x5", 240, 240, 48), ("frames 160x3", 480, 480, 160))


def _lib():
    from apex_studio_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        from apex_studio_amd import build
        build.build(verbose=False)
    return lib.load()


def test_header_signatures_and_library_carry_the_symbols():
    from apex_studio_amd import lib
    _lib()
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES, name
    # the arguments of apexmi_attn_fwd_wide up to frame_tokens | lse, lse strides, key_splits | workspace, bytes, stream
    assert len(lib.SIGNATURES["apexmi_attn_fwd_wide_split"][1]) == len(lib.SIGNATURES["apexmi_attn_fwd_wide"][1]) + 3 == 22
    assert lib.SIGNATURES["apexmi_attn_fwd_wide_split"][1][:16] == lib.SIGNATURES["apexmi_attn_fwd_wide"][1][:16]
    assert len(lib.SIGNATURES["apexmi_attn_wide_split_workspace_bytes"][1]) == 6
    assert len(lib.SIGNATURES["apexmi_attn_wide_auto_splits"][1]) == 3
    nm = shutil.which("nm")
    if nm:
        exported = subprocess.run([nm, "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        for name in SYMBOLS:
            assert re.search(r"\bT %s$" % name, exported, re.M), name
        assert "attn_merge_f32" not in exported          # the partial merge is an internal launch, not an entry point
    else:
        raw = C.CDLL(lib.LIB_PATH)
        for name in SYMBOLS:
            assert getattr(raw, name)


def test_auto_splits_properties():
    L = _lib()
    f = L.apexmi_attn_wide_auto_splits
    for cus in (1, 8, 64, 256, 304):
        for tiles in (1, 2, 3, 4, 7, 8, 16, 31, 32, 64, 256, 4096):
            prev = None
            for units in list(range(1, 40)) + [cus - 1, cus, cus + 1, 2 * cus, 100000]:
                if units < 1:
                    continue
                n = f(units, tiles, cus)
                assert 1 <= n <= 8, (units, tiles, cus, n)
                assert n <= tiles, (units, tiles, cus, n)
                if units >= cus or tiles == 1:
                    assert n == 1, (units, tiles, cus, n)
            for units in range(1, 2 * cus + 2):           # non-increasing in units at fixed tiles
                n = f(units, tiles, cus)
                assert prev is None or n <= prev, (units, tiles, cus, n, prev)
                prev = n
    # it does split somewhere: the rule is not the constant 1 (one unit, many tiles, a whole device)
    assert f(1, 64, 256) > 1
    for bad in ((0, 16, 256), (4, 0, 256), (4, 16, 0), (-1, 16, 256)):
        assert f(*bad) == 1, bad


def test_split_workspace_is_vt_plus_partials():
    L = _lib()
    old, new = L.apexmi_attn_wide_workspace_bytes, L.apexmi_attn_wide_split_workspace_bytes
    for B, H, Sq, Sk, D in ((1, 1, 129, 1021, 512), (3, 2, 240, 240, 384), (2, 1, 33, 7, 256), (1, 1, 4096, 4096, 512)):
        assert new(B, H, Sq, Sk, D, 1) == old(B, H, Sk, D) > 0
        for n in range(2, 9):   # the header states no padding: f32 partials [n,B,Sq,H,D] and lses [n,B,H,Sq] right behind V^T
            assert new(B, H, Sq, Sk, D, n) == old(B, H, Sk, D) + n * B * Sq * H * D * 4 + n * B * H * Sq * 4, (B, H, Sq, Sk, D, n)
    for D in (64, 128, 320, 640, 1024):
        assert new(1, 1, 64, 64, D, 2) == 0, D
    for n in (-1, 0, 9, 100):
        assert new(1, 1, 64, 64, 256, n) == 0, n
    for bad in ((0, 1, 64, 64, 256, 2), (1, 0, 64, 64, 256, 2), (1, 1, 0, 64, 256, 2), (1, 1, 64, 0, 256, 2)):
        assert new(*bad) == 0, bad


def test_split_entry_point_refuses():
    L = _lib()
    from apex_studio_amd import lib
    P = C.c_void_p(4096)
    i3, odd = lib.i64x3((4096, 4096, 512)), lib.i64x3((4096, 4096, 513))

    def bad(rc, text):
        assert rc != 0
        msg = L.apexmi_last_error().decode()
        assert text in msg, msg

    def call(q=P, B=1, H=1, Sq=64, Sk=64, D=512, qs=i3, ks=i3, dtype=lib.BF16, ft=0, lse=None, ls=None, n=1, ws=P, wsb=1 << 30):
        return L.apexmi_attn_fwd_wide_split(q, P, P, P, B, H, Sq, Sk, D, qs, ks, i3, i3, 1.0, dtype, ft, lse, ls, n, ws, wsb, None)

    # what is new
    bad(call(n=-1), "key_splits=-1")
    bad(call(n=9), "key_splits=9")
    bad(call(lse=P, ls=None), "lse without strides")
    bad(call(lse=C.c_void_p(4098), ls=i3), "misaligned")
    for n in (1, 2, 8):
        need = L.apexmi_attn_wide_split_workspace_bytes(1, 1, 64, 64, 512, n)
        bad(call(n=n, wsb=need - 1), "workspace too small")
    bad(call(B=1 << 15, H=1 << 14, Sq=128, n=4, wsb=1 << 62), "too many workgroups")          # 2^29 units x 4
    # every message of the old entry point, under the new name
    bad(call(q=None), "null operand")
    bad(call(Sq=0), "empty problem")
    for D in (64, 128, 320, 640, 1024):
        bad(call(D=D), "unsupported (256, 384 or 512")
    bad(call(D=1024), "materialised path")
    bad(call(dtype=lib.F32), "dtype")
    bad(call(qs=odd), "16-byte aligned")
    bad(call(ks=lib.i64x3((4096, 4096, 256))), "key row stride 256 below the head dim 512")
    bad(call(Sk=1 << 22, ks=lib.i64x3((0, 0, 512))), "4 GiB")
    bad(call(Sq=100, Sk=100, ft=30), "whole number of frames")
    bad(call(Sq=64, Sk=128, ft=32), "Sq == Sk")
    bad(call(ws=None), "workspace")
    bad(call(wsb=1024), "workspace too small")
    bad(call(B=1 << 16, H=1 << 15, Sq=128), "too many query blocks")
    assert "attn_fwd_wide_split" in L.apexmi_last_error().decode()


def test_op_refuses_bad_key_splits_before_any_device_work():
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    x = torch.zeros(1, 1, 64, 256, dtype=torch.bfloat16)
    with pytest.raises(ApexMIError, match="no CPU fallback"):          # still the first refusal
        ops.attention_wide(x, x, x, key_splits=9, return_lse=True)
    dev = _FakeCuda(torch.empty(1, 1, 64, 256, dtype=torch.bfloat16, device="meta"))
    for ks in (0, 9, "Auto", -1, 2.0, True, None):
        with pytest.raises(ApexMIError, match="key_splits"):
            ops.attention_wide(dev, dev, dev, key_splits=ks)
    # the existing checks come first
    with pytest.raises(ApexMIError, match="head dim 128 unsupported"):
        ops.attention_wide(*(_FakeCuda(torch.empty(1, 1, 64, 128, dtype=torch.bfloat16, device="meta")),) * 3, key_splits=9)
    # wide heads in attention_chunked: no masks, no grouped-query heads
    kv = _FakeCuda(torch.empty(1, 1, 64, 256, dtype=torch.bfloat16, device="meta"))
    q2 = _FakeCuda(torch.empty(1, 2, 64, 256, dtype=torch.bfloat16, device="meta"))
    with pytest.raises(ApexMIError, match="no masks"):
        ops.attention_chunked(dev, [kv], [kv], [torch.ones(64, 64, dtype=torch.bool)])
    with pytest.raises(ApexMIError, match="grouped-query"):
        ops.attention_chunked(q2, [kv], [kv], enable_gqa=True)
    with pytest.raises(ApexMIError, match="grouped-query"):
        ops.attention_chunked(q2, [kv], [kv])


@pytest.mark.parametrize("which", ["wan", "flux", "hunyuan15"])
def test_setters_take_key_splits(which):
    if which == "wan":
        from apex_studio_amd.vae_wan import AutoencoderKLWan
        make = lambda w: AutoencoderKLWan(base_dim=w // 4, z_dim=4, dim_mult=[1, 2, 4, 4], num_res_blocks=1,
                                          temperal_downsample=[False, True, True], device="meta")
    elif which == "flux":
        from apex_studio_amd.vae_flux import AutoencoderKL
        make = lambda w: AutoencoderKL(latent_channels=4, block_out_channels=(32, 32, w, w), layers_per_block=1, device="meta")
    else:
        from apex_studio_amd.vae_hunyuan15 import AutoencoderKLHunyuanVideo15
        make = lambda w: AutoencoderKLHunyuanVideo15(latent_channels=4, block_out_channels=(32, 32, w // 2, w, w),
                                                     layers_per_block=1, device="meta")
    from apex_studio_amd.module_base import MID_ATTENTION_MODES
    assert MID_ATTENTION_MODES == ("materialised", "flash")
    vae = make(256)
    assert vae.mid_attention_key_splits == 1
    with pytest.raises(ValueError, match="key_splits"):
        vae.set_mid_attention("materialised", key_splits=2)
    with pytest.raises(ValueError, match="key_splits"):
        vae.set_mid_attention("materialised", key_splits="auto")
    for ks in (9, 0, "Auto", 2.0, True):
        with pytest.raises(ValueError, match="key_splits"):
            vae.set_mid_attention("flash", key_splits=ks)
    assert vae.mid_attention == "materialised" and vae.mid_attention_key_splits == 1      # a refused call changes nothing
    assert vae.set_mid_attention("flash") is vae and vae.mid_attention_key_splits == 1
    assert vae.set_mid_attention("flash", key_splits="auto").mid_attention_key_splits == "auto"
    assert vae.set_mid_attention("flash", key_splits=4).mid_attention_key_splits == 4
    other = make(256)
    assert other.mid_attention == "materialised" and other.mid_attention_key_splits == 1    # per object
    assert vae.set_mid_attention("flash").mid_attention_key_splits == 1                     # the default again
    assert vae.set_mid_attention("materialised", key_splits=1).mid_attention_key_splits == 1


def split_ranges(t_end: int, n: int):
    """[(t_beg, t_lim)] of the n splits of a unit with t_end key tiles: the kernel's formulas"""
    per = -(-t_end // n)
    out = []
    for s in range(n):
        t_beg = min(s * per, t_end)
        out.append((t_beg, min(t_beg + per, t_end)))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_split_rule_partitions_the_allowed_keys(case, n):
    """Per (query block, split): the keys a row sees are those of the split's tiles that lie below Sk and, under the frame rule,
    at or below the row's frame end.  Their union over the splits is exactly the rule, and no two splits share a key."""
    _, Sq, Sk, ft = case
    allowed = frame_allowed(Sq, ft) if ft else torch.ones(Sq, Sk, dtype=torch.bool)
    seen = torch.zeros(Sq, Sk, dtype=torch.int64)
    some_empty = False
    for qb in range(-(-Sq // QB)):
        q0 = qb * QB
        rows = torch.arange(q0, min(q0 + QB, Sq))
        k_end = (min(q0 + QB - 1, Sq - 1) // ft + 1) * ft if ft else Sk
        t_end = -(-k_end // KV)
        lim = (rows // ft + 1) * ft - 1 if ft else torch.full_like(rows, Sk - 1)
        ranges = split_ranges(t_end, n)
        assert ranges[0][0] == 0 and max(r[1] for r in ranges) == t_end
        for t_beg, t_lim in ranges:
            some_empty |= t_beg == t_lim
            keys = torch.arange(t_beg * KV, max(t_beg * KV, min(t_lim * KV, Sk)))      # none for an empty range
            see = keys[None, :] <= lim[:, None]
            seen[rows[:, None], keys[None, :]] += see.long()
    assert int(seen.max()) <= 1                      # no key twice
    assert torch.equal(seen == 1, allowed)           # and exactly the rule
    if case[0] == "plain 7" and n > 1:
        assert some_empty                            # one tile: every split but the first is empty
