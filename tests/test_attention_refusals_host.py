"""The refusals of the one-launch flash entry points, string for string (no GPU): every argument check of apexmi_attn_fwd_masked,
apexmi_attn_fwd_masked_lse, apexmi_attn_fwd_window, apexmi_attn_fwd_prepared_window, apexmi_attn_fwd_varlen, apexmi_attn_fwd_wide and
apexmi_attn_fwd_wide_split that is reachable before the first launch, with the complete apexmi_last_error() text, and rows with two
faults that pin which of the two is reported, i.e. the order of the checks.  The same for ops.attention_varlen, whose refusals
(all but the last, the device) are reachable on CPU tensors.  The literals are what the library printed before the entry points
shared one host-side front end (csrc/attn_host.h): they are the reference, not the code under test.  The operands are fake
non-null addresses; every row returns before anything is launched or read."""
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError

P = 0x100000                       # a 16-byte aligned non-null "device address"
S3, O3 = (4096, 512, 64), (4096, 256, 64)
W3 = (1 << 20, 1 << 20, 512)       # wide heads: a row of 512 elements
S2, L2 = (512, 128), (406, 1)
BIG = 1 << 30
TOO_LONG = (1 << 20) + 1           # one key more than 2^14 tiles of 64

# argument name -> default, in the order of the C signature (include/apexmi.h); a row overrides some of them
_MASKED = dict(q=P, k=P, v=P, out=P, B=1, Hq=4, Hkv=2, Sq=8, Sk=8, D=64, qs=S3, ks=S3, vs=S3, os=O3, mask=None, mask_dtype=-1,
               ms=None, causal=0, scale=0.125, dtype=lib.BF16, ws=P, wsb=BIG, stream=None)
_MASKED_LSE = dict(q=P, k=P, v=P, out=P, lse=P, B=1, Hq=4, Hkv=2, Sq=8, Sk=8, D=64, qs=S3, ks=S3, vs=S3, os=O3, ls=(32, 8, 1),
                   mask=None, mask_dtype=-1, ms=None, causal=0, scale=0.125, dtype=lib.BF16, ws=P, wsb=BIG, stream=None)
_WINDOW = dict(q=P, k=P, v=P, out=P, B=1, Hq=4, Hkv=2, Sq=8, Sk=8, D=64, qs=S3, ks=S3, vs=S3, os=O3, qc=P, kc=P, r0=1, r1=1, r2=1,
               map=P, scale=0.125, dtype=lib.BF16, ws=P, wsb=BIG, stream=None)
_PREPARED_WINDOW = dict(q=P, k=P, vt=P, out=P, B=1, H=2, Sq=8, Sk=8, Skp=64, os=O3, qc=P, kc=P, r0=1, r1=1, r2=1, map=P, scale=0.125,
                        stream=None)
_VARLEN = dict(q=P, k=P, v=P, out=P, lse=P, cu_q=P, cu_k=P, n=5, Tq=406, Tk=531, Hq=4, Hkv=2, D=128, mq=200, mk=333, qs=S2, ks=S2,
               vs=S2, os=S2, ls=L2, causal=0, scale=0.1, dtype=lib.BF16, ws=P, wsb=BIG, stream=None)
_WIDE = dict(q=P, k=P, v=P, out=P, B=1, H=1, Sq=64, Sk=64, D=512, qs=W3, ks=W3, vs=W3, os=W3, scale=1.0, dtype=lib.BF16, ft=0, ws=P,
             wsb=BIG, stream=None)
_WIDE_SPLIT = dict(q=P, k=P, v=P, out=P, B=1, H=1, Sq=64, Sk=64, D=512, qs=W3, ks=W3, vs=W3, os=W3, scale=1.0, dtype=lib.BF16, ft=0,
                   lse=None, ls=None, n=1, ws=P, wsb=BIG, stream=None)
ENTRIES = {"apexmi_attn_fwd_masked": _MASKED, "apexmi_attn_fwd_masked_lse": _MASKED_LSE, "apexmi_attn_fwd_window": _WINDOW,
           "apexmi_attn_fwd_prepared_window": _PREPARED_WINDOW, "apexmi_attn_fwd_varlen": _VARLEN, "apexmi_attn_fwd_wide": _WIDE,
           "apexmi_attn_fwd_wide_split": _WIDE_SPLIT}
_STRIDES = {"qs": 3, "ks": 3, "vs": 3, "os": 3, "ls": 3, "ms": 4}
_MANY_BLOCKS = dict(B=1 << 16, Hq=1 << 15, Hkv=1 << 15, Sq=128)       # 2^31 query blocks


def call(entry: str, overrides: dict):
    """(rc, apexmi_last_error()) of one call of `entry` with its defaults and the row's overrides"""
    L = lib.load()
    args = dict(ENTRIES[entry], **overrides)
    assert set(args) == set(ENTRIES[entry]), sorted(set(overrides) - set(ENTRIES[entry]))
    packed = []
    for name in ENTRIES[entry]:                      # dicts keep the signature's order
        val = args[name]
        if name in _STRIDES and val is not None:
            val = (lib.c_i64p._type_ * len(val))(*val)
        packed.append(val)
    rc = getattr(L, entry)(*packed)
    return rc, L.apexmi_last_error().decode()


def _sdpa(e: str, need: int):
    """(fault, overrides, message) rows shared by the masked, masked_lse and window entries: `e` is the message prefix, `need`
    the workspace of the default problem (V^T, and the block map of the entries that take a mask)"""
    return [
        ("null q", dict(q=None), f"{e}: null operand"),
        ("null k", dict(k=None), f"{e}: null operand"),
        ("null v", dict(v=None), f"{e}: null operand"),
        ("null out", dict(out=None), f"{e}: null operand"),
        ("null q strides", dict(qs=None), f"{e}: null operand"),
        ("null k strides", dict(ks=None), f"{e}: null operand"),
        ("null v strides", dict(vs=None), f"{e}: null operand"),
        ("null out strides", dict(os=None), f"{e}: null operand"),
        ("B = 0", dict(B=0), f"{e}: empty problem (B=0 Hq=4 Hkv=2 Sq=8 Sk=8)"),
        ("Hq = 0", dict(Hq=0), f"{e}: empty problem (B=1 Hq=0 Hkv=2 Sq=8 Sk=8)"),
        ("Hkv = 0", dict(Hkv=0), f"{e}: empty problem (B=1 Hq=4 Hkv=0 Sq=8 Sk=8)"),
        ("Sq = 0", dict(Sq=0), f"{e}: empty problem (B=1 Hq=4 Hkv=2 Sq=0 Sk=8)"),
        ("Sk = -1", dict(Sk=-1), f"{e}: empty problem (B=1 Hq=4 Hkv=2 Sq=8 Sk=-1)"),
        ("D = 80", dict(D=80), f"{e}: head dim 80 unsupported (64 or 128)"),
        ("D = 256", dict(D=256), f"{e}: head dim 256 unsupported (64 or 128)"),
        ("dtype f32", dict(dtype=lib.F32), f"{e}: dtype 2 unsupported (bf16 or f16)"),
        ("ratio 4 / 3", dict(Hkv=3), f"{e}: head ratio Hq=4 / Hkv=3 is not whole"),
        ("Sk above 2^20", dict(Sk=TOO_LONG), f"{e}: Sk=1048577 above 1048576 keys"),
        ("2^31 query blocks", _MANY_BLOCKS, f"{e}: too many query blocks"),
        ("q off by 8 bytes", dict(q=P + 8), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("k off by 8 bytes", dict(k=P + 8), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("v off by 2 bytes", dict(v=P + 2), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("out off by 4 bytes", dict(out=P + 4), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("q stride 100", dict(qs=(4096, 512, 100)), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("k stride 4", dict(ks=(4096, 4, 64)), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("v stride 12", dict(vs=(12, 512, 64)), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("out stride 66", dict(os=(4096, 256, 66)), f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
        ("null workspace", dict(ws=None), f"{e}: workspace too small (1073741824 < {need})"),
        ("workspace of 16 bytes", dict(wsb=16), f"{e}: workspace too small (16 < {need})"),
        # two faults: the first of the entry's order is the one reported
        ("null q, then B = 0", dict(q=None, B=0), f"{e}: null operand"),
        ("B = 0, then D = 80", dict(B=0, D=80), f"{e}: empty problem (B=0 Hq=4 Hkv=2 Sq=8 Sk=8)"),
        ("D = 80, then dtype f32", dict(D=80, dtype=lib.F32), f"{e}: head dim 80 unsupported (64 or 128)"),
        ("dtype f32, then ratio", dict(dtype=lib.F32, Hkv=3), f"{e}: dtype 2 unsupported (bf16 or f16)"),
        ("ratio, then Sk above 2^20", dict(Hkv=3, Sk=TOO_LONG), f"{e}: head ratio Hq=4 / Hkv=3 is not whole"),
        ("2^31 query blocks, then q off", dict(_MANY_BLOCKS, q=P + 8), f"{e}: too many query blocks"),
        ("q off, then null workspace", dict(q=P + 8, ws=None),
         f"{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"),
    ]


def _mask(e: str):
    return [
        ("mask dtype code 7", dict(mask=P, mask_dtype=7, ms=(0, 0, 8, 1)), f"{e}: mask dtype code 7 unsupported (bool, f32, bf16, f16)"),
        ("mask without strides", dict(mask=P, mask_dtype=lib.MASK_BOOL), f"{e}: mask dtype code 3 unsupported (bool, f32, bf16, f16)"),
        ("mask key stride 2", dict(mask=P, mask_dtype=lib.F32, ms=(0, 0, 16, 2)), f"{e}: mask key stride 2 must be 0 or 1"),
        ("ratio, then mask dtype", dict(Hkv=3, mask=P, mask_dtype=7, ms=(0, 0, 8, 1)), f"{e}: head ratio Hq=4 / Hkv=3 is not whole"),
        ("mask dtype, then mask key stride", dict(mask=P, mask_dtype=7, ms=(0, 0, 16, 2)), f"{e}: mask dtype code 7 unsupported (bool, f32, bf16, f16)"),
        ("mask key stride, then Sk above 2^20", dict(mask=P, mask_dtype=lib.F32, ms=(0, 0, 16, 2), Sk=TOO_LONG), f"{e}: mask key stride 2 must be 0 or 1"),
    ]


def _window(e: str):
    """the window operands, checked after everything else (window_args)"""
    return [
        ("null q coordinates", dict(qc=None), f"{e}: null window operand (coordinates / block map)"),
        ("null k coordinates", dict(kc=None), f"{e}: null window operand (coordinates / block map)"),
        ("null block map", dict(map=None), f"{e}: null window operand (coordinates / block map)"),
        ("q coordinates off by 4 bytes", dict(qc=P + 4), f"{e}: coordinate records must be 8-byte aligned"),
        ("k coordinates off by 2 bytes", dict(kc=P + 2), f"{e}: coordinate records must be 8-byte aligned"),
        ("radius -1", dict(r1=-1), f"{e}: negative radius (1, -1, 1)"),
        ("null block map, then radius -1", dict(map=None, r2=-1), f"{e}: null window operand (coordinates / block map)"),
        ("coordinates off, then radius -1", dict(kc=P + 2, r0=-5), f"{e}: coordinate records must be 8-byte aligned"),
    ]


_AL_V = "attn_fwd_varlen: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"
_AL_W = "{e}: q / k / v rows must be 16-byte aligned (strides multiples of 8 elements)"


def _wide(e: str):
    al = _AL_W.format(e=e)
    return [
        ("null q", dict(q=None), f"{e}: null operand"),
        ("null k", dict(k=None), f"{e}: null operand"),
        ("null v", dict(v=None), f"{e}: null operand"),
        ("null out", dict(out=None), f"{e}: null operand"),
        ("null q strides", dict(qs=None), f"{e}: null operand"),
        ("null k strides", dict(ks=None), f"{e}: null operand"),
        ("null v strides", dict(vs=None), f"{e}: null operand"),
        ("null out strides", dict(os=None), f"{e}: null operand"),
        ("B = 0", dict(B=0), f"{e}: empty problem (B=0 H=1 Sq=64 Sk=64)"),
        ("H = 0", dict(H=0), f"{e}: empty problem (B=1 H=0 Sq=64 Sk=64)"),
        ("Sq = 0", dict(Sq=0), f"{e}: empty problem (B=1 H=1 Sq=0 Sk=64)"),
        ("Sk = 0", dict(Sk=0), f"{e}: empty problem (B=1 H=1 Sq=64 Sk=0)"),
        ("D = 128", dict(D=128), f"{e}: head dim 128 unsupported (256, 384 or 512; wider heads stay on apexmi_attn_fwd's materialised path)"),
        ("D = 320", dict(D=320), f"{e}: head dim 320 unsupported (256, 384 or 512; wider heads stay on apexmi_attn_fwd's materialised path)"),
        ("dtype f32", dict(dtype=lib.F32), f"{e}: dtype 2 unsupported (bf16 or f16)"),
        ("frame_tokens -1", dict(ft=-1), f"{e}: negative frame_tokens -1"),
        ("frames of 30 in 100", dict(Sq=100, Sk=100, ft=30), f"{e}: the frame rule needs Sq == Sk and a whole number of frames of 30 tokens (Sq=100 Sk=100)"),
        ("frames with Sq != Sk", dict(Sq=64, Sk=128, ft=32), f"{e}: the frame rule needs Sq == Sk and a whole number of frames of 32 tokens (Sq=64 Sk=128)"),
        ("2^31 query blocks", dict(B=1 << 16, H=1 << 15, Sq=128), f"{e}: too many query blocks"),
        ("key row stride 256", dict(ks=(1 << 20, 1 << 20, 256)), f"{e}: key row stride 256 below the head dim 512 (rows must not overlap)"),
        ("keys span 4 GiB", dict(Sk=1 << 22, ks=(0, 0, 512)), f"{e}: the keys of one (batch, head) span 4 GiB or more (Sk=4194304, row stride 512)"),
        ("q off by 8 bytes", dict(q=P + 8), al),
        ("k off by 8 bytes", dict(k=P + 8), al),
        ("v off by 2 bytes", dict(v=P + 2), al),
        ("out off by 4 bytes", dict(out=P + 4), al),
        ("q stride 513", dict(qs=(1 << 20, 1 << 20, 513)), al),
        ("k stride 516", dict(ks=(1 << 20, 1 << 20, 516)), al),
        ("v stride 4", dict(vs=(1 << 20, 4, 512)), al),
        ("out stride 514", dict(os=(1 << 20, 514, 512)), al),
        ("null workspace", dict(ws=None), f"{e}: workspace too small or misaligned (1073741824 < 65536)"),
        ("workspace of 1024 bytes", dict(wsb=1024), f"{e}: workspace too small or misaligned (1024 < 65536)"),
        ("workspace off by 8 bytes", dict(ws=P + 8), f"{e}: workspace too small or misaligned (1073741824 < 65536)"),
        ("null q, then B = 0", dict(q=None, B=0), f"{e}: null operand"),
        ("B = 0, then D = 128", dict(B=0, D=128), f"{e}: empty problem (B=0 H=1 Sq=64 Sk=64)"),
        ("D = 128, then dtype f32", dict(D=128, dtype=lib.F32), f"{e}: head dim 128 unsupported (256, 384 or 512; wider heads stay on apexmi_attn_fwd's materialised path)"),
        ("dtype f32, then frame_tokens -1", dict(dtype=lib.F32, ft=-1), f"{e}: dtype 2 unsupported (bf16 or f16)"),
        ("frames of 30 in 100, then key row stride", dict(Sq=100, Sk=100, ft=30, ks=(1 << 20, 1 << 20, 256)), f"{e}: the frame rule needs Sq == Sk and a whole number of frames of 30 tokens (Sq=100 Sk=100)"),
        ("key row stride 256, then q off", dict(ks=(1 << 20, 1 << 20, 256), q=P + 8), f"{e}: key row stride 256 below the head dim 512 (rows must not overlap)"),
        ("q off, then null workspace", dict(q=P + 8, ws=None), al),
    ]


ROWS = (
    [("apexmi_attn_fwd_masked",) + r for r in _sdpa("attn_fwd_masked", 16640) + _mask("attn_fwd_masked")]
    + [("apexmi_attn_fwd_masked_lse",) + r for r in _sdpa("attn_fwd_masked_lse", 16640) + _mask("attn_fwd_masked_lse") + [
        ("null lse", dict(lse=None), "attn_fwd_masked_lse: null or misaligned lse operand"),
        ("null lse strides", dict(ls=None), "attn_fwd_masked_lse: null or misaligned lse operand"),
        ("lse off by 2 bytes", dict(lse=P + 2), "attn_fwd_masked_lse: null or misaligned lse operand"),
        ("null q, then null lse", dict(q=None, lse=None), "attn_fwd_masked_lse: null operand"),
        ("null lse, then B = 0", dict(lse=None, B=0), "attn_fwd_masked_lse: null or misaligned lse operand"),
    ]]
    + [("apexmi_attn_fwd_window",) + r for r in _sdpa("attn_fwd_window", 16384) + _window("attn_fwd_window") + [
        ("null workspace, then null coordinates", dict(ws=None, qc=None), "attn_fwd_window: workspace too small (1073741824 < 16384)"),
    ]]
    + [("apexmi_attn_fwd_prepared_window",) + r for r in [
        ("null q", dict(q=None), "attn_fwd_prepared_window: null operand"),
        ("null k", dict(k=None), "attn_fwd_prepared_window: null operand"),
        ("null vt", dict(vt=None), "attn_fwd_prepared_window: null operand"),
        ("null out", dict(out=None), "attn_fwd_prepared_window: null operand"),
        ("null out strides", dict(os=None), "attn_fwd_prepared_window: null operand"),
        ("B = 0", dict(B=0), "attn_fwd_prepared_window: empty problem"),
        ("H = 0", dict(H=0), "attn_fwd_prepared_window: empty problem"),
        ("Sq = 0", dict(Sq=0), "attn_fwd_prepared_window: empty problem"),
        ("Sk = 0", dict(Sk=0), "attn_fwd_prepared_window: empty problem"),
        ("Skp = 100", dict(Skp=100), "attn_fwd_prepared_window: Skp=100 must be Sk=8 rounded up to 64"),
        ("Skp below Sk", dict(Sk=128, Skp=64), "attn_fwd_prepared_window: Skp=64 must be Sk=128 rounded up to 64"),
        ("q off by 8 bytes", dict(q=P + 8), "attn_fwd_prepared_window: operands must be 16-byte aligned"),
        ("k off by 8 bytes", dict(k=P + 8), "attn_fwd_prepared_window: operands must be 16-byte aligned"),
        ("vt off by 2 bytes", dict(vt=P + 2), "attn_fwd_prepared_window: operands must be 16-byte aligned"),
        ("out off by 4 bytes", dict(out=P + 4), "attn_fwd_prepared_window: operands must be 16-byte aligned"),
        ("out stride 66", dict(os=(4096, 256, 66)), "attn_fwd_prepared_window: output strides must be multiples of 4 elements"),
        ("out stride 2", dict(os=(2, 256, 64)), "attn_fwd_prepared_window: output strides must be multiples of 4 elements"),
        ("Sk above 2^20", dict(Sk=TOO_LONG, Skp=TOO_LONG + 63), "attn_fwd_prepared_window: Sk=1048577 above 1048576 keys"),
        ("2^31 query blocks", dict(B=1 << 16, H=1 << 15, Sq=128), "attn_fwd_prepared_window: too many query blocks"),
        ("null q, then B = 0", dict(q=None, B=0), "attn_fwd_prepared_window: null operand"),
        ("B = 0, then Skp = 100", dict(B=0, Skp=100), "attn_fwd_prepared_window: empty problem"),
        ("Skp = 100, then q off", dict(Skp=100, q=P + 8), "attn_fwd_prepared_window: Skp=100 must be Sk=8 rounded up to 64"),
        ("q off, then out stride 66", dict(q=P + 8, os=(4096, 256, 66)), "attn_fwd_prepared_window: operands must be 16-byte aligned"),
        ("out stride 66, then 2^31 query blocks", dict(os=(4096, 256, 66), B=1 << 16, H=1 << 15, Sq=128),
         "attn_fwd_prepared_window: output strides must be multiples of 4 elements"),
        ("2^31 query blocks, then null coordinates", dict(B=1 << 16, H=1 << 15, Sq=128, qc=None),
         "attn_fwd_prepared_window: too many query blocks"),
    ] + _window("attn_fwd_prepared_window")]
    + [("apexmi_attn_fwd_varlen",) + r for r in [
        ("null q", dict(q=None), "attn_fwd_varlen: null operand"),
        ("null k", dict(k=None), "attn_fwd_varlen: null operand"),
        ("null v", dict(v=None), "attn_fwd_varlen: null operand"),
        ("null out", dict(out=None), "attn_fwd_varlen: null operand"),
        ("null q strides", dict(qs=None), "attn_fwd_varlen: null operand"),
        ("null k strides", dict(ks=None), "attn_fwd_varlen: null operand"),
        ("null v strides", dict(vs=None), "attn_fwd_varlen: null operand"),
        ("null out strides", dict(os=None), "attn_fwd_varlen: null operand"),
        ("null cu_seqlens_q", dict(cu_q=None), "attn_fwd_varlen: null or misaligned cu_seqlens operand"),
        ("cu_seqlens_k off by 2 bytes", dict(cu_k=P + 2), "attn_fwd_varlen: null or misaligned cu_seqlens operand"),
        ("lse off by 2 bytes", dict(lse=P + 2), "attn_fwd_varlen: misaligned lse operand or null lse strides"),
        ("lse without strides", dict(ls=None), "attn_fwd_varlen: misaligned lse operand or null lse strides"),
        ("n = 0", dict(n=0), "attn_fwd_varlen: empty problem (n=0 Tq=406 Tk=531 Hq=4 Hkv=2)"),
        ("Tq = 0", dict(Tq=0), "attn_fwd_varlen: empty problem (n=5 Tq=0 Tk=531 Hq=4 Hkv=2)"),
        ("Tk = 0", dict(Tk=0), "attn_fwd_varlen: empty problem (n=5 Tq=406 Tk=0 Hq=4 Hkv=2)"),
        ("Hq = 0", dict(Hq=0), "attn_fwd_varlen: empty problem (n=5 Tq=406 Tk=531 Hq=0 Hkv=2)"),
        ("Hkv = 0", dict(Hkv=0), "attn_fwd_varlen: empty problem (n=5 Tq=406 Tk=531 Hq=4 Hkv=0)"),
        ("max_seqlen_q = 0", dict(mq=0), "attn_fwd_varlen: max_seqlen_q=0 / max_seqlen_k=333 must be at least 1"),
        ("max_seqlen_k = -3", dict(mk=-3), "attn_fwd_varlen: max_seqlen_q=200 / max_seqlen_k=-3 must be at least 1"),
        ("D = 80", dict(D=80), "attn_fwd_varlen: head dim 80 unsupported (64 or 128)"),
        ("dtype f32", dict(dtype=lib.F32), "attn_fwd_varlen: dtype 2 unsupported (bf16 or f16)"),
        ("ratio 4 / 3", dict(Hkv=3), "attn_fwd_varlen: head ratio Hq=4 / Hkv=3 is not whole"),
        ("70000 sequences", dict(n=70000), "attn_fwd_varlen: grid too large (n=70000 sequences, Hq=4, Hkv=2, 2 query blocks each)"),
        ("2^31 query blocks", dict(n=60000, Hq=60000, Hkv=60000, Tq=1 << 20, mq=1 << 20), "attn_fwd_varlen: grid too large (n=60000 sequences, Hq=60000, Hkv=60000, 8192 query blocks each)"),
        ("q off by 8 bytes", dict(q=P + 8), _AL_V),
        ("k off by 8 bytes", dict(k=P + 8), _AL_V),
        ("v off by 2 bytes", dict(v=P + 2), _AL_V),
        ("out off by 4 bytes", dict(out=P + 4), _AL_V),
        ("q stride 100", dict(qs=(512, 100)), _AL_V),
        ("k stride 4", dict(ks=(4, 128)), _AL_V),
        ("v stride 12", dict(vs=(512, 12)), _AL_V),
        ("out stride 130", dict(os=(512, 130)), _AL_V),
        ("null workspace", dict(ws=None), "attn_fwd_varlen: workspace too small or misaligned (1073741824 < 458752)"),
        ("workspace of 16 bytes", dict(wsb=16), "attn_fwd_varlen: workspace too small or misaligned (16 < 458752)"),
        ("workspace off by 8 bytes", dict(ws=P + 8), "attn_fwd_varlen: workspace too small or misaligned (1073741824 < 458752)"),
        ("null q, then null cu_seqlens", dict(q=None, cu_q=None), "attn_fwd_varlen: null operand"),
        ("null cu_seqlens, then lse off", dict(cu_k=None, lse=P + 2), "attn_fwd_varlen: null or misaligned cu_seqlens operand"),
        ("lse off, then n = 0", dict(lse=P + 2, n=0), "attn_fwd_varlen: misaligned lse operand or null lse strides"),
        ("n = 0, then max_seqlen_q = 0", dict(n=0, mq=0), "attn_fwd_varlen: empty problem (n=0 Tq=406 Tk=531 Hq=4 Hkv=2)"),
        ("max_seqlen_q = 0, then D = 80", dict(mq=0, D=80), "attn_fwd_varlen: max_seqlen_q=0 / max_seqlen_k=333 must be at least 1"),
        ("D = 80, then dtype f32", dict(D=80, dtype=lib.F32), "attn_fwd_varlen: head dim 80 unsupported (64 or 128)"),
        ("dtype f32, then ratio", dict(dtype=lib.F32, Hkv=3), "attn_fwd_varlen: dtype 2 unsupported (bf16 or f16)"),
        ("ratio, then 70000 sequences", dict(Hkv=3, n=70000), "attn_fwd_varlen: head ratio Hq=4 / Hkv=3 is not whole"),
        ("70000 sequences, then q off", dict(n=70000, q=P + 8), "attn_fwd_varlen: grid too large (n=70000 sequences, Hq=4, Hkv=2, 2 query blocks each)"),
        ("q off, then null workspace", dict(q=P + 8, ws=None), _AL_V),
    ]]
    + [("apexmi_attn_fwd_wide",) + r for r in _wide("attn_fwd_wide")]
    + [("apexmi_attn_fwd_wide_split",) + r for r in _wide("attn_fwd_wide_split") + [
        ("key_splits -1", dict(n=-1), "attn_fwd_wide_split: key_splits=-1 unsupported (0 = auto, 1 to 8)"),
        ("key_splits 9", dict(n=9), "attn_fwd_wide_split: key_splits=9 unsupported (0 = auto, 1 to 8)"),
        ("lse without strides", dict(lse=P), "attn_fwd_wide_split: lse without strides, or misaligned"),
        ("lse off by 2 bytes", dict(lse=P + 2, ls=(64, 64, 1)), "attn_fwd_wide_split: lse without strides, or misaligned"),
        ("2^31 workgroups", dict(B=1 << 15, H=1 << 14, Sq=128, n=4, wsb=1 << 62), "attn_fwd_wide_split: too many workgroups (536870912 query blocks x 4 key splits)"),
        ("workspace one byte short, 2 splits", dict(n=2, wsb=65536 + 2 * 64 * 513 * 4 - 1), "attn_fwd_wide_split: workspace too small or misaligned (328191 < 328192)"),
        ("workspace one byte short, 8 splits", dict(n=8, wsb=65536 + 8 * 64 * 513 * 4 - 1), "attn_fwd_wide_split: workspace too small or misaligned (1116159 < 1116160)"),
        ("q off, then key_splits 9", dict(q=P + 8, n=9), _AL_W.format(e="attn_fwd_wide_split")),
        ("key_splits 9, then lse off", dict(n=9, lse=P + 2, ls=(64, 64, 1)), "attn_fwd_wide_split: key_splits=9 unsupported (0 = auto, 1 to 8)"),
        ("lse off, then 2^31 workgroups", dict(lse=P + 2, ls=(64, 64, 1), B=1 << 15, H=1 << 14, Sq=128, n=4, wsb=1 << 62),
         "attn_fwd_wide_split: lse without strides, or misaligned"),
        ("2^31 workgroups, then null workspace", dict(B=1 << 15, H=1 << 14, Sq=128, n=4, ws=None), "attn_fwd_wide_split: too many workgroups (536870912 query blocks x 4 key splits)"),
    ]]
)


@pytest.mark.parametrize("entry,fault,overrides,message", ROWS, ids=[f"{r[0][12:]}: {r[1]}" for r in ROWS])
def test_entry_point_refuses_with_the_exact_message(entry, fault, overrides, message):
    rc, msg = call(entry, overrides)
    assert rc != 0, fault
    assert msg == message


def test_every_entry_has_rows_for_two_faults():
    for entry in ENTRIES:
        assert sum(1 for r in ROWS if r[0] == entry and ", then " in r[1]) >= 4, entry
    assert len({(r[0], r[1]) for r in ROWS}) == len(ROWS)                       # no row twice


# ------------------------------------------------------------------------------------------------ ops.attention_varlen, on the CPU
BF = torch.bfloat16


def _operands(Tq=12, Tk=20, Hq=4, Hkv=2, D=64, dtype=BF):
    q = torch.zeros(Tq, Hq, D, dtype=dtype)
    k = torch.zeros(Tk, Hkv, D, dtype=dtype)
    cu_q, cu_k = torch.tensor([0, 5, Tq], dtype=torch.int32), torch.tensor([0, 9, Tk], dtype=torch.int32)
    return q, k, k.clone(), cu_q, cu_k


def _varlen_rows():
    q, k, v, cu_q, cu_k = _operands()
    k80, k128, k3 = k.new_zeros(20, 2, 80), k.new_zeros(20, 2, 128), k.new_zeros(20, 3, 64)
    gqa = dict(enable_gqa=True)
    return [
        ("f32", (q.float(), k.float(), v.float(), cu_q, cu_k, 7, 11), gqa, "attention_varlen: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)"),
        ("k of another dtype", (q, k.half(), v, cu_q, cu_k, 7, 11), gqa, "attention_varlen: dtypes torch.bfloat16/torch.float16/torch.bfloat16 unsupported (bf16 or f16, all equal)"),
        ("4-D", (q[None], k[None], v[None], cu_q, cu_k, 7, 11), gqa, "attention_varlen: q, k, v must be 3-D packed [T, H, D]"),
        ("head dim 80", (q.new_zeros(12, 4, 80), k80, k80, cu_q, cu_k, 7, 11), gqa, "attention_varlen: head dim 80 unsupported (64 or 128)"),
        ("v shorter than k", (q, k, v[:10], cu_q, cu_k, 7, 11), gqa, "attention_varlen: shapes q (12, 4, 64) k (20, 2, 64) v (10, 2, 64) do not match"),
        ("k of another head dim", (q, k128, k128, cu_q, cu_k, 7, 11), gqa, "attention_varlen: shapes q (12, 4, 64) k (20, 2, 128) v (20, 2, 128) do not match"),
        ("no queries", (q[:0], k, v, cu_q, cu_k, 7, 11), gqa, "attention_varlen: empty problem"),
        ("no keys", (q, k[:0], v[:0], cu_q, cu_k, 7, 11), gqa, "attention_varlen: empty problem"),
        ("4 heads over 2 without enable_gqa", (q, k, v, cu_q, cu_k, 7, 11), {}, "attention_varlen: 4 query heads over 2 key/value heads needs enable_gqa=True and a whole ratio"),
        ("4 heads over 3", (q, k3, k3, cu_q, cu_k, 7, 11), gqa, "attention_varlen: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio"),
        ("k and v on another device", (q, k.to("meta"), v.to("meta"), cu_q, cu_k, 7, 11), gqa, "attention_varlen: k / v are on meta / meta, q on cpu"),
        ("int64 cu_seqlens_q", (q, k, v, cu_q.long(), cu_k, 7, 11), gqa, "attention_varlen: cu_seqlens_q must be a contiguous 1-D int32 tensor"),
        ("cu_seqlens_q a list", (q, k, v, [0, 5, 12], cu_k, 7, 11), gqa, "attention_varlen: cu_seqlens_q must be a contiguous 1-D int32 tensor"),
        ("2-D cu_seqlens_k", (q, k, v, cu_q, cu_k[None], 7, 11), gqa, "attention_varlen: cu_seqlens_k must be a contiguous 1-D int32 tensor"),
        ("cu_seqlens_k on another device", (q, k, v, cu_q, cu_k.to("meta"), 7, 11), gqa, "attention_varlen: cu_seqlens_k is on meta, q on cpu"),
        ("cu_seqlens of different lengths", (q, k, v, cu_q, cu_k[:2], 7, 11), gqa, "attention_varlen: cu_seqlens_q has 3 entries, cu_seqlens_k 2 (n + 1 of each, n >= 1)"),
        ("cu_seqlens of one entry", (q, k, v, cu_q[:1], cu_k[:1], 7, 11), gqa, "attention_varlen: cu_seqlens_q has 1 entries, cu_seqlens_k 1 (n + 1 of each, n >= 1)"),
        ("max_seqlen_q = 0", (q, k, v, cu_q, cu_k, 0, 11), gqa, "attention_varlen: max_seqlen_q=0 / max_seqlen_k=11 must be at least 1"),
        ("max_seqlen_k = -1", (q, k, v, cu_q, cu_k, 7, -1), gqa, "attention_varlen: max_seqlen_q=7 / max_seqlen_k=-1 must be at least 1"),
        # two faults: the order of the checks
        ("f32, then 4-D", (q.float()[None], k.float()[None], v.float()[None], cu_q, cu_k, 7, 11), gqa, "attention_varlen: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)"),
        ("4-D, then head dim 80", (q.new_zeros(1, 12, 4, 80), k80[None], k80[None], cu_q, cu_k, 7, 11), gqa, "attention_varlen: q, k, v must be 3-D packed [T, H, D]"),
        ("head dim 80, then v shorter than k", (q.new_zeros(12, 4, 80), k80, k80[:10], cu_q, cu_k, 7, 11), gqa, "attention_varlen: head dim 80 unsupported (64 or 128)"),
        ("v shorter than k, then no queries", (q[:0], k, v[:10], cu_q, cu_k, 7, 11), gqa, "attention_varlen: shapes q (0, 4, 64) k (20, 2, 64) v (10, 2, 64) do not match"),
        ("no queries, then 4 heads over 3", (q[:0], k3, k3, cu_q, cu_k, 7, 11), gqa, "attention_varlen: empty problem"),
        ("4 heads over 3, then int64 cu_seqlens_q", (q, k3, k3, cu_q.long(), cu_k, 7, 11), gqa, "attention_varlen: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio"),
        ("cu_seqlens of different lengths, then max_seqlen_q = 0", (q, k, v, cu_q, cu_k[:2], 0, 11), gqa, "attention_varlen: cu_seqlens_q has 3 entries, cu_seqlens_k 2 (n + 1 of each, n >= 1)"),
        # the last refusal, everything valid but the device
        ("CPU tensors", (q, k, v, cu_q, cu_k, 7, 11), gqa, "attention_varlen.q: expected a ROCm device tensor, got cpu (no CPU fallback)"),
    ]


VARLEN_ROWS = _varlen_rows()


@pytest.mark.parametrize("fault,args,kwargs,message", VARLEN_ROWS, ids=[r[0] for r in VARLEN_ROWS])
def test_ops_attention_varlen_refuses_with_the_exact_message(fault, args, kwargs, message):
    with pytest.raises(ApexMIError) as e:
        ops.attention_varlen(*args, **kwargs)
    assert str(e.value) == message


@pytest.mark.parametrize("key,value", [("attn.xv", 1), ("attn.stages", 3)])
def test_removed_attention_experiment_keys_are_unknown(key, value):
    """`attn.xv` and `attn.stages` selected experiment arms of the 4-cluster kernel that are no longer built: the library refuses
    them like any key it never had, while a surviving key of the same kernel (`attn.c4`) is still accepted (and restored)."""
    L = lib.load()
    assert L.apexmi_tune_set(key.encode(), value) != 0
    assert L.apexmi_last_error().decode() == "tune_set: unknown key"
    with pytest.raises(ApexMIError, match="unknown key"):
        lib.tune_set(key, value)
    try:
        lib.tune_set("attn.c4", 1)
    finally:
        lib.tune_set("attn.c4", 3)       # the shipped default
