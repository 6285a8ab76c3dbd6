"""Host side of the wide-head attention (ops.attention_wide, apexmi_attn_fwd_wide) and of the VAEs' set_mid_attention: no GPU.
The header and the ctypes table agree, the workspace is V^T and nothing else, the wrappers refuse what the kernel does not
cover, and the frame rule has one CPU restatement that the GPU test uses."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("apexmi_attn_wide_workspace_bytes", "apexmi_attn_fwd_wide")


def frame_allowed(S: int, ft: int) -> torch.Tensor:
    """allowed[i, j] = j // ft <= i // ft: query i sees the keys of the frames up to its own (ft tokens a frame)"""
    i, j = torch.arange(S)[:, None], torch.arange(S)[None, :]
    return (j // ft) <= (i // ft)


def _lib():
    from apex_studio_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        from apex_studio_amd import build
        build.build(verbose=False)
    return lib.load()


def test_header_and_signatures_carry_the_symbols():
    from apex_studio_amd import lib
    with open(os.path.join(ROOT, "include", "apexmi.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in lib.SIGNATURES, name
    # q, k, v, out | B, H, Sq, Sk, D | four stride triples | scale, dtype, frame_tokens | workspace, bytes, stream
    assert len(lib.SIGNATURES["apexmi_attn_fwd_wide"][1]) == 4 + 5 + 4 + 3 + 3
    assert len(lib.SIGNATURES["apexmi_attn_wide_workspace_bytes"][1]) == 4


def test_frame_rule_restatement():
    a = frame_allowed(6, 2)
    assert a.tolist() == [[True, True, False, False, False, False]] * 2 + [[True] * 4 + [False] * 2] * 2 + [[True] * 6] * 2
    assert frame_allowed(5, 5).all()                      # one frame: nothing excluded
    assert torch.equal(frame_allowed(4, 1), torch.tril(torch.ones(4, 4, dtype=torch.bool)))   # one token a frame: causal


def test_workspace_is_vt_only_and_linear_in_sk():
    L = _lib()
    from apex_studio_amd import lib

    def vt(B, H, Sk, D):      # V^T [B, H, D, Skp], Skp = Sk rounded up to 64, the total rounded up to 256 bytes
        return (B * H * D * (-(-Sk // 64) * 64) * 2 + 255) // 256 * 256

    for args in ((1, 1, 16384, 512), (3, 2, 65, 384), (2, 1, 1000, 256), (1, 1, 1, 256), (4, 1, 1024, 384)):
        assert L.apexmi_attn_wide_workspace_bytes(*args) == vt(*args), args
    # linear in Sk (whole 64-key tiles): twice the keys, twice the bytes; no term in Sq at all (it is no argument)
    for D in (256, 384, 512):
        one = L.apexmi_attn_wide_workspace_bytes(1, 1, 4096, D)
        assert L.apexmi_attn_wide_workspace_bytes(1, 1, 8192, D) == 2 * one
        assert L.apexmi_attn_wide_workspace_bytes(1, 1, 16384, D) == 4 * one
    wide = L.apexmi_attn_wide_workspace_bytes(1, 1, 16384, 512)
    mat = L.apexmi_attn_workspace_bytes(1, 1, 16384, 16384, 512, lib.BF16)
    assert wide * 50 < mat, (wide, mat)
    for bad in ((1, 1, 64, 128), (1, 1, 64, 320), (1, 1, 64, 640), (0, 1, 64, 256), (1, 1, 0, 256)):
        assert L.apexmi_attn_wide_workspace_bytes(*bad) == 0, bad


def test_entry_point_refuses_and_never_falls_back():
    import ctypes as C
    L = _lib()
    from apex_studio_amd import lib
    P = C.c_void_p(4096)
    i3, odd = lib.i64x3((4096, 4096, 512)), lib.i64x3((4096, 4096, 513))

    def bad(rc, text):
        assert rc != 0
        msg = L.apexmi_last_error().decode()
        assert text in msg, msg

    def call(q=P, B=1, H=1, Sq=64, Sk=64, D=512, qs=i3, ks=i3, dtype=lib.BF16, ft=0, ws=P, wsb=1 << 30):
        return L.apexmi_attn_fwd_wide(q, P, P, P, B, H, Sq, Sk, D, qs, ks, i3, i3, 1.0, dtype, ft, ws, wsb, None)

    bad(call(q=None), "null operand")
    bad(call(Sq=0), "empty problem")
    for D in (64, 128, 320, 640, 1024):
        bad(call(D=D), "unsupported (256, 384 or 512")
    bad(call(D=1024), "materialised path")
    bad(call(dtype=lib.F32), "dtype")
    bad(call(qs=odd), "16-byte aligned")
    bad(call(ks=lib.i64x3((4096, 4096, 256))), "key row stride 256 below the head dim 512")      # overlapping rows
    bad(call(Sk=1 << 22, ks=lib.i64x3((0, 0, 512))), "4 GiB")                                    # 2^31 elements of keys a head
    bad(call(Sq=100, Sk=100, ft=30), "whole number of frames")
    bad(call(Sq=64, Sk=128, ft=32), "Sq == Sk")
    bad(call(ws=None), "workspace")
    bad(call(wsb=1024), "workspace too small")


def test_op_raises_on_what_the_kernel_does_not_cover():
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    x = torch.zeros(1, 1, 64, 256, dtype=torch.bfloat16)
    with pytest.raises(ApexMIError, match="no CPU fallback"):
        ops.attention_wide(x, x, x)
    # the remaining checks precede any device work; a meta tensor passes the device check without a GPU
    def dev(*shape, dtype=torch.bfloat16):
        t = torch.empty(*shape, dtype=dtype, device="meta")
        return _FakeCuda(t)

    with pytest.raises(ApexMIError, match="unsupported"):
        ops.attention_wide(*(dev(1, 1, 64, 256, dtype=torch.float32),) * 3)
    for D in (128, 320):
        with pytest.raises(ApexMIError, match=f"head dim {D} unsupported"):
            ops.attention_wide(*(dev(1, 1, 64, D),) * 3)
    with pytest.raises(ApexMIError, match="whole number of frames"):
        ops.attention_wide(*(dev(1, 1, 100, 256),) * 3, frame_tokens=30)
    with pytest.raises(ApexMIError, match="whole number of frames"):
        ops.attention_wide(dev(1, 1, 64, 256), dev(1, 1, 128, 256), dev(1, 1, 128, 256), frame_tokens=32)


class _FakeCuda:
    """A tensor stand-in that says it lives on the device: the argument checks of the wrapper read is_cuda, dtype, dim, shape"""

    def __init__(self, t):
        self._t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.mark.parametrize("which", ["wan", "flux", "hunyuan15"])
def test_setters_default_and_reject(which):
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
    vae = make(256)
    assert vae.mid_attention == "materialised"
    for mode in ("Flash", "", "sdpa", None):
        with pytest.raises(ValueError, match="mid_attention"):
            vae.set_mid_attention(mode)
    assert vae.set_mid_attention("flash") is vae and vae.mid_attention == "flash"
    assert vae.set_mid_attention("materialised").mid_attention == "materialised"
    # the verification mode has no flash mid block
    vae.set_storage_dtype(torch.float32)
    with pytest.raises(NotImplementedError, match="verification"):
        vae.set_mid_attention("flash")
    assert vae.mid_attention == "materialised"
    vae.set_mid_attention("materialised")
    # a mid block the kernel does not cover (HunyuanVideo-1.5 ships 1024 channels) accepts "materialised" only, and says why
    wide = make(1024)
    with pytest.raises(ValueError, match="1024"):
        wide.set_mid_attention("flash")
    assert wide.set_mid_attention("materialised").mid_attention == "materialised"
    # per object: another instance keeps its own setting
    a, b = make(256), make(256)
    a.set_mid_attention("flash")
    assert b.mid_attention == "materialised"
