"""The "hip_mfma_sdpa" backend's host side (no GPU): torch's mask broadcast rule as in-place strides, the refusals, the
registration of both keys and the C-ABI argument checks of apexmi_attn_fwd_masked."""
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError

B, H, SQ, SK = 2, 3, 5, 7


def _mask_forms():
    g = torch.Generator().manual_seed(0)
    full = torch.rand(B, H, SQ, SK, generator=g) > 0.3
    return {
        "[Sq,Sk]": torch.rand(SQ, SK, generator=g) > 0.5,
        "[Hq,Sq,Sk]": torch.randn(H, SQ, SK, generator=g),
        "[B,1,Sq,Sk]": torch.randn(B, 1, SQ, SK, generator=g),
        "[1,Hq,Sq,Sk]": torch.randn(1, H, SQ, SK, generator=g),
        "[B,1,1,Sk]": torch.rand(B, 1, 1, SK, generator=g) > 0.5,
        "[B,1,Sq,1]": torch.rand(B, 1, SQ, 1, generator=g) > 0.5,
        "[B,Hq,Sq,Sk]": full,
        "expand [B,Hq,Sq,Sk] of [B,1,1,Sk]": (torch.rand(B, 1, 1, SK, generator=g) > 0.5).expand(B, H, SQ, SK),
        "expand [B,Hq,Sq,Sk] of [1,1,Sq,Sk]": torch.randn(1, 1, SQ, SK, generator=g).expand(B, H, SQ, SK),
        "transposed [Sk,Sq].T": torch.randn(SK, SQ, generator=g).t(),
        "bf16 [Sq,Sk]": torch.randn(SQ, SK, generator=g).to(torch.bfloat16),
    }


@pytest.mark.parametrize("name", list(_mask_forms()))
def test_mask_operand_matches_broadcast_to(name):
    m = _mask_forms()[name]
    t, code, st = ops._mask_operand(m, B, H, SQ, SK, torch.bfloat16)
    want = torch.broadcast_to(m, (B, H, SQ, SK))
    assert code == {torch.bool: lib.MASK_BOOL, torch.float32: lib.F32, torch.bfloat16: lib.BF16}[m.dtype]
    assert st[3] in (0, 1)
    # every element the kernel addresses (b sb + h sh + i sq + j sk from the operand's storage) is torch's broadcast value
    flat = t.as_strided((t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
    idx = torch.zeros(B, H, SQ, SK, dtype=torch.int64)
    for d, (n, s) in enumerate(zip((B, H, SQ, SK), st)):
        shape = [1, 1, 1, 1]
        shape[d] = n
        idx = idx + (torch.arange(n) * s).view(shape)
    got = flat[idx + t.storage_offset()]
    assert torch.equal(got, want)
    # broadcast dims are read with stride 0: nothing is expanded to [B, Hq, Sq, Sk]
    for d, n in enumerate(m.shape[::-1]):
        if n == 1:
            assert st[3 - d] == 0
    assert t.untyped_storage().nbytes() <= m.untyped_storage().nbytes()


def test_mask_operand_none():
    assert ops._mask_operand(None, B, H, SQ, SK) == (None, -1, (0, 0, 0, 0))


@pytest.mark.parametrize("mask", [torch.ones(SQ, SK, dtype=torch.uint8), torch.ones(SQ, SK, dtype=torch.int32),
                                  torch.zeros(SQ, SK, dtype=torch.float16), torch.zeros(SQ, SK, dtype=torch.float64)])
def test_mask_operand_rejects_dtypes(mask):
    with pytest.raises(ApexMIError, match="dtype"):
        ops._mask_operand(mask, B, H, SQ, SK, torch.bfloat16)


@pytest.mark.parametrize("shape", [(SQ, SK + 1), (H + 1, SQ, SK), (B + 1, 1, SQ, SK), (SQ,), (1, 1, 1, SQ, SK)])
def test_mask_operand_rejects_non_broadcastable(shape):
    with pytest.raises(ApexMIError):
        ops._mask_operand(torch.zeros(shape, dtype=torch.bool), B, H, SQ, SK)


def test_backend_refuses_cpu_dropout_dtype_and_heads():
    q = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q, q, q)
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q, q, q, attn_mask=torch.ones(8, 8, dtype=torch.bool), is_causal=True)
    with pytest.raises(ApexMIError, match="dropout"):
        ab.hip_mfma_sdpa(q, q, q, dropout_p=0.1)
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q.float(), q.float(), q.float())


def test_register_puts_both_keys():
    from apex_studio_amd.register import FunctionRegister
    reg = ab.register(FunctionRegister(), set_default=True)
    assert reg.get(ab.KEY) is ab.hip_mfma and reg.get(ab.KEY_SDPA) is ab.hip_mfma_sdpa
    assert ab.KEY_SDPA == "hip_mfma_sdpa" and reg.get_default() == ab.KEY
    assert reg.is_available(ab.KEY) == reg.is_available(ab.KEY_SDPA)


def test_cabi_argument_checks():
    L = lib.load()
    P = 0x100000
    s3 = lib.i64x3((8 * 128 * 64, 8 * 128, 128))
    m4 = lib.i64x4((0, 0, 64, 1))
    big = 1 << 30

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    def call(q=P, B=1, Hq=8, Hkv=8, Sq=64, Sk=64, D=128, mask=None, mcode=lib.MASK_BOOL, mst=m4, dtype=lib.BF16, ws=P,
             wsb=big, st=s3):
        return L.apexmi_attn_fwd_masked(q, P, P, P, B, Hq, Hkv, Sq, Sk, D, st, st, st, st, mask, mcode, mst, 0, 0.1,
                                        dtype, ws, wsb, None)

    bad(call(q=None), "null operand")
    bad(call(Sq=0), "empty problem")
    bad(call(B=0), "empty problem")
    bad(call(D=96), "head dim 96")
    bad(call(dtype=lib.F32), "dtype")
    bad(call(Hkv=3), "head ratio")
    bad(call(mask=P, mcode=7), "mask dtype code 7")
    bad(call(mask=P, mst=lib.i64x4((0, 0, 64, 2))), "mask key stride")
    bad(call(st=lib.i64x3((8 * 128 * 64, 8 * 128, 100))), "16-byte aligned")
    bad(call(wsb=16), "workspace too small")
    bad(call(ws=None), "workspace too small")
    assert L.apexmi_attn_masked_workspace_bytes(1, 8, 2, 64, 64, 128) > 0
    assert L.apexmi_attn_masked_workspace_bytes(1, 8, 2, 64, 64, 80) == 0
