"""The "hip_mfma_sdpa" backend on the GPU against the exact witness: torch's F.scaled_dot_product_attention on the CPU in
f32, on the upcast bf16 / f16 inputs (the reference's default "sdpa" backend is that call)."""
import pytest
import torch
import torch.nn.functional as F

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _qkv(B, Hq, Sq, Sk, D, dtype=torch.bfloat16, Hkv=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    Hkv = Hq if Hkv is None else Hkv
    q = torch.randn(B, Hq, Sq, D, generator=g).to(dtype)
    k = torch.randn(B, Hkv, Sk, D, generator=g).to(dtype)
    v = torch.randn(B, Hkv, Sk, D, generator=g).to(dtype)
    return q, k, v


def _ref(q, k, v, mask=None, causal=False, gqa=False):
    m = mask
    if m is not None and m.dtype != torch.bool:
        m = m.float()
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=m, is_causal=causal, enable_gqa=gqa)


def _run(q, k, v, mask=None, causal=False, gqa=False):
    d = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    out = ab.hip_mfma_sdpa(d(q), d(k), d(v), attn_mask=d(mask), is_causal=causal, enable_gqa=gqa)
    torch.cuda.synchronize()
    return out.cpu()


def _rel(out, ref):
    return float((out.float() - ref).norm() / ref.norm())


def _band(Sq, Sk, w):
    i, j = torch.arange(Sq)[:, None], torch.arange(Sk)[None, :]
    return (j <= i) & (j > i - w)


def _cases():
    g = torch.Generator().manual_seed(1)
    cases = {}
    for name, (Sq, Sk) in {"causal Sq==Sk": (512, 512), "causal Sq<Sk": (200, 700), "causal Sq>Sk": (700, 200)}.items():
        cases[name] = dict(shape=(2, 4, Sq, Sk, 128), causal=True)
    cases["bool [Sq,Sk]"] = dict(shape=(2, 4, 333, 777, 128), mask=torch.rand(333, 777, generator=g) > 0.5)
    alibi = -0.05 * (torch.arange(4)[:, None, None] + 1) * (torch.arange(640)[None, :] - torch.arange(640)[:, None]).abs()
    alibi = alibi.float()[None]
    alibi[..., 500:520] = 60.0           # deep in every row, far above the first tiles' maximum: the running maximum rises
    cases["additive f32 [1,H,Sq,Sk] alibi +60"] = dict(shape=(1, 4, 640, 640, 128), mask=alibi)
    bm = torch.randn(1, 1, 300, 450, generator=g).to(torch.bfloat16)
    bm[torch.rand(1, 1, 300, 450, generator=g) > 0.7] = float("-inf")
    cases["additive bf16 -inf"] = dict(shape=(2, 2, 300, 450, 128), mask=bm)
    cases["full [B,H,Sq,Sk]"] = dict(shape=(2, 3, 256, 320, 128), mask=torch.rand(2, 3, 256, 320, generator=g) > 0.4)
    cases["sliding window 128"] = dict(shape=(1, 4, 1024, 1024, 128), mask=_band(1024, 1024, 128))
    cases["mask + causal"] = dict(shape=(2, 2, 400, 400, 128), mask=torch.rand(400, 400, generator=g) > 0.3, causal=True)
    cases["gqa 8/2"] = dict(shape=(1, 8, 300, 300, 128), Hkv=2, gqa=True, mask=torch.rand(300, 300, generator=g) > 0.5)
    cases["gqa Hkv=1 causal"] = dict(shape=(1, 4, 256, 256, 64), Hkv=1, causal=True)
    cases["f16 D64 probe 1,2,8,64"] = dict(shape=(1, 2, 8, 8, 64), dtype=torch.float16)
    cases["f16 D64 causal"] = dict(shape=(2, 4, 333, 333, 64), dtype=torch.float16, causal=True)
    cases["f16 D64 additive f16"] = dict(shape=(1, 4, 200, 257, 64), dtype=torch.float16,
                                         mask=torch.randn(4, 200, 257, generator=g).to(torch.float16))
    for Sq in (77, 333):
        for Sk in (77, 333):
            cases[f"tails {Sq}x{Sk}"] = dict(shape=(1, 2, Sq, Sk, 128), mask=torch.rand(1, 1, 1, Sk, generator=g) > 0.2)
    return cases


# rel-L2 vs the f32 witness; bars about 2x the first MI355X run
BARS = {"bf16": 5e-3, "f16": 6e-4}             # measured 2.2e-3 .. 2.4e-3 / 2.7e-4 .. 2.9e-4


@pytest.mark.parametrize("name", list(_cases()))
def test_matches_torch_sdpa(name):
    c = _cases()[name]
    B, H, Sq, Sk, D = c["shape"]
    dtype = c.get("dtype", torch.bfloat16)
    q, k, v = _qkv(B, H, Sq, Sk, D, dtype, c.get("Hkv"))
    mask, causal, gqa = c.get("mask"), c.get("causal", False), c.get("gqa", False)
    out = _run(q, k, v, mask, causal, gqa)
    assert out.shape == (B, H, Sq, D) and out.dtype == dtype and torch.isfinite(out).all()
    ref = _ref(q, k, v, mask, causal, gqa)
    measured(f"sdpa_masked {name}", _rel(out, ref), BARS["bf16" if dtype == torch.bfloat16 else "f16"])


def test_joint_padding_fully_masked_rows_are_zero():
    B, H, S, D = 2, 4, 384, 128
    q, k, v = _qkv(B, H, S, S, D)
    keep = torch.ones(B, S, dtype=torch.bool)
    keep[0, 300:] = False
    keep[1, 100:] = False
    mask = (keep[:, None, :, None] & keep[:, None, None, :])     # [B,1,S,S]: padded queries see nothing
    out = _run(q, k, v, mask)
    ref = _ref(q, k, v, mask)
    assert torch.equal(out[0, :, 300:], torch.zeros_like(out[0, :, 300:]))
    assert torch.equal(out[1, :, 100:], torch.zeros_like(out[1, :, 100:]))
    measured("sdpa_masked joint padding", _rel(out, ref), 5e-3)              # 2.35e-3


def test_expand_view_equals_compact_mask_bitwise():
    q, k, v = _qkv(2, 4, 256, 300, 128)
    compact = torch.randn(2, 1, 256, 300)
    a = _run(q, k, v, compact)
    b = _run(q, k, v, compact.expand(2, 4, 256, 300))
    c = _run(q, k, v, compact.expand(2, 4, 256, 300).contiguous())
    assert torch.equal(a, b) and torch.equal(a, c)


def test_permuted_bshd_views():
    B, S, H, D = 2, 320, 4, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, S, 3, H, D, generator=g).to(torch.bfloat16).to(DEV)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    mask = (torch.rand(S, S, generator=g) > 0.3).to(DEV)
    out = ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, is_causal=True)
    torch.cuda.synchronize()
    ref = _ref(q.cpu(), k.cpu(), v.cpu(), mask.cpu(), True)
    assert out.stride(3) == 1 and out.permute(0, 2, 1, 3).is_contiguous()
    measured("sdpa_masked permuted views", _rel(out.cpu(), ref), 5e-3)      # 2.32e-3


def test_all_true_mask_and_repeat_are_bit_identical():
    q, k, v = _qkv(1, 4, 500, 700, 128)
    a = _run(q, k, v)
    b = _run(q, k, v, torch.ones(500, 700, dtype=torch.bool))
    c = _run(q, k, v, torch.zeros(1, 4, 500, 700))
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a, _run(q, k, v))
    m = torch.rand(500, 700) > 0.5
    assert torch.equal(_run(q, k, v, m, True), _run(q, k, v, m, True))


def test_key_padding_agrees_with_hip_mfma():
    q, k, v = _qkv(2, 4, 256, 384, 128)
    keep = torch.ones(2, 1, 1, 384, dtype=torch.bool)
    keep[0, ..., 300:] = False
    keep[1, ..., 50:] = False
    d = [t.to(DEV) for t in (q, k, v, keep)]
    a = ab.hip_mfma_sdpa(*d[:3], attn_mask=d[3]).float()
    b = ab.hip_mfma(*d[:3], attn_mask=d[3]).float()
    measured("sdpa_masked vs hip_mfma key padding", float((a - b).norm() / b.norm()), 4e-5)   # 1.84e-5


def test_no_host_sync():
    q, k, v = (t.to(DEV) for t in _qkv(1, 4, 300, 300, 128))
    mask = (torch.rand(300, 300) > 0.3).to(DEV)
    ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, is_causal=True)   # workspace allocated outside the checked region
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ab.hip_mfma_sdpa(q, k, v, attn_mask=mask, is_causal=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()


def test_long_causal_sampled_rows():
    B, H, S, D = 1, 2, 8192, 128
    q, k, v = _qkv(B, H, S, S, D, seed=5)
    out = _run(q, k, v, causal=True)
    rows = torch.tensor([0, 1, 63, 64, 127, 128, 1000, 4095, 4096, 6000, 8000, 8190, 8191])
    qs = q[:, :, rows]
    allowed = torch.arange(S)[None, :] <= rows[:, None]
    ref = F.scaled_dot_product_attention(qs.float(), k.float(), v.float(), attn_mask=allowed)
    measured("sdpa_masked causal 8192 sampled rows", _rel(out[:, :, rows], ref), 3e-3)   # 1.42e-3


def test_refuses_on_device():
    from apex_studio_amd.lib import ApexMIError
    q, k, v = (t.to(DEV) for t in _qkv(1, 2, 64, 64, 128))
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q, k, v, dropout_p=0.1)
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q.float(), k.float(), v.float())
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q[..., :96].contiguous(), k[..., :96].contiguous(), v[..., :96].contiguous())
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q, k, v, attn_mask=torch.ones(64, 65, dtype=torch.bool, device=DEV))
    kv3 = torch.zeros(1, 3, 64, 128, dtype=q.dtype, device=DEV)
    with pytest.raises(ApexMIError, match="key/value heads"):
        ab.hip_mfma_sdpa(q, kv3, kv3, enable_gqa=True)
