"""Per-block key bands on the large-attention kernel, on the GPU (ops.band_plan / frame_band_plan / attention_prepared_band /
attention_band, the "hip_mfma_band" backend, WanTransformer3DModel.set_attention_band).  The reference is the dense launch forced
onto the same kernel (tests/attention_band_ref.forced_dense) on one block's query rows and freshly prepared k[lo:hi] / v[lo:hi]:
the band must equal it bit for bit.  Against an f32 softmax over plan.dense_mask() the bar is test_attention_w64_kernel's."""
import functools

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError
from tests import attention_band_ref as R
from tests.golden.seeded import seeded
from tests.test_gpu_ops import _check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
SCALE = 128 ** -0.5


def _qkv(B, H, Sq, Sk, seed):
    return (seeded((B, H, Sq, 128), seed, BF).to(DEV), seeded((B, H, Sk, 128), seed + 1, BF).to(DEV),
            seeded((B, H, Sk, 128), seed + 2, BF).to(DEV))


def _assert_blocks_equal_sliced_dense(out, q, k, v, lo, hi, scale=None):
    """out [B, Sq, H, 128] of a shared plan (lo, hi per block) against the dense launch on every block's rows and key slice"""
    with R.forced_dense():
        for b, (a, e) in enumerate(zip(lo, hi)):
            want = R.dense_block(q, k, v, b, a, e, scale)
            assert torch.equal(out[:, 256 * b:256 * b + 256], want), (b, a, e)


def test_every_block_is_the_dense_launch_on_its_key_slice():
    """Six blocks with bands of 1, 2, 3, 4, 5 and 24 tiles (every tail body of the generated loop), lo = 0 and lo > 0; the launch
    repeats to the bit."""
    q, k, v = _qkv(1, 2, 1536, 1536, 901)
    lo = [0, 128, 640, 1280, 64, 0]
    hi = [64, 256, 832, 1536, 384, 1536]
    assert [(e - a) // 64 for a, e in zip(lo, hi)] == [1, 2, 3, 4, 5, 24]
    plan = ops.band_plan(lo, hi, 1536, 1536, DEV)
    assert plan.Hb == 1 and plan.bands.shape == (1, 6, 2) and plan.bands.dtype == torch.int32
    lib.attn_w64_fallbacks()
    out = R.band_prepared(q, k, v, plan).clone()
    again = R.band_prepared(q, k, v, plan)
    assert lib.attn_w64_fallbacks() == 0
    assert torch.isfinite(out).all() and torch.equal(out, again)
    _assert_blocks_equal_sliced_dense(out, q, k, v, lo, hi)


def test_ragged_rows_and_keys():
    """Sq 700: the last block has 188 rows; Sk 1000: a band that ends at Sk has 40 keys in its last tile."""
    q, k, v = _qkv(1, 2, 700, 1000, 911)
    lo, hi = [0, 512, 64], [1000, 1000, 128]
    plan = ops.band_plan(lo, hi, 700, 1000, DEV)
    out = R.band_prepared(q, k, v, plan)
    _assert_blocks_equal_sliced_dense(out, q, k, v, lo, hi)
    ref = R.masked_softmax_ref(q, k, v, plan.dense_mask()[None], SCALE)                  # [1, 2, 700, 128]
    _check(out.permute(0, 2, 1, 3), ref, 1e-2, "band attention, ragged", ulp=3.0)


def test_keys_outside_the_band_are_never_read():
    q, k, v = _qkv(1, 2, 1024, 1024, 921)
    plan = ops.band_plan([256] * 4, [768] * 4, 1024, 1024, DEV)
    clean = R.band_prepared(q, k, v, plan).clone()
    kp, vp = k.clone(), v.clone()
    for t in (kp, vp):
        t[:, :, :256] = float("nan")
        t[:, :, 768:] = float("nan")
    poisoned = R.band_prepared(q, kp, vp, plan)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, clean)


def test_fallback_inside_a_band():
    """A key inside the band, past its first tile, that towers over one row: exactly the workgroups that hold the row re-run with
    the running-maximum loop, as the dense launch on the slice does; the same key outside the band is never seen."""
    H = 2
    q, k, v = _qkv(1, H, 1024, 1024, 931)
    lo, hi = [256] * 4, [1024] * 4
    plan = ops.band_plan(lo, hi, 1024, 1024, DEV)
    inside = k.clone()
    inside[0, :, 600] = q[0, :, 100] * 8.0                    # tile 5 of the band of block 0, which holds row 100
    lib.attn_w64_fallbacks()
    out = R.band_prepared(q, inside, v, plan)
    assert lib.attn_w64_fallbacks() == H                      # one workgroup per head holds row 100
    _assert_blocks_equal_sliced_dense(out, q, inside, v, lo, hi)
    ref = R.masked_softmax_ref(q, inside, v, plan.dense_mask()[None], SCALE)
    _check(out.permute(0, 2, 1, 3), ref, 1e-2, "band attention, fallback", ulp=3.0)
    outside = k.clone()
    outside[0, :, 100] = q[0, :, 100] * 8.0
    lib.attn_w64_fallbacks()
    R.band_prepared(q, outside, v, plan)
    assert lib.attn_w64_fallbacks() == 0


def test_per_head_plan_and_batch():
    B, H = 2, 3
    q, k, v = _qkv(B, H, 768, 768, 941)
    lo = [[0, 256, 512], [0, 0, 0], [640, 64, 128]]
    hi = [[256, 512, 768], [768, 768, 768], [768, 128, 448]]
    plan = ops.band_plan(lo, hi, 768, 768, DEV)
    assert plan.Hb == 3 and plan.bands.shape == (3, 3, 2)
    out = R.band_prepared(q, k, v, plan)
    for h in range(H):
        shared = R.band_prepared(q, k, v, ops.band_plan(lo[h], hi[h], 768, 768, DEV))
        assert torch.equal(out[:, :, h], shared[:, :, h]), h
        for o in range(H):
            if lo[o] != lo[h] or hi[o] != hi[h]:
                assert not torch.equal(out[:, :, o], shared[:, :, o]), (h, o)       # the heads do differ
    ref = R.masked_softmax_ref(q, k, v, plan.dense_mask()[None], SCALE)
    _check(out.permute(0, 2, 1, 3), ref, 1e-2, "band attention, per-head plan", ulp=3.0)


def test_attention_band_and_the_backend_key_on_permuted_views():
    B, H, S = 2, 2, 768
    q, k, v = (seeded((B, S, H, 128), 951 + i, BF).to(DEV).permute(0, 2, 1, 3) for i in range(3))
    assert not q.is_contiguous()
    plan = ops.frame_band_plan(6, 128, 1, DEV)               # blocks of two frames: bands of three frames at the ends, four between
    assert (plan.lo, plan.hi) == ([[0, 128, 384]], [[384, 640, 768]])
    scale = 0.05
    out = ops.attention_band(q, k, v, plan, softmax_scale=scale)
    assert out.shape == (B, H, S, 128) and out.permute(0, 2, 1, 3).is_contiguous()
    assert torch.equal(out.permute(0, 2, 1, 3), R.band_prepared(q.contiguous(), k.contiguous(), v.contiguous(), plan, scale))
    _check(out, R.masked_softmax_ref(q, k, v, plan.dense_mask()[None], scale), 1e-2, "attention_band", ulp=3.0)
    assert torch.equal(ab.hip_mfma_band(q, k, v, softmax_scale=scale, band_plan=plan), out)
    with pytest.raises(ApexMIError, match=r"the band plan is for \(Sq, Sk\) = \(768, 768\), the operands have \(512, 768\)"):
        ops.attention_band(q[:, :, :512], k, v, plan)
    per_head = ops.band_plan([[0, 0, 0]] * 3, [[768] * 3] * 3, S, S, DEV)
    with pytest.raises(ApexMIError, match="bands for 3 heads, the operands have 2"):
        ops.attention_band(q, k, v, per_head)
    with pytest.raises(ApexMIError, match="must be an ops.BandPlan"):
        ops.attention_band(q, k, v, object())
    with pytest.raises(ApexMIError, match="bf16 only"):
        ops.attention_band(q.half(), k.half(), v.half(), plan)
    with pytest.raises(ApexMIError, match="head dim 64 unsupported"):
        ops.attention_band(q[..., :64], k[..., :64], v[..., :64], plan)


def test_no_host_synchronisation_graph_capture():
    q, k, v = _qkv(1, 2, 768, 768, 961)
    plan = ops.band_plan([0, 128, 384], [512, 768, 768], 768, 768, DEV)
    kp, vt = R.prepared(k, v)
    out = torch.empty((1, 768, 2, 128), dtype=BF, device=DEV)
    eager = ops.attention_prepared_band(q, kp, vt, out, 768, plan).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_prepared_band(q, kp, vt, out, 768, plan)        # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.attention_prepared_band(q, kp, vt, out, 768, plan)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- the Wan switch --------------------------------------------------------------------------------------------------------
WAN = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=512, num_layers=1, cross_attn_norm=True, eps=1e-6)
LATENT = (1, 16, 6, 16, 16)       # token grid (6, 8, 8): 64 tokens per frame, a block of 256 rows is four whole frames


@functools.lru_cache(maxsize=None)
def _wan_inputs():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(LATENT, generator=g)
    x2 = x.clone()
    x2[:, :, 0] += 0.5 * torch.randn(x[:, :, 0].shape, generator=g)          # latent frame 0 changes
    txt = torch.randn(1, 20, 64, generator=g)
    return x, x2, txt


@functools.lru_cache(maxsize=None)
def _wan():
    from apex_studio_amd.wan import WanTransformer3DModel
    return WanTransformer3DModel(**WAN, device=DEV, dtype=BF).init_synthetic(3)


def _wan_run(m, x):
    txt = _wan_inputs()[2]
    out = m(hidden_states=x.to(DEV), timestep=torch.tensor([500.0], device=DEV), encoder_hidden_states=txt.to(DEV, BF),
            return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def test_wan_full_band_is_the_dense_model_to_the_bit():
    m = _wan()
    x = _wan_inputs()[0]
    with R.forced_dense():
        dense = _wan_run(m, x)
        try:
            m.set_attention_band(LATENT[2])
            full = _wan_run(m, x)
            plan = next(iter(m._band_plans.values()))
            assert plan.kept_fraction == 1.0 and (plan.lo, plan.hi) == ([[0, 0]], [[384, 384]])
        finally:
            m.set_attention_band(None)
        assert torch.isfinite(full).all() and full.abs().max() > 0
        assert torch.equal(full, dense)
        assert torch.equal(_wan_run(m, x), dense)             # cleared: the dense launch again


@pytest.mark.parametrize("radius", [0, 1])
def test_wan_band_is_exactly_local_in_time(radius):
    """One block of the model; latent frame 0 changes.  No output token whose block's band excludes frame 0 changes, to the bit;
    every token whose band holds it does.  With the band off the perturbation reaches every frame."""
    m = _wan()
    x, x2, _ = _wan_inputs()
    try:
        m.set_attention_band(radius)
        a, b = _wan_run(m, x), _wan_run(m, x2)
        plan = next(iter(m._band_plans.values()))
    finally:
        m.set_attention_band(None)
    assert plan.nqb == 2 and torch.isfinite(a).all() and a.abs().max() > 0
    excluded = 0
    for blk in range(plan.nqb):
        frames = slice(4 * blk, min(4 * blk + 4, LATENT[2]))                   # 256 rows = four frames of 64 tokens
        sees_frame0 = plan.lo[0][blk] < 64
        excluded += not sees_frame0
        for f in range(frames.start, frames.stop):
            assert torch.equal(a[:, :, f], b[:, :, f]) != sees_frame0, (blk, f)
    assert excluded == 1                                                         # frames 4 and 5: band [256, 384) / [192, 384)
    a, b = _wan_run(m, x), _wan_run(m, x2)
    for f in range(LATENT[2]):
        assert not torch.equal(a[:, :, f], b[:, :, f]), f


def test_wan_band_and_window_are_mutually_exclusive():
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**WAN, device=DEV, dtype=BF)
    m.set_attention_window((1, 2, 2))
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.set_attention_band(1)
    m.set_attention_window(None)
    m.set_attention_band(1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        m.set_attention_window((1, 2, 2))


def test_wan_band_refuses_the_f32_storage_mode():
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**WAN, device=DEV, dtype=BF).init_synthetic(3)
    m.set_storage_dtype(torch.float32)
    m.set_attention_band(1)
    with pytest.raises(NotImplementedError, match="band"):
        _wan_run(m, _wan_inputs()[0])
