"""Coordinate-window sparse attention on the GPU (ops.window_plan / attention_window / attention_prepared_window, the
"hip_mfma_window" backend, WanTransformer3DModel.set_attention_window).  The witness everywhere is torch's CPU sdpa in f32 on the
upcast inputs with the dense bool mask of the window rule; against ops.attention_masked on that mask the window kernel is
bit-identical."""
import functools

import pytest
import torch
import torch.nn.functional as F

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import ops
from tests.conftest import measured
from tests.test_gpu_sdpa_masked import BARS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16

# (grid, radius): S and the SKIP / DENSE / PARTIAL tile counts of the equivalent dense mask over 128 x 64 blocks
CASES = {
    1: ((6, 10, 12), (1, 9, 11)),     # 720: 28 / 20 / 24
    2: ((6, 10, 12), (1, 2, 3)),      # 720: 32 / 0 / 40
    3: ((5, 9, 13), (1, 8, 12)),      # 585, both tails ragged: 15 / 17 / 18
    4: ((12, 8, 8), (2, 7, 7)),       # 768: 40 / 22 / 10
    5: ((12, 8, 8), (1, 2, 2)),       # 768: 50 / 0 / 22
}
COUNTS = {1: (28, 20, 24), 2: (32, 0, 40), 3: (15, 17, 18), 4: (40, 22, 10), 5: (50, 0, 22)}


def _raster(grid):
    f, h, w = grid
    return torch.stack(torch.meshgrid(torch.arange(f), torch.arange(h), torch.arange(w), indexing="ij"), dim=-1).reshape(-1, 3)


def _dense_mask(cq, ck, radius):
    d = (cq[:, None, :] - ck[None, :, :]).abs()
    return (d <= torch.tensor(radius)).all(dim=-1)


def _map_of(mask):
    """CPU restatement of the block map of a dense bool mask: 0 SKIP (no allowed pair), 1 DENSE (all pairs allowed), 2 PARTIAL, per
    (128-row query block, 64-key tile); rows / keys past the ends belong to no pair."""
    Sq, Sk = mask.shape
    nqb, nkt = (Sq + 127) // 128, (Sk + 63) // 64
    out = torch.empty(nqb, nkt, dtype=torch.uint8)
    for i in range(nqb):
        for j in range(nkt):
            blk = mask[i * 128:(i + 1) * 128, j * 64:(j + 1) * 64]
            out[i, j] = 0 if not blk.any() else 1 if blk.all() else 2
    return out


def _counts(bmap):
    return tuple(int((bmap == c).sum()) for c in (0, 1, 2))


@functools.lru_cache(maxsize=None)
def _case(n):
    grid, radius = CASES[n]
    c = _raster(grid)
    mask = _dense_mask(c, c, radius)
    bmap = _map_of(mask)
    skip, dense, part = _counts(bmap)
    assert (skip, dense, part) == COUNTS[n]
    assert skip > 0 and part > 0 and (dense > 0 or n in (2, 5))         # no case degenerates
    assert mask.any(dim=1).all()                                         # every row has an allowed key
    return c, radius, mask, bmap


@functools.lru_cache(maxsize=None)
def _qkv(B, Hq, Sq, Sk, D, dtype, Hkv=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    Hkv = Hq if Hkv is None else Hkv
    return (torch.randn(B, Hq, Sq, D, generator=g).to(dtype), torch.randn(B, Hkv, Sk, D, generator=g).to(dtype),
            torch.randn(B, Hkv, Sk, D, generator=g).to(dtype))


@functools.lru_cache(maxsize=None)
def _witness(n, D, dtype, Hq=4, Hkv=None):
    mask = _case(n)[2]
    q, k, v = _qkv(2, Hq, mask.shape[0], mask.shape[1], D, dtype, Hkv)
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=mask, enable_gqa=Hkv is not None)


def _rel(out, ref):
    return float((out.float() - ref).norm() / ref.norm())


def _plan(n):
    c, radius = _case(n)[:2]
    return ops.window_plan(c.to(DEV), radius=radius)


@pytest.mark.parametrize("n,D,dtype", [(n, 128, BF) for n in CASES] + [(1, 64, torch.float16), (3, 64, torch.float16)])
def test_matches_torch_sdpa_on_the_dense_mask(n, D, dtype):
    S = _case(n)[2].shape[0]
    q, k, v = (t.to(DEV) for t in _qkv(2, 4, S, S, D, dtype))
    out = ops.attention_window(q, k, v, _plan(n))
    torch.cuda.synchronize()
    name = "bf16" if dtype == BF else "f16"
    measured(f"window case {n} D{D} {name}", _rel(out.cpu(), _witness(n, D, dtype)), BARS[name])


@pytest.mark.parametrize("n", list(CASES))
def test_device_map_equals_the_dense_masks_map(n):
    _, _, mask, bmap = _case(n)
    plan = _plan(n)
    assert plan.block_map.dtype == torch.uint8 and tuple(plan.block_map.shape) == tuple(bmap.shape)
    assert torch.equal(plan.block_map.cpu(), bmap)
    assert plan.tile_counts() == COUNTS[n]
    assert (plan.Sq, plan.Sk) == tuple(mask.shape) and plan.k_coords is plan.q_coords


@pytest.mark.parametrize("n,D,dtype", [(n, 128, BF) for n in CASES] + [(1, 64, torch.float16), (3, 64, torch.float16)])
def test_bit_identical_to_the_masked_kernel(n, D, dtype):
    mask = _case(n)[2]
    S = mask.shape[0]
    q, k, v = (t.to(DEV) for t in _qkv(2, 4, S, S, D, dtype))
    out = ops.attention_window(q, k, v, _plan(n))
    ref = ops.attention_masked(q, k, v, mask.to(DEV))
    assert torch.equal(out, ref)


@pytest.mark.parametrize("n", [1, 3])
def test_prepared_entry_is_bit_identical_too(n):
    mask = _case(n)[2]
    S, H = mask.shape[0], 4
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(S, 3 * H * 128, generator=g).to(BF).to(DEV)
    q_in, k_in, v_in = qkv[:, :H * 128], qkv[:, H * 128:2 * H * 128], qkv[:, 2 * H * 128:]
    Q, K = torch.empty(1, H, S, 128, dtype=BF, device=DEV), torch.empty(1, H, S, 128, dtype=BF, device=DEV)
    VT = torch.zeros(1, H, 128, (S + 63) // 64 * 64, dtype=BF, device=DEV)
    ops.qkv_prepare(q_in, k_in, v_in, H, Q[0], K[0], VT[0])
    out = torch.empty(1, S, H, 128, dtype=BF, device=DEV)
    ops.attention_prepared_window(Q, K, VT, out, S, _plan(n))
    v4 = v_in.unflatten(-1, (H, 128)).permute(1, 0, 2).unsqueeze(0)          # [1, H, S, 128] view of the projection
    ref = ops.attention_masked(Q, K, v4, mask.to(DEV))
    assert torch.equal(out.permute(0, 2, 1, 3), ref)


def test_cross_shapes_and_a_row_without_keys():
    cq, ck, radius = _raster((5, 9, 13)).clone(), _raster((6, 10, 12)), (1, 4, 6)
    planted = 301
    cq[planted] = torch.tensor([100, 100, 100])                              # far from every key
    mask = _dense_mask(cq, ck, radius)
    assert not mask[planted].any() and mask.any(dim=1).sum() == mask.shape[0] - 1
    skip, dense, part = _counts(_map_of(mask))
    assert skip > 0 and part > 0
    Sq, Sk = mask.shape
    q, k, v = _qkv(2, 4, Sq, Sk, 128, BF, seed=3)
    plan = ops.window_plan(cq, ck.to(DEV), radius=radius)                    # a CPU tensor is moved once
    assert torch.equal(plan.block_map.cpu(), _map_of(mask))
    out = ab.hip_mfma_window(q.to(DEV), k.to(DEV), v.to(DEV), window_plan=plan).cpu()
    assert out.shape == q.shape and (out[:, :, planted] == 0).all()
    ref = F.scaled_dot_product_attention(q.float(), k.float(), v.float(), attn_mask=mask)
    rows = [i for i in range(Sq) if i != planted]
    measured("window cross shapes", _rel(out[:, :, rows], ref[:, :, rows]), BARS["bf16"])
    assert torch.equal(out.to(DEV), ops.attention_masked(q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV)))


def test_grouped_query_heads():
    S = _case(1)[2].shape[0]
    q, k, v = (t.to(DEV) for t in _qkv(2, 8, S, S, 128, BF, 2))
    out = ops.attention_window(q, k, v, _plan(1), enable_gqa=True)
    measured("window gqa 8/2", _rel(out.cpu(), _witness(1, 128, BF, 8, 2)), BARS["bf16"])
    assert torch.equal(out, ops.attention_masked(q, k, v, _case(1)[2].to(DEV), enable_gqa=True))
    with pytest.raises(ops._l.ApexMIError, match="enable_gqa"):
        ops.attention_window(q, k, v, _plan(1))


def test_permuted_views_scale_and_plan_mismatch():
    S = _case(3)[2].shape[0]
    q, k, v = (t.to(DEV) for t in _qkv(2, 4, S, S, 128, BF))
    plan = _plan(3)
    qv, kv, vv = (t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) for t in (q, k, v))     # [B, S, H, D] storage
    assert torch.equal(ops.attention_window(qv, kv, vv, plan, softmax_scale=0.05),
                       ops.attention_masked(q, k, v, _case(3)[2].to(DEV), softmax_scale=0.05))
    with pytest.raises(ops._l.ApexMIError, match="window plan is for"):
        ops.attention_window(q[:, :, :100], k, v, plan)
    with pytest.raises(ops._l.ApexMIError, match="window_plan"):
        ab.hip_mfma_window(q, k, v)


def test_no_host_sync_and_graph_capture():
    S = _case(3)[2].shape[0]
    q, k, v = (t.to(DEV) for t in _qkv(2, 4, S, S, 128, BF))
    plan = _plan(3)
    eager = ops.attention_window(q, k, v, plan)          # warm-up: workspace allocated, kernel attributes set
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ops.attention_window(q, k, v, plan)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.equal(again, eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_window(q, k, v, plan)              # warm-up on the capture stream (its own workspace)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = ops.attention_window(q, k, v, plan)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


# ---- the Wan switch --------------------------------------------------------------------------------------------------------
WAN = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=512, num_layers=1, cross_attn_norm=True, eps=1e-6)
LATENT = (1, 16, 6, 16, 16)       # token grid (6, 8, 8): 64 tokens per frame, so no 32-row wave holds rows of two frames
BIG = 1000


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


def test_wan_window_is_exactly_local_in_time():
    """One block, window (f, all, all): a token's output depends on the latent frames within f of its own and on nothing else, to
    the bit (a 32-row wave of the kernel holds rows of ONE frame here, so no rescaling decision crosses frames).  With the window
    off the same perturbation reaches every frame."""
    m = _wan()
    x, x2, _ = _wan_inputs()
    try:
        m.set_attention_window((0, BIG, BIG))
        a, b = _wan_run(m, x), _wan_run(m, x2)
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a[:, :, 1:], b[:, :, 1:]) and not torch.equal(a[:, :, 0], b[:, :, 0])
        m.set_attention_window((1, BIG, BIG))
        a, b = _wan_run(m, x), _wan_run(m, x2)
        assert torch.equal(a[:, :, 2:], b[:, :, 2:])
        assert not torch.equal(a[:, :, 1], b[:, :, 1]) and not torch.equal(a[:, :, 0], b[:, :, 0])
    finally:
        m.set_attention_window(None)
    a, b = _wan_run(m, x), _wan_run(m, x2)
    for f in range(LATENT[2]):
        assert not torch.equal(a[:, :, f], b[:, :, f]), f


LATENT_W64 = (1, 16, 70, 32, 32)  # token grid (70, 16, 16): 17 920 tokens x 2 heads = 140 workgroups of 256 rows, the dense w64 launch
WAN_FULL_BAR = 1.6e-4             # measured 8.07e-5 (rel L2 of the model output, full window vs the dense forward)


def _wan_full_window(x):
    m = _wan()
    dense = _wan_run(m, x)
    try:
        m.set_attention_window((BIG, BIG, BIG))
        full = _wan_run(m, x)
        assert m._window_plans and next(iter(m._window_plans.values())).tile_counts()[0::2] == (0, 0)     # every tile DENSE
    finally:
        m.set_attention_window(None)
    assert torch.equal(_wan_run(m, x), dense)                                 # cleared: the dense launch again, same bits
    return full, dense


def test_wan_full_window_is_the_dense_model():
    """Radii >= the grid allow every key: the dense model's function through the window kernel.  At video sizes the dense path
    launches another kernel (256-row workgroups, a fixed integer maximum per row), so the two agree to like-for-like rounding
    noise and not to the bit: the bar is 2 x the value measured on the MI355X against the dense forward."""
    g = torch.Generator().manual_seed(12)
    full, dense = _wan_full_window(torch.randn(LATENT_W64, generator=g))
    measured("wan full window vs dense (w64 launch)", _rel(full, dense), WAN_FULL_BAR)


def test_wan_full_window_small_launch_is_bit_equal():
    """Under 140 dense workgroups the dense path runs the 4-wave kernel the window kernel is built from (128-row workgroups, the
    same tile order and rescaling rule), and the full window reproduces it exactly: rel L2 measured 0.0 on the MI355X, so the bar
    is equality."""
    full, dense = _wan_full_window(_wan_inputs()[0])
    assert torch.equal(full, dense)


def test_wan_window_refuses_the_f32_storage_mode():
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**WAN, device=DEV, dtype=BF).init_synthetic(3)
    m.set_storage_dtype(torch.float32)
    m.set_attention_window((1, 2, 2))
    with pytest.raises(NotImplementedError, match="window"):
        _wan_run(m, _wan_inputs()[0])
