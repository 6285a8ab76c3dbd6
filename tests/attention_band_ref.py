"""Shared pieces of the band-attention tests (tests/test_attention_band_host.py, tests/test_gpu_attention_band.py): the frame-band
arithmetic restated as a brute-force loop over rows and keys, the exact +-radius frame mask, the slack the plan's docstring allows,
an f32 softmax over a bool mask, and the GPU helpers: prepared operands, the dense launch forced onto the kernel the band shares,
and the dense call on one block's rows and key slice."""
import contextlib

import torch

BF = torch.bfloat16
QB, KV = 256, 64          # rows of a query block (one workgroup), keys of a tile


def frame_of(i: int, tokens_per_frame: int) -> int:
    return i // tokens_per_frame


def brute_frame_bands(frames: int, tokens_per_frame: int, radius: int):
    """(lo, hi) per block of 256 rows: the smallest 64-aligned key range (hi capped at S) that holds every key whose frame is
    within `radius` of the frame of any row of the block.  Loops over every row and every key."""
    S = frames * tokens_per_frame
    lo, hi = [], []
    for b in range((S + QB - 1) // QB):
        row_frames = {frame_of(i, tokens_per_frame) for i in range(QB * b, min(QB * b + QB, S))}
        keys = [j for j in range(S) if any(abs(f - frame_of(j, tokens_per_frame)) <= radius for f in row_frames)]
        lo.append(min(keys) // KV * KV)
        hi.append(min(S, (max(keys) + 1 + KV - 1) // KV * KV))
    return lo, hi


def exact_frame_mask(frames: int, tokens_per_frame: int, radius: int) -> torch.Tensor:
    """bool [S, S]: |frame(i) - frame(j)| <= radius"""
    f = torch.arange(frames * tokens_per_frame) // tokens_per_frame
    return (f[:, None] - f[None, :]).abs() <= radius


def slack_frame_mask(frames: int, tokens_per_frame: int, radius: int) -> torch.Tensor:
    """bool [S, S]: the most a frame band may hold.  Row i of the block with frames f0 ... f1 may see the keys of the frames
    f0 - radius ... f1 + radius (what the frames one block straddles add) and less than one 64-key tile beyond each end."""
    S = frames * tokens_per_frame
    m = torch.zeros(S, S, dtype=torch.bool)
    for b in range((S + QB - 1) // QB):
        r0, r1 = QB * b, min(QB * b + QB, S)
        f0, f1 = r0 // tokens_per_frame, (r1 - 1) // tokens_per_frame
        a = max(0, max(0, f0 - radius) * tokens_per_frame - (KV - 1))
        e = min(S, (f1 + radius + 1) * tokens_per_frame + (KV - 1))
        m[r0:r1, a:e] = True
    return m


def masked_softmax_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, scale: float) -> torch.Tensor:
    """f32 softmax(q k^T scale over mask) v on the CPU; q [B,H,Sq,D], k / v [B,H,Sk,D], mask bool broadcastable to [B,H,Sq,Sk]"""
    s = torch.matmul(q.float().cpu(), k.float().cpu().transpose(-1, -2)) * scale
    s = s.masked_fill(~mask, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v.float().cpu())


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------
def prepared(k: torch.Tensor, v: torch.Tensor):
    """k, v [B,H,Sk,128] bf16 on the device -> (k packed, V^T [B,H,128,Skp] zero padded): the prepared operands"""
    from apex_studio_amd import ops
    B, H, Sk, D = k.shape
    skp = (Sk + KV - 1) // KV * KV
    vt = torch.empty((B, H, D, skp), dtype=BF, device=k.device)
    for b in range(B):
        ops.v_transpose(v[b].permute(1, 0, 2), vt[b])
    return k.contiguous(), vt


@contextlib.contextmanager
def forced_dense():
    """dense launches on the kernel the band shares, whatever their size: 256-row workgroups, no split tail, the shipped loop"""
    from apex_studio_amd import lib
    lib.tune_set("attn.waves", 8)
    lib.tune_set("attn.split", 0)
    lib.tune_set("attn.w64", 1)
    try:
        yield
    finally:
        lib.tune_set("attn.waves", 0)
        lib.tune_set("attn.split", 1)
        lib.tune_set("attn.w64", 1)


def dense_block(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, b: int, lo: int, hi: int, scale=None) -> torch.Tensor:
    """ops.attention_prepared (call inside forced_dense) on the rows of query block b and freshly prepared k[lo:hi] / v[lo:hi]:
    [B, rows, H, 128]"""
    from apex_studio_amd import ops
    qb = q[:, :, QB * b:QB * b + QB].contiguous()
    kp, vt = prepared(k[:, :, lo:hi].contiguous(), v[:, :, lo:hi].contiguous())
    out = torch.empty((q.shape[0], qb.shape[2], q.shape[1], 128), dtype=BF, device=q.device)
    return ops.attention_prepared(qb, kp, vt, out, hi - lo, scale)


def band_prepared(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, plan, scale=None) -> torch.Tensor:
    """ops.attention_prepared_band on freshly prepared operands: [B, Sq, H, 128]"""
    from apex_studio_amd import ops
    kp, vt = prepared(k, v)
    out = torch.empty((q.shape[0], q.shape[2], q.shape[1], 128), dtype=BF, device=q.device)
    return ops.attention_prepared_band(q.contiguous(), kp, vt, out, k.shape[2], plan, scale)
