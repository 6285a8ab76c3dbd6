"""The "hip_mfma", "hip_mfma_sdpa", "hip_mfma_window", "hip_mfma_varlen" and "hip_mfma_band" attention backends — B-op plug-in point.

Honours the calling convention of every backend in the reference's attention_register
(apps/api/src/attention/functions.py:84, e.g. `sdpa` :338-377):

    fn(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False, softmax_scale=None, **kwargs) -> Tensor

q:[B,H,Sq,D], k,v:[B,H,Sk,D] (possibly permuted, non-contiguous views); returns [B,H,Sq,D] in q's
dtype without aliasing or modifying the inputs; enqueues on torch's current stream; no host sync when
`attn_mask` is None (every hot-path call: the reference forwards `attn_mask=attention_mask`, which is None there —
flux/base/attention.py:89-94, wan/base/attention.py:397-399, qwenimage/base/model.py:555-562).

A KEY-PADDING mask (bool keep-mask or additive 0 / -inf mask that does not vary along the query or head dimension:
[B, Sk], [B, 1, 1, Sk], [1, 1, 1, Sk], ...) — what a padded prompt batch brings — is honoured exactly: softmax over the
kept keys only, by running the same kernel over each sample's kept keys (a prefix is a view, anything else one gather).
It costs one host sync (the kept-key count sizes the launch).  Masks that vary along the query dimension, dropout and causal
attention are not on any call site of the path: they raise, they do not fall back.

"hip_mfma_sdpa" (KEY_SDPA) is the whole `sdpa` contract for manifests that need it (ops.attention_masked, one flash kernel):
any attn_mask broadcastable to [B, Hq, Sq, Sk] (bool keep-mask, or additive float32 / q's dtype), is_causal (top-left
aligned, AND-ed with the mask), grouped-query heads with enable_gqa, bf16 / f16, D = 64 or 128.  A query row with no allowed
key returns zeros (as torch's CPU sdpa).  No host sync for any input.  Dropout, other dtypes or head sizes and CPU tensors
raise ApexMIError; nothing falls back to torch.  `return_lse=True` (flash-attn's convention) returns (out, lse): lse [B, Hq, Sq]
float32, the natural-log row normaliser, -inf for a row with no allowed key; ops.attention_merge combines such pairs over
separate key sets.

"hip_mfma_window" (KEY_WINDOW) is coordinate-window sparse attention (ops.attention_window): the reference
calling convention plus `window_plan=` (an ops.WindowPlan from ops.window_plan) in **kwargs.  An opt-in approximation of the
caller's choosing: keys outside the window are not attended.  attn_mask, is_causal, dropout and a missing plan raise; nothing
falls back to dense attention.

"hip_mfma_varlen" (KEY_VARLEN) is attention over a packed variable-length batch (ops.attention_varlen), the
job of the reference's "sdpa_varlen" / "flash_varlen": the reference calling convention plus `cu_seqlens_q=, cu_seqlens_k=`
(int32 [n + 1] on the operands' device), `max_seqlen_q=, max_seqlen_k=` (host integers) and `enable_gqa=, return_lse=` in
**kwargs.  The operands are packed [T, H, D], or the registry's [1, H, T, D] views of such a batch; the result comes back in the
layout it was given ([T, Hq, D], or [1, Hq, T, D]; lse [Hq, T] or [1, Hq, T]).  One launch, no host sync: every sequence attends
its own keys only.  is_causal is top-left aligned per sequence.  attn_mask, dropout, a batch dimension other than 1 and missing
cu_seqlens / max_seqlen raise ApexMIError; nothing falls back to a per-sequence loop.

"hip_mfma_band" (KEY_BAND) is attention over per-block key bands (ops.attention_band): the reference calling
convention plus `band_plan=` (an ops.BandPlan from ops.band_plan / ops.frame_band_plan) in **kwargs.  Every block of 256 query
rows attends one contiguous key range, on the dense large-attention kernel: bf16, D = 128.  An opt-in approximation of the
caller's choosing, like the window.  attn_mask, is_causal, dropout and a missing plan raise; nothing falls back to dense
attention.  Registered on request (register(..., band=True)).
"""
from __future__ import annotations

import torch

from . import ops
from .lib import ApexMIError

KEY = "hip_mfma"
KEY_SDPA = "hip_mfma_sdpa"
KEY_WINDOW = "hip_mfma_window"
KEY_VARLEN = "hip_mfma_varlen"
KEY_BAND = "hip_mfma_band"


def hip_mfma(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False,
             softmax_scale=None, **kwargs):
    if dropout_p:
        raise ApexMIError("hip_mfma: dropout is not supported (inference only)")
    if is_causal:
        raise ApexMIError("hip_mfma: causal attention is not supported")
    if attn_mask is None:
        return ops.attention(q, k, v, softmax_scale)
    keep = _key_keep_mask(attn_mask, q.shape[0], k.shape[2])
    if bool(keep.all()):
        return ops.attention(q, k, v, softmax_scale)
    B, H, Sq, D = q.shape
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device).permute(0, 2, 1, 3)
    counts = keep.sum(dim=1).tolist()
    for b in range(B):
        n = int(counts[b])
        if n == 0:
            raise ApexMIError(f"hip_mfma: attn_mask drops every key of sample {b}")
        kb, vb = k[b:b + 1], v[b:b + 1]
        if bool(keep[b, :n].all()):               # a padded tail: the kept keys are a prefix (views, no copy)
            kb, vb = kb[:, :, :n], vb[:, :, :n]
        else:
            idx = keep[b].nonzero().flatten()
            kb, vb = kb.index_select(2, idx), vb.index_select(2, idx)
        out[b:b + 1].copy_(ops.attention(q[b:b + 1], kb, vb, softmax_scale))
    return out


def hip_mfma_sdpa(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False, softmax_scale=None,
                  enable_gqa: bool = False, return_lse: bool = False, **kwargs):
    if dropout_p > 0:
        raise ApexMIError("hip_mfma_sdpa: dropout is not supported (inference only)")
    # return_lse: (out, lse [B,Hq,Sq] float32), the partial result ops.attention_merge combines over key sets
    return ops.attention_masked(q, k, v, attn_mask, is_causal=is_causal, softmax_scale=softmax_scale, enable_gqa=enable_gqa,
                                return_lse=return_lse)


def hip_mfma_window(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False, softmax_scale=None,
                    enable_gqa: bool = False, window_plan=None, **kwargs):
    if dropout_p:
        raise ApexMIError("hip_mfma_window: dropout is not supported (inference only)")
    if is_causal:
        raise ApexMIError("hip_mfma_window: causal attention is not supported (use hip_mfma_sdpa)")
    if attn_mask is not None:
        raise ApexMIError("hip_mfma_window: attn_mask is not supported next to a window (use hip_mfma_sdpa with a mask)")
    if window_plan is None:
        raise ApexMIError("hip_mfma_window: window_plan= (ops.window_plan(...)) is required; there is no dense fallback")
    return ops.attention_window(q, k, v, window_plan, softmax_scale=softmax_scale, enable_gqa=enable_gqa)


def hip_mfma_varlen(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False, softmax_scale=None,
                    cu_seqlens_q=None, cu_seqlens_k=None, max_seqlen_q=None, max_seqlen_k=None, enable_gqa: bool = False,
                    return_lse: bool = False, **kwargs):
    if dropout_p:
        raise ApexMIError("hip_mfma_varlen: dropout is not supported (inference only)")
    if attn_mask is not None:
        raise ApexMIError("hip_mfma_varlen: attn_mask is not supported next to cu_seqlens (use hip_mfma_sdpa with a mask)")
    if cu_seqlens_q is None or cu_seqlens_k is None or max_seqlen_q is None or max_seqlen_k is None:
        raise ApexMIError("hip_mfma_varlen: cu_seqlens_q=, cu_seqlens_k=, max_seqlen_q= and max_seqlen_k= are required; there is "
                          "no dense fallback")
    dims = (q.dim(), k.dim(), v.dim())
    if dims not in ((3, 3, 3), (4, 4, 4)):
        raise ApexMIError(f"hip_mfma_varlen: q, k, v must all be packed [T, H, D] or all [1, H, T, D], got {dims} dims")
    batched = dims[0] == 4
    if batched:
        if q.shape[0] != 1 or k.shape[0] != 1 or v.shape[0] != 1:
            raise ApexMIError(f"hip_mfma_varlen: a packed batch has batch dimension 1, got {q.shape[0]} / {k.shape[0]} / {v.shape[0]} "
                              "(the sequences are told apart by cu_seqlens)")
        q, k, v = q[0].permute(1, 0, 2), k[0].permute(1, 0, 2), v[0].permute(1, 0, 2)      # [T, H, D] views
    res = ops.attention_varlen(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale=softmax_scale,
                               is_causal=is_causal, enable_gqa=enable_gqa, return_lse=return_lse)
    if not batched:
        return res
    if return_lse:
        return res[0][None].permute(0, 2, 1, 3), res[1][None]
    return res[None].permute(0, 2, 1, 3)


def hip_mfma_band(q, k, v, attn_mask=None, dropout_p: float = 0.0, is_causal: bool = False, softmax_scale=None, band_plan=None,
                  **kwargs):
    if dropout_p:
        raise ApexMIError("hip_mfma_band: dropout is not supported (inference only)")
    if is_causal:
        raise ApexMIError("hip_mfma_band: causal attention is not supported (use hip_mfma_sdpa)")
    if attn_mask is not None:
        raise ApexMIError("hip_mfma_band: attn_mask is not supported next to a band plan (use hip_mfma_sdpa with a mask)")
    if band_plan is None:
        raise ApexMIError("hip_mfma_band: band_plan= (ops.band_plan(...) / ops.frame_band_plan(...)) is required; there is no "
                          "dense fallback")
    return ops.attention_band(q, k, v, band_plan, softmax_scale=softmax_scale)


def _key_keep_mask(attn_mask: torch.Tensor, B: int, Sk: int) -> torch.Tensor:
    """attn_mask (bool keep-mask, or additive: finite-and-not-hugely-negative = keep) -> bool [B, Sk]; raises unless the mask
    is constant along the head and query dimensions."""
    m = attn_mask
    if m.dim() == 2:
        if m.shape[-1] != Sk or m.shape[0] not in (1, B):
            raise ApexMIError(f"hip_mfma: attn_mask shape {tuple(m.shape)} is not a [B, Sk] key-padding mask")
        m = m[:, None, None, :]
    if m.dim() == 3:
        m = m[:, None]
    if m.dim() != 4 or m.shape[-1] != Sk or m.shape[1] != 1 or m.shape[2] != 1 or m.shape[0] not in (1, B):
        raise ApexMIError(f"hip_mfma: attn_mask of shape {tuple(attn_mask.shape)} varies along the head / query dimension; only "
                          "key-padding masks ([B, Sk], [B, 1, 1, Sk]) are supported")
    keep = m[:, 0, 0, :]
    if keep.dtype != torch.bool:
        keep = torch.isfinite(keep) & (keep > -1e4)
    return keep.expand(B, Sk)


def available() -> bool:
    """True when the HIP library is built and a ROCm device is visible."""
    try:
        from . import lib
        lib.load()
    except Exception:
        return False
    return torch.cuda.is_available()


def register(attention_register, set_default: bool = False, overwrite: bool = True, varlen: bool = False, band: bool = False):
    """Register under KEY, KEY_SDPA and KEY_WINDOW in the given FunctionRegister (the reference's, or register.attention_register);
    set_default makes KEY the default.  varlen=True adds KEY_VARLEN next to them: the key takes packed operands and cu_seqlens,
    so a manifest asks for it.  band=True adds KEY_BAND in the same way: the key needs a band plan."""
    ok = available()
    attention_register(KEY, overwrite=overwrite, available=ok)(hip_mfma)
    attention_register(KEY_SDPA, overwrite=overwrite, available=ok)(hip_mfma_sdpa)
    attention_register(KEY_WINDOW, overwrite=overwrite, available=ok)(hip_mfma_window)
    if varlen:
        attention_register(KEY_VARLEN, overwrite=overwrite, available=ok)(hip_mfma_varlen)
    if band:
        attention_register(KEY_BAND, overwrite=overwrite, available=ok)(hip_mfma_band)
    if set_default:
        attention_register.set_default(KEY)
    return attention_register


def register_models(transformers_registry, vae_registry=None):
    """Register the drop-in component classes (B-model) next to "flux.base" / "wan.base" /
    "qwenimage.base" / "hunyuanvideo15.base" (reference transformer/base.py:3; auto-scan transformer/__init__.py:21-84)."""
    from .flux import FluxTransformer2DModel
    from .hunyuan15 import HunyuanVideo15Transformer3DModel
    from .qwenimage import QwenImageTransformer2DModel
    from .wan import WanTransformer3DModel
    ok = available()
    transformers_registry("flux.mi355", overwrite=True, available=ok)(FluxTransformer2DModel)
    transformers_registry("wan.mi355", overwrite=True, available=ok)(WanTransformer3DModel)
    transformers_registry("qwenimage.mi355", overwrite=True, available=ok)(QwenImageTransformer2DModel)
    transformers_registry("hunyuanvideo15.mi355", overwrite=True, available=ok)(HunyuanVideo15Transformer3DModel)
    if vae_registry is not None:   # reference vae/__init__.py:9-73 (keys "auto" | "wan" | "qwenimage" | "hunyuanvideo15")
        from .vae_flux import AutoencoderKL
        from .vae_hunyuan15 import AutoencoderKLHunyuanVideo15
        from .vae_wan import AutoencoderKLWan
        vae_registry("auto_mi355", overwrite=True, available=ok)(AutoencoderKL)
        vae_registry("wan_mi355", overwrite=True, available=ok)(AutoencoderKLWan)
        vae_registry("qwenimage_mi355", overwrite=True, available=ok)(AutoencoderKLWan)
        vae_registry("hunyuanvideo15_mi355", overwrite=True, available=ok)(AutoencoderKLHunyuanVideo15)
    return transformers_registry
