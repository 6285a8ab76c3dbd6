"""WanTransformer3DModel on the MI355X HIP ops — drop-in for registry key "wan.base" (text-to-video).

Mirrors the reference class (apps/api/src/transformer/wan/base/model.py:1336-1891): same config, same
state-dict keys (blocks.N.attn1.to_q.weight, blocks.N.scale_shift_table, condition_embedder.*), same
`forward(hidden_states [B,16,F,H,W], timestep [B], encoder_hidden_states [B,512,4096], return_dict=False)`.
Memory knobs of the reference that exist for 8-24 GB GPUs (`set_chunking_profile`, `rope_on_cpu`,
`enable_easy_cache`) are accepted and ignored: one 75 600-token activation is 0.77 GB of 288 GB.

Per block (reference model.py:1101-1333 + attention.py:305-413), as libapex_mi355.so launches:
  ln_modulate -> fused QKV gemm -> RMSNorm over all 5120 channels on q and k (in place)
  -> qkv_prepare (RoPE + attention layout + V^T) -> attention -> out-proj gemm (gate * y + residual)
  -> affine LayerNorm -> q gemm + RMSNorm | text k,v gemm + RMSNorm -> prepare x2 -> cross attention
  -> out-proj gemm (+ residual) -> ln_modulate -> FFN-up gemm (+GELU) -> FFN-down gemm (gate + residual)

Image conditioning (Wan-2.1 I2V / FLF2V: `image_dim`, `added_kv_proj_dim`, optional `pos_embed_seq_len`; diffusers
WanImageEmbedding / WanAttnProcessor with add_k_proj, which the reference's base model mirrors: model.py:207, 391-394):
`forward(..., encoder_hidden_states_image [B, 257 n, image_dim])` runs the image embedder once per call
(+pos_embed -> affine LayerNorm -> Linear + erf GELU -> Linear -> affine LayerNorm), and each block's cross-attention adds
  fused image k|v gemm -> RMSNorm (norm_added_k) on k -> prepare -> ONE two-context attention launch
  (apexmi_attn_fwd_prepared_dual: text and image keys in separate softmaxes, bf16 branch results added in bf16)
in place of the single text attention.  Without image input (or without `added_kv_proj_dim`) the text-only path runs the
same launches as before.  The IP adapter and `use_enhance` raise NotImplementedError.
"""
from __future__ import annotations

import math
import os
from types import SimpleNamespace
from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn


from . import lib as _l
from . import ops
from .module_base import F32ResidualMixin, Fp4ComputeMixin, Fp6ComputeMixin, Fp8ResidentMixin, HipTransformer, _Config, _FF, _Linear, _Norm, _fuse_linears


class _WanAttn(nn.Module):
    def __init__(self, dim: int, heads: int, **kw):
        super().__init__()
        self.heads = heads
        self.to_q, self.to_k, self.to_v = _Linear(dim, dim, **kw), _Linear(dim, dim, **kw), _Linear(dim, dim, **kw)
        self.to_out = nn.ModuleList([_Linear(dim, dim, **kw), nn.Identity()])
        self.norm_q, self.norm_k = _Norm(dim, **kw), _Norm(dim, **kw)


class _AffineNorm(nn.Module):
    def __init__(self, dim: int, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=dtype), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(dim, device=device, dtype=dtype), requires_grad=False)


class _WanBlock(nn.Module):
    def __init__(self, dim: int, ffn_dim: int, heads: int, cross_attn_norm: bool, added_kv_proj_dim: Optional[int] = None,
                 **kw):
        super().__init__()
        self.attn1 = _WanAttn(dim, heads, **kw)
        self.attn2 = _WanAttn(dim, heads, **kw)
        if added_kv_proj_dim is not None:   # image branch of the cross-attention (diffusers WanAttention, added_kv_proj_dim)
            self.attn2.add_k_proj = _Linear(added_kv_proj_dim, dim, **kw)
            self.attn2.add_v_proj = _Linear(added_kv_proj_dim, dim, **kw)
            self.attn2.norm_added_k = _Norm(dim, **kw)
        self.norm2 = _AffineNorm(dim, **kw) if cross_attn_norm else nn.Identity()
        self.ffn = _FF(dim, ffn_dim, **kw)
        self.scale_shift_table = nn.Parameter(torch.empty(1, 6, dim, **kw), requires_grad=False)


class _ImageEmbedder(nn.Module):
    """diffusers WanImageEmbedding: FP32LayerNorm (affine, eps 1e-5) -> FeedForward(mult=1, exact GELU) -> FP32LayerNorm; an
    optional learned position embedding over the FLF2V pair's 2 x 257 tokens."""

    def __init__(self, image_dim: int, dim: int, pos_embed_seq_len: Optional[int], **kw):
        super().__init__()
        self.norm1 = _AffineNorm(image_dim, **kw)
        self.ff = nn.Module()
        proj = nn.Module()
        proj.proj = _Linear(image_dim, image_dim, **kw)
        self.ff.net = nn.ModuleList([proj, nn.Identity(), _Linear(image_dim, dim, **kw)])
        self.norm2 = _AffineNorm(dim, **kw)
        if pos_embed_seq_len is not None:
            self.pos_embed = nn.Parameter(torch.zeros(1, pos_embed_seq_len, image_dim, **kw), requires_grad=False)
        else:
            self.pos_embed = None


class _TimeEmb(nn.Module):
    def __init__(self, a: int, b: int, **kw):
        super().__init__()
        self.linear_1, self.linear_2 = _Linear(a, b, **kw), _Linear(b, b, **kw)


class _Cond(nn.Module):
    def __init__(self, dim: int, freq_dim: int, proj_dim: int, text_dim: int, image_dim: Optional[int] = None,
                 pos_embed_seq_len: Optional[int] = None, **kw):
        super().__init__()
        self.time_embedder = _TimeEmb(freq_dim, dim, **kw)
        self.time_proj = _Linear(dim, proj_dim, **kw)
        self.text_embedder = _TimeEmb(text_dim, dim, **kw)
        if image_dim is not None:
            self.image_embedder = _ImageEmbedder(image_dim, dim, pos_embed_seq_len, **kw)


class _Conv3dParams(nn.Module):
    def __init__(self, cin: int, cout: int, k, **kw):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, *k, **kw), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout, **kw), requires_grad=False)


class WanTransformer3DModel(Fp8ResidentMixin, Fp4ComputeMixin, Fp6ComputeMixin, F32ResidualMixin, HipTransformer):
    _converter_base = "wan.base"      # which key-converter table original-format weight files / LoRAs go through (converters.py)
    _tag = "wan.mi355"
    _drops = {"moved": ("_packed", "_ws", "_rope", "_window_plans", "_band_plans"), "loaded": ("_packed",), "storage": ("_ws",)}
    _no_split_modules = ["_WanBlock"]

    def __init__(self, patch_size: Tuple[int, int, int] = (1, 2, 2), num_attention_heads: int = 40,
                 attention_head_dim: int = 128, in_channels: int = 16, out_channels: int = 16,
                 text_dim: int = 4096, freq_dim: int = 256, ffn_dim: int = 13824, num_layers: int = 40,
                 cross_attn_norm: bool = True, qk_norm: Optional[str] = "rms_norm_across_heads",
                 eps: float = 1e-6, image_dim: Optional[int] = None, added_kv_proj_dim: Optional[int] = None,
                 rope_max_seq_len: int = 1024, pos_embed_seq_len: Optional[int] = None, ip_adapter: bool = False,
                 use_enhance: bool = False, ffn_chunk_size: Optional[int] = None, ffn_chunk_dim: int = 1,
                 device=None, dtype=torch.bfloat16):
        super().__init__()
        if attention_head_dim != 128:
            raise _l.ApexMIError("wan.mi355: attention_head_dim must be 128 (MFMA attention tile)")
        if ip_adapter or use_enhance:
            raise NotImplementedError("wan.mi355: IP adapter / enhance are outside the hot-path scope")
        if image_dim is not None and added_kv_proj_dim is None:
            raise NotImplementedError("wan.mi355: image_dim without added_kv_proj_dim (image tokens that no cross-attention "
                                      "reads) is not a Wan image-to-video configuration")
        if added_kv_proj_dim is not None and image_dim is None:
            raise ValueError("wan.mi355: added_kv_proj_dim needs image_dim (the image embedder feeds add_k_proj / add_v_proj)")
        if image_dim is not None and image_dim % 64:
            raise ValueError(f"wan.mi355: image_dim={image_dim} must be a multiple of 64 (the image embedder's GEMM K)")
        if added_kv_proj_dim is not None and added_kv_proj_dim != num_attention_heads * attention_head_dim:
            raise ValueError(f"wan.mi355: added_kv_proj_dim={added_kv_proj_dim} must equal the model width "
                             f"{num_attention_heads * attention_head_dim} (the image embedder's output)")
        if qk_norm != "rms_norm_across_heads":
            raise NotImplementedError(f"wan.mi355: qk_norm={qk_norm!r}")
        self.config = _Config(patch_size=tuple(patch_size), num_attention_heads=num_attention_heads,
                              attention_head_dim=attention_head_dim, in_channels=in_channels,
                              out_channels=out_channels, text_dim=text_dim, freq_dim=freq_dim, ffn_dim=ffn_dim,
                              num_layers=num_layers, cross_attn_norm=cross_attn_norm, qk_norm=qk_norm, eps=eps,
                              image_dim=image_dim, added_kv_proj_dim=added_kv_proj_dim,
                              rope_max_seq_len=rope_max_seq_len, pos_embed_seq_len=pos_embed_seq_len)
        kw = dict(device=device, dtype=dtype)
        self.inner_dim = dim = num_attention_heads * attention_head_dim
        self.patch_embedding = _Conv3dParams(in_channels, dim, tuple(patch_size), **kw)
        self.condition_embedder = _Cond(dim, freq_dim, dim * 6, text_dim, image_dim, pos_embed_seq_len, **kw)
        self.blocks = nn.ModuleList([_WanBlock(dim, ffn_dim, num_attention_heads, cross_attn_norm, added_kv_proj_dim, **kw)
                                     for _ in range(num_layers)])
        self.proj_out = _Linear(dim, out_channels * math.prod(patch_size), **kw)
        self.scale_shift_table = nn.Parameter(torch.empty(1, 2, dim, **kw), requires_grad=False)
        self._packed = False
        self._ws: Dict[Any, Any] = {}
        self.fuse_qkv = os.environ.get("APEX_FUSE_QKV", "1") != "0"     # see _forward_one
        self._rope: Dict[Any, torch.Tensor] = {}
        self._attention_window: Optional[Tuple[int, int, int]] = None     # set_attention_window
        self._window_plans: Dict[Any, Any] = {}
        self._attention_band: Optional[int] = None     # set_attention_band
        self._band_plans: Dict[Any, Any] = {}

    # ---- reference-compatible plumbing: module_base (from_config, set_storage_dtype / set_residual_dtype, the no-op knobs, ...) ----
    def _anchor(self):
        return self.proj_out.weight

    def enable_easy_cache(self, num_steps: int, thresh: float, ret_steps: int = 10, should_reset_global_cache: bool = True):
        """The reference's EasyCache switch (R/src/transformer/wan/base/model.py:1645-1672): from now on `forward` serves
        conditional / unconditional call pairs from the cache while the accumulated predicted change stays under `thresh`
        (easycache.py).  `should_reset_global_cache=False` keeps the running state (the reference's state is global)."""
        from .easycache import EasyCache
        if should_reset_global_cache or getattr(self, "_easy_cache", None) is None:
            self._easy_cache = EasyCache(num_steps, thresh, ret_steps)
        else:
            ec = self._easy_cache
            ec.num_steps, ec.thresh, ec.ret_steps = int(num_steps) * 2, float(thresh), int(ret_steps) * 2
        return self

    def share_easy_cache_state(self, other):
        """Continue `other`'s EasyCache state on this model (the reference's state is module-global, so the low-noise expert
        picks up where the high-noise one stopped: R/src/engine/wan/shared/__init__.py:435-444 enables it with
        `should_reset_global_cache=False`).  Follow with `enable_easy_cache(..., should_reset_global_cache=False)`."""
        self._easy_cache = getattr(other, "_easy_cache", None)
        return self

    def disable_easy_cache(self):
        self._easy_cache = None
        return self

    def set_attention_window(self, radius: Optional[Tuple[int, int, int]]):
        """Opt-in approximation: self-attention attends only the keys within `radius` = (frames, rows, cols) of
        the query on the post-patch token grid (|df| <= frames, |dh| <= rows, |dw| <= cols); None restores dense attention.
        Cross-attention and everything else is untouched.  Not a quality claim: the caller picks the window."""
        if radius is not None:
            try:
                radius = tuple(int(r) for r in radius)
            except TypeError as err:
                raise ValueError(f"wan.mi355: attention window radius must be (frames, rows, cols), got {radius!r}") from err
            if len(radius) != 3 or any(r < 0 for r in radius):
                raise ValueError(f"wan.mi355: attention window radius must be three non-negative integers, got {radius!r}")
            if self._attention_band is not None:
                raise ValueError("wan.mi355: an attention band is set (set_attention_band); clear it (set_attention_band(None)) "
                                 "before setting a window: the two are mutually exclusive")
        self._attention_window = radius
        self._window_plans = {}
        return self

    def set_attention_band(self, frames: Optional[int]):
        """Opt-in approximation: self-attention attends only the keys within about `frames` latent frames of the
        query, as per-block key bands on the dense large-attention kernel (ops.frame_band_plan over the post-patch token grid,
        which is frame-major: a superset of the exact +-frames window, coarser by the frames one 256-row block straddles and
        one 64-key tile at each end); None restores dense attention.  Cross-attention and everything else is untouched.
        Mutually exclusive with set_attention_window.  Not a quality claim: the caller picks the radius."""
        if frames is not None:
            if isinstance(frames, bool) or not isinstance(frames, int) or frames < 0:
                raise ValueError(f"wan.mi355: attention band radius must be a non-negative integer number of frames, got {frames!r}")
            if self._attention_window is not None:
                raise ValueError("wan.mi355: an attention window is set (set_attention_window); clear it "
                                 "(set_attention_window(None)) before setting a band: the two are mutually exclusive")
        self._attention_band = frames
        self._band_plans = {}
        return self

    def set_fp8_compute(self, on: bool, lora: bool = False, fused_quant: bool = False, mx_ffn: bool = False):
        """Opt-in approximation: the block Linears whose weights are RESIDENT e4m3 records (a `keep_fp8=True` load:
        the fused q|k|v, the attention outputs, the cross-attention q and k|v, the two FFN Linears) quantise their activations per
        row to e4m3 and multiply in fp8 (`ops.gemm_fp8`) instead of dequantising the weight and multiplying in bf16.  Everything
        else — embedders, modulation GEMVs, proj_out, attention — stays bf16, and so does any such Linear `ops.gemm` cannot route
        (run-time LoRA attached, e5m2 records, the f32 residual stream).  False restores today's launches bit for bit.  A speed
        option: about 3.7e-2 rel-L2 per GEMM against the f32 product.

        `lora=True` (needs `on=True`): a record that carries run-time LoRA factors stays on the fp8 GEMM as well — the adapter term
        `(x A^T) B'^T` is added in bf16 x bf16 by a tail of the same kernel, into the scaled f32 accumulators
        (`ops.fp8_lora_route`) — instead of falling back to the bf16 path.  The flag lives on the records, so adapters loaded
        before or after this call both take it.  `lora=False` (the default) leaves every launch as it is today.

        `fused_quant=True` (needs `on=True`): the three Linears that read a buffer a norm wrote one launch earlier — the fused
        q|k|v, the cross-attention query behind an affine `norm2`, the FFN-up projection — get their e4m3 codes and row scales
        from the norm kernel itself (`ops.ln_modulate_quant_fp8`, passed on through `ops.gemm(quantised=)`) wherever
        `ops.fp8_norm_quant_route` allows it, so their `quant_rows_fp8` launch disappears and, without adapters, the bf16
        normalised rows are never stored (3 bytes per element instead of 7; 5 with run-time LoRA, whose skinny GEMM reads them).
        A launch and traffic change only: the forward is bit-identical to `set_fp8_compute(True, lora=...)` without it, and the
        f32 residual stream takes it too.  The other four fp8 Linears, e5m2 / GGUF records, the f32-storage mode and the query
        projection without an affine `norm2` run the launches they run today.  `fused_quant=False` (the default) leaves every
        launch as it is today.

        `mx_ffn=True` (needs `on=True`, composes with `fused_quant`): the FFN hidden state stays in fp8 between the two FFN Linears.
        Where `ops.fp8_mx_route` holds, FFN-up quantises its own GELU output per 32-column block in the epilogue
        (`ops.gemm_fp8(out_mx=)`: e4m3 codes + one e8m0 scale byte per block) and FFN-down multiplies those codes with the hardware
        block scales (`ops.gemm_fp8(block_scales=)`), so the `quant_rows_fp8` launch of the hidden state and its bf16 round trip
        disappear.  Codes and scale bytes live in the storage of the bf16 hidden buffer, which is not written in this mode.  This
        CHANGES the numbers (block scales instead of one scale per row of the hidden state).  Blocks with run-time LoRA on either
        FFN Linear and the f32 residual stream keep today's launches; `mx_ffn=False` (the default) leaves every launch as it is."""
        if mx_ffn and not on:
            raise ValueError("wan.mi355: set_fp8_compute(mx_ffn=True) needs on=True: the MX hidden state belongs to the fp8 GEMMs")
        if lora and not on:
            raise ValueError("wan.mi355: set_fp8_compute(lora=True) needs on=True: the adapter tail belongs to the fp8 GEMM")
        if fused_quant and not on:
            raise ValueError("wan.mi355: set_fp8_compute(fused_quant=True) needs on=True: the fused norm quantises for the fp8 GEMM")
        for r in self._fp8_set_compute(on):
            r.lora_compute = "fp8" if lora else "bf16"
        self._fp8_compute = bool(on)
        self._fp8_fused_quant = bool(fused_quant)
        self._fp8_mx_ffn = bool(mx_ffn)
        return self

    _FP4_LINEARS = ("qkv", "attn_out", "cross_q", "cross_kv", "cross_out", "ffn_up", "ffn_down")

    def set_fp4_compute(self, on: bool, linears=None, fused_quant: bool = False, mx_ffn: bool = False):
        """Opt-in approximation: the selected block Linears of a bf16 model — `linears`, a subset of ("qkv",
        "attn_out", "cross_q", "cross_kv", "cross_out", "ffn_up", "ffn_down"), None = all seven (the Linears of `_fp8_plan`) —
        quantise their activations per block of 32 to MXFP4 and multiply e2m1 x e2m1 (`ops.quant_blocks_mxfp4` +
        `ops.gemm_mxfp4`) against an MXFP4 copy of the weight (`ops.Mxfp4Weight.from_bf16`, one record per Linear and block, the
        fused q|k|v and cross k|v as one record each) that sits BESIDE the bf16 weight, on its `_fp4` slot: 0.53 bytes per
        selected weight element on top of the model.  The image k|v projection, the embedders, proj_out and attention stay bf16.
        False detaches the records: the next forward is the original, bit for bit.  The records follow the model's invalidation
        rule (`_weights_changed`: a load, `.to`, a merged LoRA): they are dropped there and rebuilt before the next forward
        while the mode is on, so a LoRA merged after the switch is quantised in.  A speed option, not a parity mode; no quality
        claim on real checkpoints.

        Refused: a model with resident quantised records (a keep_fp8 / keep_quantized load has no bf16 weight to copy, and the
        `fp8_*` switches need exactly such records, so the two modes cannot meet), f32 activation storage and the f32 residual
        stream (their GEMMs read or write float rows, which this mode does not route; `set_storage_dtype` / `set_residual_dtype`
        refuse float32 while the mode is on), and an unknown name in `linears`.

        `fused_quant=True` (needs `on=True`): the fp4-selected ones of the three Linears that read a buffer a norm wrote one
        launch earlier — the fused q|k|v, the cross-attention query behind an affine `norm2`, the FFN-up projection — get their
        e2m1 codes and scale bytes from the norm kernel itself (`ops.ln_modulate_quant_mxfp4`, passed on through
        `ops.gemm(quantised_mxfp4=)`) wherever `ops.mxfp4_norm_quant_route` allows it: their `quant_blocks_mxfp4` launch
        disappears and the bf16 normalised rows are never stored.  `mx_ffn=True` (needs `on=True`, composes with `fused_quant`):
        with `ffn_up` and `ffn_down` both on fp4 and where `ops.mxfp4_mx_route` holds, FFN-up quantises its own GELU output in the
        epilogue (`ops.gemm_mxfp4(out_mx=)`) into the bytes of the hidden buffer and FFN-down reads those codes, so the hidden
        state's `quant_blocks_mxfp4` launch and its bf16 round trip disappear.  Both change launches and traffic only: the
        forward is bit-identical to `set_fp4_compute(True, linears)` without them.  A name selected for fp6 keeps its launches.
        The defaults (False) leave every launch as it is."""
        return self._fp4_switch(on, linears, fused_quant, mx_ffn)      # module_base.Fp4ComputeMixin: the part shared with Flux

    def set_fp6_compute(self, on: bool, linears=None):
        """Opt-in approximation: `set_fp4_compute` with MXFP6 in the place of MXFP4 — the selected block Linears
        (the same seven names, None = all) quantise their activations per block of 32 to OCP e2m3 and multiply e2m3 x e2m3
        (`ops.quant_blocks_mxfp6` + `ops.gemm_mxfp6`) against an MXFP6 copy of the weight (`ops.Mxfp6Weight.from_bf16`) on the
        weight's `_fp6` slot: 0.78 bytes per selected weight element on top of the model.  The error class of the fp8 mode (three
        mantissa bits) on the fp4 matrix instruction's rate; no quality claim on real checkpoints.  The records follow the same
        invalidation rule, and the refusals are those of `set_fp4_compute`.

        Both modes may be on at once when their `linears` are disjoint (fp6 for the attention projections, fp4 for the FFN pair):
        a name selected by both is refused, by either switch, before anything touches the device.  False detaches the fp6 records
        only."""
        return self._fp6_switch(on, linears)      # module_base.Fp6ComputeMixin

    def _fp4_blocks(self):
        return self.blocks

    def _fp4_weights(self, blk) -> dict:
        a1, a2 = blk.attn1, blk.attn2
        return {"qkv": blk._wqkv, "attn_out": a1.to_out[0].weight, "cross_q": a2.to_q.weight, "cross_kv": blk._wkv2,
                "cross_out": a2.to_out[0].weight, "ffn_up": blk.ffn.net[0].proj.weight, "ffn_down": blk.ffn.net[2].weight}

    def _norm_gemm(self, x, xn, w, bias, out, lora_buf, epilogue="bias", out_mx=None, out_mxfp4=None, **norm):
        """ln_modulate(x, **norm, out=xn) -> gemm(xn, w, bias, out=out, epilogue=epilogue, lora_buf=lora_buf); with
        `set_fp8_compute(fused_quant=True)`, where `ops.fp8_norm_quant_route` allows it, the norm quantises for the GEMM in its own
        launch (and stores `xn` only if the GEMM's adapter tail reads it).  Nothing else reads `xn` between the two.  `out_mx`: see
        `ops.gemm` (the caller has asked `ops.fp8_mx_route`).  With `set_fp4_compute(fused_quant=True)` the same for an fp4
        Linear, where `ops.mxfp4_norm_quant_route` allows it: `xn` is not stored (the fp4 mode has no adapter tail).  `out_mxfp4`:
        see `ops.gemm` (the caller has asked `ops.mxfp4_mx_route`)."""
        mx = {} if out_mx is None else {"out_mx": out_mx}
        if out_mxfp4 is not None:
            mx["out_mxfp4"] = out_mxfp4
        if self._fp4_fused_quant and ops.mxfp4_norm_quant_route(x, xn, w, out, epilogue):
            q = ops.ln_modulate_quant_mxfp4(x, **norm)
            return ops.gemm(xn, w, bias, out=out, epilogue=epilogue, quantised_mxfp4=q, **mx)
        if getattr(self, "_fp8_fused_quant", False):
            fuse, need_row = ops.fp8_norm_quant_route(x, xn, w, out, epilogue, lora_buf)
            if fuse:
                q = ops.ln_modulate_quant_fp8(x, out=xn if need_row else None, **norm)
                return ops.gemm(xn, w, bias, out=out, epilogue=epilogue, lora_buf=lora_buf, quantised=q, **mx)
        ops.ln_modulate(x, out=xn, **norm)
        return ops.gemm(xn, w, bias, out=out, epilogue=epilogue, lora_buf=lora_buf, **mx)

    def _grid_ids(self, grid) -> torch.Tensor:
        """(frame, row, column) of every token in sequence order: what RoPE rotates by and what the attention window measures"""
        f, h, w = grid
        dev = self.device
        return torch.stack(torch.meshgrid(torch.arange(f, device=dev), torch.arange(h, device=dev),
                                          torch.arange(w, device=dev), indexing="ij"), dim=-1).reshape(-1, 3)

    def _window_plan(self, grid):
        key = (grid, self._attention_window)
        plan = self._window_plans.get(key)
        if plan is None:
            plan = ops.window_plan(self._grid_ids(grid), radius=self._attention_window)
            self._window_plans = {key: plan}
        return plan

    def _band_plan(self, grid):
        key = (grid, self._attention_band)
        plan = self._band_plans.get(key)
        if plan is None:
            plan = ops.frame_band_plan(grid[0], grid[1] * grid[2], self._attention_band, device=self.device)
            self._band_plans = {key: plan}
        return plan

    def init_synthetic(self, seed: int = 0, std: float = 0.02):
        return self._fill_synthetic(
            seed, std, ones=lambda name, p: name.endswith(("norm_q.weight", "norm_k.weight", "norm2.weight", "norm1.weight",
                                                            "norm_added_k.weight")),
            row_scaled=lambda name, p: name.endswith("scale_shift_table"))

    @torch.no_grad()
    def pack(self):
        if self._packed:
            return
        self._fp8_guard("pack")
        dev, _ = self._pack_target()
        for blk in self.blocks:
            a1, a2 = blk.attn1, blk.attn2
            blk._wqkv, blk._bqkv = _fuse_linears([a1.to_q, a1.to_k, a1.to_v])
            blk._wkv2, blk._bkv2 = _fuse_linears([a2.to_k, a2.to_v])
            if hasattr(a2, "add_k_proj"):      # image k|v, packed like _wkv2
                blk._wkvi, blk._bkvi = _fuse_linears([a2.add_k_proj, a2.add_v_proj])
        self._ones = torch.ones(self.inner_dim, device=dev, dtype=torch.float32)
        self._packed = True
        self._weights_changed()

    # ---- quantised expert weights resident in HBM: fp8-scaled and GGUF blocks.  The `_fp8*` names date from the
    # first of the two formats; a parameter's `_fp8` slot holds any ops.ResidentWeight --------------------------------------------
    @staticmethod
    def _fp8_resident_key(key: str) -> bool:
        """Which quantised checkpoint tensors `weights.load_checkpoint_into(keep_fp8=True / keep_quantized=True)` keeps as stored: the
        Linear weights of the blocks (attention projections and FFN: 99 % of an expert's bytes).  The embedders feed GEMVs and the
        modulation tables are f32 copies: those stay dequantised.  The image branch's add_k_proj / add_v_proj stay bf16."""
        return key.startswith("blocks.") and key.endswith(".weight") and ".norm" not in key and ".add_" not in key

    def _fp8_plan(self):
        plan = []
        for blk in self.blocks:
            a1, a2 = blk.attn1, blk.attn2
            plan += [(blk, "_wqkv", [a1.to_q.weight, a1.to_k.weight, a1.to_v.weight]), (blk, "_wkv2", [a2.to_k.weight, a2.to_v.weight])]
            plan += [(blk, None, [p]) for p in (a1.to_out[0].weight, a2.to_q.weight, a2.to_out[0].weight, blk.ffn.net[0].proj.weight,
                                                 blk.ffn.net[2].weight)]
        return plan

    # ---- LoRA on resident-fp8 weights: applied at RUN TIME, as the reference does (R/src/lora/manager.py:454-606 around
    # FPScaledLinear) — there is no bf16 weight to merge into.  Modules whose weights are ordinary bf16 parameters still merge.
    @torch.no_grad()
    def _lora_remerge(self, modules):
        recs = getattr(self, "_fp8_records", None) or {}
        modules = set(modules)
        resident = {m for m in modules if m in recs}
        if resident:
            for m in resident:
                if any("bias" in d[m] for d in self._lora_adapters.values() if m in d):
                    raise NotImplementedError(f"wan.mi355: a lora_B.bias on the resident-fp8 Linear '{m}' is not supported")
            touched = {id(recs[m]): recs[m] for m in resident}
            pad = 0
            for rec in touched.values():
                act = [(m, d[m]["A"], d[m]["B"], self._lora_scales[n]) for m, _, _ in rec.parts
                       for n, d in self._lora_adapters.items()
                       if m in d and self._lora_scales[n] != 0.0 and self._lora_enabled]
                rec.set_lora(act)
            for rec in {id(r): r for r in recs.values()}.values():
                pad = max(pad, 0 if rec.lora_A is None else int(rec.lora_A.shape[0]))
            if pad != getattr(self, "_lora_pad", 0):
                self._lora_pad = pad         # the activation buffers grow by this many columns (see _workspace)
                self._ws = {}
        super()._lora_remerge(modules - resident)
        if modules - resident:
            self._fp4_detach()      # merged into the bf16 weights: the MXFP4 copies are rebuilt before the next forward
            self._fp6_detach()      # and the MXFP6 ones

    def state_dict(self, *a, **k):
        self._fp8_guard("state_dict")
        return super().state_dict(*a, **k)

    @torch.no_grad()
    def _weights_changed(self):
        """Rebuild what is DERIVED from parameter values (f32 copies of the modulation tables, [L, 6*dim] and
        [2*dim]).  `weights.load_checkpoint_into` writes parameters in place after `pack()` and calls this.  The MXFP4 copies
        of `set_fp4_compute` and the MXFP6 copies of `set_fp6_compute` are dropped here and rebuilt before the next forward."""
        self._fp4_detach()
        self._fp6_detach()
        if not self._packed:
            return
        dim, dev = self.inner_dim, self.device
        self._sst = torch.stack([b.scale_shift_table.data.float().reshape(-1) for b in self.blocks]) \
            if len(self.blocks) else torch.empty(0, 6 * dim, device=dev)
        self._sst_out = self.scale_shift_table.data.float().reshape(-1).contiguous()
        # patch_embedding as a GEMM needs K = C pt ph pw in multiples of 64: 64 for the 16-channel text-to-video experts; the
        # image-to-video experts take 36 channels (K = 144) -> the weight gets zero columns up to 192 (exact zeros in the f32 sums)
        w = self.patch_embedding.weight.data.reshape(dim, -1)
        kp = (w.shape[1] + 63) // 64 * 64
        self._pe_w = w if kp == w.shape[1] else torch.cat([w, w.new_zeros(dim, kp - w.shape[1])], dim=1).contiguous()

    def _workspace(self, S: int, s_txt: int, s_img: int = 0):
        key = (S, s_txt, s_img)
        ws = self._ws.get(key)
        if ws is not None:
            return ws
        dev, dim, H = self.device, self.inner_dim, self.config.num_attention_heads
        ffn = self.config.ffn_dim
        skp = (S + 63) // 64 * 64
        tkp = (s_txt + 63) // 64 * 64
        bf = dict(device=dev, dtype=self.storage_dtype)     # activation buffers
        f32 = dict(device=dev, dtype=torch.float32)
        # run-time LoRA on resident-fp8 weights (ops._gemm_fp8_lora): the buffers a Linear READS carry `pad` spare columns behind
        # their rows for the adapters' rank-space activations; pad = 0 (no such adapter) is the plain layout
        pad = int(getattr(self, "_lora_pad", 0))
        XNf, ATTf = torch.empty(S, dim + pad, **bf), torch.empty(S, dim + pad, **bf)
        FFHf, CTXf = torch.empty(S, ffn + pad, **bf), torch.empty(s_txt, dim + pad, **bf)
        xdt = torch.float32 if self.residual_dtype == torch.float32 else self.storage_dtype      # the residual stream
        ws = SimpleNamespace(
            X=torch.empty(S, dim, device=dev, dtype=xdt), XN=XNf[:, :dim], QKV=torch.empty(S, 3 * dim, **bf),
            Q=torch.empty(1, H, S, 128, **bf), K=torch.empty(1, H, S, 128, **bf),
            VT=torch.zeros(1, H, 128, skp, **bf), ATT=ATTf[:, :dim], FFH=FFHf[:, :ffn],
            CTX=CTXf[:, :dim], CTXH=torch.empty(s_txt, dim, **bf), XNf=XNf, ATTf=ATTf, FFHf=FFHf, CTXf=CTXf,
            KV2=torch.empty(s_txt, 2 * dim, **bf), K2=torch.empty(1, H, s_txt, 128, **bf),
            VT2=torch.zeros(1, H, 128, tkp, **bf),
            MOD=torch.empty(max(len(self.blocks), 1), 6 * dim, **f32), MOD2=torch.empty(1, 2 * dim, **f32),
            TEMB=torch.empty(1, dim, **f32), TPROJ=torch.empty(1, 6 * dim, **f32))
        if s_img:           # image branch of the cross-attention: embedded image tokens, their k|v, prepared k and V^T
            ikp = (s_img + 63) // 64 * 64
            ws.IMG = torch.empty(s_img, dim, **bf)
            ws.KVI = torch.empty(s_img, 2 * dim, **bf)
            ws.KI = torch.empty(1, H, s_img, 128, **bf)
            ws.VTI = torch.zeros(1, H, 128, ikp, **bf)
        self._ws = {key: ws}
        return ws

    def _rope_table(self, grid):
        t = self._rope.get(grid)
        if t is None:
            ids = self._grid_ids(grid).float().contiguous()
            hd = self.config.attention_head_dim
            hw_dim = 2 * (hd // 6)
            t = ops.rope_table_axes(ids, (hd - 2 * hw_dim, hw_dim, hw_dim), 10000.0)
            self._rope = {grid: t}
        return t

    def _embed_image(self, img: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """condition_embedder.image_embedder on one sample's image tokens [s_img, image_dim] (storage dtype) -> out [s_img, dim]."""
        ie = self.condition_embedder.image_embedder
        if ie.pos_embed is not None:
            img = ops.add(img.contiguous(), ie.pos_embed[0].to(img.dtype).contiguous())
        h = ops.ln_modulate(img, gamma=ie.norm1.weight, beta=ie.norm1.bias, eps=1e-5)
        h = ops.gemm(h, ie.ff.net[0].proj.weight, ie.ff.net[0].proj.bias, epilogue="gelu_erf")
        h = ops.gemm(h, ie.ff.net[2].weight, ie.ff.net[2].bias)
        return ops.ln_modulate(h, gamma=ie.norm2.weight, beta=ie.norm2.bias, eps=1e-5, out=out)

    @torch.no_grad()
    def _forward_one(self, hidden_states, timestep, text, image=None):
        cfg = self.config
        dim, H = self.inner_dim, cfg.num_attention_heads
        C, T, Hh, Ww = hidden_states.shape
        pt, ph, pw = cfg.patch_size
        grid = (T // pt, Hh // ph, Ww // pw)
        S = grid[0] * grid[1] * grid[2]
        s_txt = text.shape[0]
        s_img = 0 if image is None else image.shape[0]
        ws = self._workspace(S, s_txt, s_img)
        X, XN, QKV, ATT, FFH = ws.X, ws.XN, ws.QKV, ws.ATT, ws.FFH
        eps = cfg.eps

        # patchify (layout only) + patch_embedding as a K = C*pt*ph*pw GEMM
        tok = hidden_states.to(self.storage_dtype).reshape(C, grid[0], pt, grid[1], ph, grid[2], pw) \
            .permute(1, 3, 5, 0, 2, 4, 6).reshape(S, C * pt * ph * pw).contiguous()
        pe = self.patch_embedding
        if self._pe_w.shape[1] != tok.shape[1]:
            tok = torch.cat([tok, tok.new_zeros(S, self._pe_w.shape[1] - tok.shape[1])], dim=1)
        ops.gemm(tok, self._pe_w, pe.bias, out=X)

        ce = self.condition_embedder
        tp = ops.timestep_embedding(timestep.float().reshape(1), cfg.freq_dim)
        h = ops.gemv(ce.time_embedder.linear_1.weight, tp, ce.time_embedder.linear_1.bias, post="silu")
        ops.gemv(ce.time_embedder.linear_2.weight, h, ce.time_embedder.linear_2.bias, out=ws.TEMB)
        ops.gemv(ce.time_proj.weight, ws.TEMB, ce.time_proj.bias, out=ws.TPROJ, pre_silu=True)
        ops.gemm(text, ce.text_embedder.linear_1.weight, ce.text_embedder.linear_1.bias, out=ws.CTXH,
                 epilogue="gelu")
        ops.gemm(ws.CTXH, ce.text_embedder.linear_2.weight, ce.text_embedder.linear_2.bias, out=ws.CTX)
        if s_img:
            self._embed_image(image, ws.IMG)
        if len(self.blocks):
            ops.add_bcast(self._sst, ws.TPROJ[0], out=ws.MOD)    # scale_shift_table + temb.float()
        ops.add_bcast(self._sst_out.reshape(1, -1), torch.cat([ws.TEMB[0], ws.TEMB[0]]), out=ws.MOD2)
        rope = self._rope_table(grid)
        wplan = None
        if self._attention_window is not None:
            if self.storage_dtype != torch.bfloat16:
                raise NotImplementedError("wan.mi355: the f32-storage verification mode has no window attention; clear the "
                                          "window (set_attention_window(None)) or run with bfloat16 storage")
            wplan = self._window_plan(grid)
        bplan = None
        if self._attention_band is not None:
            if self.storage_dtype != torch.bfloat16:
                raise NotImplementedError("wan.mi355: the f32-storage verification mode has no band attention; clear the "
                                          "band (set_attention_band(None)) or run with bfloat16 storage")
            bplan = self._band_plan(grid)

        q_in, k_in, v_in = QKV[:, :dim], QKV[:, dim:2 * dim], QKV[:, 2 * dim:]
        att_v = ATT.unflatten(-1, (H, 128)).unsqueeze(0)
        # q / k across-heads RMSNorm + RoPE + layout (+ V^T) as one pass (apexmi_qk_rms_rope_rows, bit-identical to the three it
        # replaces); `fuse_qkv = False` keeps the normalised [S, dim] q / k as storage points (tests/stage_parity.py)
        fuse = self.fuse_qkv and dim in (3072, 5120)
        for i, blk in enumerate(self.blocks):
            a1, a2 = blk.attn1, blk.attn2
            m = lambda j: ws.MOD[i, j * dim:(j + 1) * dim]  # noqa: E731 shift, scale, gate, c_shift, c_scale, c_gate
            # 1. self attention
            self._norm_gemm(X, XN, blk._wqkv, blk._bqkv, QKV, ws.XNf, scale=m(1), shift=m(0), eps=eps)
            if fuse:       # across-heads RMSNorm of q and k + RoPE + layout + V^T in one read of the projection
                ops.qk_rms_rope_rows(q_in, k_in, v_in, H, ws.Q[0], ws.K[0], ws.VT[0], wq=a1.norm_q.weight, wk=a1.norm_k.weight,
                                     eps=eps, rope=rope, rope_mode=_l.ROPE_INTERLEAVED)
            else:
                ops.ln_modulate(q_in, gamma=a1.norm_q.weight, out=q_in, eps=eps, rms=True)
                ops.ln_modulate(k_in, gamma=a1.norm_k.weight, out=k_in, eps=eps, rms=True)
                ops.qkv_prepare(q_in, k_in, v_in, H, ws.Q[0], ws.K[0], ws.VT[0], rope=rope,
                                rope_mode=_l.ROPE_INTERLEAVED)
            if bplan is not None:
                ops.attention_prepared_band(ws.Q, ws.K, ws.VT, att_v, S, bplan)
            elif wplan is None:
                ops.attention_prepared(ws.Q, ws.K, ws.VT, att_v, S)
            else:
                ops.attention_prepared_window(ws.Q, ws.K, ws.VT, att_v, S, wplan)
            ops.gemm(ATT, a1.to_out[0].weight, a1.to_out[0].bias, out=X, epilogue="gate_res", gate=m(2),
                     residual=X, lora_buf=ws.ATTf)
            # 2. cross attention over the text tokens (no RoPE, ungated residual)
            if isinstance(blk.norm2, _AffineNorm):
                self._norm_gemm(X, XN, a2.to_q.weight, a2.to_q.bias, q_in, ws.XNf, gamma=blk.norm2.weight, beta=blk.norm2.bias,
                                eps=eps)
            else:
                if X.dtype != XN.dtype:    # float residual stream without norm2: the query projection reads X rounded to bf16
                    XN.copy_(ops.to_bf16(X))
                    src = XN
                else:
                    src = X
                ops.gemm(src, a2.to_q.weight, a2.to_q.bias, out=q_in, lora_buf=ws.XNf if src is XN else None)
            if fuse:
                ops.qk_rms_rope_rows(q_in, None, None, H, ws.Q[0], None, None, wq=a2.norm_q.weight, eps=eps)
            else:
                ops.ln_modulate(q_in, gamma=a2.norm_q.weight, out=q_in, eps=eps, rms=True)
            ops.gemm(ws.CTX, blk._wkv2, blk._bkv2, out=ws.KV2, lora_buf=ws.CTXf)
            ops.ln_modulate(ws.KV2[:, :dim], gamma=a2.norm_k.weight, out=ws.KV2[:, :dim], eps=eps, rms=True)
            if not fuse:
                ops.qkv_prepare(q_in, None, None, H, ws.Q[0], None, None)
            ops.qkv_prepare(ws.KV2[:, :dim], None, ws.KV2[:, dim:], H, ws.K2[0], None, ws.VT2[0])
            if s_img:      # image keys: add_k|v gemm, RMSNorm over all heads on k, prepare, then one two-context launch
                ops.gemm(ws.IMG, blk._wkvi, blk._bkvi, out=ws.KVI)
                ops.ln_modulate(ws.KVI[:, :dim], gamma=a2.norm_added_k.weight, out=ws.KVI[:, :dim], eps=eps, rms=True)
                ops.qkv_prepare(ws.KVI[:, :dim], None, ws.KVI[:, dim:], H, ws.KI[0], None, ws.VTI[0])
                ops.attention_prepared_dual(ws.Q, ws.K2, ws.VT2, s_txt, ws.KI, ws.VTI, s_img, att_v)
            else:
                ops.attention_prepared(ws.Q, ws.K2, ws.VT2, att_v, s_txt)
            ops.gemm(ATT, a2.to_out[0].weight, a2.to_out[0].bias, out=X, epilogue="gate_res", gate=self._ones,
                     residual=X, lora_buf=ws.ATTf)
            # 3. feed-forward
            w_up, w_down = blk.ffn.net[0].proj.weight, blk.ffn.net[2].weight
            if getattr(self, "_fp8_mx_ffn", False) and ops.fp8_mx_route(XN, w_up, w_down, "gelu", "gate_res", out=X):
                # the hidden state as MX codes + block scales in the bytes of FFHf, which holds no bf16 row in this mode
                raw = ws.FFHf.view(torch.uint8)
                ffn = FFH.shape[1]
                hq, hs = raw[:, :ffn], raw[:, ffn:ffn + ffn // 32]
                self._norm_gemm(X, XN, w_up, blk.ffn.net[0].proj.bias, None, ws.XNf, epilogue="gelu", out_mx=(hq, hs),
                                scale=m(4), shift=m(3), eps=eps)
                ops.gemm_fp8(hq, None, ops._fp8_of(w_down), blk.ffn.net[2].bias, out=X, epilogue="gate_res", gate=m(5), residual=X,
                             block_scales=hs)
                continue
            if self._fp4_mx_ffn and ws.FFHf.stride(0) % 8 == 0 and ops.mxfp4_mx_route(XN, w_up, w_down, "gelu", "gate_res", out=X):
                # the hidden state as MXFP4 codes + scale bytes in the bytes of FFHf (ffn / 2 + ffn / 32 of a row's 2 ffn), which
                # holds no bf16 row in this mode
                raw = ws.FFHf.view(torch.uint8)
                ffn = FFH.shape[1]
                hq, hs = raw[:, :ffn // 2], raw[:, ffn // 2:ffn // 2 + ffn // 32]
                self._norm_gemm(X, XN, w_up, blk.ffn.net[0].proj.bias, None, ws.XNf, epilogue="gelu", out_mxfp4=(hq, hs),
                                scale=m(4), shift=m(3), eps=eps)
                ops.gemm_mxfp4(hq, hs, w_down._fp4, blk.ffn.net[2].bias, out=X, epilogue="gate_res", gate=m(5), residual=X)
                continue
            self._norm_gemm(X, XN, w_up, blk.ffn.net[0].proj.bias, FFH, ws.XNf, epilogue="gelu",
                            scale=m(4), shift=m(3), eps=eps)
            ops.gemm(FFH, w_down, blk.ffn.net[2].bias, out=X, epilogue="gate_res", gate=m(5),
                     residual=X, lora_buf=ws.FFHf)

        # (scale_shift_table + temb).chunk(2): shift first, then scale (model.py:1849-1856)
        ops.ln_modulate(X, ws.MOD2[0, dim:], ws.MOD2[0, :dim], out=XN, eps=eps)
        out = ops.gemm(XN, self.proj_out.weight, self.proj_out.bias)
        out = out.reshape(grid[0], grid[1], grid[2], pt, ph, pw, -1).permute(6, 0, 3, 1, 4, 2, 5)
        return out.reshape(-1, T, Hh, Ww)

    def _image_tokens(self, image: torch.Tensor, batch: int) -> torch.Tensor:
        """encoder_hidden_states_image [B, 257 n, image_dim] -> [B, s_img, image_dim] in the storage dtype.  With pos_embed (FLF2V)
        the tokens are viewed as rows of pos_embed_seq_len first (diffusers WanImageEmbedding: the pair's 2 x 257 tokens as 514)."""
        if self.storage_dtype != torch.bfloat16:
            raise NotImplementedError("wan.mi355: the f32-storage verification mode has no image-conditioned cross-attention; "
                                      "run the image branch with bfloat16 storage")
        cfg = self.config
        if image.dim() != 3 or image.shape[-1] != cfg.image_dim:
            raise ValueError(f"wan.mi355: encoder_hidden_states_image must be [B, tokens, {cfg.image_dim}], got {tuple(image.shape)}")
        if cfg.pos_embed_seq_len is not None:
            image = image.reshape(-1, cfg.pos_embed_seq_len, cfg.image_dim)
        if image.shape[0] != batch:
            raise ValueError(f"wan.mi355: {image.shape[0]} image-token rows for a batch of {batch}")
        return image.to(self.device, self.storage_dtype)

    @ops.on_model_device
    @torch.no_grad()
    def forward(self, hidden_states: torch.Tensor, timestep: torch.Tensor = None,
                encoder_hidden_states: torch.Tensor = None, encoder_hidden_states_image=None,
                ip_image_hidden_states=None, return_dict: bool = True, attention_kwargs=None,
                enhance_kwargs=None, rope_on_cpu=None):
        if ip_image_hidden_states is not None:
            raise NotImplementedError("wan.mi355: the IP adapter is outside the hot-path scope")
        if timestep.ndim != 1:
            raise NotImplementedError("wan.mi355: per-token timesteps are not supported")
        self.pack()
        self._fp4_refresh()
        self._fp6_refresh()
        enc = encoder_hidden_states.to(self.storage_dtype)
        img = None
        if encoder_hidden_states_image is not None and self.config.added_kv_proj_dim is not None:
            img = self._image_tokens(encoder_hidden_states_image, hidden_states.shape[0])

        def run():
            return torch.stack([self._forward_one(hidden_states[b], timestep[b:b + 1], enc[b].contiguous(),
                                                  None if img is None else img[b].contiguous())
                                for b in range(hidden_states.shape[0])], dim=0)
        ec = getattr(self, "_easy_cache", None)
        if ec is not None:       # EasyCache: this call may be served from the cache; float32 out, as the reference returns
            out = ec(hidden_states, self.config.out_channels, run)
        else:
            out = run().to(hidden_states.dtype)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
