"""FluxTransformer2DModel on the MI355X HIP ops — drop-in for registry key "flux.base".

Mirrors the interface of the reference class (apps/api/src/transformer/flux/base/model.py:362-657):
same constructor config, same state-dict keys (transformer_blocks.N.attn.to_q.weight, ...), same
keyword forward returning a 1-tuple when return_dict=False, `.config` with attribute/`.get`
access, `.dtype`/`.device`, `cache_context(name)`, `from_config`.  Underneath, a denoise step is
a fixed sequence of libapex_mi355.so kernels over one joint [S_txt + S_img, dim] residual buffer
(text rows first), so none of the reference's torch.cat / split / permute copies exist:

  per step      : timestep/guidance/pooled embeds (gemv) -> ONE batched gemv for every block's AdaLN
                  modulation vectors -> rope table
  double block  : ln_modulate x2 -> QKV gemm x2 (img / txt weights, one joint output)
                  -> qkv_prepare (per-head RMSNorm + RoPE + V^T) -> attention
                  -> out-proj gemm x2 with fused gate*y + residual -> ln_modulate x2
                  -> MLP-up gemm (+GELU) x2 -> MLP-down gemm x2 with fused gate + residual
  single block  : ln_modulate -> QKV gemm + MLP gemm(+GELU) into the concat buffer -> qkv_prepare
                  -> attention (writes into the concat buffer) -> 15360->3072 gemm with fused
                  gate + residual

Weights are packed once after loading (fused QKV, all modulation projections in one matrix) and the
original nn.Parameters are re-pointed at views of the packed storage, so state_dict()/load_state_dict
keep working and memory is not doubled.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn


from . import lib as _l
from .schedule import ModulationSchedule, ScheduleRegistry
from . import ops
# the parameter holders live in module_base; they stay importable from here (the name older code and checkpoints' tools use)
from .module_base import (F32ResidualMixin, Fp4ComputeMixin, Fp8ResidentMixin, HipTransformer, _AdaNorm, _Config, _FF, _Linear, _Norm, _TimestepEmbedding,  # noqa: F401
                          _fuse_linears, _repoint)


class _Attn(nn.Module):
    def __init__(self, dim: int, heads: int, head_dim: int, joint: bool, pre_only: bool, **kw):
        super().__init__()
        inner = heads * head_dim
        self.heads, self.head_dim = heads, head_dim
        self.processor = None          # an _IPAdapterProcessor on the double blocks once IP adapters are loaded
        self.norm_q, self.norm_k = _Norm(head_dim, **kw), _Norm(head_dim, **kw)
        self.to_q, self.to_k, self.to_v = (_Linear(dim, inner, **kw), _Linear(dim, inner, **kw),
                                           _Linear(dim, inner, **kw))
        if not pre_only:
            self.to_out = nn.ModuleList([_Linear(inner, dim, **kw), nn.Identity()])
        if joint:
            self.norm_added_q, self.norm_added_k = _Norm(head_dim, **kw), _Norm(head_dim, **kw)
            self.add_q_proj, self.add_k_proj, self.add_v_proj = (
                _Linear(dim, inner, **kw), _Linear(dim, inner, **kw), _Linear(dim, inner, **kw))
            self.to_add_out = _Linear(inner, dim, **kw)


class _IPAdapterProcessor(nn.Module):
    """Parameters of `FluxIPAdapterAttnProcessor` (R/src/transformer/flux/base/attention.py:115-173) on a double block's attention:
    per adapter one key and one value projection of the image-prompt tokens (`...attn.processor.to_k_ip.M.weight`) and a scale."""

    def __init__(self, hidden_size: int, cross_attention_dim: int, num_tokens=(4,), scale=1.0, **kw):
        super().__init__()
        num_tokens = list(num_tokens) if isinstance(num_tokens, (tuple, list)) else [num_tokens]
        self.scale = list(scale) if isinstance(scale, (list, tuple)) else [float(scale)] * len(num_tokens)
        if len(self.scale) != len(num_tokens):
            raise ValueError("`scale` should be a list with the same length as `num_tokens`.")
        self.to_k_ip = nn.ModuleList([_Linear(cross_attention_dim, hidden_size, **kw) for _ in num_tokens])
        self.to_v_ip = nn.ModuleList([_Linear(cross_attention_dim, hidden_size, **kw) for _ in num_tokens])


class _ImageProjection(nn.Module):
    """diffusers `ImageProjection` (what `_load_ip_adapter_weights` builds for the Flux IP-adapter; the class is diffusers' and
    absent from this image — restated from its definition, parity unpinned): Linear(image_embed_dim -> tokens x cross_attention_dim),
    reshape to [B, tokens, cross_attention_dim], LayerNorm(cross_attention_dim, eps 1e-5)."""

    def __init__(self, image_embed_dim: int, cross_attention_dim: int, num_image_text_embeds: int, **kw):
        super().__init__()
        self.num_image_text_embeds, self.cross_attention_dim = num_image_text_embeds, cross_attention_dim
        self.image_embeds = _Linear(image_embed_dim, num_image_text_embeds * cross_attention_dim, **kw)
        self.norm = nn.LayerNorm(cross_attention_dim, **kw)

    def forward(self, image_embeds: torch.Tensor) -> torch.Tensor:
        B = image_embeds.shape[0]
        x = image_embeds.reshape(B, -1).to(self.image_embeds.weight.dtype).contiguous()
        y = ops.gemm(x, self.image_embeds.weight, self.image_embeds.bias).reshape(B * self.num_image_text_embeds, -1)
        y = ops.ln_modulate(y, gamma=self.norm.weight, beta=self.norm.bias, eps=self.norm.eps)
        return y.reshape(B, self.num_image_text_embeds, self.cross_attention_dim)


class _MultiIPAdapterImageProjection(nn.Module):
    """diffusers `MultiIPAdapterImageProjection` (the model's `encoder_hid_proj` once IP adapters are loaded; engines read its
    `num_ip_adapters`, R/src/engine/flux/shared.py:84-96): one `ImageProjection` per adapter; each entry of the input list is
    [B, num_images, image_embed_dim] (or [B, image_embed_dim]) -> [B, num_images x tokens, cross_attention_dim]."""

    def __init__(self, layers):
        super().__init__()
        self.image_projection_layers = nn.ModuleList(layers)

    @property
    def num_ip_adapters(self) -> int:
        return len(self.image_projection_layers)

    def forward(self, image_embeds):
        if not isinstance(image_embeds, (list, tuple)):
            image_embeds = [image_embeds.unsqueeze(1)]
        if len(image_embeds) != len(self.image_projection_layers):
            raise ValueError(f"image_embeds must have the same length as image_projection_layers, got {len(image_embeds)} and "
                             f"{len(self.image_projection_layers)}")
        out = []
        for e, layer in zip(image_embeds, self.image_projection_layers):
            e = e if e.dim() == 3 else e.unsqueeze(1)
            B, n = e.shape[0], e.shape[1]
            out.append(layer(e.reshape(B * n, -1)).reshape(B, n * layer.num_image_text_embeds, -1))
        return out


class _DoubleBlock(nn.Module):
    def __init__(self, dim: int, heads: int, head_dim: int, **kw):
        super().__init__()
        self.norm1 = _AdaNorm(dim, 6, **kw)
        self.norm1_context = _AdaNorm(dim, 6, **kw)
        self.attn = _Attn(dim, heads, head_dim, joint=True, pre_only=False, **kw)
        self.ff = _FF(dim, 4 * dim, **kw)
        self.ff_context = _FF(dim, 4 * dim, **kw)


class _SingleBlock(nn.Module):
    def __init__(self, dim: int, heads: int, head_dim: int, mlp_ratio: float = 4.0, **kw):
        super().__init__()
        self.mlp_hidden_dim = int(dim * mlp_ratio)
        self.norm = _AdaNorm(dim, 3, **kw)
        self.proj_mlp = _Linear(dim, self.mlp_hidden_dim, **kw)
        self.proj_out = _Linear(dim + self.mlp_hidden_dim, dim, **kw)
        self.attn = _Attn(dim, heads, head_dim, joint=False, pre_only=True, **kw)


class _TimeTextEmbed(nn.Module):
    def __init__(self, dim: int, pooled_dim: int, guidance: bool, **kw):
        super().__init__()
        self.timestep_embedder = _TimestepEmbedding(256, dim, **kw)
        if guidance:
            self.guidance_embedder = _TimestepEmbedding(256, dim, **kw)
        self.text_embedder = _TimestepEmbedding(pooled_dim, dim, **kw)


class FluxTransformer2DModel(Fp8ResidentMixin, Fp4ComputeMixin, F32ResidualMixin, HipTransformer):
    _converter_base = "flux.base"      # which key-converter table original-format weight files / LoRAs go through (converters.py)
    _tag = "flux.mi355"
    _drops = {"moved": ("_packed", "_ws"), "loaded": ("_packed",), "storage": ("_ws",)}
    _supports_gradient_checkpointing = False
    _no_split_modules = ["_DoubleBlock", "_SingleBlock"]

    def __init__(self, patch_size: int = 1, in_channels: int = 64, out_channels: Optional[int] = None,
                 num_layers: int = 19, num_single_layers: int = 38, attention_head_dim: int = 128,
                 num_attention_heads: int = 24, joint_attention_dim: int = 4096,
                 pooled_projection_dim: int = 768, guidance_embeds: bool = False,
                 axes_dims_rope: Tuple[int, int, int] = (16, 56, 56), device=None,
                 dtype=torch.bfloat16):
        super().__init__()
        if attention_head_dim != 128:
            raise _l.ApexMIError("flux.mi355: attention_head_dim must be 128 (MFMA attention tile)")
        self.config = _Config(patch_size=patch_size, in_channels=in_channels, out_channels=out_channels,
                              num_layers=num_layers, num_single_layers=num_single_layers,
                              attention_head_dim=attention_head_dim,
                              num_attention_heads=num_attention_heads,
                              joint_attention_dim=joint_attention_dim,
                              pooled_projection_dim=pooled_projection_dim,
                              guidance_embeds=guidance_embeds, axes_dims_rope=tuple(axes_dims_rope))
        kw = dict(device=device, dtype=dtype)
        self.out_channels = out_channels or in_channels
        self.inner_dim = dim = num_attention_heads * attention_head_dim
        self.time_text_embed = _TimeTextEmbed(dim, pooled_projection_dim, guidance_embeds, **kw)
        self.context_embedder = _Linear(joint_attention_dim, dim, **kw)
        self.x_embedder = _Linear(in_channels, dim, **kw)
        self.transformer_blocks = nn.ModuleList(
            [_DoubleBlock(dim, num_attention_heads, attention_head_dim, **kw) for _ in range(num_layers)])
        self.single_transformer_blocks = nn.ModuleList(
            [_SingleBlock(dim, num_attention_heads, attention_head_dim, **kw)
             for _ in range(num_single_layers)])
        self.norm_out = _AdaNorm(dim, 2, **kw)
        self.proj_out = _Linear(dim, patch_size * patch_size * self.out_channels, **kw)
        self._packed = False
        self._ws: Dict[Any, Any] = {}
        self._side = None
        self._rope_cache = None
        self._scheds = ScheduleRegistry()  # modulation schedules of the clips in flight (begin_schedule), one handle per clip
        self.batch_streams = 2           # images of a batch run side by side on HIP streams (see forward); 1 = sequential
        self._bstreams: List[Any] = []
        # q/k/v preparation in the QKV GEMM's epilogue where the launch allows it (see _forward_one; APEX_FLUX_FUSE_QKV=0: A/B)
        self.fuse_qkv = os.environ.get("APEX_FLUX_FUSE_QKV", "1") != "0"
        self._fp8_compute = self._fp8_fused_quant = self._fp8_mx_ffn = self._fp8_lora = False      # set_fp8_compute

    # ---- reference-compatible plumbing: module_base (from_config, set_storage_dtype / set_residual_dtype, cache_context, ...) ----
    def _anchor(self):
        return self.x_embedder.weight

    def init_synthetic(self, seed: int = 0, std: float = 0.02):
        return self._fill_synthetic(seed, std, ones=lambda name, p: name.endswith(
            ("norm_q.weight", "norm_k.weight", "norm_added_q.weight", "norm_added_k.weight")))

    # ---- weight packing ----------------------------------------------------------------------
    @torch.no_grad()
    def pack(self):
        if self._packed:
            return
        self._fp8_guard("pack")
        self._scheds.clear()
        self._pack_target()
        mods = []
        self._mod_off = {}
        off = 0

        def reg(key, lin):
            nonlocal off
            mods.append(lin)
            self._mod_off[key] = off
            off += lin.weight.shape[0]

        for i, blk in enumerate(self.transformer_blocks):
            a = blk.attn
            blk._wqkv, blk._bqkv = _fuse_linears([a.to_q, a.to_k, a.to_v])
            blk._wqkv_c, blk._bqkv_c = _fuse_linears([a.add_q_proj, a.add_k_proj, a.add_v_proj])
            reg(("d", i, "img"), blk.norm1.linear)
            reg(("d", i, "txt"), blk.norm1_context.linear)
        for i, blk in enumerate(self.single_transformer_blocks):
            a = blk.attn
            blk._wqkv, blk._bqkv = _fuse_linears([a.to_q, a.to_k, a.to_v])
            reg(("s", i), blk.norm.linear)
        reg(("out",), self.norm_out.linear)
        self._stack_modulation(mods)
        # rows of the first block that runs (its modulation is needed before the side stream is joined)
        offs = sorted(self._mod_off.values())
        self._mod_first = offs[1] if len(offs) > 1 else off
        if self.transformer_blocks and len(offs) > 2:
            self._mod_first = offs[2]  # img + txt projections of double block 0
        self._packed = True

    # ---- fp8-scaled block weights resident in HBM (weights.load_checkpoint_into(keep_fp8=True)) and opt-in FP8 compute on them
    #  ------------------------------------------------------------------------------------------------------
    _fp8_formats = ("fp8",)            # GGUF blocks have no resident mode here (keep_quantized keeps raising)
    _FP8_QKV = (("to_q", "to_k", "to_v"), ("add_q_proj", "add_k_proj", "add_v_proj"))

    @staticmethod
    def _fp8_resident_key(key: str) -> bool:
        """Which fp8-scaled checkpoint tensors a `keep_fp8=True` load keeps as stored: the Linear weights of the double and single
        blocks (attention projections, feed-forwards, proj_mlp, proj_out).  Embedders, the AdaLN projections (`norm*.linear`) and
        the final projection stay dequantised at load."""
        return key.startswith(("transformer_blocks.", "single_transformer_blocks.")) and key.endswith(".weight") \
            and ".norm" not in key and ".processor." not in key

    @classmethod
    def _fp8_preflight(cls, keys) -> None:
        """Called by the loader on the CONVERTED key list before any tensor is written.  The resident mode fuses q | k | v into
        one record with a scale per row, so every part needs a `scale_weight` of its own, as diffusers-keyed fp8-scaled files
        have.  A BFL-format file stores one fused `qkv` / `linear1` tensor with ONE scale, which the key converter splits by
        rows: such a file is refused here, whole, instead of being half-loaded."""
        keys = set(keys)
        scaled = {k[:-len("scale_weight")] for k in keys if k.endswith("scale_weight")}
        if not any(k.endswith(".weight") and cls._fp8_resident_key(k) and k[:-len("weight")] in scaled for k in keys):
            raise NotImplementedError("flux.mi355 keep_fp8: the files hold no fp8-scaled block Linear of this model (no "
                                      "transformer_blocks.* / single_transformer_blocks.* weight with a scale_weight partner): "
                                      "there is nothing to keep resident; load without keep_fp8")
        for k in sorted(keys):
            for group in cls._FP8_QKV:
                if k.endswith(f".attn.{group[0]}.weight") and cls._fp8_resident_key(k):
                    base = k[:-len(f"{group[0]}.weight")]
                    have = [f"{base}{n}." in scaled for n in group if f"{base}{n}.weight" in keys]
                    if not all(have):
                        raise _l.ApexMIError(
                            f"flux.mi355 keep_fp8: '{base}{{{'|'.join(group)}}}' do not each carry a scale_weight after key "
                            "conversion.  This is what a BFL-format fp8 file gives (one fused qkv / linear1 tensor with ONE scale, "
                            "split by the converter): the resident mode takes diffusers-keyed fp8-scaled files (a separate to_q / "
                            "to_k / to_v with a scale_weight each).  Load it without keep_fp8 (dequantised at load) instead; "
                            "nothing was loaded.")

    def _fp8_plan(self):
        plan = []
        for blk in self.transformer_blocks:
            a, ff, ffc = blk.attn, blk.ff.net, blk.ff_context.net
            plan += [(blk, "_wqkv", [a.to_q.weight, a.to_k.weight, a.to_v.weight]),
                     (blk, "_wqkv_c", [a.add_q_proj.weight, a.add_k_proj.weight, a.add_v_proj.weight])]
            plan += [(blk, None, [p]) for p in (a.to_out[0].weight, a.to_add_out.weight, ff[0].proj.weight, ff[2].weight,
                                                 ffc[0].proj.weight, ffc[2].weight)]
        for blk in self.single_transformer_blocks:
            a = blk.attn
            plan += [(blk, "_wqkv", [a.to_q.weight, a.to_k.weight, a.to_v.weight]), (blk, None, [blk.proj_mlp.weight]),
                     (blk, None, [blk.proj_out.weight])]
        return plan

    def state_dict(self, *a, **k):
        self._fp8_guard("state_dict")
        return super().state_dict(*a, **k)

    def _lora_param(self, module: str, what: str):
        if module in (getattr(self, "_fp8_records", None) or {}):
            if not self._fp8_lora:
                raise _l.ApexMIError(f"flux.mi355: '{module}' is a resident fp8 Linear (keep_fp8 load): there is no bf16 weight to merge a "
                                     "LoRA into, and run-time LoRA on resident Flux weights is not supported — load without keep_fp8 "
                                     "to use adapters, or `set_fp8_compute(True, lora=True)` first")
            # what load_lora_adapter validates the factors against: a resident parameter has no bf16 storage, only `_fp8_shape`
            return next(p for k, p in self.named_parameters() if k == f"{module}.weight")
        return super()._lora_param(module, what)

    def _fp8_factors(self) -> bool:
        """whether any resident record carries run-time LoRA factors, or a registered adapter (active or not) could give it some"""
        recs = getattr(self, "_fp8_records", None) or {}
        return any(r.lora_A is not None for r in recs.values()) or \
            any(m in recs for d in getattr(self, "_lora_adapters", {}).values() for m in d)

    # ---- LoRA on resident fp8 weights: applied at RUN TIME inside the fp8 GEMMs (`set_fp8_compute(True, lora=True)`), as the
    # reference does around FPScaledLinear (R/src/lora/manager.py:454-606).  Modules whose weights are bf16 parameters still merge.
    def _lora_validate(self, adapter_name, mods):
        """the refusals of an adapter that touches resident records, before it is registered: the model stays as it is"""
        recs = getattr(self, "_fp8_records", None) or {}
        hit = [m for m in mods if m in recs]
        if not hit:
            return
        for m in hit:
            if "bias" in mods[m]:
                raise NotImplementedError(f"flux.mi355: adapter '{adapter_name}' carries a lora_B.bias for the resident-fp8 Linear "
                                          f"'{m}', which is not supported — drop the bias, or load without keep_fp8")
        if self.residual_dtype == torch.float32:
            raise _l.ApexMIError("flux.mi355: run-time LoRA on resident fp8 weights needs the bf16 residual stream (the float-output "
                                 "launches cannot take the fp8 route and there is no bf16 run-time-LoRA path): "
                                 "set_residual_dtype(torch.bfloat16) first")
        if self.storage_dtype == torch.float32:
            raise _l.ApexMIError("flux.mi355: run-time LoRA on resident fp8 weights needs bf16 storage (float activations cannot take the "
                                 "fp8 route and there is no bf16 run-time-LoRA path): set_storage_dtype(torch.bfloat16) first")

    @torch.no_grad()
    def _lora_remerge(self, modules):
        recs = getattr(self, "_fp8_records", None) or {}
        modules = set(modules)
        resident = {m for m in modules if m in recs}
        for rec in {id(recs[m]): recs[m] for m in resident}.values():
            rec.set_lora([(m, d[m]["A"], d[m]["B"], self._lora_scales[n]) for m, _, _ in rec.parts
                          for n, d in self._lora_adapters.items() if m in d and self._lora_scales[n] != 0.0 and self._lora_enabled])
        super()._lora_remerge(modules - resident)
        if modules - resident:
            self._fp4_detach()      # merged into the bf16 weights: the MXFP4 copies are rebuilt before the next forward

    def _invalidate(self, event: str):
        if event in ("moved", "loaded", "written"):
            self._fp4_detach()      # the weights change (`.to`, a load, `_weights_changed`): the MXFP4 copies go, and `forward` rebuilds them
        super()._invalidate(event)

    def set_storage_dtype(self, dtype: torch.dtype):
        if dtype == torch.float32 and self._fp8_factors():
            raise _l.ApexMIError("flux.mi355: resident fp8 records carry run-time LoRA factors, which need bf16 storage (the float "
                                 "activations of set_storage_dtype(torch.float32) cannot take the fp8 route and there is no bf16 "
                                 "run-time-LoRA path): delete or unload the adapters first")
        return super().set_storage_dtype(dtype)

    def set_residual_dtype(self, dtype: torch.dtype):
        if dtype == torch.float32 and self._fp8_factors():
            raise _l.ApexMIError("flux.mi355: resident fp8 records carry run-time LoRA factors, which need the bf16 residual stream "
                                 "(the float-output launches of set_residual_dtype(torch.float32) cannot take the fp8 route and there "
                                 "is no bf16 run-time-LoRA path): delete or unload the adapters first")
        return super().set_residual_dtype(dtype)

    def set_fp8_compute(self, on: bool, fused_quant: bool = False, mx_ffn: bool = False, lora: bool = False):
        """Opt-in approximation: the block launches whose weights are RESIDENT e4m3 records (a `keep_fp8=True`
        load) quantise their activations per row to e4m3 and multiply in fp8 — `ops.gemm_fp8_grouped` for the grouped launches
        (the QKV pair with the fused q/k/v epilogue when `fuse_qkv` is set and no IP adapter is active), `ops.gemm`'s fp8 route
        for the single block's proj_out — wherever `ops.fp8_grouped_route` / `ops.fp8_compute_route` hold.  Launches they refuse
        (the f32-storage mode, a float `out` = gate_res of the f32 residual stream, e5m2 records) run today's path, and so does
        everything outside the blocks.  False restores today's launches bit for bit.

        `fused_quant=True` (needs `on=True`): the norms in front of the QKV launches and of the double block's FF-up launch write
        the e4m3 codes and row scales themselves (`ops.ln_modulate_quant_fp8`); the bf16 rows, which nothing else reads, are not
        stored.  A launch and traffic change only: the forward is bit-identical to `fused_quant=False`.

        `mx_ffn=True` (needs `on=True`, composes with `fused_quant`): the double block's FF hidden state stays in fp8 between the
        FF-up pair and the FF-down pair.  Where `ops.fp8_mx_route` holds for both streams, the FF-up pair quantises its own GELU
        output per 32-column block in the epilogue (`ops.gemm_fp8_grouped(out_mx_list=)`: e4m3 codes + one e8m0 scale byte per
        block, both streams as row slices of one buffer) and the FF-down pair multiplies those codes with the hardware block
        scales (`block_scales_list=`), so the `quant_rows_fp8` launch of the hidden state and its bf16 round trip disappear.
        Codes and scale bytes live in the storage of the bf16 hidden buffer, which is not written in this mode.  This CHANGES
        the numbers (block scales instead of one scale per row of the hidden state).  The single block (its MLP-up output shares
        proj_out's K with the attention output) and the f32 residual stream keep today's launches; `mx_ffn=False` (the default)
        leaves every launch as it is.  An FF pair in which either record carries run-time LoRA factors keeps the per-row launches
        (`ops.fp8_mx_route` refuses factors).

        `lora=True` (needs `on=True`): RUN-TIME LoRA on the resident records.  `load_lora_adapter` / `set_adapters` /
        `delete_adapters` / `disable_lora` / `enable_lora` then give every resident record the active adapters of its parts
        (`ResidentWeight.set_lora`: block-diagonal B' for the fused q|k|v records) instead of refusing them; adapters on
        non-resident modules merge as always.  A launch with such a record stays on the fp8 GEMM: one grouped skinny GEMM
        (`ops.gemm_grouped` over the problems' `lora_A`; QKV and MLP-up of a single block share it) writes t = x A^T into a
        per-stream workspace, and the grouped / fused-qkv launch adds t B'^T per problem by the bf16 MFMA tail
        (`lora_t_list=` / `lora_B_list=`, where `ops.fp8_grouped_lora_route` holds; the single block's proj_out through
        `ops.gemm_fp8(lora_t=, lora_B=)`).  With `fused_quant` the norm also stores the bf16 rows a skinny GEMM reads.  The flag
        lives on the records (`lora_compute`); adapters that touch a resident module must be loaded AFTER this call (before it
        they are refused, as always).  Adapters on resident Flux
        weights exist in this mode ONLY: there is no bf16-compute run-time-LoRA path, so switching fp8 compute or `lora` off
        while records carry factors is refused (delete or unload the adapters first), as is the f32 residual stream together
        with factors and a `lora_B.bias` on a resident module.  `lora=False` (the default) leaves every launch as it is."""
        if lora and not on:
            raise ValueError("flux.mi355: set_fp8_compute(lora=True) needs on=True: the adapter tail belongs to the fp8 GEMM")
        if not (on and lora) and self._fp8_factors():
            raise _l.ApexMIError("flux.mi355: resident fp8 records carry run-time LoRA factors, which exist in fp8-compute mode only "
                                 f"(set_fp8_compute(True, lora=True)); set_fp8_compute({bool(on)}, lora={bool(lora)}) would leave them "
                                 "without a launch — delete or unload the adapters first (delete_adapters / unload_lora_weights)")
        if mx_ffn and not on:
            raise ValueError("flux.mi355: set_fp8_compute(mx_ffn=True) needs on=True: the MX hidden state belongs to the fp8 GEMMs")
        if fused_quant and not on:
            raise ValueError("flux.mi355: set_fp8_compute(fused_quant=True) needs on=True: the fused norm quantises for the fp8 GEMM")
        for r in self._fp8_set_compute(on):
            r.lora_compute = "fp8" if lora else "bf16"
        self._fp8_compute, self._fp8_fused_quant, self._fp8_mx_ffn, self._fp8_lora = bool(on), bool(fused_quant), bool(mx_ffn), bool(lora)
        return self

    # ---- opt-in MXFP4 compute on a bf16 model; the switch itself is module_base.Fp4ComputeMixin ----
    _FP4_LINEARS = ("qkv", "attn_out", "ffn_up", "ffn_down", "single_in", "single_out")

    def set_fp4_compute(self, on: bool, linears=None, fused_quant: bool = False, mx_ffn: bool = False):
        """Opt-in approximation: the selected block launches of a bf16 model quantise their activations per block of
        32 to MXFP4 — ONE `ops.quant_blocks_mxfp4` over the joint buffer both streams are row slices of — and multiply e2m1 x e2m1
        in one grouped launch (`ops.gemm_mxfp4_grouped`; `ops.gemm_mxfp4_grouped_qkv` with the fused q/k/v epilogue when `fuse_qkv`
        is set and no IP adapter is active) against MXFP4 copies of the weights (`ops.Mxfp4Weight.from_bf16`) that sit BESIDE the
        bf16 weights, on their `_fp4` slot: 0.53 bytes per selected weight element on top of the model.  `linears`, a subset of
          "qkv"         `_wqkv` and `_wqkv_c` of a double block
          "attn_out"    `to_out[0]` and `to_add_out`
          "ffn_up", "ffn_down"   both streams each
          "single_in"   a single block's `_wqkv` and `proj_mlp` (one launch, hence one name)
          "single_out"  `proj_out` of a single block (K = dim + mlp; through `ops.gemm`'s fp4 route)
        None = all six.  The embedders, the final proj_out, the modulation GEMVs, the IP-adapter projections and attention stay
        bf16.  A launch class is routed where `ops.mxfp4_grouped_route` holds (decided on block 0); a class it refuses keeps today's
        launch.  False detaches the records: the next forward is the original, bit for bit.  The records follow the model's
        invalidation rule (a load, `.to`, a merged LoRA): dropped there, rebuilt before the next forward while the mode is on.  A
        speed option, not a parity mode; no quality claim on real checkpoints.

        Refused: a resident (`keep_fp8`) model — so the mode never meets the `fp8_*` switches —, f32 activation storage and the
        f32 residual stream (`set_storage_dtype` / `set_residual_dtype` refuse float32 while the mode is on), an unknown name, and
        `linears` together with `on=False`.

        `fused_quant=True` (needs `on=True`): the norms in front of the QKV pair, the FF-up pair and the single block's QKV +
        MLP-up launch write the MXFP4 codes and scale bytes of the joint buffer themselves (`ops.ln_modulate_quant_mxfp4`) where
        those classes route to fp4, so their `quant_blocks_mxfp4` launch disappears and the bf16 normalised rows are never stored;
        the streams stay row slices of one codes buffer.  `mx_ffn=True` (needs `on=True`, composes with `fused_quant`): where
        `ops.mxfp4_grouped_mx_route` holds, the FF-up pair of a double block writes its GELU output as MXFP4 into the bytes of the
        hidden buffer (`ops.gemm_mxfp4_grouped(out_mx_list=)`) and the FF-down pair reads it; in a single block (dim % 128 == 0,
        "single_in" and "single_out" both routed) the MLP-up problem writes its codes into columns [dim, dim + mlp) of a codes /
        scales buffer for the concatenated rows, ONE `quant_blocks_mxfp4` covers the attention columns only, and `proj_out` reads
        the joint codes.  Both change launches and traffic only: the forward is bit-identical to the mode without them.  A class
        that `ops.mxfp4_grouped_route` refuses, the APEX_FLUX_OVERLAP path and the QKV pair with an active IP adapter keep their
        launches.  The defaults (False) leave every launch as it is."""
        return self._fp4_switch(on, linears, fused_quant, mx_ffn)

    def _fp4_blocks(self):
        return list(self.transformer_blocks) + list(self.single_transformer_blocks)

    def _fp4_weights(self, blk) -> dict:
        a = blk.attn
        if isinstance(blk, _SingleBlock):
            return {"single_in": (blk._wqkv, blk.proj_mlp.weight), "single_out": (blk.proj_out.weight,)}
        ff, ffc = blk.ff.net, blk.ff_context.net
        return {"qkv": (blk._wqkv, blk._wqkv_c), "attn_out": (a.to_out[0].weight, a.to_add_out.weight),
                "ffn_up": (ff[0].proj.weight, ffc[0].proj.weight), "ffn_down": (ff[2].weight, ffc[2].weight)}

    def _rows_fp4(self, src, quantised=None):
        """(codes, scale bytes) of the rows of the joint buffer `src`: the fused norm's (`quantised`), or ONE quantise launch into
        the per-stream fp4 scratch; the streams of a grouped launch are row slices of both."""
        if quantised is not None:
            return quantised
        qa, sa = ops._act_scratch_mx(ops._MXFP4, src.device, src.shape[0], src.shape[1])
        return ops.quant_blocks_mxfp4(src, out=qa, scale_out=sa)

    def _norm_rows(self, X, XN, rows, w_list, epilogue, *mod, fp4=False, **kw):
        """ln_modulate(X, *mod, out=XN, **kw) in front of a grouped launch (bf16 outputs) over the row ranges `rows` of XN and the
        weights `w_list`, which is the ONLY reader of XN.  With `set_fp8_compute(fused_quant=True)`, where that launch takes its
        fp8 route and the fused norm accepts the rows, the norm quantises in its own launch and does not store XN: returns
        (codes, scales), else None.  An empty `w_list` = the caller already knows that the launch does not route.  `fp4`: the
        launch is an fp4 one (the caller has asked `ops.mxfp4_grouped_route`); with `set_fp4_compute(fused_quant=True)` the norm
        then writes the MXFP4 pair of the joint buffer and returns it."""
        if fp4 and self._fp4_fused_quant and ops.fp8_norm_quant_rows(X, XN):
            return ops.ln_modulate_quant_mxfp4(X, *mod, **kw)
        if self._fp8_fused_quant and w_list:
            ws = [w if ops._fp8_of(w) is None else ops._fp8_of(w) for w in w_list]
            probe = XN.new_empty((0,), dtype=torch.bfloat16)     # the predicates read the dtype of `out` only
            epis = [epilogue] * len(ws) if isinstance(epilogue, str) else list(epilogue)
            if ops.fp8_grouped_route([XN[r] for r in rows], ws, [probe] * len(ws), epis) \
                    and ops.fp8_norm_quant_route(X, XN, ws[0], probe, epis[0])[0]:
                return ops.ln_modulate_quant_fp8(X, *mod, **kw)
            # a reader with run-time LoRA factors: its skinny GEMM reads the bf16 rows, so the norm stores them too (need_row)
            if self._fp8_lora and ops.fp8_grouped_lora_route([XN[r] for r in rows], ws, [probe] * len(ws), epis) \
                    and ops.fp8_norm_quant_rows(X, XN):
                return ops.ln_modulate_quant_fp8(X, *mod, out=XN, **kw)
        ops.ln_modulate(X, *mod, out=XN, **kw)
        return None

    def _lora_t(self, a_list, w_list):
        """(lora_t_list, lora_B_list) of a launch whose records `w_list` may carry run-time LoRA factors: t_i = a_i A_i^T for every
        problem with factors, by ONE grouped skinny GEMM (the problems share K), into the per-stream workspace — valid until this
        stream's next call.  None entries = no adapter on that problem."""
        idx = [i for i, w in enumerate(w_list) if w.lora_A is not None]
        sizes = [a_list[i].shape[0] * w_list[i].lora_A.shape[0] for i in idx]
        dev = a_list[0].device
        buf = ops._workspace(("flux_lora_t", dev.index, torch.cuda.current_stream().cuda_stream), dev, 2 * sum(sizes)).view(torch.bfloat16)
        ts, off = [None] * len(w_list), 0
        for i, n in zip(idx, sizes):
            ts[i] = buf[off:off + n].view(a_list[i].shape[0], w_list[i].lora_A.shape[0])
            off += n
        ops.gemm_grouped([a_list[i] for i in idx], [w_list[i].lora_A for i in idx], None, [ts[i] for i in idx])
        return ts, [w.lora_B for w in w_list]

    def _rows_fp8(self, src, quantised):
        """(codes, scales) of the rows of the joint buffer `src`: the fused norm's, or one `quant_rows_fp8` launch into the
        per-stream scratch.  The codes of one joint buffer serve both streams as row slices."""
        if quantised is not None:
            return quantised
        qa, sa = ops._act_scratch(src.device, src.shape[0], src.shape[1])
        return ops.quant_rows_fp8(src, out=qa, scale_out=sa)

    def _grouped(self, src, rows, w_list, bias_list, out_list, epilogue, gate_list=None, residual_list=None, quantised=None,
                 fp4=False, out_mx_list=None):
        """One grouped launch whose problems read the row ranges `rows` (slices) of ONE activation buffer `src`: today's
        `ops.gemm_grouped`, or — in fp8-compute mode, when `ops.fp8_grouped_route` holds for every problem — one quantise launch
        over `src` (unless `quantised` brings the codes) and `ops.gemm_fp8_grouped`.  `fp4`: the caller has asked
        `ops.mxfp4_grouped_route` for this launch class (set_fp4_compute): one `quant_blocks_mxfp4` over `src` and
        `ops.gemm_mxfp4_grouped` on the weights' MXFP4 records (`quantised`: the fused norm's MXFP4 pair; `out_mx_list`: see
        `ops.gemm_mxfp4_grouped`, fp4 only)."""
        if fp4:
            qa, sa = self._rows_fp4(src, quantised)
            mx = {} if out_mx_list is None else {"out_mx_list": out_mx_list}
            return ops.gemm_mxfp4_grouped([qa[r] for r in rows], [sa[r] for r in rows], [w._fp4 for w in w_list], bias_list, out_list,
                                          epilogue=epilogue, gate_list=gate_list, residual_list=residual_list, **mx)
        assert out_mx_list is None
        w_list = [w if ops._fp8_of(w) is None else ops._fp8_of(w) for w in w_list]
        a_list = [src[r] for r in rows]
        if self._fp8_compute and ops.fp8_grouped_route(a_list, w_list, out_list, epilogue):
            qa, sa = self._rows_fp8(src, quantised)
            return ops.gemm_fp8_grouped([qa[r] for r in rows], [sa[r] for r in rows], w_list, bias_list, out_list, epilogue=epilogue,
                                        gate_list=gate_list, residual_list=residual_list)
        if self._fp8_compute and self._fp8_lora and ops.fp8_grouped_lora_route(a_list, w_list, out_list, epilogue):
            lt, lb = self._lora_t(a_list, w_list)          # the skinny launch first: it reads the bf16 rows
            qa, sa = self._rows_fp8(src, quantised)
            return ops.gemm_fp8_grouped([qa[r] for r in rows], [sa[r] for r in rows], w_list, bias_list, out_list, epilogue=epilogue,
                                        gate_list=gate_list, residual_list=residual_list, lora_t_list=lt, lora_B_list=lb)
        assert quantised is None, "the fused norm did not store the rows this launch reads"
        return ops.gemm_grouped(a_list, w_list, bias_list, out_list, epilogue=epilogue, gate_list=gate_list,
                                residual_list=residual_list)

    def _workspace(self, s_txt: int, s_img: int):
        # one workspace per (shape, HIP stream): two clips may run through one resident model on two streams
        key = (s_txt, s_img, torch.cuda.current_stream().cuda_stream)
        ws = self._ws.get(key)
        if ws is not None and ws.shipped == ops.shipped_verification():
            return ws
        dev, dim = self.device, self.inner_dim
        H = self.config.num_attention_heads
        S = s_txt + s_img
        skp = (S + 63) // 64 * 64
        bf = dict(device=dev, dtype=self.storage_dtype)     # activation buffers
        f32 = dict(device=dev, dtype=torch.float32)
        mlp = 4 * dim
        xdt = torch.float32 if self.residual_dtype == torch.float32 else self.storage_dtype      # the residual stream
        ws = SimpleNamespace(
            X=torch.empty(S, dim, device=dev, dtype=xdt), XN=torch.empty(S, dim, **bf), QKV=torch.empty(S, 3 * dim, **bf),
            Q=torch.empty(1, H, S, 128, **bf), K=torch.empty(1, H, S, 128, **bf),
            VT=torch.zeros(1, H, 128, skp, **bf), CAT=torch.empty(S, dim + mlp, **bf),
            FFH=torch.empty(S, mlp, **bf), MOD=torch.empty(1, self._mod_total, **f32),
            TEMB=torch.empty(1, dim, **f32), OUT=torch.empty(s_img, self.proj_out.out_features, **bf),
            shipped=ops.shipped_verification(),
        )
        if ws.shipped and self.storage_dtype == torch.float32:
            # verification through the shipped kernels (ops.verify_through_shipped_kernels): the fused QKV epilogue and the flash
            # attention kernel exchange q / k / v^T in bf16, as in production
            b16 = dict(device=dev, dtype=torch.bfloat16)
            ws.Qb, ws.Kb, ws.VTb = torch.empty(1, H, S, 128, **b16), torch.empty(1, H, S, 128, **b16), torch.zeros(1, H, 128, skp, **b16)
        self._ws = {k: v for k, v in self._ws.items() if k[:2] == key[:2]}  # one shape resident at a time
        self._ws[key] = ws
        return ws

    # ---- the denoise step --------------------------------------------------------------------
    def _mod(self, mod, key, idx):
        off = self._mod_off[key] + idx * self.inner_dim
        return mod[0, off:off + self.inner_dim]

    # ---- the whole clip's modulation vectors in one pass over the AdaLN weights ------------------------------------------
    def _cond_rows(self, timestep, guidance, pooled):
        """Conditioning vectors `time_text_embed(timestep, guidance, pooled)` (model.py:535-545) for R rows at once, f32 [R, dim];
        row r is bit-identical to what `_forward_one` builds for (timestep[r], guidance[r], pooled[r]) — same kernels (the
        multi-row GEMV reproduces the single-row arithmetic), same accumulation order t, + guidance, + text."""
        cfg, tte, cdt = self.config, self.time_text_embed, self.storage_dtype
        t = (timestep.to(cdt) * 1000).float().reshape(-1)
        R = t.shape[0]

        def emb(e, proj):
            h = ops.gemv(e.linear_1.weight, proj, e.linear_1.bias, post="silu")
            return ops.gemv(e.linear_2.weight, h, e.linear_2.bias)
        out = emb(tte.timestep_embedder, ops.timestep_embedding(t, 256))
        if cfg.guidance_embeds:
            if guidance is None:
                raise ValueError("guidance_embeds=True model called without `guidance`")
            g = (guidance.to(cdt) * 1000).float().reshape(-1)
            out = emb(tte.guidance_embedder, ops.timestep_embedding(g, 256)) + out      # the ACCUM epilogue's `new + old`
        return emb(tte.text_embedder, pooled.float().reshape(R, -1).contiguous()) + out

    @torch.no_grad()
    def begin_schedule(self, timesteps, guidance, pooled_projections):
        """Every AdaLN shift / scale / gate vector of EVERY step of a clip, computed once when the sampler's timesteps are known
        (VERDICT r3 item 1b).  Per step the stacked `norm*.linear` projections are a 6.4 GB weight-streaming GEMV whose input
        depends only on (t, guidance, pooled) — all known before the loop — so the n steps become ONE pass over those weights
        (`apexmi_gemv` with M = n·B rows, each row bit-identical to the per-step launch) instead of n.

        `timesteps`: [n] or [n, B], the values `forward(timestep=…)` will receive (i.e. already / 1000); `guidance`: [B] or
        None; `pooled_projections`: one [B, P] tensor or a list of them (conditional / unconditional pass of true CFG).
        `begin_schedule` returns the clip's HANDLE (schedule.ModulationSchedule).  `forward(..., joint_attention_kwargs=
        {"modulation_step": i, "modulation_schedule": handle})` with one of these pooled tensors then reads row i of its table;
        any other call computes its vectors as before.  Without a handle the call is served only while exactly one schedule is
        live on the model (two clips through one resident model on two streams must pass theirs).  `end_schedule(handle)` frees
        the tables (n·B × 4.2 MB each) and raises if a scheduled step was called with another timestep / guidance."""
        self.pack()
        n = int(timesteps.shape[0])
        pls = pooled_projections if isinstance(pooled_projections, (list, tuple)) else [pooled_projections]
        sched = None
        for pooled in pls:
            if pooled is None:
                continue
            pooled = pooled.to(self.device)
            B = pooled.shape[0]
            ts = timesteps.to(self.device)
            ts = ts.reshape(n, 1).expand(n, B) if ts.dim() == 1 else ts
            if ts.shape != (n, B):
                raise ValueError(f"begin_schedule: timesteps {tuple(timesteps.shape)} do not match a batch of {B}")
            g = None if guidance is None else guidance.to(self.device).reshape(1, -1).expand(n, B)
            cond = self._cond_rows(ts.reshape(-1), None if g is None else g.reshape(-1),
                                   pooled.unsqueeze(0).expand(n, B, pooled.shape[-1]).reshape(n * B, -1))
            if sched is None:
                sched = ModulationSchedule(n, B, ts, None if g is None else g[0])
                sched.pooled = []
            elif B != sched.B:
                raise ValueError("begin_schedule: the pooled tensors of one clip must share a batch size")
            sched.tables[(pooled.data_ptr(), tuple(pooled.shape))] = ops.gemv(self._mod_w, cond, self._mod_b, pre_silu=True)  # [n B, mod_total] f32
            sched.pooled.append(pooled)           # keeps the key's storage alive for the clip
        return None if sched is None else self._scheds.add(sched)

    def end_schedule(self, handle=None):
        self._scheds.end(handle)
        return self

    def _sched_row(self, pooled_projections, jkw, b, timestep=None, guidance=None):
        """[1, mod_total] view of the table row for (step, image b), or None when this call is not part of a scheduled clip."""
        sc = self._scheds.find(jkw)
        if sc is None:
            return None
        return sc.row((pooled_projections.data_ptr(), tuple(pooled_projections.shape)), int(jkw["modulation_step"]), b,
                      timestep, guidance)

    def _embed_t(self, emb: _TimestepEmbedding, proj: torch.Tensor, out: torch.Tensor, accum: bool):
        h = ops.gemv(emb.linear_1.weight, proj, emb.linear_1.bias, post="silu")
        ops.gemv(emb.linear_2.weight, h, emb.linear_2.bias, out=out, accum=accum)

    def _rope(self, txt_ids, img_ids):
        """The rotary table depends on the position ids only, which a sampler loop passes unchanged every step: keep the last table
        while the SAME tensor objects come back unmodified (the cache holds references to them, so their storage cannot be
        recycled under another tensor, and an in-place edit bumps `_version`)."""
        rk = self._rope_cache
        ver = (ops.tensor_version(txt_ids), ops.tensor_version(img_ids))
        # inference tensors (ids built inside the host's `@torch.inference_mode()` run, R/src/engine/registry.py:196) carry no
        # version counter: an in-place edit would go unseen, so the table is rebuilt for them (one ~20 us launch per step)
        cacheable = ver[0] is not None and ver[1] is not None
        if (cacheable and rk is not None and rk[0] is txt_ids and rk[1] is img_ids and rk[2] == ver
                and rk[4] == self.storage_dtype):
            return rk[3]
        ids = torch.cat((txt_ids, img_ids), dim=0).float()
        rope = ops.rope_table_axes(ids, self.config.axes_dims_rope, 10000.0)
        ops.rope_pairs(rope, trusted=True)      # the compact copy the fused q/k/v epilogue reads, made HERE with the table (before any stream forks)
        self._rope_cache = (txt_ids, img_ids, ver, rope, self.storage_dtype) if cacheable else None
        return rope

    def _step_modulation(self, ws, pooled, timestep, guidance):
        """This step's modulation vectors into ws.MOD (a call outside a scheduled clip).  Returns the event to join before the
        second block, or None."""
        cfg = self.config
        # conditioning vector (f32): timestep.to(dtype) * 1000 as the reference does (model.py:535)
        tte = self.time_text_embed
        cdt = self.storage_dtype     # the reference's `hidden_states.dtype`: bf16 in production, f32 when verifying
        t = (timestep.to(cdt) * 1000).float().reshape(1)
        self._embed_t(tte.timestep_embedder, ops.timestep_embedding(t, 256), ws.TEMB, accum=False)
        if cfg.guidance_embeds:
            if guidance is None:
                raise ValueError("guidance_embeds=True model called without `guidance`")
            g = (guidance.to(cdt) * 1000).float().reshape(1)
            self._embed_t(tte.guidance_embedder, ops.timestep_embedding(g, 256), ws.TEMB, accum=True)
        self._embed_t(tte.text_embedder, pooled.float().reshape(1, -1), ws.TEMB, accum=True)
        return self._modulation_gemv(ws.MOD, ws.TEMB)     # the first block's rows now, the rest on the side stream

    @torch.no_grad()
    def _forward_one(self, hidden_states, encoder_hidden_states, pooled, timestep, img_ids, txt_ids,
                     guidance, mod_row=None, cn_d=None, cn_s=None, ip=None):
        cfg = self.config
        dim, H = self.inner_dim, cfg.num_attention_heads
        s_img, s_txt = hidden_states.shape[0], encoder_hidden_states.shape[0]
        S = s_txt + s_img
        ws = self._workspace(s_txt, s_img)
        X, XN, QKV, CAT, FFH = ws.X, ws.XN, ws.QKV, ws.CAT, ws.FFH
        Xt, Xi = X[:s_txt], X[s_txt:]
        XNt, XNi = XN[:s_txt], XN[s_txt:]

        ops.gemm(hidden_states, self.x_embedder.weight, self.x_embedder.bias, out=Xi)
        ops.gemm(encoder_hidden_states, self.context_embedder.weight, self.context_embedder.bias, out=Xt)

        MOD = mod_row if mod_row is not None else ws.MOD
        mod_ready = None
        if mod_row is None:
            mod_ready = self._step_modulation(ws, pooled, timestep, guidance)

        rope = self._rope(txt_ids, img_ids)

        q_in, k_in, v_in = QKV[:, :dim], QKV[:, dim:2 * dim], QKV[:, 2 * dim:]
        Qp, Kp, VT = ws.Q, ws.K, ws.VT
        att = CAT[:, :dim]
        att_v = att.unflatten(-1, (H, 128)).unsqueeze(0)  # [1, S, H, 128] strided view

        nblk = 0
        overlap = os.environ.get("APEX_FLUX_OVERLAP") == "1"
        # fused q/k/v preparation (apexmi_gemm_bf16_grouped_qkv): bit-identical to the two-pass path; `fuse_qkv = False` keeps
        # the [S, 3 dim] projection as a storage point (tests/stage_parity.py reads it)
        mixed = self.storage_dtype == torch.float32 and ops.shipped_verification()
        fuse = self.fuse_qkv and (self.storage_dtype == torch.bfloat16 or mixed) and self.transformer_blocks is not None
        # IP-adapter: the image queries are needed normalised but NOT rotated (attention.py:199) -> the two-pass q/k/v preparation
        # resident fp8 weights: gemm_grouped_qkv needs bf16 weights, so bf16 compute on them takes the two-pass path; fp8 compute
        # has its own fused form (gemm_fp8_grouped_qkv: any row count), decided per launch class by the routing predicate
        resident = bool(getattr(self, "_fp8_bytes", 0))
        fuse_d = fuse and not resident and ip is None and len(self.transformer_blocks) > 0 and ops.qkv_fusable(
            [XNi, XNt], [self.transformer_blocks[0]._wqkv, self.transformer_blocks[0]._wqkv_c], [s_txt, 0], H)
        fuse_s = fuse and not resident and len(self.single_transformer_blocks) > 0 and ops.qkv_fusable(
            [XN, XN], [self.single_transformer_blocks[0]._wqkv, self.single_transformer_blocks[0].proj_mlp.weight], [0, 0], H)
        fp8 = resident and self._fp8_compute
        rec = lambda w: w if ops._fp8_of(w) is None else ops._fp8_of(w)      # noqa: E731  (the resident record behind a parameter)
        both, img_txt = [slice(None), slice(None)], [slice(s_txt, None), slice(0, s_txt)]
        fp8_d = fp8 and len(self.transformer_blocks) > 0 and ops.fp8_grouped_route(
            [XNi, XNt], [self.transformer_blocks[0]._wqkv, self.transformer_blocks[0]._wqkv_c], [QKV[s_txt:], QKV[:s_txt]], "bias")
        fp8_s = fp8 and not overlap and len(self.single_transformer_blocks) > 0 and ops.fp8_grouped_route(
            [XN, XN], [self.single_transformer_blocks[0]._wqkv, rec(self.single_transformer_blocks[0].proj_mlp.weight)],
            [QKV, CAT[:, dim:]], ["bias", "gelu"])
        # opt-in MXFP4 compute (set_fp4_compute; a bf16 model, never a resident one): each launch class is decided ONCE, on block 0
        # of its kind — every block carries records for the same names —, by the pure predicate; a class it refuses (a name that
        # is not selected, an ineligible shape) keeps today's launch
        f4_qkv = f4_out = f4_up = f4_down = f4_sin = False
        if self._fp4_linears is not None and len(self.transformer_blocks) > 0:
            b0 = self.transformer_blocks[0]
            att_it, ffh_it = [att[s_txt:], att[:s_txt]], [FFH[s_txt:], FFH[:s_txt]]
            f4_qkv = ops.mxfp4_grouped_route([XNi, XNt], [b0._wqkv, b0._wqkv_c], [QKV[s_txt:], QKV[:s_txt]], "bias")
            f4_out = ops.mxfp4_grouped_route(att_it, [b0.attn.to_out[0].weight, b0.attn.to_add_out.weight], [Xi, Xt], "gate_res")
            f4_up = ops.mxfp4_grouped_route([XNi, XNt], [b0.ff.net[0].proj.weight, b0.ff_context.net[0].proj.weight], ffh_it, "gelu")
            f4_down = ops.mxfp4_grouped_route(ffh_it, [b0.ff.net[2].weight, b0.ff_context.net[2].weight], [Xi, Xt], "gate_res")
        if self._fp4_linears is not None and not overlap and len(self.single_transformer_blocks) > 0:
            s0 = self.single_transformer_blocks[0]
            f4_sin = ops.mxfp4_grouped_route([XN, XN], [s0._wqkv, s0.proj_mlp.weight], [QKV, CAT[:, dim:]], ["bias", "gelu"])
        # set_fp4_compute(mx_ffn=True): the FF hidden state of the double blocks as MXFP4 codes + scale bytes in the bytes of FFH, and
        # the single block's MLP columns as codes in a codes / scales buffer for CAT (ws.CATQ / ws.CATS) that proj_out reads
        mx4_d = mx4_s = False
        if self._fp4_mx_ffn and f4_up and f4_down and FFH.stride(0) % 8 == 0:
            b0 = self.transformer_blocks[0]
            mx4_d = ops.mxfp4_grouped_mx_route([XNi, XNt], [b0.ff.net[0].proj.weight, b0.ff_context.net[0].proj.weight],
                                               [b0.ff.net[2].weight, b0.ff_context.net[2].weight], "gelu", "gate_res", [Xi, Xt])
        if mx4_d:
            raw4 = FFH.view(torch.uint8)
            hq4, hs4 = raw4[:, :FFH.shape[1] // 2], raw4[:, FFH.shape[1] // 2:FFH.shape[1] // 2 + FFH.shape[1] // 32]
        if self._fp4_mx_ffn and f4_sin and dim % 128 == 0 and (CAT.shape[1] - dim) % 128 == 0:
            mx4_s = ops.mxfp4_route(CAT, self.single_transformer_blocks[0].proj_out.weight, X, "gate_res")
        if mx4_s:
            if getattr(ws, "CATQ", None) is None:
                ws.CATQ = torch.empty(S, (CAT.shape[1] // 2 + 15) // 16 * 16, device=X.device, dtype=torch.uint8)[:, :CAT.shape[1] // 2]
                ws.CATS = torch.empty(S, (CAT.shape[1] // 32 + 3) // 4 * 4, device=X.device, dtype=torch.uint8)[:, :CAT.shape[1] // 32]
            cat_mx = [None, (ws.CATQ[:, dim // 2:], ws.CATS[:, dim // 32:])]
        # run-time LoRA on resident records (set_fp8_compute(lora=True)): which blocks carry factors is the adapter's business, so
        # with factors anywhere every launch class is decided PER BLOCK: False = the plain fp8 launch, True = the fp8 launch with
        # the adapter tail (one grouped skinny GEMM in front of it), None = not routed.  Without factors the block-0 decisions
        # above hold for every block, as they always did.
        lora_live = fp8 and self._fp8_lora and any(r.lora_A is not None for r in self._fp8_records.values())
        if lora_live and overlap:
            raise _l.ApexMIError("flux.mi355: the APEX_FLUX_OVERLAP=1 experiment has no launch for resident records with run-time LoRA "
                                 "factors — unset it, or delete / unload the adapters")

        def fp8_kind(a_list, w_list, out_list, epis):
            if ops.fp8_grouped_route(a_list, w_list, out_list, epis):
                return False
            return True if ops.fp8_grouped_lora_route(a_list, w_list, out_list, epis) else None

        def mx_route(blk):
            return all(ops.fp8_mx_route(xn, net[0].proj.weight, net[2].weight, "gelu", "gate_res", out=x) for xn, net, x in
                       ((XNi, blk.ff.net, Xi), (XNt, blk.ff_context.net, Xt)))
        # mx_ffn: the FF hidden state of the double blocks as MX codes + block scales in the bytes of FFH (no bf16 row is stored);
        # a block whose FF records carry factors keeps the per-row launches (mx_route refuses factors)
        mlp = FFH.shape[1]
        mx_d = fp8 and self._fp8_mx_ffn and len(self.transformer_blocks) > 0 and (lora_live or mx_route(self.transformer_blocks[0]))
        if mx_d:
            raw = FFH.view(torch.uint8)
            hq, hs = raw[:, :mlp], raw[:, mlp:mlp + mlp // 32]
        if overlap and self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        if mixed:        # the fused launches and the flash kernel behind them exchange bf16 q / k / v^T (ws.Qb ..), as in production
            qkv_d = (ws.Qb, ws.Kb, ws.VTb) if fuse_d else (ws.Q, ws.K, ws.VT)
            qkv_s = (ws.Qb, ws.Kb, ws.VTb) if fuse_s else (ws.Q, ws.K, ws.VT)
        else:
            qkv_d = qkv_s = (ws.Q, ws.K, ws.VT)

        def join_mod():
            nonlocal mod_ready
            if mod_ready is not None:
                torch.cuda.current_stream().wait_event(mod_ready)
                mod_ready = None

        for i, blk in enumerate(self.transformer_blocks):
            if nblk == 1:
                join_mod()
            nblk += 1
            a = blk.attn
            Qp, Kp, VT = qkv_d
            mi = lambda j: self._mod(MOD, ("d", i, "img"), j)  # noqa: E731
            mt = lambda j: self._mod(MOD, ("d", i, "txt"), j)  # noqa: E731
            # chunk order: shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp
            kind = fp8_kind([XNi, XNt], [blk._wqkv, blk._wqkv_c], [QKV[s_txt:], QKV[:s_txt]], "bias") if lora_live else \
                (False if fp8_d else None)
            fuse8_d = kind is not None and self.fuse_qkv and ip is None
            qn = self._norm_rows(X, XN, img_txt, [blk._wqkv, blk._wqkv_c] if kind is not None else [], "bias", mi(1), mi(0), split=s_txt,
                                 scale2=mt(1), shift2=mt(0), fp4=f4_qkv and ip is None)
            if f4_qkv and self.fuse_qkv and ip is None:
                qa, sa = self._rows_fp4(XN, qn)
                ops.gemm_mxfp4_grouped_qkv([qa[s_txt:], qa[:s_txt]], [sa[s_txt:], sa[:s_txt]], [blk._wqkv._fp4, blk._wqkv_c._fp4],
                                           [blk._bqkv, blk._bqkv_c], [None, None], "bias", [1, 1],
                                           [a.norm_q.weight, a.norm_added_q.weight], [a.norm_k.weight, a.norm_added_k.weight],
                                           [s_txt, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0])
            elif fuse8_d:
                lt, lb = self._lora_t([XNi, XNt], [blk._wqkv, blk._wqkv_c]) if kind else (None, None)
                qa, sa = self._rows_fp8(XN, qn)
                ops.gemm_fp8_grouped_qkv([qa[s_txt:], qa[:s_txt]], [sa[s_txt:], sa[:s_txt]], [blk._wqkv, blk._wqkv_c],
                                         [blk._bqkv, blk._bqkv_c], [None, None], "bias", [1, 1],
                                         [a.norm_q.weight, a.norm_added_q.weight], [a.norm_k.weight, a.norm_added_k.weight],
                                         [s_txt, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0], lora_t_list=lt, lora_B_list=lb)
            elif fuse_d:
                # q/k norm + RoPE + [H, S, D] layout and V^T leave the QKV GEMM's epilogue: no [S, 3 dim] round trip
                ops.gemm_grouped_qkv([XNi, XNt], [blk._wqkv, blk._wqkv_c], [blk._bqkv, blk._bqkv_c], [None, None], "bias",
                                     [1, 1], [a.norm_q.weight, a.norm_added_q.weight], [a.norm_k.weight, a.norm_added_k.weight],
                                     [s_txt, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0])
            else:
                self._grouped(XN, img_txt, [blk._wqkv, blk._wqkv_c], [blk._bqkv, blk._bqkv_c], [QKV[s_txt:], QKV[:s_txt]], "bias",
                              quantised=qn, fp4=f4_qkv)
                ops.qkv_prepare(q_in, k_in, v_in, H, Qp[0], Kp[0], VT[0], wq=a.norm_q.weight,
                                wk=a.norm_k.weight, wq2=a.norm_added_q.weight, wk2=a.norm_added_k.weight,
                                split=s_txt, eps=1e-6, rope=rope, rope_mode=_l.ROPE_INTERLEAVED)
            if ip is not None:
                if getattr(ws, "IPQ", None) is None:
                    ws.IPQ = torch.empty(1, H, s_img, 128, device=X.device, dtype=self.storage_dtype)
                ops.qkv_prepare(q_in[s_txt:], None, None, H, ws.IPQ[0], None, None, wq=a.norm_q.weight, eps=1e-6)
            ops.attention_prepared(Qp, Kp, VT, att_v, S)
            self._grouped(att, img_txt, [a.to_out[0].weight, a.to_add_out.weight], [a.to_out[0].bias, a.to_add_out.bias], [Xi, Xt],
                          "gate_res", gate_list=[mi(2), mt(2)], residual_list=[Xi, Xt], fp4=f4_out)
            ff, ffc = blk.ff.net, blk.ff_context.net
            qn = self._norm_rows(X, XN, img_txt, [ff[0].proj.weight, ffc[0].proj.weight] if fp8 else [], "gelu", mi(4), mi(3),
                                 split=s_txt, scale2=mt(4), shift2=mt(3), fp4=f4_up)
            if mx4_d:
                qa, sa = self._rows_fp4(XN, qn)
                ops.gemm_mxfp4_grouped([qa[r] for r in img_txt], [sa[r] for r in img_txt], [ff[0].proj.weight._fp4, ffc[0].proj.weight._fp4],
                                       [ff[0].proj.bias, ffc[0].proj.bias], [None, None], "gelu",
                                       out_mx_list=[(hq4[r], hs4[r]) for r in img_txt])
                ops.gemm_mxfp4_grouped([hq4[r] for r in img_txt], [hs4[r] for r in img_txt], [ff[2].weight._fp4, ffc[2].weight._fp4],
                                       [ff[2].bias, ffc[2].bias], [Xi, Xt], "gate_res", gate_list=[mi(5), mt(5)],
                                       residual_list=[Xi, Xt])
            elif mx_d and (not lora_live or mx_route(blk)):
                qa, sa = self._rows_fp8(XN, qn)
                ops.gemm_fp8_grouped([qa[r] for r in img_txt], [sa[r] for r in img_txt], [rec(ff[0].proj.weight), rec(ffc[0].proj.weight)],
                                     [ff[0].proj.bias, ffc[0].proj.bias], [None, None], "gelu",
                                     out_mx_list=[(hq[r], hs[r]) for r in img_txt])
                ops.gemm_fp8_grouped([hq[r] for r in img_txt], [None, None], [rec(ff[2].weight), rec(ffc[2].weight)],
                                     [ff[2].bias, ffc[2].bias], [Xi, Xt], "gate_res", gate_list=[mi(5), mt(5)],
                                     residual_list=[Xi, Xt], block_scales_list=[hs[r] for r in img_txt])
            else:
                self._grouped(XN, img_txt, [ff[0].proj.weight, ffc[0].proj.weight], [ff[0].proj.bias, ffc[0].proj.bias],
                              [FFH[s_txt:], FFH[:s_txt]], "gelu", quantised=qn, fp4=f4_up)
                self._grouped(FFH, img_txt, [ff[2].weight, ffc[2].weight], [ff[2].bias, ffc[2].bias], [Xi, Xt], "gate_res",
                              gate_list=[mi(5), mt(5)], residual_list=[Xi, Xt], fp4=f4_down)
            if ip is not None:
                # `hidden_states + ip_attn_output` AFTER the feed-forward (model.py:308-309); ip_attn_output = sum over adapters of
                # scale x attention(image queries, to_k_ip(tokens), to_v_ip(tokens)) (attention.py:232-262): a few keys per adapter
                proc = a.processor
                for h_ip, sc, wk, wv in zip(ip, proc.scale, proc.to_k_ip, proc.to_v_ip):
                    n = h_ip.shape[0]
                    ik = ops.gemm(h_ip, wk.weight, wk.bias).view(1, n, H, 128).permute(0, 2, 1, 3)
                    iv = ops.gemm(h_ip, wv.weight, wv.bias).view(1, n, H, 128).permute(0, 2, 1, 3)
                    o = ops.attention(ws.IPQ, ik, iv).permute(0, 2, 1, 3).reshape(s_img, dim)
                    if self.storage_dtype == torch.bfloat16:
                        ops.euler_step(Xi, o, float(sc), out=Xi)      # x + scale x o in f32, one rounding
                    else:
                        Xi.add_(o, alpha=float(sc))                    # float-storage verification mode
            if cn_d is not None:
                ops.add(Xi, cn_d[i], out=Xi)

        for i, blk in enumerate(self.single_transformer_blocks):
            if nblk == 1:
                join_mod()
            nblk += 1
            a = blk.attn
            Qp, Kp, VT = qkv_s
            ms = lambda j: self._mod(MOD, ("s", i), j)  # noqa: E731  (shift, scale, gate)
            kind = (False if fp8_s else None) if not lora_live else fp8_kind(
                [XN, XN], [blk._wqkv, rec(blk.proj_mlp.weight)], [QKV, CAT[:, dim:]], ["bias", "gelu"])
            fuse8_s = kind is not None and self.fuse_qkv
            qn = self._norm_rows(X, XN, both, [blk._wqkv, blk.proj_mlp.weight] if kind is not None else [], ["bias", "gelu"], ms(1), ms(0),
                                 fp4=f4_sin)
            if overlap:
                # experiment (APEX_FLUX_OVERLAP=1): the MLP-up GEMM on the side stream underneath q/k prepare +
                # attention, whose 1.69-round launch leaves 80 CUs idle in its second round
                main = torch.cuda.current_stream()
                ev = torch.cuda.Event()
                ev.record(main)
                with torch.cuda.stream(self._side):
                    self._side.wait_event(ev)
                    ops.gemm(XN, blk.proj_mlp.weight, blk.proj_mlp.bias, out=CAT[:, dim:], epilogue="gelu")
                    mlp_done = torch.cuda.Event()
                    mlp_done.record(self._side)
                ops.gemm(XN, blk._wqkv, blk._bqkv, out=QKV)
            elif f4_sin and self.fuse_qkv:
                qa, sa = self._rows_fp4(XN, qn)
                ops.gemm_mxfp4_grouped_qkv([qa, qa], [sa, sa], [blk._wqkv._fp4, blk.proj_mlp.weight._fp4], [blk._bqkv, blk.proj_mlp.bias],
                                           [None, CAT[:, dim:]], ["bias", "gelu"], [1, 0], [a.norm_q.weight, None],
                                           [a.norm_k.weight, None], [0, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0],
                                           **({"out_mx_list": cat_mx} if mx4_s else {}))
            elif fuse8_s:
                # with adapters: QKV and MLP-up read the same rows, so their two skinny problems share one launch
                lt, lb = self._lora_t([XN, XN], [blk._wqkv, rec(blk.proj_mlp.weight)]) if kind else (None, None)
                qa, sa = self._rows_fp8(XN, qn)
                ops.gemm_fp8_grouped_qkv([qa, qa], [sa, sa], [blk._wqkv, rec(blk.proj_mlp.weight)], [blk._bqkv, blk.proj_mlp.bias],
                                         [None, CAT[:, dim:]], ["bias", "gelu"], [1, 0], [a.norm_q.weight, None],
                                         [a.norm_k.weight, None], [0, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0],
                                         lora_t_list=lt, lora_B_list=lb)
            elif fuse_s:
                ops.gemm_grouped_qkv([XN, XN], [blk._wqkv, blk.proj_mlp.weight], [blk._bqkv, blk.proj_mlp.bias],
                                     [None, CAT[:, dim:]], ["bias", "gelu"], [1, 0], [a.norm_q.weight, None],
                                     [a.norm_k.weight, None], [0, 0], H, 1e-6, rope, Qp[0], Kp[0], VT[0])
            else:
                # QKV and MLP-up read the same XN: one launch, 1512 tiles = 5.9 rounds of the 256 CUs
                self._grouped(XN, both, [blk._wqkv, blk.proj_mlp.weight], [blk._bqkv, blk.proj_mlp.bias], [QKV, CAT[:, dim:]],
                              ["bias", "gelu"], quantised=qn, fp4=f4_sin, out_mx_list=cat_mx if mx4_s else None)
            if overlap or not (fuse_s or fuse8_s or (f4_sin and self.fuse_qkv)):
                ops.qkv_prepare(q_in, k_in, v_in, H, Qp[0], Kp[0], VT[0], wq=a.norm_q.weight,
                                wk=a.norm_k.weight, split=0, eps=1e-6, rope=rope,
                                rope_mode=_l.ROPE_INTERLEAVED)
            ops.attention_prepared(Qp, Kp, VT, att_v, S)
            if overlap:
                torch.cuda.current_stream().wait_event(mlp_done)
            po = rec(blk.proj_out.weight)
            if lora_live and getattr(po, "lora_A", None) is not None:
                # the single-problem route with the adapter tail: t from the same kind of workspace as the grouped launches
                if not ops.fp8_grouped_lora_route([CAT], [po], [X], "gate_res"):
                    raise _l.ApexMIError("flux.mi355: the single block's proj_out carries run-time LoRA factors and its launch cannot "
                                         "take the fp8 route (bf16 storage and the bf16 residual stream are required)")
                lt, lb = self._lora_t([CAT], [po])
                qa, sa = self._rows_fp8(CAT, None)
                ops.gemm_fp8(qa, sa, po, blk.proj_out.bias, out=X, epilogue="gate_res", gate=ms(2), residual=X, lora_t=lt[0],
                             lora_B=lb[0])
            elif mx4_s:
                # the MLP columns of the codes came from the MLP-up epilogue: quantise the attention columns only
                ops.quant_blocks_mxfp4(CAT[:, :dim], out=ws.CATQ[:, :dim // 2], scale_out=ws.CATS[:, :dim // 32])
                ops.gemm(CAT, blk.proj_out.weight, blk.proj_out.bias, out=X, epilogue="gate_res", gate=ms(2), residual=X,
                         quantised_mxfp4=(ws.CATQ, ws.CATS))
            else:
                ops.gemm(CAT, blk.proj_out.weight, blk.proj_out.bias, out=X, epilogue="gate_res", gate=ms(2),
                         residual=X)
            if cn_s is not None:
                ops.add(Xi, cn_s[i], out=Xi)

        join_mod()
        # AdaLayerNormContinuous: scale first, then shift
        ops.ln_modulate(Xi, self._mod(MOD, ("out",), 0), self._mod(MOD, ("out",), 1), out=XNi)
        out = torch.empty(s_img, self.proj_out.out_features, device=X.device, dtype=self.storage_dtype)
        ops.gemm(XNi, self.proj_out.weight, self.proj_out.bias, out=out)
        return out

    # ---- IP-adapter (optional; off in every BASELINE config) ---------------------------------------------------------------
    @torch.no_grad()
    def load_ip_adapter_weights(self, state_dicts, scale=1.0):
        """diffusers `FluxTransformer2DLoadersMixin._load_ip_adapter_weights(state_dicts)` for already-converted adapter files:
        each state dict = {"image_proj": {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}, "ip_adapter": {"<block>.to_k_ip.
        weight", "<block>.to_k_ip.bias", "<block>.to_v_ip.weight", "<block>.to_v_ip.bias"}} (block = double-block index).  Builds
        `encoder_hid_proj` and one `attn.processor` per double block; several adapters stack (one projection + one k / v pair each)."""
        if not isinstance(state_dicts, (list, tuple)):
            state_dicts = [state_dicts]
        kw = dict(device=self.device, dtype=self.dtype)
        dim, ctx = self.inner_dim, self.config.joint_attention_dim
        layers, tokens = [], []
        for sd in state_dicts:
            pw = sd["image_proj"]["proj.weight"]
            n_tok = pw.shape[0] // ctx
            lay = _ImageProjection(pw.shape[1], ctx, n_tok, **kw)
            lay.image_embeds.weight.data.copy_(pw)
            lay.image_embeds.bias.data.copy_(sd["image_proj"]["proj.bias"])
            lay.norm.weight.data.copy_(sd["image_proj"]["norm.weight"])
            lay.norm.bias.data.copy_(sd["image_proj"]["norm.bias"])
            layers.append(lay)
            tokens.append(n_tok)
        self.encoder_hid_proj = _MultiIPAdapterImageProjection(layers)
        for i, blk in enumerate(self.transformer_blocks):
            proc = _IPAdapterProcessor(dim, ctx, tokens, scale, **kw)
            for j, sd in enumerate(state_dicts):
                for name in ("to_k_ip", "to_v_ip"):
                    lin = getattr(proc, name)[j]
                    lin.weight.data.copy_(sd["ip_adapter"][f"{i}.{name}.weight"])
                    lin.bias.data.copy_(sd["ip_adapter"][f"{i}.{name}.bias"])
            blk.attn.processor = proc
        return self

    def set_ip_adapter(self, num_tokens=(4,), scale=1.0):
        """Empty IP-adapter processors on every double block (their weights then arrive with `load_state_dict`: keys
        `transformer_blocks.N.attn.processor.to_k_ip.M.weight`, as a diffusers model with adapters saves them)."""
        kw = dict(device=self.device, dtype=self.dtype)
        for blk in self.transformer_blocks:
            blk.attn.processor = _IPAdapterProcessor(self.inner_dim, self.config.joint_attention_dim, num_tokens, scale, **kw)
        return self

    def set_ip_adapter_scale(self, scale):
        for blk in self.transformer_blocks:
            p = blk.attn.processor
            if p is not None:
                p.scale = list(scale) if isinstance(scale, (list, tuple)) else [float(scale)] * len(p.to_k_ip)
        return self

    def unload_ip_adapter(self):
        for blk in self.transformer_blocks:
            blk.attn.processor = None
        if hasattr(self, "encoder_hid_proj"):
            del self.encoder_hid_proj
        return self

    @ops.on_model_device
    @torch.no_grad()
    def forward(self, hidden_states: torch.Tensor, encoder_hidden_states: torch.Tensor = None,
                pooled_projections: torch.Tensor = None, timestep: torch.Tensor = None,
                img_ids: torch.Tensor = None, txt_ids: torch.Tensor = None,
                guidance: torch.Tensor = None, joint_attention_kwargs: Optional[Dict[str, Any]] = None,
                controlnet_block_samples=None, controlnet_single_block_samples=None,
                return_dict: bool = True, controlnet_blocks_repeat: bool = False):
        # ControlNet residuals (reference model.py:594-612, :631-640): per-block tensors [B, S_img, dim] added to the image stream
        # after the block — sample index = block // ceil(blocks / samples), or block % samples with `controlnet_blocks_repeat`
        # (double blocks only).  The ControlNet that produces them is not part of this path.
        def _cn(samples, nblocks, repeat):
            if samples is None:
                return None
            n = len(samples)
            if n == 0:
                return None
            step = -(-nblocks // n)
            idx = [(i % n if repeat else i // step) for i in range(nblocks)]
            ss = [smp.to(self.device, self.storage_dtype).contiguous() for smp in samples]
            return [ss[j] for j in idx]
        cn_d = _cn(controlnet_block_samples, len(self.transformer_blocks), controlnet_blocks_repeat)
        cn_s = _cn(controlnet_single_block_samples, len(self.single_transformer_blocks), False)
        # IP-adapter inputs (model.py:562-571): image embeddings through `encoder_hid_proj`, or the projected tokens directly
        ip = None
        if joint_attention_kwargs and ("ip_adapter_image_embeds" in joint_attention_kwargs or "ip_hidden_states" in joint_attention_kwargs):
            if any(blk.attn.processor is None for blk in self.transformer_blocks) or not len(self.transformer_blocks):
                raise _l.ApexMIError("flux.mi355: IP-adapter inputs were passed but no adapter is loaded (load_ip_adapter_weights / "
                                     "set_ip_adapter)")
            if "ip_adapter_image_embeds" in joint_attention_kwargs:
                if not hasattr(self, "encoder_hid_proj"):
                    raise _l.ApexMIError("flux.mi355: `ip_adapter_image_embeds` needs `encoder_hid_proj` (load_ip_adapter_weights)")
                emb = joint_attention_kwargs["ip_adapter_image_embeds"]
                emb = [e.to(self.device) for e in emb] if isinstance(emb, (list, tuple)) else emb.to(self.device)
                ip = self.encoder_hid_proj(emb)
            else:
                ip = list(joint_attention_kwargs["ip_hidden_states"])
            n_ad = len(self.transformer_blocks[0].attn.processor.to_k_ip)
            if len(ip) != n_ad:
                raise ValueError(f"{len(ip)} image-prompt tensors for {n_ad} IP adapters")
            ip = [t.to(self.device, self.storage_dtype) for t in ip]
        self.pack()
        self._fp4_refresh()
        if txt_ids.ndim == 3:
            txt_ids = txt_ids[0]
        if img_ids.ndim == 3:
            img_ids = img_ids[0]
        B = hidden_states.shape[0]
        hs = hidden_states.to(self.storage_dtype)
        enc = encoder_hidden_states.to(self.storage_dtype)
        def one(b):
            return self._forward_one(
                hs[b].contiguous(), enc[b].contiguous(), pooled_projections[b], timestep[b:b + 1],
                img_ids, txt_ids, None if guidance is None else guidance[b:b + 1],
                mod_row=self._sched_row(pooled_projections, joint_attention_kwargs, b, timestep[b:b + 1],
                                        None if guidance is None else guidance[b:b + 1]),
                cn_d=None if cn_d is None else [t[b] for t in cn_d], cn_s=None if cn_s is None else [t[b] for t in cn_s],
                ip=None if ip is None else [t[b if t.shape[0] > 1 else 0].contiguous() for t in ip])

        ns = min(int(self.batch_streams), B)
        if ns <= 1 or not hs.is_cuda:
            outs = [one(b) for b in range(B)]
        else:
            # The images of a batch (`num_images`, reference engine/flux/t2i.py:88) are independent and one B=1 step leaves tile-
            # quantisation gaps (216 / 648 / 864 GEMM tiles and 432 attention workgroups on 256 CUs): `batch_streams` images run
            # side by side on their own HIP streams (own workspaces, `_workspace`) and fill them — +4 % images/s measured
            # (profiles/r03_two_clips_ab.json), same kernels on the same data, bit-identical to the sequential walk.
            self._rope(txt_ids, img_ids)        # table made on the calling stream, before the side streams fork from it
            outs = ops.run_on_streams(self._bstreams, ns, B, one, hs.device)
        out = torch.stack(outs, dim=0).to(hidden_states.dtype)
        if not return_dict:
            return (out,)
        return SimpleNamespace(sample=out)
