"""CLIP vision tower on the MI355X HIP ops: a drop-in for `transformers.CLIPVisionModel`, the image encoder of the Wan-2.1 I2V /
FLF2V models (ViT-H/14: width 1280, 32 layers, 16 heads of 80, MLP 5120, exact GELU, 224 px, 257 tokens).  Wan conditions on
`hidden_states[-2]` (diffusers WanImageToVideoPipeline.encode_image).

Same state-dict keys as the checkpoints (`vision_model.embeddings.{patch_embedding, class_embedding, position_embedding}`,
`vision_model.pre_layrnorm`, `vision_model.encoder.layers.N.*`, `vision_model.post_layernorm`; a state dict without the
`vision_model.` prefix, as newer transformers versions name it, loads too), same `_from_config`, same outputs
(`last_hidden_state`, `pooler_output`, `hidden_states`).  bf16 on a ROCm device only — no CPU fallback.

Launches: the 14 x 14 patch embedding as ONE GEMM over the flattened patches (K = 3 * 14 * 14 = 588 zero-padded to 640, as
qwen2_5_vl's patch weight), class token and position embedding (`add`), pre-LN; per layer the pre-LN layer of CLIPTextModel
without the causal mask: LayerNorm, fused QKV GEMM, attention (`apexmi_attn_fwd_bias`), out-projection with the residual in the
epilogue, LayerNorm, fc1 with the activation in the epilogue, fc2 with the residual.  Heads of 80 sit in 128-wide slots (zero
rows of the QKV weight, zero columns of the out-projection: exact), as qwen2_5_vl's vision tower does.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Sequence

import torch
import torch.nn as nn

from . import lib as _l
from . import ops
from .module_base import HipEncoder, _CLIPLayer, _Config, _Emb, _N, _cfg_dict

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _pad_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def clip_preprocess(images, size: int = 224, crop_size: int = 224, mean: Sequence[float] = CLIP_MEAN,
                    std: Sequence[float] = CLIP_STD) -> torch.Tensor:
    """`transformers.CLIPImageProcessor` with its defaults: RGB, PIL bicubic resize of the shortest edge to `size` (the long edge
    to int(size * long / short)), centre crop `crop_size`, x / 255, (x - mean) / std.  images: a PIL image / HWC uint8 array or
    a list of them -> pixel_values [N, 3, crop_size, crop_size] float32 (CPU)."""
    import numpy as np
    from PIL import Image
    if not isinstance(images, (list, tuple)):
        images = [images]
    out = []
    for im in images:
        im = (im if isinstance(im, Image.Image) else Image.fromarray(np.asarray(im))).convert("RGB")
        w, h = im.size
        short, long = (w, h) if w <= h else (h, w)
        ns, nl = size, int(size * long / short)
        nw, nh = (ns, nl) if w <= h else (nl, ns)
        a = np.asarray(im.resize((nw, nh), Image.Resampling.BICUBIC))
        top, left = (nh - crop_size) // 2, (nw - crop_size) // 2
        if top < 0 or left < 0:
            raise ValueError(f"clip_preprocess: resized image {nh}x{nw} is smaller than the crop {crop_size}")
        a = a[top:top + crop_size, left:left + crop_size].transpose(2, 0, 1)
        x = (a.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
        x = ((x.T - np.array(mean, dtype=np.float32)) / np.array(std, dtype=np.float32)).T
        out.append(torch.from_numpy(np.ascontiguousarray(x)))
    return torch.stack(out)


class CLIPVisionModel(HipEncoder):
    """transformers.CLIPVisionModel: patch embedding, class token, pre-LN encoder (non-causal), CLS pooling + post-LN."""

    def __init__(self, config=None, device=None, dtype=torch.bfloat16, **kwargs):
        super().__init__()
        cfg = _cfg_dict(config, kwargs)
        c = self.config = _Config(
            hidden_size=cfg.get("hidden_size", 768), intermediate_size=cfg.get("intermediate_size", 3072),
            num_hidden_layers=cfg.get("num_hidden_layers", 12), num_attention_heads=cfg.get("num_attention_heads", 12),
            num_channels=cfg.get("num_channels", 3), image_size=cfg.get("image_size", 224), patch_size=cfg.get("patch_size", 32),
            layer_norm_eps=cfg.get("layer_norm_eps", 1e-5), hidden_act=cfg.get("hidden_act", "quick_gelu"))
        if c.hidden_act not in ("quick_gelu", "gelu"):
            raise NotImplementedError(f"clip vision (mi355): hidden_act={c.hidden_act!r}")
        if c.hidden_size % 64 or c.hidden_size % c.num_attention_heads:
            raise NotImplementedError(f"clip vision (mi355): hidden_size={c.hidden_size} must be a multiple of 64 and of the head count")
        kw = dict(device=device, dtype=dtype)
        d = c.hidden_size
        vm = self.vision_model = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.empty(d, **kw), requires_grad=False)
        vm.embeddings.patch_embedding = nn.Module()     # Conv2d(C, d, P, stride P, bias=False)
        vm.embeddings.patch_embedding.weight = nn.Parameter(torch.empty(d, c.num_channels, c.patch_size, c.patch_size, **kw),
                                                            requires_grad=False)
        vm.embeddings.position_embedding = _Emb((c.image_size // c.patch_size) ** 2 + 1, d, **kw)
        vm.pre_layrnorm = _N(d, True, **kw)
        vm.encoder = nn.Module()
        vm.encoder.layers = nn.ModuleList([_CLIPLayer(d, c.intermediate_size, **kw) for _ in range(c.num_hidden_layers)])
        vm.post_layernorm = _N(d, True, **kw)
        self._fused = {}

    def load_state_dict(self, state_dict, *a, **k):
        if state_dict and not any(key.startswith("vision_model.") for key in state_dict):
            state_dict = {"vision_model." + key: v for key, v in state_dict.items()}     # newer transformers: no prefix
        state_dict = {key: v for key, v in state_dict.items() if not key.endswith("embeddings.position_ids")}
        return super().load_state_dict(state_dict, *a, **k)

    # ---- packed weights (built once per load) ----------------------------------------------------------------------
    def _patch_weight(self):
        f = self._fused.get("patch")
        if f is None:
            w = self.vision_model.embeddings.patch_embedding.weight.data
            k = w[0].numel()
            kp = _pad_to(k, 64)
            wp = torch.zeros(w.shape[0], kp, dtype=w.dtype, device=w.device)
            wp[:, :k] = w.reshape(w.shape[0], k)
            f = (wp, k, kp)
            self._fused["patch"] = f
        return f

    def _layer_pack(self, i: int, layer: _CLIPLayer):
        """Heads in slots of a multiple of 64 (zero rows / columns), intermediate size padded to a multiple of 64 (zeros)."""
        key = ("layer", i)
        f = self._fused.get(key)
        if f is None:
            c = self.config
            d, H = c.hidden_size, c.num_attention_heads
            hd, slot = d // H, _pad_to(d // H, 64)
            at = layer.self_attn
            w = torch.stack([at.q_proj.weight.data, at.k_proj.weight.data, at.v_proj.weight.data]).view(3, H, hd, d)
            b = torch.stack([at.q_proj.bias.data, at.k_proj.bias.data, at.v_proj.bias.data]).view(3, H, hd)
            wq = w.new_zeros(3, H, slot, d)
            wq[:, :, :hd] = w
            bq = b.new_zeros(3, H, slot)
            bq[:, :, :hd] = b
            wo = w.new_zeros(d, H, slot)
            wo[:, :, :hd] = at.out_proj.weight.data.view(d, H, hd)
            inter = c.intermediate_size
            ip = _pad_to(inter, 64)
            w1 = layer.mlp.fc1.weight.data.new_zeros(ip, d)
            w1[:inter] = layer.mlp.fc1.weight.data
            b1 = layer.mlp.fc1.bias.data.new_zeros(ip)
            b1[:inter] = layer.mlp.fc1.bias.data
            w2 = layer.mlp.fc2.weight.data.new_zeros(d, ip)
            w2[:, :inter] = layer.mlp.fc2.weight.data
            f = dict(slot=slot, wqkv=wq.reshape(3 * H * slot, d).contiguous(), bqkv=bq.reshape(-1).contiguous(),
                     wo=wo.reshape(d, H * slot).contiguous(), w1=w1, b1=b1, w2=w2)
            self._fused[key] = f
        return f

    @ops.on_model_device
    @torch.no_grad()
    def forward(self, pixel_values=None, output_hidden_states=False, return_dict=True, **_):
        c, vm = self.config, self.vision_model
        if self.device.type != "cuda" or self.dtype != torch.bfloat16:
            raise _l.ApexMIError("CLIPVisionModel (mi355) needs bf16 weights on a ROCm device (no CPU fallback)")
        P, C = c.patch_size, c.num_channels
        if pixel_values is None or pixel_values.dim() != 4 or pixel_values.shape[1] != C \
                or tuple(pixel_values.shape[-2:]) != (c.image_size, c.image_size):
            raise ValueError(f"pixel_values must be [B, {C}, {c.image_size}, {c.image_size}], got "
                             f"{None if pixel_values is None else tuple(pixel_values.shape)}")
        B, g = pixel_values.shape[0], c.image_size // P
        S, d, H, eps = g * g + 1, c.hidden_size, c.num_attention_heads, c.layer_norm_eps
        dev, st = self.device, self.storage_dtype
        if st != torch.bfloat16:
            raise NotImplementedError("CLIPVisionModel (mi355): bfloat16 activation storage only")

        # patch embedding: flattened (channel, row, column) patches as one GEMM, K zero-padded to a multiple of 64
        wp, k, kp = self._patch_weight()
        px = torch.zeros(B * g * g, kp, dtype=st, device=dev)
        px[:, :k] = pixel_values.to(dev, st).reshape(B, C, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, k)
        emb = torch.empty(B, S, d, dtype=st, device=dev)
        emb[:, 0] = vm.embeddings.class_embedding.data
        emb[:, 1:] = ops.gemm(px, wp).view(B, g * g, d)
        pos = vm.embeddings.position_embedding.weight.data
        for b in range(B):
            ops.add(emb[b], pos, out=emb[b])
        x = ops.ln_modulate(emb.view(B * S, d), gamma=vm.pre_layrnorm.weight.data, beta=vm.pre_layrnorm.bias.data, eps=eps)

        ones = self._ones(d)
        act = "quick_gelu" if c.hidden_act == "quick_gelu" else "gelu_erf"
        hidden: List[torch.Tensor] = [x.view(B, S, d)] if output_hidden_states else []
        for i, layer in enumerate(vm.encoder.layers):
            p = self._layer_pack(i, layer)
            inner = H * p["slot"]
            h = ops.ln_modulate(x, gamma=layer.layer_norm1.weight.data, beta=layer.layer_norm1.bias.data, eps=eps)
            qkv = ops.gemm(h, p["wqkv"], p["bqkv"])
            a = torch.empty((B * S, inner), dtype=st, device=dev)
            for b in range(B):
                r = slice(b * S, (b + 1) * S)
                ops.attention_bias(qkv[r, :inner], qkv[r, inner:2 * inner], qkv[r, 2 * inner:], H, (d // H) ** -0.5, out=a[r])
            x = ops.gemm(a, p["wo"], layer.self_attn.out_proj.bias.data, epilogue="gate_res", gate=ones, residual=x)
            h = ops.ln_modulate(x, gamma=layer.layer_norm2.weight.data, beta=layer.layer_norm2.bias.data, eps=eps)
            h = ops.gemm(h, p["w1"], p["b1"], epilogue=act)
            x = ops.gemm(h, p["w2"], layer.mlp.fc2.bias.data, epilogue="gate_res", gate=ones, residual=x)
            if output_hidden_states:
                hidden.append(x.view(B, S, d))
        last = x.view(B, S, d)
        pooled = ops.ln_modulate(last[:, 0].contiguous(), gamma=vm.post_layernorm.weight.data,
                                 beta=vm.post_layernorm.bias.data, eps=eps)
        out = SimpleNamespace(last_hidden_state=last, pooler_output=pooled,
                              hidden_states=tuple(hidden) if output_hidden_states else None)
        return out if return_dict else (last, pooled) + ((out.hidden_states,) if output_hidden_states else ())
