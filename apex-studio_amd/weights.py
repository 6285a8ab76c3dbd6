"""Checkpoint shards -> the packed device layout, without a host-side state dict.

The reference loads every weight file into a full state dict, runs the key converter, optionally patches the
model with FP-scaled layers that dequantise `weight * scale_weight` on EVERY forward, and calls
`model.load_state_dict(sd, strict=False, assign=True)` per file (`R/src/mixins/loader_mixin.py:439-531`;
`R/src/quantize/scaled_layer.py:496-549`, `fp8_activation_dequant` :154-167).

Here tensors are streamed one at a time out of the safetensors shards (`safe_open`, lazy) straight into the model's
parameters on the GPU — which, once `model.pack()` has run, are views of the fused QKV / modulation matrices, so
the "fused/tiled device layout" is written exactly once.  FP8-scaled pairs (`<m>.weight` in float8_e4m3fn / e5m2
plus `<m>.scale_weight`) are dequantised once at load by `apexmi_dequant_fp8_scaled` into the same bf16 values the
reference recomputes per forward, so the denoise kernels are unchanged.

GGUF files (`*.gguf`; the reference's `load_gguf`, R/src/quantize/load.py:364) are read by `gguf_file` — a memory map, no
`gguf` package: F32 / F16 / BF16 tensors are copied like any other, quantised tensors (Q4_0 ... Q6_K) are uploaded as their raw
block bytes and expanded ON THE GPU by `apexmi_dequant_gguf` straight into the bf16 parameter, or — `keep_quantized=True`, the
block Linears of `wan.mi355` — stay as blocks in HBM (`ops.GgufWeight`) and are expanded per call as `GGMLLinear` does.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import torch

FP8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)


def iter_checkpoint(files: Sequence[str], converter=None, key_map: Optional[Dict[str, str]] = None,
                    model_keys: Optional[Sequence[str]] = None) -> Iterator[Tuple[str, Callable[[], torch.Tensor]]]:
    """(key, loader) for every tensor of every shard; `loader()` reads that one tensor to the host.

    With a `converter` (converters.get_transformer_converter: original-format Wan / BFL-Flux files), every file's keys go
    through `key_map` and the converter FIRST, as the reference does per weight file (loader_mixin.py:462-473) — but on
    placeholders: no tensor is read to decide the plan, and a target that is a row range of a fused tensor (q / k / v of
    `img_attn.qkv.weight`, the four parts of `linear1`) is read with safetensors' `get_slice`."""
    from .converters import Src
    for path in files:
        if path.endswith(".safetensors"):
            from safetensors import safe_open
            f = safe_open(path, framework="pt", device="cpu")
            if converter is None:
                for k in f.keys():
                    yield remap_key(k, key_map), (lambda f=f, k=k: f.get_tensor(k))
                continue
            plan = {remap_key(k, key_map): Src(k, tuple(f.get_slice(k).get_shape())) for k in f.keys()}
            get, rows = f.get_tensor, (lambda k, a, b, f=f: f.get_slice(k)[a:b])
        elif path.endswith(".gguf"):
            # loaders return a torch tensor (F32 / F16 / BF16) or a gguf_file.Quantized (block bytes); a row range of a fused
            # quantised tensor is a byte range of it — blocks run along K
            from .gguf_file import GGUFReader
            g = GGUFReader(path)
            if converter is None:
                for k, t in g.tensors.items():
                    yield remap_key(k, key_map), t.read
                continue
            plan = {remap_key(k, key_map): Src(k, t.shape) for k, t in g.tensors.items()}
            get, rows = (lambda k, g=g: g[k].read()), (lambda k, a, b, g=g: g[k].read(a, b))
        else:
            sd = torch.load(path, map_location="cpu", weights_only=True, mmap=True)
            if converter is None:
                for k, v in sd.items():
                    yield remap_key(k, key_map), (lambda v=v: v)
                continue
            plan = {remap_key(k, key_map): Src(k, tuple(v.shape)) for k, v in sd.items()}
            get, rows = sd.__getitem__, None
        converter.convert(plan, list(model_keys) if model_keys is not None else None)
        for k, src in plan.items():
            yield k, (lambda src=src, get=get, rows=rows: _read_src(src, get, rows))


def _read_src(src, get, rows):
    """`src.read`, with the half swap of a quantised GGUF tensor done on its row segments (it is not a torch tensor)."""
    if not src.swap:
        return src.read(get, rows)
    from dataclasses import replace
    t = replace(src, swap=False).read(get, rows)
    if hasattr(t, "swap_halves"):
        return t.swap_halves()
    a, b = t.chunk(2, dim=0)
    return torch.cat([b, a], dim=0)


def remap_key(key: str, key_map: Optional[Dict[str, str]]) -> str:
    """`key_map` semantics of the reference loader (loader_mixin.py:462-471): replace a substring."""
    if key_map:
        for src, dst in key_map.items():
            if src in key:
                key = key.replace(src, dst)
    return key


@torch.no_grad()
def load_checkpoint_into(model: torch.nn.Module, files: Sequence[str], key_map: Optional[Dict[str, str]] = None,
                         strict: bool = False, converter="auto", keep_fp8: bool = False,
                         keep_quantized: bool = False) -> Tuple[List[str], List[str]]:
    """Stream `files` into `model` (already on the GPU, bf16).  Returns (missing_keys, unexpected_keys) like
    `load_state_dict(strict=False)`; `strict=True` raises on either.  Shapes must match exactly, except that a
    0-d / 1-element `scale_weight` may pair with any weight (scaled_layer.py:444-493).

    `converter`: the checkpoint key converter the files go through per file, as the reference's loader does
    (loader_mixin.py:473 `converter.convert(state_dict, model_keys)`): "auto" = the table of the model's family
    (`model._converter_base`; original-format Wan / BFL-Flux files are renamed and split on the fly, diffusers-keyed files
    pass through the converter's own already-converted test), None = keys are taken as they are, or a converters.KeyConverter.

    `keep_fp8`: fp8-scaled weights the model can hold RESIDENT (`model._fp8_resident_key(key)`: the block Linears of
    `wan.mi355` and `flux.mi355`) stay float8 + scale in HBM — `ops.Fp8Weight`, dequantised per call as the reference's
    FPScaledLinear does (scaled_layer.py:390-552) — instead of being dequantised once into the bf16 parameter; the parameter's bf16 storage is
    released (`model._fp8_adopt()`).  Forwards are bit-identical to the dequantise-at-load path; half the weight bytes.

    `keep_quantized`: the same for GGUF files — quantised tensors of those weights stay ggml blocks in HBM (`ops.GgufWeight`,
    dequantised per call as the reference's GGMLLinear does, ggml_layer.py:220); 0.56 (Q4_K) to 1.06 (Q8_0) bytes a weight."""
    from . import ops
    from .gguf_file import Quantized
    resident = getattr(model, "_fp8_resident_key", None) if keep_fp8 or keep_quantized else None
    if (keep_fp8 or keep_quantized) and resident is None:
        raise NotImplementedError(f"{type(model).__name__} has no resident quantised weight mode "
                                  f"({'keep_fp8' if keep_fp8 else 'keep_quantized'}=True): wan.mi355 has")
    if keep_quantized and "gguf" not in getattr(model, "_fp8_formats", ("fp8", "gguf")):
        raise NotImplementedError(f"{type(model).__name__} has no resident quantised weight mode (keep_quantized=True): wan.mi355 has")
    targets: Dict[str, torch.Tensor] = dict(model.named_parameters())
    targets.update({k: v for k, v in model.named_buffers() if k not in targets})
    if any(not t.is_cuda for t in targets.values()):
        raise RuntimeError("load_checkpoint_into: move the model to the GPU first (there is no CPU path)")
    if converter == "auto":
        from .converters import NoOpKeyConverter, get_transformer_converter
        converter = get_transformer_converter(getattr(model, "_converter_base", ""))
        if isinstance(converter, NoOpKeyConverter):
            converter = None
    entries = list(iter_checkpoint(files, converter, key_map, list(targets)))
    if resident is not None and hasattr(model, "_fp8_preflight"):
        model._fp8_preflight([k for k, _ in entries])      # a file the resident mode cannot take is refused before anything is written
    scales = {k[:-len("scale_weight")]: ld for k, ld in entries if k.endswith("scale_weight")}
    seen, unexpected = set(), []
    for key, ld in entries:
        if key.endswith("scale_weight"):
            if key[:-len("scale_weight")] + "weight" not in targets:
                unexpected.append(key)
            continue
        if key not in targets:
            unexpected.append(key)
            continue
        dst = targets[key]
        src = ld()
        if isinstance(src, Quantized):
            # GGUF blocks: uploaded as bytes, expanded on the GPU (files flatten > 4-D tensors: rows and element count must agree)
            if src.shape[0] != dst.shape[0] or src.numel() != dst.numel():
                raise ValueError(f"{key}: GGUF tensor of shape {src.shape} does not fill the parameter of shape {tuple(dst.shape)}")
            if dst.dtype != torch.bfloat16:
                raise TypeError(f"{key}: quantised GGUF weights load into bf16 parameters, not {dst.dtype}")
            segs = [(t, n, torch.from_numpy(b).to(dst.device, non_blocking=True)) for t, n, b in src.segments]
            K = dst.numel() // dst.shape[0]
            if keep_quantized and dst.dim() == 2 and resident(key):
                dst._fp8 = ops.GgufWeight(segs, K)                       # adopted after the loop (model._fp8_adopt)
            else:
                out2d, r0 = dst.data.view(dst.shape[0], K), 0
                for t, n, b in segs:
                    ops.dequant_gguf(b, t, (n, K), out=out2d[r0:r0 + n])
                    r0 += n
            seen.add(key)
            continue
        if tuple(src.shape) != tuple(dst.shape):
            raise ValueError(f"{key}: checkpoint shape {tuple(src.shape)} != parameter shape {tuple(dst.shape)}")
        prefix = key[:-len("weight")] if key.endswith("weight") else None
        if src.dtype in FP8_DTYPES:
            if prefix is None or prefix not in scales:
                raise ValueError(f"{key}: fp8 tensor without a '{(prefix or key)}scale_weight' partner")
            if dst.dtype != torch.bfloat16:
                raise TypeError(f"{key}: fp8-scaled weights load into bf16 parameters, not {dst.dtype}")
            q = src.view(torch.uint8).to(dst.device, non_blocking=True).view(src.dtype)
            if resident is not None and dst.dim() == 2 and resident(key):
                dst._fp8 = ops.Fp8Weight(q, scales[prefix]())            # adopted after the loop (model._fp8_adopt)
            else:
                out2d = dst.data.view(dst.shape[0], -1) if dst.dim() != 2 else dst.data
                ops.dequant_fp8_scaled(q, scales[prefix](), out=out2d)
        else:
            if prefix is not None and prefix in scales:
                # the reference raises here too (`physical_dtype in (torch.uint8)`, scaled_layer.py:525)
                raise TypeError(f"{key}: '{prefix}scale_weight' is present but the weight is {src.dtype}, not fp8")
            dst.data.copy_(src.to(dst.device, non_blocking=True))
        seen.add(key)
    # derived state (f32 modulation tables, padded patch-embed operand, packed conv weights) follows the new values
    for m in model.modules():
        hook = getattr(m, "_weights_changed", None)
        if callable(hook):
            hook()
    if resident is not None:
        model._fp8_adopt()
    missing = [k for k in targets if k not in seen]
    if strict and (missing or unexpected):
        raise RuntimeError(f"load_checkpoint_into: missing {missing[:8]}{'...' if len(missing) > 8 else ''}, "
                           f"unexpected {unexpected[:8]}{'...' if len(unexpected) > 8 else ''}")
    return missing, unexpected
