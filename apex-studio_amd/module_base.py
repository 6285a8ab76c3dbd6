"""What every HIP model wrapper shares: the small parameter holders, the reference-compatible plumbing (`from_config`,
`dtype` / `device`, `set_storage_dtype`), ONE rule for which event drops which derived cache, the encoders' fused-weight
cache, and — for the four DiT transformers — the packing helpers, the split modulation GEMV and the synthetic-weight fill.

Nothing here adds a parameter, a buffer or a submodule: state-dict keys are those of the classes that derive from these.
"""
from __future__ import annotations

import contextlib
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import lib as _l
from . import ops
from .lora import LoraAdapterMixin


class _Config(SimpleNamespace):
    def get(self, key, default=None):
        return getattr(self, key, default)

    def __getitem__(self, key):
        return getattr(self, key)

    def __contains__(self, key):
        return hasattr(self, key)


class _Linear(nn.Module):
    """Parameter holder with nn.Linear's names/shapes (weight [out,in], bias [out])."""

    def __init__(self, in_features: int, out_features: int, device=None, dtype=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features, device=device, dtype=dtype),
                                   requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_features, device=device, dtype=dtype), requires_grad=False)


class _Norm(nn.Module):
    def __init__(self, dim: int, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, device=device, dtype=dtype), requires_grad=False)


class _AdaNorm(nn.Module):
    def __init__(self, dim: int, mult: int, cond_dim: Optional[int] = None, **kw):
        super().__init__()
        self.linear = _Linear(cond_dim or dim, mult * dim, **kw)


class _FF(nn.Module):
    def __init__(self, dim: int, inner: int, **kw):
        super().__init__()
        proj = nn.Module()
        proj.proj = _Linear(dim, inner, **kw)
        self.net = nn.ModuleList([proj, nn.Identity(), _Linear(inner, dim, **kw)])


class _TimestepEmbedding(nn.Module):
    def __init__(self, in_dim: int, dim: int, **kw):
        super().__init__()
        self.linear_1 = _Linear(in_dim, dim, **kw)
        self.linear_2 = _Linear(dim, dim, **kw)


class _JointAttn(nn.Module):
    """Attention parameters of an MM-DiT double-stream block (QwenImage, HunyuanVideo-1.5): q/k/v + out projections and per-head
    RMSNorm weights for the image stream and for the text stream (`add_*`, `norm_added_*`, `to_add_out`)."""

    def __init__(self, dim: int, heads: int, head_dim: int, **kw):
        super().__init__()
        inner = heads * head_dim
        self.heads = heads
        self.to_q, self.to_k, self.to_v = _Linear(dim, inner, **kw), _Linear(dim, inner, **kw), _Linear(dim, inner, **kw)
        self.add_q_proj, self.add_k_proj, self.add_v_proj = (_Linear(dim, inner, **kw), _Linear(dim, inner, **kw),
                                                             _Linear(dim, inner, **kw))
        self.norm_q, self.norm_k = _Norm(head_dim, **kw), _Norm(head_dim, **kw)
        self.norm_added_q, self.norm_added_k = _Norm(head_dim, **kw), _Norm(head_dim, **kw)
        self.to_out = nn.ModuleList([_Linear(inner, dim, **kw), nn.Identity()])
        self.to_add_out = _Linear(inner, dim, **kw)


class _Conv(nn.Module):
    """Parameter holder of a 2-D / 3-D convolution of the VAEs (weight [out, in, *ksize], bias [out])."""

    def __init__(self, cin, cout, ksize, **kw):
        super().__init__()
        self.ksize = tuple(ksize)
        self.weight = nn.Parameter(torch.empty(cout, cin, *ksize, **kw), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(cout, **kw), requires_grad=False)


def _repoint(params, packed_rows):
    """Copy each parameter into its slice of `packed_rows` and make the parameter a view of it."""
    r = 0
    for p in params:
        n = p.shape[0]
        dst = packed_rows[r:r + n]
        dst.copy_(p.data)
        p.data = dst
        r += n
    assert r == packed_rows.shape[0]


def _fuse_linears(linears):
    """One packed weight [sum of out, in] and bias [sum of out] for `linears` (fused QKV / KV projections, the stacked AdaLN
    table): the original nn.Parameters are re-pointed at views of the packed storage, so state_dict() / load_state_dict keep
    working and memory is not doubled."""
    w0 = linears[0].weight
    rows = sum(lin.weight.shape[0] for lin in linears)
    w = torch.empty(rows, w0.shape[1], device=w0.device, dtype=w0.dtype)
    b = torch.empty(rows, device=w0.device, dtype=w0.dtype)
    _repoint([lin.weight for lin in linears], w)
    _repoint([lin.bias for lin in linears], b)
    return w, b


class HipModule(nn.Module):
    """Base of every HIP model wrapper (transformers, VAEs, text / vision encoders, TAEHV).

    A class names the parameter that stands for the module's `dtype` / `device` (`_anchor`) and states ONCE, in `_drops`,
    which derived caches each event drops:
      "moved"   `_apply`: `.to()`, `.cuda()`, `.bfloat16()` — storage of every parameter may be new
      "loaded"  `load_state_dict`
      "written" `_weights_changed`: parameters were written in place (`weights.load_checkpoint_into`, render_queue broadcast)
      "storage" `set_storage_dtype` (and `set_residual_dtype`): the activation buffers change type
    """

    storage_dtype = torch.bfloat16
    _drops: dict = {}

    @classmethod
    def from_config(cls, config, **kwargs):
        cfg = dict(config) if isinstance(config, dict) else dict(vars(config))
        cfg = {k: v for k, v in cfg.items() if not k.startswith("_")}
        cfg.update(kwargs)
        return cls(**cfg)

    @classmethod
    def _from_config(cls, config, **kwargs):      # the name LoaderMixin._load_model calls
        return cls.from_config(config, **kwargs)

    def _anchor(self) -> torch.Tensor:
        return next(self.parameters())

    @property
    def dtype(self):
        return self._anchor().dtype

    @property
    def device(self):
        return self._anchor().device

    def _invalidate(self, event: str):
        for name in self._drops.get(event, ()):
            setattr(self, name, type(getattr(self, name))())      # {} for a cache dict, False for the `_packed` flag

    def _apply(self, fn, *a, **k):
        self._invalidate("moved")
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._invalidate("loaded")
        return super().load_state_dict(*a, **k)

    def _weights_changed(self):
        self._invalidate("written")

    def set_storage_dtype(self, dtype: torch.dtype):
        """torch.bfloat16 (production) or torch.float32: the f32-STORAGE VERIFICATION MODE — the same
        kernel sequence with every activation buffer float and the library's `_f32` entry points, which is what
        north_star's "within 1e-3 of the CPU fp32 reference" is tested with.  Weights stay bf16."""
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"activation storage must be bfloat16 or float32, got {dtype}")
        self.storage_dtype = dtype
        self._invalidate("storage")
        return self


MID_ATTENTION_MODES = ("materialised", "flash")


class MidAttentionMixin:
    """The VAEs' choice of kernel for the one-head mid-block attention (C = 384 / 512 / ...): "materialised" (default: the calls
    made before the setting existed, to the bit) or "flash" (`ops.attention_wide`: one launch, no O(S^2) workspace, the flash
    kernels' rounding — DESIGN.md §3.4.3).  A per-object setting, not a process-global knob.  key_splits (with "flash" only: an
    int 1 .. 8 or "auto") is ops.attention_wide's: a launch split over keys for mid blocks too short to fill the device."""

    mid_attention = "materialised"
    mid_attention_key_splits = 1

    def _mid_attention_widths(self) -> tuple:      # channels of every mid block this object runs (encoder, decoder)
        raise NotImplementedError

    def set_mid_attention(self, mode: str, key_splits=1):
        if mode not in MID_ATTENTION_MODES:
            raise ValueError(f"mid_attention must be one of {MID_ATTENTION_MODES}, got {mode!r}")
        if key_splits != "auto" and (isinstance(key_splits, (bool, str)) or not isinstance(key_splits, int) or not 1 <= key_splits <= 8):
            raise ValueError(f"key_splits must be an int 1 to 8 or \"auto\", got {key_splits!r}")
        if mode != "flash" and key_splits != 1:
            raise ValueError(f"key_splits={key_splits!r} belongs to mid_attention='flash' (ops.attention_wide); the "
                             f"'{mode}' path has no key splits")
        if mode == "flash":
            if self.storage_dtype != torch.bfloat16:
                raise NotImplementedError("the f32-storage verification mode has no flash mid-block attention; keep "
                                          "set_mid_attention('materialised') or set_storage_dtype(torch.bfloat16)")
            widths = tuple(self._mid_attention_widths())
            if any(w not in (256, 384, 512) for w in widths):
                raise ValueError(f"mid_attention='flash' covers mid blocks of 256, 384 or 512 channels (ops.attention_wide); this "
                                 f"model's are {widths} wide and stay on the materialised path: only 'materialised' is accepted")
        self.mid_attention = mode
        self.mid_attention_key_splits = key_splits
        return self

    def _flash_mid(self, x: torch.Tensor) -> bool:
        """True when this call goes through ops.attention_wide; the verification mode set after the mode raises here."""
        if self.mid_attention != "flash":
            return False
        if x.dtype != torch.bfloat16:
            raise NotImplementedError("the f32-storage verification mode has no flash mid-block attention; "
                                      "set_mid_attention('materialised')")
        return True


# ---- the text / vision encoders --------------------------------------------------------------------------------------

def _cfg_dict(config, kwargs) -> dict:
    if config is None:
        cfg = {}
    elif isinstance(config, dict):
        cfg = dict(config)
    elif hasattr(config, "to_dict"):
        cfg = dict(config.to_dict())
    else:
        cfg = dict(vars(config))
    cfg.update(kwargs)
    return cfg


class _W(nn.Module):
    def __init__(self, cout, cin, bias, **kw):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, **kw), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.empty(cout, **kw), requires_grad=False)
        else:
            self.bias = None


class _N(nn.Module):
    def __init__(self, dim, bias, **kw):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, **kw), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(dim, **kw), requires_grad=False)


class _Emb(nn.Module):
    def __init__(self, n, dim, **kw):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, dim, **kw), requires_grad=False)


class HipEncoder(HipModule):
    """Common surface of the encoders: fused-weight cache invalidation, the no-CPU-fallback check.  `set_storage_dtype(float32)` is
    their verification mode: every activation between the kernels in f32 (GEMMs through the exact bf16 split, attention through
    the f32 row kernel) so the bf16-weight encoder can be compared with the fp32 reference at ~1e-6 per element instead of the
    bf16 rounding floor.  Not a production path.  `dtype` / `device` are those of the first parameter."""
    _drops = {"moved": ("_fused",), "loaded": ("_fused",), "written": ("_fused",)}      # the fused / padded weight copies

    @classmethod
    def from_config(cls, config=None, **kwargs):      # transformers' convention: the config object is the first argument
        return cls(config, **kwargs)

    def _check(self, input_ids):
        if self.device.type != "cuda" or self.dtype != torch.bfloat16:
            raise _l.ApexMIError(f"{type(self).__name__} (mi355) needs bf16 weights on a ROCm device (no CPU fallback)")
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [batch, sequence]")

    def _qkv(self, key, mods):
        """Fused [3 inner, d] projection weight (and bias) of one attention layer, built once."""
        f = self._fused.get(key)
        if f is None:
            w = torch.cat([m.weight.data for m in mods], dim=0).contiguous()
            b = torch.cat([m.bias.data for m in mods], dim=0).contiguous() if mods[0].bias is not None else None
            f = (w, b)
            self._fused[key] = f
        return f

    def _ones(self, n):
        o = self._fused.get(("ones", n))
        if o is None:
            o = (torch.ones(n, dtype=torch.float32, device=self.device),)
            self._fused[("ones", n)] = o
        return o[0]


class _CLIPLayer(nn.Module):
    def __init__(self, d, inter, **kw):
        super().__init__()
        self.self_attn = nn.Module()
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            setattr(self.self_attn, n, _W(d, d, True, **kw))
        self.layer_norm1, self.layer_norm2 = _N(d, True, **kw), _N(d, True, **kw)
        self.mlp = nn.Module()
        self.mlp.fc1, self.mlp.fc2 = _W(inter, d, True, **kw), _W(d, inter, True, **kw)


# ---- the DiT transformers -----------------------------------------------------------------------------------------------

class HipTransformer(LoraAdapterMixin, HipModule):
    """The layer the four DiT transformers add: the reference's no-op knobs, the `pack()` guard and helpers, the split
    modulation GEMV, the synthetic-weight fill.  A class sets `_tag`, the prefix of its error messages."""

    _tag = "mi355"

    @contextlib.contextmanager
    def cache_context(self, name: str):
        yield

    def set_chunking_profile(self, *a, **k):  # memory knobs of the reference (they exist to fit 8-24 GB cards): no-ops on 288 GB
        return None

    def set_chunk_feed_forward(self, *a, **k):
        return None

    def _pack_target(self):
        """(device, dtype) of the weights `pack()` is about to fuse; raises unless they are bf16 on a ROCm device."""
        dev, dt = self.device, self.dtype
        if dev.type != "cuda" or dt != torch.bfloat16:
            raise _l.ApexMIError(f"{self._tag} needs bf16 weights on a ROCm device (got {dt} on {dev}); "
                                 "there is no CPU fallback")
        return dev, dt

    def _stack_modulation(self, linears):
        """All AdaLN modulation projections as ONE matrix (`_mod_w` [total, dim], `_mod_b`, `_mod_total`), in the order given."""
        self._mod_w, self._mod_b = _fuse_linears(linears)
        self._mod_total = self._mod_w.shape[0]

    def _modulation_gemv(self, MOD, TEMB):
        """This step's modulation vectors: silu(TEMB) through the stacked projections into MOD.  Every AdaLN projection of every
        block is one weight-streaming GEMV (6.4 GB for FLUX-dev).  Only the first block's slice (`_mod_first` rows) is needed right
        away and runs on the calling stream: the rest streams on a side HIP stream underneath the first block's MFMA-bound GEMMs.
        Returns the event to join before the second block, or None."""
        n_first = self._mod_first
        ops.gemv(self._mod_w[:n_first], TEMB, self._mod_b[:n_first], out=MOD[:, :n_first], pre_silu=True)
        mod_ready = None
        if n_first < self._mod_total:
            main = torch.cuda.current_stream()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            ev = torch.cuda.Event()
            ev.record(main)
            with torch.cuda.stream(self._side):
                self._side.wait_event(ev)
                ops.gemv(self._mod_w[n_first:], TEMB, self._mod_b[n_first:], out=MOD[:, n_first:],
                         pre_silu=True)
                mod_ready = torch.cuda.Event()
                mod_ready.record(self._side)
        return mod_ready

    @torch.no_grad()
    def _fill_synthetic(self, seed: int, std: float, ones, row_scaled=None):
        """N(0, std^2) weights, small biases (N(0, 0.01^2)), ones where `ones(name, p)` says so (norm weights), N(0, 1 / last dim)
        where `row_scaled(name, p)` does (SURVEY.md §8d synthetic inputs).  One generator on the model's device, parameters in
        `named_parameters()` order: goldens and the benchmark's weights depend on the order and sizes of these draws."""
        g = torch.Generator(device=self.device)
        g.manual_seed(seed)
        for name, p in self.named_parameters():
            if ones(name, p):
                p.data.fill_(1.0)
            elif row_scaled is not None and row_scaled(name, p):
                p.data.copy_((torch.randn(p.shape, generator=g, device=p.device) / p.shape[-1] ** 0.5).to(p.dtype))
            elif name.endswith(".bias"):
                p.data.copy_((torch.randn(p.shape, generator=g, device=p.device) * 0.01).to(p.dtype))
            else:
                # chunked to keep the f32 temporary small for the 12B-parameter model
                flat = p.data.view(-1)
                step = 1 << 26
                for i in range(0, flat.numel(), step):
                    n = min(step, flat.numel() - i)
                    flat[i:i + n] = (torch.randn(n, generator=g, device=p.device) * std).to(p.dtype)
        self._invalidate("loaded")
        return self


class F32ResidualMixin:
    """The F32 RESIDUAL STREAM mode of the Flux and Wan transformers, in front of HipTransformer in the bases."""

    residual_dtype = torch.bfloat16      # set_residual_dtype(float32): X alone in float, everything else bf16

    def set_storage_dtype(self, dtype: torch.dtype):
        if dtype == torch.float32 and self.residual_dtype == torch.float32:
            raise ValueError("a float residual stream is for bfloat16 storage: set_residual_dtype(torch.bfloat16) first")
        return super().set_storage_dtype(dtype)

    def set_residual_dtype(self, dtype: torch.dtype):
        """torch.bfloat16 (default) or torch.float32: the F32 RESIDUAL STREAM.  The residual stream X, and only
        X, is kept in float32: the embedders write it through the GEMM's float epilogue, every gated residual update reads and
        writes it in float, every norm reads float rows and writes the bf16 GEMM operand (apexmi_ln_modulate2_f32in).  All GEMM
        and attention operands, and every other buffer, stay bf16 -- the rounding of X after each of its updates is what leaves
        the bf16 chain.  Not to be combined with `set_storage_dtype(float32)`, which is all-float already."""
        if dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"the residual stream must be bfloat16 or float32, got {dtype}")
        if dtype == torch.float32 and self.storage_dtype == torch.float32:
            raise ValueError("storage_dtype=float32 already keeps every buffer in float: a float residual stream is for bfloat16 storage")
        self.residual_dtype = dtype
        self._invalidate("storage")
        return self


class _MxComputeSwitch:
    """What the switches of the two opt-in block-format compute modes share (`Fp4ComputeMixin`: MXFP4,
    `Fp6ComputeMixin`: MXFP6): name validation, the refusals, attaching / detaching the records that sit BESIDE the bf16 block weights,
    the byte count, and the two dtype guards — ONE implementation, parameterised by the mode's name `n` ("fp4" / "fp6"): the
    weight's slot is `_<n>`, the record class `_MX_RECORDS[n]`, the switch `set_<n>_compute`, the state `_<n>_linears` (the selected
    names while the mode is on, else None), `_<n>_live` (the weights that carry a record) and `_<n>_bytes`.

    Both modes take the names `_FP4_LINEARS` and find the weights through `_fp4_blocks()` (the blocks) and `_fp4_weights(blk)` ({name:
    the weight, or a tuple of weights, of that name in that block}; a name a block does not have is absent), which the class supplies.
    A Linear takes at most one of the modes: a name selected by both is refused.  The messages start with the class's `_tag`."""

    _MX_RECORDS = {"fp4": "Mxfp4Weight", "fp6": "Mxfp6Weight"}
    _FP4_LINEARS: tuple = ()

    def _fp4_blocks(self):
        raise NotImplementedError

    def _fp4_weights(self, blk) -> dict:
        raise NotImplementedError

    def _mx_switch(self, n: str, on: bool, linears=None):
        """`set_<n>_compute(on, linears)` of the class: the names are checked before anything else, so that needs no device."""
        if linears is not None:
            try:
                linears = tuple(linears)
            except TypeError as err:
                raise _l.ApexMIError(f"{self._tag}: set_{n}_compute(linears=) takes names out of {self._FP4_LINEARS}, got {linears!r}") from err
            bad = [name for name in linears if name not in self._FP4_LINEARS]
            if bad:
                raise _l.ApexMIError(f"{self._tag}: set_{n}_compute(linears=): unknown Linear name(s) {bad}; the block Linears are "
                                     f"{self._FP4_LINEARS}")
        if not on:
            if linears is not None:
                raise _l.ApexMIError(f"{self._tag}: set_{n}_compute(False) takes no `linears`: it detaches every record")
            setattr(self, f"_{n}_linears", None)
            self._mx_detach(n)
            return self
        selected = tuple(name for name in self._FP4_LINEARS if linears is None or name in linears)
        for other in self._MX_RECORDS:
            both = [name for name in selected if other != n and name in (getattr(self, f"_{other}_linears", None) or ())]
            if both:
                raise _l.ApexMIError(f"{self._tag}: set_{n}_compute(linears=): {both} multiply as {other} already (set_{other}_compute): "
                                     f"a Linear takes one of the two modes, so select disjoint names or switch {other} compute off first")
        if getattr(self, "_fp8_bytes", 0):
            raise _l.ApexMIError(f"{self._tag}: set_{n}_compute needs the bf16 block weights, and this model's are resident quantised "
                                 f"records ({self._fp8_options()} load).  The fp8_* switches need exactly such records, so the two "
                                 f"modes cannot be combined: load without those options for {n} compute")
        if self.storage_dtype != torch.bfloat16:
            raise _l.ApexMIError(f"{self._tag}: set_{n}_compute is for bfloat16 activation storage; the f32-storage verification "
                                 "mode keeps the bf16 GEMMs (set_storage_dtype(torch.bfloat16) first)")
        if self.residual_dtype != torch.bfloat16:
            raise _l.ApexMIError(f"{self._tag}: set_{n}_compute does not take the f32 residual stream: its residual GEMMs write "
                                 f"float rows, which the {n} GEMM does not (set_residual_dtype(torch.bfloat16) first)")
        self.pack()
        setattr(self, f"_{n}_linears", selected)
        self._mx_detach(n)
        self._mx_attach(n)
        return self

    def _mx_guard_storage(self, n: str, dtype: torch.dtype):
        if dtype == torch.float32 and getattr(self, f"_{n}_linears") is not None:
            raise _l.ApexMIError(f"{self._tag}: {n} compute is on and is for bfloat16 activation storage: float rows would quietly "
                                 f"return every Linear to bf16; set_{n}_compute(False) first")

    def _mx_guard_residual(self, n: str, dtype: torch.dtype):
        if dtype == torch.float32 and getattr(self, f"_{n}_linears") is not None:
            raise _l.ApexMIError(f"{self._tag}: {n} compute is on and does not take the f32 residual stream: its residual GEMMs "
                                 f"would quietly return to bf16; set_{n}_compute(False) first")

    @torch.no_grad()
    def _mx_attach(self, n: str):
        """One record per weight of the selected names of every block, on the slot `ops.gemm` reads (`weight._<n>`)."""
        record, slot, live = getattr(ops, self._MX_RECORDS[n]), f"_{n}", []
        for blk in self._fp4_blocks():
            ws = self._fp4_weights(blk)
            for name in getattr(self, f"_{n}_linears"):
                for w in ((ws[name],) if isinstance(ws.get(name), torch.Tensor) else ws.get(name, ())):
                    setattr(w, slot, record.from_bf16(w))
                    live.append(w)
        setattr(self, f"_{n}_live", live)
        setattr(self, f"_{n}_bytes", sum(getattr(w, slot).nbytes() for w in live))

    def _mx_detach(self, n: str):
        for w in getattr(self, f"_{n}_live"):
            if getattr(w, f"_{n}", None) is not None:
                delattr(w, f"_{n}")
        setattr(self, f"_{n}_live", [])
        setattr(self, f"_{n}_bytes", 0)

    def _mx_refresh(self, n: str):
        """Before a forward: the records a weight change dropped while the mode is on are rebuilt from the weights as they are now."""
        if getattr(self, f"_{n}_linears") is not None and not getattr(self, f"_{n}_live"):
            self._mx_attach(n)


class Fp4ComputeMixin(_MxComputeSwitch):
    """The switch of the opt-in MXFP4 compute mode of the Flux and Wan transformers, in front of F32ResidualMixin
    in the bases: name validation, the refusals, attaching / detaching the `ops.Mxfp4Weight` records that sit BESIDE the bf16 block
    weights (on each weight's `_fp4` slot), `_fp4_bytes`, and the two dtype guards (`_MxComputeSwitch` with the mode "fp4").

    A class supplies `_FP4_LINEARS` (the names `linears=` takes), `_fp4_blocks()` (its blocks) and `_fp4_weights(blk)` ({name: the
    weight, or a tuple of weights, of that name in that block}; a name a block does not have is absent), calls `_fp4_detach()` where
    its weights change (`_weights_changed`, a merged LoRA) and `_fp4_refresh()` after `pack()` in `forward`.  The messages start with
    the class's `_tag`."""

    _fp4_linears = None      # the selected names while the mode is on
    _fp4_live: tuple = ()    # the weights that carry a record
    _fp4_bytes = 0

    # the two launch fusions of the mode (`set_fp4_compute(fused_quant=, mx_ffn=)`): which norms and GEMM epilogues write MXFP4
    # themselves is the class's business, the flags and their refusals are shared
    _fp4_fused_quant = False
    _fp4_mx_ffn = False

    def _fp4_switch(self, on: bool, linears=None, fused_quant: bool = False, mx_ffn: bool = False):
        if fused_quant and not on:
            raise ValueError(f"{self._tag}: set_fp4_compute(fused_quant=True) needs on=True: the fused norm quantises for the fp4 GEMM")
        if mx_ffn and not on:
            raise ValueError(f"{self._tag}: set_fp4_compute(mx_ffn=True) needs on=True: the MXFP4 hidden state belongs to the fp4 GEMMs")
        self._mx_switch("fp4", on, linears)
        self._fp4_fused_quant, self._fp4_mx_ffn = bool(fused_quant), bool(mx_ffn)
        return self

    def set_storage_dtype(self, dtype: torch.dtype):
        self._mx_guard_storage("fp4", dtype)
        return super().set_storage_dtype(dtype)

    def set_residual_dtype(self, dtype: torch.dtype):
        self._mx_guard_residual("fp4", dtype)
        return super().set_residual_dtype(dtype)

    def _fp4_attach(self):
        self._mx_attach("fp4")

    def _fp4_detach(self):
        self._mx_detach("fp4")

    def _fp4_refresh(self):
        self._mx_refresh("fp4")


class Fp6ComputeMixin(_MxComputeSwitch):
    """The switch of the opt-in MXFP6 compute mode, beside Fp4ComputeMixin in the bases of a class that supplies what
    that mixin asks for: `ops.Mxfp6Weight` records on each selected weight's `_fp6` slot, `_fp6_bytes`, the same names, refusals and
    dtype guards (`_MxComputeSwitch` with the mode "fp6").  The class calls `_fp6_detach()` / `_fp6_refresh()` where it calls the fp4
    ones.  Both modes may be on when their `linears` are disjoint."""

    _fp6_linears = None
    _fp6_live: tuple = ()
    _fp6_bytes = 0

    def _fp6_switch(self, on: bool, linears=None):
        return self._mx_switch("fp6", on, linears)

    def set_storage_dtype(self, dtype: torch.dtype):
        self._mx_guard_storage("fp6", dtype)
        return super().set_storage_dtype(dtype)

    def set_residual_dtype(self, dtype: torch.dtype):
        self._mx_guard_residual("fp6", dtype)
        return super().set_residual_dtype(dtype)

    def _fp6_detach(self):
        self._mx_detach("fp6")

    def _fp6_refresh(self):
        self._mx_refresh("fp6")


class Fp8ResidentMixin:
    """Quantised block weights RESIDENT in HBM (`weights.load_checkpoint_into(keep_fp8=True / keep_quantized=True)`: fp8-scaled,
    SURVEY.md §8f-2, and GGUF blocks) of the Flux and Wan transformers, in front of HipTransformer in the bases: adopting the
    records after the load, the refusals of a resident model and the switch of the opt-in FP8 compute.  The
    `_fp8*` names date from the first of the two formats; a parameter's `_fp8` slot holds any ops.ResidentWeight.

    A class supplies `_fp8_resident_key` (which checkpoint tensors stay as stored), `_fp8_plan()` and, without a resident mode
    for GGUF blocks, `_fp8_formats = ("fp8",)`.  The messages start with the class's `_tag`."""

    _fp8_formats = ("fp8", "gguf")

    def _fp8_plan(self):
        """[(holder, attribute or None, [weight parameters])] over the blocks: a projection fused from several Linears, read
        through `holder.attribute`, or (None) one Linear, which keeps its record on the parameter."""
        raise NotImplementedError

    def _fp8_options(self) -> str:      # the load options of the class's resident modes, as the messages name them
        return "keep_fp8 / keep_quantized" if "gguf" in self._fp8_formats else "keep_fp8"

    @torch.no_grad()
    def _fp8_adopt(self):
        """After a keep_fp8 / keep_quantized load: every fused projection of the plan becomes ONE fused record (`ops.Fp8Weight`:
        per-row scales; `ops.GgufWeight`: row segments), every other Linear keeps its record on the parameter, and the adopted
        parameters' bf16 storage is released.  The blocks' GEMMs then dequantise per call (`ops._bf16_weight`) until
        `set_fp8_compute(True)`.  Every group is checked BEFORE anything is released: a refusal leaves the model as loaded."""
        self.pack()
        dev, dt = self.device, self.dtype
        names = {id(p): k[:-len(".weight")] for k, p in self.named_parameters() if k.endswith(".weight")}
        for p in self.parameters():            # every record knows which Linear its rows are (run-time LoRA addresses them by name)
            f = getattr(p, "_fp8", None)
            if f is not None:
                f.parts = [(names[id(p)], 0, int(f.shape[0]))]
                p._fp8_shape = tuple(f.shape)
        plan = self._fp8_plan()
        for _, _, parts in plan:
            f8 = [getattr(p, "_fp8", None) for p in parts]
            if any(f is None for f in f8) != all(f is None for f in f8) or len({type(f) for f in f8}) > 1 \
                    or len({f.q.dtype for f in f8 if isinstance(f, ops.Fp8Weight)}) > 1:
                raise _l.ApexMIError(f"{self._tag} {self._fp8_options()}: the fused projection {[names[id(p)] for p in parts]} mixes "
                                     "quantised and plain weights (or two quantised formats)")
        n = 0
        self._fp8_records = {}                 # module path -> the record holding its rows
        for holder, attr, parts in plan:
            f8 = [getattr(p, "_fp8", None) for p in parts]
            if f8[0] is None:
                continue
            if attr is not None:
                rec = type(f8[0]).cat(f8)
                setattr(holder, attr, rec)     # the fused record is the one that is read; the parts' views of the bf16 buffer go
                for p in parts:
                    del p._fp8
            else:
                rec = f8[0]
            for p in parts:
                p.data = torch.empty(0, device=dev, dtype=dt)
            n += rec.nbytes()
            self._fp8_records.update({m: rec for m, _, _ in rec.parts})
        self._fp8_bytes = n
        torch.cuda.empty_cache()
        return self

    def _fp8_guard(self, what: str):
        """`pack()` and `state_dict()` call this first: a model whose block weights are resident records has neither."""
        if not getattr(self, "_fp8_bytes", 0):
            return
        opts = self._fp8_options()
        kind = "quantised" if "gguf" in self._fp8_formats else "fp8"
        if what == "pack":
            raise _l.ApexMIError(f"{self._tag}: the block weights are resident {kind} records ({opts} load) and their bf16 storage is "
                                 "gone; moving / re-packing such a model is not supported — construct and load again")
        raise _l.ApexMIError(f"{self._tag}: this model was loaded with {opts.replace(' /', '=True /')}=True — its block weights live as "
                             f"{kind} records (inference only); it has no bf16 state dict to save.  Load without {opts} to serialise.")

    def _fp8_set_compute(self, on: bool) -> list:
        """The distinct resident fp8 records (GGUF records have no fp8 compute), switched to fp8 or back to bf16 compute."""
        recs = {id(r): r for r in (getattr(self, "_fp8_records", None) or {}).values() if isinstance(r, ops.Fp8Weight)}
        if not recs:
            raise _l.ApexMIError(f"{self._tag}: set_fp8_compute needs resident fp8 weight records and this model has none — load an "
                                 "fp8-scaled checkpoint with keep_fp8=True")
        for r in recs.values():
            r.compute = "fp8" if on else "bf16"
        return list(recs.values())
