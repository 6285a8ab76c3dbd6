"""torch.Tensor-level wrappers over the C-ABI (include/apexmi.h).

PyTorch supplies device memory and the current HIP stream; all arithmetic happens in
libapex_mi355.so.  Every wrapper refuses CPU tensors: the product path has no fallback.
"""
from __future__ import annotations

import dataclasses
import math
import operator
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib as _l


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype, name: str) -> None:
    if not t.is_cuda:
        raise _l.ApexMIError(f"{name}: expected a ROCm device tensor, got {t.device} (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise _l.ApexMIError(f"{name}: expected {dtype}, got {t.dtype}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_I64N = {2: type(_l.i64x2((0, 0))), 3: type(_l.i64x3((0, 0, 0)))}


def _st(t: torch.Tensor, n: int = 3):
    """t's first n element strides as the int64[n] the C entry points take"""
    return _I64N[n](*t.stride()[:n])


def _rows16(t: torch.Tensor) -> torch.Tensor:
    """t itself where the attention kernels can read it in place, else one contiguous copy: they take 16 bytes of a row at a
    time, so the last dim is contiguous, the data 16-byte aligned and every other stride a multiple of 8 elements"""
    st = t.stride()
    ok = st[-1] == 1 and t.data_ptr() % 16 == 0 and all(x % 8 == 0 for x in st[:-1])
    return t if ok else t.contiguous()


# attention workspaces, one per key: (tag, device index, stream) with the tag of a kernel family ("masked" serves the masked and
# the window wrappers, "varlen", "wide", "prep", "band"), (device index, stream) for attention / attention_framecausal / attention_bias
_ws_cache: dict = {}


def _workspace(key, device, need: int, at_least: int = 0) -> torch.Tensor:
    """the cached uint8 buffer of `key`, replaced by a larger one when it holds fewer than max(need, at_least) bytes"""
    if need < at_least:
        need = at_least
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def _flash_qkv(who: str, q, k, v, rank: int, head_dims, enable_gqa):
    """The type and shape refusals the flash wrappers share, for q / k / v [B,H,S,D] (rank 4) or packed [T,H,D] (rank 3);
    returns (Hq, Hkv, Sq, Sk, D).  enable_gqa=None: a kernel without grouped-query heads (k and v need q's head count).  No
    device check: each wrapper places its own."""
    if q.dtype not in (torch.bfloat16, torch.float16) or k.dtype != q.dtype or v.dtype != q.dtype:
        raise _l.ApexMIError(f"{who}: dtypes {q.dtype}/{k.dtype}/{v.dtype} unsupported (bf16 or f16, all equal)")
    if q.dim() != rank or k.dim() != rank or v.dim() != rank:
        raise _l.ApexMIError(f"{who}: q, k, v must be " + ("4-D [B, H, S, D]" if rank == 4 else "3-D packed [T, H, D]"))
    qs, ks, seq = q.shape, k.shape, 2 if rank == 4 else 0
    Hq, Hkv, Sq, Sk, D = qs[1], ks[1], qs[seq], ks[seq], qs[-1]
    if D not in head_dims:
        if enable_gqa is None:
            raise _l.ApexMIError(f"{who}: head dim {D} unsupported {head_dims}; other head sizes go through `attention`")
        raise _l.ApexMIError(f"{who}: head dim {D} unsupported (64 or 128)")
    if ks[:rank - 3] != qs[:rank - 3] or ks[-1] != D or v.shape != ks or (enable_gqa is None and Hkv != Hq):
        raise _l.ApexMIError(f"{who}: shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} do not match")
    empty = q.numel() == 0 or k.numel() == 0
    # the 4-D wrappers refuse a ratio before an empty problem, the packed one an empty problem first
    if enable_gqa is not None and not (empty and rank == 3) and (Hq % Hkv != 0 or (Hkv != Hq and not enable_gqa and Hkv != 1)):
        raise _l.ApexMIError(f"{who}: {Hq} query heads over {Hkv} key/value heads needs enable_gqa=True and a whole ratio")
    if empty:
        raise _l.ApexMIError(f"{who}: empty problem")
    return Hq, Hkv, Sq, Sk, D


# ---- activation storage type -----------------------------------------------------------------------------------------
# Production stores activations as bf16.  A float32 activation tensor selects the f32-STORAGE VERIFICATION MODE of the
# library (include/apexmi.h, last section): the same kernels instantiated with float storage, the MFMA
# kernels fed the exact three-way bf16 split of the activations.  Weights, gains and biases are bf16 in both modes.
_ACT = (torch.bfloat16, torch.float32)


def _req_act(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _l.ApexMIError(f"{name}: expected a ROCm device tensor, got {t.device} (no CPU fallback)")
    if t.dtype not in _ACT:
        raise _l.ApexMIError(f"{name}: activations are stored as bfloat16 (or float32 in the verification mode), got {t.dtype}")


def _fn(name: str, t: torch.Tensor):
    """The entry point `name` for t's storage type (`name_f32` for float activations)."""
    return getattr(_l.load(), name + ("_f32" if t.dtype == torch.float32 else ""))


def split3(a: torch.Tensor) -> torch.Tensor:
    """[M, K] float (row stride free) -> [M, 3K] bf16 = [hi | mid | lo], hi + mid + lo == a exactly."""
    _req(a, torch.float32, "split3.a")
    assert a.dim() == 2 and a.stride(1) == 1 and a.shape[1] % 8 == 0
    M, K = a.shape
    out = torch.empty((M, 3 * K), dtype=torch.bfloat16, device=a.device)
    _l.check(_l.load().apexmi_split_bf16x3(a.data_ptr(), a.stride(0), M, K, out.data_ptr(), out.stride(0), _stream()),
             "split_bf16x3")
    return out


_w3_cache: dict = {}
_w3_bytes = 0
_W3_CAP = 16 << 30


def clear_verification_caches() -> None:
    """Drop the repeated-weight copies the f32-storage verification mode keeps (they hold their source weights alive)."""
    global _w3_bytes
    _w3_cache.clear()
    _w3c_cache.clear()
    _w3_bytes = 0


# ---- verification through the SHIPPED kernels ------------------------------------------------------------
# The f32-storage mode replaces three kernel families by float-capable stand-ins (generic attention, the 128x128 convolution,
# the two-pass q/k/v preparation).  With this switch on, float activations still flow everywhere else, but those three points run
# the kernels production launches — the flash attention kernels, the slab / conv-shaped convolution tiles (with their fused norm
# epilogue), the fused QKV epilogue — on the bf16 ROUNDING of their float operands, and their bf16 results are widened back to
# float: the chain error then contains exactly those kernels' own storage roundings and nothing else of the bf16 path.
_shipped_verify = False


def verify_through_shipped_kernels(on: bool = True) -> None:
    global _shipped_verify
    _shipped_verify = bool(on)


def shipped_verification() -> bool:
    return _shipped_verify


def tensor_version(t: torch.Tensor):
    """`t._version`, or None for an inference tensor (created under `torch.inference_mode()`, as everything inside the
    reference's `UniversalEngine.run` is — `R/src/engine/registry.py:196`): those do not track a version counter and
    reading it raises, so callers must not cache on them across calls."""
    return None if t.is_inference() else t._version


def _w3(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 weight -> [N, 3K] = [w | w | w] (layout only), the partner of split3(); cached per weight version.
    An entry keeps a reference to its source view, so the address in the key cannot be recycled while the entry lives."""
    global _w3_bytes
    ver = tensor_version(w)
    if ver is None:                 # inference tensor: no version counter to key on — rebuild, never cache
        return w.repeat(1, 3).contiguous()
    key = (w.data_ptr(), ver, tuple(w.shape), w.stride(0))
    hit = _w3_cache.get(key)
    if hit is None:
        if _w3_bytes > _W3_CAP:
            clear_verification_caches()
        hit = (w, w.repeat(1, 3).contiguous())
        _w3_cache[key] = hit
        _w3_bytes += hit[1].numel() * 2
    return hit[1]


# ---- quantised weights RESIDENT in HBM: fp8-scaled and GGUF blocks (rows 16 / 18) -------------------------------------
class ResidentWeight:
    """What a Linear weight that stays quantised in HBM has in common, whatever its format: the [N, K] `shape`, which model Linears
    its rows belong to (`parts`), `dequant(out=)` into a bf16 operand right before the GEMM that reads it, `nbytes()`, and the
    RUN-TIME LoRA factors (`set_lora`).  Subclasses: Fp8Weight (float8 + scale), GgufWeight (ggml blocks)."""

    def _init_record(self, shape, device) -> None:
        self.shape = torch.Size(shape)
        self.device = device
        # which model Linears the rows belong to: [(module path, first row, rows)] (set by the model that adopts the record)
        self.parts: List[Tuple[str, int, int]] = []
        # RUN-TIME LoRA on a weight whose bf16 form does not exist (set_lora): lora_A [Rp, K] = the active adapters' down factors
        # stacked along the rank (zero rows up to a multiple of 64), lora_B [N, Rp] = their up factors x scale, placed on the rows
        # of their part (block-diagonal for a fused projection)
        self.lora_A: Optional[torch.Tensor] = None
        self.lora_B: Optional[torch.Tensor] = None

    def _cat_parts(self, parts: Sequence["ResidentWeight"]) -> None:
        r0 = 0
        for p in parts:
            self.parts += [(m, r0 + a, n) for m, a, n in p.parts]
            r0 += p.shape[0]

    def nbytes(self) -> int:
        raise NotImplementedError

    def dequant(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        raise NotImplementedError

    @torch.no_grad()
    def set_lora(self, adapters: Sequence[Tuple[str, torch.Tensor, torch.Tensor, float]]) -> int:
        """`adapters`: (module path, A [r, K], B [rows of that part, r], scale) of every ACTIVE adapter touching this record.
        The reference keeps quantised base weights and runs `base(x) + scale * B(A(x))` per Linear at run time (PEFT layers
        around FPScaledLinear, R/src/lora/manager.py:454-606); gemm() below does the same as ONE extra skinny GEMM and a K
        extended by the padded rank (see _gemm_fp8_lora).  Returns the padded rank (0 = no adapter left)."""
        if not adapters:
            self.lora_A = self.lora_B = None
            return 0
        N, K = self.shape
        row_of = {m: (a, n) for m, a, n in self.parts}
        R = sum(int(a.shape[0]) for _, a, _, _ in adapters)
        Rp = (R + 63) // 64 * 64
        A = torch.zeros((Rp, K), dtype=torch.float32, device=self.device)
        B = torch.zeros((N, Rp), dtype=torch.float32, device=self.device)
        c = 0
        for m, a, b, sc in adapters:
            if m not in row_of:
                raise KeyError(f"{type(self).__name__}.set_lora: '{m}' is not a part of this record ({[p[0] for p in self.parts]})")
            r0, n = row_of[m]
            r = int(a.shape[0])
            if tuple(a.shape) != (r, K) or tuple(b.shape) != (n, r):
                raise ValueError(f"LoRA factors {tuple(b.shape)} x {tuple(a.shape)} do not fit the {n} x {K} weight of '{m}'")
            A[c:c + r] = a.to(self.device, torch.float32)
            B[r0:r0 + n, c:c + r] = b.to(self.device, torch.float32) * float(sc)
            c += r
        self.lora_A, self.lora_B = A.to(torch.bfloat16), B.to(torch.bfloat16)
        return Rp


class Fp8Weight(ResidentWeight):
    """A Linear weight kept as the checkpoint stores it — float8 (e4m3fn / e5m2) [N, K] + `scale_weight` (one value, or one per
    row) — and dequantised PER CALL into a per-stream bf16 scratch right before the GEMM that reads it, as the reference's
    `FPScaledLinear.forward` does (`_scale_and_cast_weight`, scaled_layer.py:496-549: `weight.to(bf16) * scale.to(bf16)`, then a
    bf16 matmul).  Same dequantisation kernel as the load-time path (`apexmi_dequant_fp8_scaled`, every code point pinned by
    tests/golden/fp_scaled.pt), so a forward is bit-identical to dequantise-at-load; the model holds half the weight bytes.

    `compute`: "bf16" (the default: the path above) or "fp8" — the OPT-IN approximation of DESIGN.md §3.6: `gemm` quantises the
    activations per row to e4m3 and multiplies the resident codes directly (`gemm_fp8`), where `fp8_compute_route` allows it."""

    compute = "bf16"
    # with compute == "fp8": what a record carrying run-time LoRA factors does.  "bf16" (the default) = the bf16 path above
    # (_gemm_fp8_lora), "fp8" = the fp8 GEMM with the adapter tail (`fp8_lora_route`, `gemm_fp8(lora_t=, lora_B=)`)
    lora_compute = "bf16"

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype not in (torch.float8_e4m3fn, torch.float8_e5m2) or q.dim() != 2:
            raise TypeError(f"Fp8Weight: expected a 2-D float8 tensor, got {q.dtype} {tuple(q.shape)}")
        self.q = q.contiguous()
        s = scale.to(q.device).to(torch.bfloat16).reshape(-1).contiguous()
        if s.numel() not in (1, q.shape[0]):
            raise ValueError(f"Fp8Weight: scale has {s.numel()} values for {q.shape[0]} rows")
        self.scale = s
        self._init_record(q.shape, q.device)

    @classmethod
    def cat(cls, parts: Sequence["Fp8Weight"]) -> "Fp8Weight":
        """Rows of several weights stacked (a fused q | k | v projection): per-tensor scales become per-row vectors."""
        if len({p.q.dtype for p in parts}) != 1 or len({p.shape[1] for p in parts}) != 1:
            raise ValueError("Fp8Weight.cat: parts must share the fp8 format and the input width")
        q = torch.cat([p.q.view(torch.uint8) for p in parts], dim=0).view(parts[0].q.dtype)
        s = torch.cat([p.scale if p.scale.numel() == p.shape[0] else p.scale.expand(p.shape[0]) for p in parts])
        out = cls(q, s)
        out._cat_parts(parts)
        return out

    def nbytes(self) -> int:
        return self.q.numel() + 2 * self.scale.numel()

    def dequant(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        return dequant_fp8_scaled(self.q, self.scale, out=out)


class GgufWeight(ResidentWeight):
    """A Linear weight kept as a GGUF file stores it: ggml blocks, as a list of ROW SEGMENTS (ggml type, rows, uint8 bytes on the
    device) — a fused projection may mix types (Q4_K_M files store some tensors as Q6_K) — dequantised PER CALL, one
    `apexmi_dequant_gguf` launch per segment, as the reference's `GGMLLinear.forward` does (R/src/quantize/ggml_layer.py:220).
    Same kernel as the load-time path, so a forward is bit-identical to dequantise-at-load."""

    def __init__(self, segments: Sequence[Tuple[int, int, torch.Tensor]], K: int):
        segs = []
        for t, n, b in segments:
            if b.dtype != torch.uint8 or not b.is_cuda:
                raise TypeError(f"GgufWeight: block bytes must be a uint8 device tensor, got {b.dtype} on {b.device}")
            if segs and segs[-1][0] == t:                       # neighbours of one type: one launch
                segs[-1] = (t, segs[-1][1] + n, torch.cat([segs[-1][2].reshape(-1), b.reshape(-1)]))
            else:
                segs.append((int(t), int(n), b.reshape(-1).contiguous()))
        self.segments = segs
        self._init_record((sum(n for _, n, _ in segs), int(K)), segs[0][2].device)

    @classmethod
    def cat(cls, parts: Sequence["GgufWeight"]) -> "GgufWeight":
        """Rows of several weights stacked (a fused q | k | v projection)."""
        if len({p.shape[1] for p in parts}) != 1:
            raise ValueError("GgufWeight.cat: parts must share the input width")
        out = cls([seg for p in parts for seg in p.segments], parts[0].shape[1])
        out._cat_parts(parts)
        return out

    def nbytes(self) -> int:
        return sum(b.numel() for _, _, b in self.segments)

    def dequant(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        N, K = self.shape
        if out is None:
            out = torch.empty((N, K), dtype=torch.bfloat16, device=self.device)
        r0 = 0
        for t, n, b in self.segments:
            dequant_gguf(b, t, (n, K), out=out[r0:r0 + n])
            r0 += n
        return out


_fp8_scratch: dict = {}


def _fp8_of(w):
    """The resident record behind `w` (an Fp8Weight / GgufWeight, or a parameter carrying one in `_fp8`), or None."""
    return w if isinstance(w, ResidentWeight) else getattr(w, "_fp8", None)


def _stream_scratch(store: dict, dev, *wants):
    """The current stream's buffers in `store`, one flat buffer per (numel, dtype) of `wants`, each replaced by a larger one when it
    holds fewer elements than asked (grow-only).  Stream order makes the reuse safe: the next writer is queued behind the last
    reader.  Every store is a dict of its own: what lives in one is not overwritten by a request to another."""
    key = (dev.index, torch.cuda.current_stream().cuda_stream)
    bufs = list(store.get(key, (None,) * len(wants)))
    for i, (n, dtype) in enumerate(wants):
        if bufs[i] is None or bufs[i].numel() < n:
            bufs[i] = torch.empty(n, dtype=dtype, device=dev)
    store[key] = tuple(bufs)
    return bufs


def _scratch(dev, n: int) -> torch.Tensor:
    return _stream_scratch(_fp8_scratch, dev, (n, torch.bfloat16))[0]


def _is_lora_buf(a, f8: "ResidentWeight", lora_buf) -> bool:
    """Whether `lora_buf` is the padded activation buffer of `a` that run-time LoRA needs: same storage, rows and row stride,
    at least K + Rp columns."""
    return lora_buf is not None and lora_buf.data_ptr() == a.data_ptr() and lora_buf.stride(0) == a.stride(0) \
        and lora_buf.shape[1] >= a.shape[1] + f8.lora_A.shape[0] and lora_buf.shape[0] == a.shape[0]


def _gemm_fp8_lora(a, f8: "ResidentWeight", bias, out, epilogue, gate, residual, lora_buf):
    """epi(a W^T + (a A^T) B'^T + bias) for a resident-fp8 weight W with run-time LoRA factors, as TWO launches:
         t = a A^T                      [M, Rp] bf16 — the reference's `lora_A(x)` output, rounded as it is there — written into
                                        the columns right behind `a` in its padded buffer (`lora_buf`: same rows, >= K + Rp wide);
         out = epi([a | t] [W | B']^T)  one GEMM over K + Rp: W dequantised into the per-stream scratch with row stride K + Rp
                                        (the kernel of the load-time path), B' = scale x B copied behind it.
    The adapter term is accumulated in f32 with the base product and rounded ONCE, under any epilogue (GELU included) — at least as
    accurate as the reference's bf16 `result + lora_B(lora_A(x)) * scaling`.  Cost: Rp / K more K-tiles (1.25 % at rank 64 on
    d = 5120) + the skinny GEMM; no pass over the [M, N] output."""
    M, K = a.shape
    N = f8.shape[0]
    Rp = f8.lora_A.shape[0]
    if a.dtype != torch.bfloat16:
        raise NotImplementedError("run-time LoRA on resident-fp8 weights exists for bf16 activation storage only")
    if not _is_lora_buf(a, f8, lora_buf):
        raise _l.ApexMIError(f"gemm: the weight carries run-time LoRA factors (rank {Rp} padded) and needs `lora_buf` = the activation "
                             f"buffer of `a` with >= {K + Rp} columns (got {None if lora_buf is None else tuple(lora_buf.shape)})")
    gemm(a, f8.lora_A, None, out=lora_buf[:, K:K + Rp])
    w2 = _scratch(f8.device, N * (K + Rp))[:N * (K + Rp)].view(N, K + Rp)
    f8.dequant(out=w2[:, :K])
    w2[:, K:].copy_(f8.lora_B)
    return gemm(lora_buf[:, :K + Rp], w2, bias, out=out, epilogue=epilogue, gate=gate, residual=residual)


def _bf16_weight(w, float_acts: bool = False):
    """`w` as the bf16 [N, K] operand of a GEMM launched next on the current stream: the tensor itself, or — for an Fp8Weight / a
    parameter carrying one (`param._fp8`, weights.load_checkpoint_into(keep_fp8=True)) — its dequantisation into the stream's
    scratch.  Stream order makes the reuse safe: the next dequantisation is queued behind the GEMM that read the last one."""
    f8 = _fp8_of(w)
    if f8 is None:
        return w
    if f8.lora_A is not None:
        raise _l.ApexMIError("this resident-fp8 weight carries run-time LoRA factors: only gemm(..., lora_buf=) applies them")
    if float_acts:           # verification mode caches on (data_ptr, version): never hand it a recycled buffer
        return f8.dequant()
    n = f8.shape[0] * f8.shape[1]
    return f8.dequant(out=_scratch(f8.device, n)[:n].view(f8.shape[0], f8.shape[1]))


# ---- opt-in FP8 compute on resident e4m3 weights ---------------------------------------------------------------------
_FP8_EPI = ("bias", "gelu", "gate_res")


def _block_gemm_route(a: torch.Tensor, w_shape, out: Optional[torch.Tensor], epilogue: str, k_mult: int,
                      max_row_stride: Optional[int] = None) -> bool:
    """The rules every route onto a block-scaled-MFMA GEMM shares (`fp8_compute_route`, `fp8_lora_route`, `mxfp4_route`; each asks
    its own question about the weight record first).  Pure.  `a` bf16 and `out` bf16 or None; `a` 2-D with contiguous rows; the
    epilogue one of bias / gelu / gate_res; M >= 1, K the record's K = `w_shape[1]` and a multiple of `k_mult` (the codes of one
    K-tile), N = `w_shape[0]` a multiple of 16; 16-byte rows of `a`, with a row stride of at most `max_row_stride` where given."""
    if a.dtype != torch.bfloat16 or (out is not None and out.dtype != torch.bfloat16):
        return False
    if a.dim() != 2 or a.stride(1) != 1 or epilogue not in _FP8_EPI:
        return False
    M, K = a.shape
    N = w_shape[0]
    return M >= 1 and K == w_shape[1] and K % k_mult == 0 and N % 16 == 0 and a.stride(0) % 8 == 0 \
        and (max_row_stride is None or a.stride(0) <= max_row_stride)


def _updown_route(route, record_of, n_mult: int, a_or_shape, w_up, w_down, epilogue_up: str, epilogue_down: str, out) -> bool:
    """Whether the pair `h = gemm(a, w_up, epilogue=epilogue_up)` -> `gemm(h, w_down, out=out, epilogue=epilogue_down)` may keep `h`
    in the MX form of `route` (`fp8_compute_route`, `mxfp4_route`) between the two launches.  Pure.  `a_or_shape`: the bf16 input
    [M, K] of the up projection, or its shape.  True only when both launches take `route`, the up epilogue is bias or gelu and
    N_up (read from the record `record_of(w_up)`) is a multiple of `n_mult`."""
    a = a_or_shape if isinstance(a_or_shape, torch.Tensor) else torch.empty(tuple(a_or_shape), dtype=torch.bfloat16, device="meta")
    f_up = record_of(w_up)
    if epilogue_up not in ("bias", "gelu") or not route(a, f_up, None, epilogue_up):
        return False
    n_up = f_up.shape[0]
    if n_up % n_mult != 0:
        return False
    h = torch.empty((a.shape[0], n_up), dtype=torch.bfloat16, device="meta")
    return route(h, w_down, out, epilogue_down)


def fp8_compute_route(a: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias") -> bool:
    """Whether `gemm(a, w, out=out, epilogue=epilogue)` goes out as quantise + `gemm_fp8`.  Pure: reads dtypes, shapes and strides
    only (CPU tensors are fine).  True only when ALL of these hold:
      * `w` is (or carries) an `Fp8Weight` in float8_e4m3fn with `compute == "fp8"`;
      * `a` is bf16 and `out` is bf16 or None (float activations = the f32-storage mode and a float `out` = the f32 residual
        stream keep the bf16 path);
      * the weight carries no run-time LoRA factors (`set_lora`);
      * the shape is eligible: M >= 1, K % 128 == 0, N % 16 == 0, 16-byte rows of `a` with a row stride <= 2^22, and the epilogue
        is one of bias / gelu / gate_res."""
    f8 = _fp8_of(w)
    if not isinstance(f8, Fp8Weight) or f8.compute != "fp8" or f8.q.dtype != torch.float8_e4m3fn or f8.lora_A is not None:
        return False
    return _block_gemm_route(a, f8.shape, out, epilogue, 128, 1 << 22)


def fp8_lora_route(a: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias",
                   lora_buf: Optional[torch.Tensor] = None) -> bool:
    """Whether `gemm(a, w, out=out, epilogue=epilogue, lora_buf=lora_buf)` on a record WITH run-time LoRA factors goes out as
    skinny GEMM + quantise + `gemm_fp8(lora_t=, lora_B=)` (the fp8 GEMM with the bf16 adapter tail) instead of `_gemm_fp8_lora`.
    Pure, like `fp8_compute_route`.  True only when ALL of these hold:
      * `w` is (or carries) an e4m3 `Fp8Weight` with `compute == "fp8"` AND `lora_compute == "fp8"`, and it carries factors;
      * `a` is bf16 and `out` is bf16 or None;
      * the shape rules of `fp8_compute_route` hold;
      * `lora_buf` is the padded activation buffer `_gemm_fp8_lora` requires (the skinny GEMM writes t behind `a`)."""
    f8 = _fp8_of(w)
    return _fp8_lora_problem_route(a, f8, out, epilogue) and _is_lora_buf(a, f8, lora_buf)


def _fp8_lora_problem_route(a: torch.Tensor, f8, out: Optional[torch.Tensor], epilogue: str) -> bool:
    """The rules of `fp8_lora_route` that do not concern `lora_buf` (shared with `fp8_grouped_lora_route`)."""
    if not isinstance(f8, Fp8Weight) or f8.compute != "fp8" or f8.lora_compute != "fp8" or f8.q.dtype != torch.float8_e4m3fn \
            or f8.lora_A is None:
        return False
    return _block_gemm_route(a, f8.shape, out, epilogue, 128, 1 << 22)


def fp8_norm_quant_rows(x: torch.Tensor, xn: torch.Tensor) -> bool:
    """Whether the fused norm `ln_modulate_quant_fp8` accepts the pair (input rows `x`, normalised rows `xn`), whatever reads the
    codes: the rules of `fp8_norm_quant_route` that concern the rows alone.  Pure."""
    if x.dim() != 2 or xn.dim() != 2 or tuple(x.shape) != tuple(xn.shape) or x.stride(1) != 1 or xn.stride(1) != 1:
        return False
    if x.dtype not in (torch.bfloat16, torch.float32) or xn.dtype != torch.bfloat16:
        return False
    M, Cc = x.shape
    return not (M < 1 or Cc % 128 != 0 or Cc > 8192 or x.stride(0) % (16 // x.element_size()) != 0 or xn.stride(0) % 8 != 0)


def fp8_norm_quant_route(x: torch.Tensor, xn: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias",
                         lora_buf: Optional[torch.Tensor] = None, row_read_later: bool = False) -> Tuple[bool, bool]:
    """Whether the pair `ln_modulate(x, ..., out=xn)` -> `gemm(xn, w, out=out, epilogue=epilogue, lora_buf=lora_buf)` may go out as
    `ln_modulate_quant_fp8` -> `gemm(..., quantised=)`, i.e. the norm writes the e4m3 codes and row scales itself and the GEMM's
    own `quant_rows_fp8` launch disappears.  Returns (fuse, need_row).  Pure, like `fp8_compute_route`: dtypes, shapes and strides
    only (CPU tensors are fine).
      fuse      the GEMM takes its fp8 route (`fp8_compute_route` or `fp8_lora_route` on `xn`) AND the fused norm accepts the
                pair: `x` bf16 or float32 (the f32 residual stream) [M, C] with 16-byte rows, `xn` bf16 of the same shape,
                C % 128 == 0 and C <= 8192.  False = run today's launches.
      need_row  the bf16 row must still be stored (pass `out=xn` to the fused norm): the weight carries run-time LoRA factors
                (the skinny GEMM reads `xn`), or the caller says something else reads `xn` (`row_read_later`).  False only
                with `fuse`."""
    if not fp8_norm_quant_rows(x, xn):
        return False, True
    if fp8_compute_route(xn, w, out, epilogue):
        return True, bool(row_read_later)
    if fp8_lora_route(xn, w, out, epilogue, lora_buf):
        return True, True
    return False, True


_fp8_act_scratch: dict = {}


def _act_scratch(dev, M: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-stream home of the activation codes [M, K] and their row scales [M] (as `_scratch`: stream order makes the reuse safe)."""
    q, s = _stream_scratch(_fp8_act_scratch, dev, (M * K, torch.uint8), (M, torch.float32))
    return q[:M * K].view(M, K), s[:M]


def quant_rows_fp8(a: torch.Tensor, out: Optional[torch.Tensor] = None,
                   scale_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-row e4m3 quantisation of bf16 `a` [M, K] (row stride free, K % 128 == 0) -> (codes uint8 [M, K] = float8_e4m3fn bit
    patterns, scales float32 [M]).  Per row, in IEEE float32 with every operation rounded on its own (true division, no FMA):
        absmax = max |a|;  scale = 1 if absmax == 0 else absmax / 448;  code = e4m3fn_rne(clamp(a / scale, -448, 448))
    An all-zero row has scale 1 and zero codes; no code is NaN.  Inputs must be finite."""
    _req(a, torch.bfloat16, "quant_rows_fp8.a")
    assert a.dim() == 2 and a.stride(1) == 1
    M, K = a.shape
    if out is None:
        out = torch.empty((M, K), dtype=torch.uint8, device=a.device)
    if scale_out is None:
        scale_out = torch.empty(M, dtype=torch.float32, device=a.device)
    _req(out, torch.uint8, "quant_rows_fp8.out")
    _req(scale_out, torch.float32, "quant_rows_fp8.scale_out")
    assert out.shape == (M, K) and out.stride(1) == 1 and scale_out.is_contiguous() and scale_out.numel() == M
    _l.check(_l.load().apexmi_quant_rows_fp8(a.data_ptr(), a.stride(0), M, K, out.data_ptr(), out.stride(0), scale_out.data_ptr(),
                                             _stream()), "quant_rows_fp8")
    return out, scale_out


def quant_blocks_mxfp8(a: torch.Tensor, out: Optional[torch.Tensor] = None,
                       scale_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MX block quantisation of bf16 `a` [M, K] (row stride free, K % 128 == 0) -> (codes uint8 [M, K] = float8_e4m3fn bit
    patterns, block_scales uint8 [M, K / 32] = e8m0 exponents; row strides free).  Per block of 32 consecutive columns:
        amax = max |a| with unbiased f32 exponent E and mantissa bits man;  e = clamp(E - 8 + (man > 0x600000), -126, 127)
        (0 for a zero block);  scale byte = e + 127;  code = e4m3fn_rne(clamp(a * 2^-e, -448, 448))
    2^e is the smallest power of two with amax / 2^e <= 448, so the clamp clips nothing; a zero block has byte 127 and no byte is
    255; no code is NaN.  Inputs must be finite.  One launch, no row reduction: what `gemm_fp8(block_scales=)` reads, and what
    `gemm_fp8(out_mx=)` writes from its epilogue."""
    if a.dtype != torch.bfloat16:
        raise _l.ApexMIError(f"quant_blocks_mxfp8.a: expected torch.bfloat16, got {a.dtype}")
    if a.dim() != 2 or a.stride(1) != 1 or a.shape[1] % 128 != 0 or a.shape[0] < 1:
        raise _l.ApexMIError(f"quant_blocks_mxfp8.a: expected [M >= 1, K % 128 == 0] with contiguous rows, got {tuple(a.shape)}")
    M, K = a.shape
    if out is None:
        out = torch.empty((M, K), dtype=torch.uint8, device=a.device)
    if scale_out is None:
        scale_out = torch.empty((M, K // 32), dtype=torch.uint8, device=a.device)
    _check_mx_pair("quant_blocks_mxfp8.out", (out, scale_out), M, K)
    _req(a, torch.bfloat16, "quant_blocks_mxfp8.a")
    _l.check(_l.load().apexmi_quant_blocks_mxfp8(a.data_ptr(), a.stride(0), M, K, out.data_ptr(), out.stride(0), scale_out.data_ptr(),
                                                 scale_out.stride(0), _stream()), "quant_blocks_mxfp8")
    return out, scale_out


def _check_mx_pair(who: str, pair, M: int, N: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """An MX (codes [M, N], block_scales [M, N / 32]) pair, both uint8 with contiguous rows: dtype and shape first, then device."""
    try:
        q, s = pair
    except (TypeError, ValueError):
        raise _l.ApexMIError(f"{who}: expected a (codes, block_scales) pair") from None
    for t, nm in ((q, "codes"), (s, "block_scales")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise _l.ApexMIError(f"{who} {nm}: expected torch.uint8, got {getattr(t, 'dtype', type(t).__name__)}")
    if q.dim() != 2 or tuple(q.shape) != (M, N) or q.stride(1) != 1:
        raise _l.ApexMIError(f"{who} codes: expected [{M}, {N}] with contiguous rows, got {tuple(q.shape)}")
    _check_block_scales(who + " block_scales", s, M, N)
    _req(q, torch.uint8, who + " codes")
    return q, s


def _check_block_scales(who: str, s: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """The e8m0 block scales [M, K / 32] (uint8, contiguous rows) of an activation [M, K]: dtype and shape first, then device."""
    if not isinstance(s, torch.Tensor) or s.dtype != torch.uint8:
        raise _l.ApexMIError(f"{who}: expected torch.uint8, got {getattr(s, 'dtype', type(s).__name__)}")
    if s.dim() != 2 or tuple(s.shape) != (M, K // 32) or s.stride(1) != 1:
        raise _l.ApexMIError(f"{who}: expected [{M}, {K // 32}] (one byte per 32 columns) with contiguous rows, got {tuple(s.shape)}")
    _req(s, torch.uint8, who)
    return s


def _check_quantised(a: torch.Tensor, quantised) -> Tuple[torch.Tensor, torch.Tensor]:
    """`gemm(quantised=)`: (codes, scales) must be what quant_rows_fp8(a) would return in shape and type."""
    qa, sa = quantised
    _req(qa, torch.uint8, "gemm.quantised codes")
    _req(sa, torch.float32, "gemm.quantised scales")
    if tuple(qa.shape) != tuple(a.shape) or qa.stride(1) != 1 or sa.numel() != a.shape[0] or not sa.is_contiguous():
        raise _l.ApexMIError(f"gemm: quantised=(codes {tuple(qa.shape)}, scales {tuple(sa.shape)}) does not fit a {tuple(a.shape)}")
    return qa, sa


def _fp8_acts(a: torch.Tensor, quantised) -> Tuple[torch.Tensor, torch.Tensor]:
    """The e4m3 codes and row scales of `a` for the fp8 routes of `gemm`: `quantised` where the caller brought them, else
    `quant_rows_fp8(a)` into the stream's activation scratch."""
    if quantised is not None:
        return _check_quantised(a, quantised)
    qa, sa = _act_scratch(a.device, a.shape[0], a.shape[1])
    quant_rows_fp8(a, out=qa, scale_out=sa)
    return qa, sa


def _norm_quant_operands(who: str, x, out, scale, shift, scale2, shift2, gamma, beta, told: bool = False) -> Tuple[int, int]:
    """The operands the quantising norms (`ln_modulate_quant_fp8`, `ln_modulate_quant_mxfp4`) share: the rows `x` [M, C] (bf16 or
    float32), the optional bf16 `out` of the same shape, the float32 modulation vectors and the bf16 affine vectors of C elements.
    Returns (M, C).  `told`: a wrong shape of `x` (C % 128 and M >= 1 included) raises ApexMIError with a reason (what the fp4 form
    does) instead of failing an assertion on its rank and rows."""
    _req(x, None, who + ".x")
    if x.dtype not in (torch.bfloat16, torch.float32):
        raise _l.ApexMIError(f"{who}.x: expected torch.bfloat16 or torch.float32, got {x.dtype}")
    if told and (x.dim() != 2 or x.stride(1) != 1 or x.shape[1] % 128 != 0 or x.shape[0] < 1):
        raise _l.ApexMIError(f"{who}.x: expected [M >= 1, C % 128 == 0] with contiguous rows, got {tuple(x.shape)}")
    assert x.dim() == 2 and x.stride(1) == 1
    M, Cc = x.shape
    if out is not None:
        _req(out, torch.bfloat16, who + ".out")
        assert out.shape == (M, Cc) and out.stride(1) == 1
    for t, nm in ((scale, "scale"), (shift, "shift"), (scale2, "scale2"), (shift2, "shift2")):
        if t is not None:
            _req(t, torch.float32, f"{who}.{nm}")
            assert t.is_contiguous() and t.numel() == Cc
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _req(t, torch.bfloat16, f"{who}.{nm}")
            assert t.is_contiguous() and t.numel() == Cc
    return M, Cc


def ln_modulate_quant_fp8(x: torch.Tensor, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                          gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, eps: float = 1e-6,
                          rms: bool = False, split: int = 0, scale2: Optional[torch.Tensor] = None,
                          shift2: Optional[torch.Tensor] = None, codes: Optional[torch.Tensor] = None,
                          scale_out: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`ln_modulate(x, ...)` into bf16 followed by `quant_rows_fp8` on its output, as ONE launch: -> (codes uint8 [M, C], scales
    float32 [M]), bit-identical to the two launches.  `x` bf16, or float32 (the f32 residual stream); C % 128 == 0.  `out`
    (optional, bf16 [M, C], row stride free): also receives the normalised rows, bit-identical to `ln_modulate(x, ..., out=out)`;
    None = the bf16 rows are never stored (3 bytes per element moved instead of 7).  `codes` / `scale_out` default to the
    per-stream activation scratch of `gemm`'s fp8 route, valid until that stream's next fp8 GEMM or fused norm."""
    M, Cc = _norm_quant_operands("ln_modulate_quant_fp8", x, out, scale, shift, scale2, shift2, gamma, beta)
    if codes is None and scale_out is None:
        codes, scale_out = _act_scratch(x.device, M, Cc)
    if codes is None:
        codes = torch.empty((M, Cc), dtype=torch.uint8, device=x.device)
    if scale_out is None:
        scale_out = torch.empty(M, dtype=torch.float32, device=x.device)
    _req(codes, torch.uint8, "ln_modulate_quant_fp8.codes")
    _req(scale_out, torch.float32, "ln_modulate_quant_fp8.scale_out")
    assert codes.shape == (M, Cc) and codes.stride(1) == 1 and scale_out.is_contiguous() and scale_out.numel() == M
    rc = _l.load().apexmi_ln_modulate_quant_fp8(
        x.data_ptr(), x.stride(0), _l.F32 if x.dtype == torch.float32 else _l.BF16, _ptr(out), 0 if out is None else out.stride(0),
        codes.data_ptr(), codes.stride(0), scale_out.data_ptr(), M, Cc, _ptr(scale), _ptr(shift), _ptr(gamma), _ptr(beta),
        float(eps), 1 if rms else 0, int(split), _ptr(scale2), _ptr(shift2), _stream())
    _l.check(rc, "ln_modulate_quant_fp8")
    return codes, scale_out


def _fp8_problem(who, codes, scales, w, bias, out, epilogue, gate, residual, K=None, fused=False, alloc=False,
                 block_scales=None, out_mx=None):
    """The checks of ONE fp8 GEMM problem, for `gemm_fp8` and for every problem of a grouped launch (`K`: the K they share).
    Returns (out, flag): `out` (made here if None and `alloc`) and the epilogue flag of a float `out`, which the entry point
    rejects with its own message, as it does e5m2 records.  `fused`: the problem writes no `out`.  `block_scales` (then `scales`
    is None) / `out_mx` (then `out` is not written): the MX forms, see `gemm_fp8`."""
    if block_scales is not None:
        if scales is not None:
            raise _l.ApexMIError(f"{who}: `scales` (one per row) and `block_scales` (one per 32 columns) were both given: "
                                 "an activation carries one kind")
        if codes.dim() == 2:
            _check_block_scales(who + ".block_scales", block_scales, codes.shape[0], codes.shape[1])
    if out_mx is not None:
        if epilogue not in ("bias", "gelu"):
            raise _l.ApexMIError(f"{who}: out_mx exists for the bias and gelu epilogues, not '{epilogue}'")
        if isinstance(w, Fp8Weight) and w.shape[0] % 128 != 0:
            raise _l.ApexMIError(f"{who}: out_mx needs N % 128 == 0, got N={w.shape[0]}")
        if isinstance(w, Fp8Weight) and codes.dim() == 2:
            _check_mx_pair(who + ".out_mx", out_mx, codes.shape[0], w.shape[0])
        fused = True
    _req(codes, torch.uint8, who + ".codes")
    if block_scales is None:
        _req(scales, torch.float32, who + ".scales")
    if not isinstance(w, Fp8Weight):
        raise _l.ApexMIError(f"{who}: expected an Fp8Weight, got {type(w).__name__}")
    if epilogue not in _FP8_EPI:
        raise _l.ApexMIError(f"{who}: epilogue '{epilogue}' is not one of {_FP8_EPI}")
    assert codes.dim() == 2 and codes.stride(1) == 1 and (scales is None or scales.is_contiguous())
    M, N = codes.shape[0], w.shape[0]
    K = codes.shape[1] if K is None else K
    assert codes.shape[1] == K and w.shape[1] == K and (scales is None or scales.numel() == M)
    return _epilogue_operands(who, M, N, codes.device, bias, out, epilogue, gate, residual, fused=fused, alloc=alloc)


def _epilogue_operands(who, M: int, N: int, dev, bias, out, epilogue, gate, residual, fused=False, alloc=False, told=False):
    """The output side of one [M, N] problem of `gemm_fp8` / `gemm_fp8_grouped` / `gemm_mxfp4`: `out` (made here if None and
    `alloc`; not looked at if `fused`), `bias`, and the `gate` / `residual` of gate_res.  Returns (out, flag), flag = the epilogue
    flag of a float `out`, which the entry point rejects with its own message.  `told`: a wrong `out` shape and a missing gate /
    residual raise ApexMIError with a reason (what `gemm_mxfp4` does) instead of failing an assertion."""
    flag = 0
    if not fused:
        if out is None and alloc:
            out = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
        _req(out, None, who + ".out")
        if told and (tuple(out.shape) != (M, N) or out.stride(1) != 1):
            raise _l.ApexMIError(f"{who}.out: expected [{M}, {N}] with contiguous rows, got {tuple(out.shape)}")
        assert out.shape == (M, N) and out.stride(1) == 1
        if out.dtype == torch.float32:
            flag = _l.EPI_F32_IO
        else:
            _req(out, torch.bfloat16, who + ".out")
    if bias is not None:
        _req(bias, torch.bfloat16, who + ".bias")
        assert bias.is_contiguous() and bias.numel() == N
    if epilogue == "gate_res":
        if told and (gate is None or residual is None):
            raise _l.ApexMIError(f"{who}: the gate_res epilogue needs `gate` and `residual`")
        _req(gate, torch.float32, who + ".gate")
        _req(residual, out.dtype, who + ".residual")
        assert gate.is_contiguous() and gate.numel() == N and residual.shape == (M, N) and residual.stride(1) == 1
    return out, flag


def gemm_fp8(codes: torch.Tensor, scales: torch.Tensor, w: "Fp8Weight", bias: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None, epilogue: str = "bias", gate: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, lora_t: Optional[torch.Tensor] = None,
             lora_B: Optional[torch.Tensor] = None, block_scales: Optional[torch.Tensor] = None, out_mx=None):
    """out[M, N] (bf16) = epi((codes . w.q^T) * scales[m] * w.scale[n] + bias): e4m3 x e4m3 with f32 accumulation, both scales
    applied in the f32 epilogue.  `codes` / `scales` as `quant_rows_fp8` returns them; `w` an e4m3 `Fp8Weight` (e5m2 raises);
    epilogue bias / gelu / gate_res.

    `lora_t` [M, Rp] and `lora_B` [N, Rp] (bf16, both or neither, Rp a multiple of 64, row strides free): the run-time LoRA form,
        out = epi(((codes . w.q^T) * scales[m]) * w.scale[n] + sum_r lora_t[m, r] lora_B[n, r] + bias)
    — the scaled base product stays in the f32 accumulators, a bf16 MFMA tail adds the adapter term (rank ascending) into them,
    and the result is rounded once.

    MX forms (not with `lora_t`):
    `block_scales` (uint8 [M, K / 32], `scales` must be None): `codes` carry one e8m0 scale per 32 columns, as
        `quant_blocks_mxfp8` or an `out_mx` launch writes them; the block-scaled MFMA applies them and the epilogue uses
        scales[m] = 1.  All bytes 127 give the bits of `scales = 1`.  Every epilogue takes it.
    `out_mx=(codes_out uint8 [M, N], block_scales_out uint8 [M, N / 32])` (bias / gelu, N % 128 == 0): the launch quantises its
        own output in the epilogue and writes those instead of `out` (which is ignored); bit-identical to the bf16 launch
        followed by `quant_blocks_mxfp8`.  Returns the pair."""
    if (lora_t is None) != (lora_B is None):
        raise _l.ApexMIError("gemm_fp8: lora_t and lora_B go together (both or neither)")
    if lora_t is not None and (block_scales is not None or out_mx is not None):
        raise _l.ApexMIError("gemm_fp8: the run-time LoRA form (lora_t / lora_B) takes per-row scales and writes bf16: "
                             "block_scales / out_mx are not supported with it")
    out, flag = _fp8_problem("gemm_fp8", codes, scales, w, bias, out, epilogue, gate, residual, alloc=True,
                             block_scales=block_scales, out_mx=out_mx)
    (M, K), N = codes.shape, w.shape[0]
    # what every entry point takes: the weight side, and the shape, epilogue and gate_res operands
    wargs = (w.q.data_ptr(), w.q.stride(0), 0 if w.q.dtype == torch.float8_e4m3fn else 1, w.scale.data_ptr(), w.scale.numel(), _ptr(bias))
    tail = (M, N, K, _EPI[epilogue] | flag, _ptr(gate), _ptr(residual), residual.stride(0) if epilogue == "gate_res" else 0)
    if block_scales is not None or out_mx is not None:
        mq, ms = out_mx if out_mx is not None else (None, None)
        rc = _l.load().apexmi_gemm_fp8_mx(
            codes.data_ptr(), codes.stride(0), _ptr(scales), _ptr(block_scales), 0 if block_scales is None else block_scales.stride(0),
            *wargs, None if out_mx is not None else out.data_ptr(), 0 if out_mx is not None else out.stride(0), _ptr(mq),
            0 if mq is None else mq.stride(0), _ptr(ms), 0 if ms is None else ms.stride(0), *tail, _stream())
        _l.check(rc, "gemm_fp8_mx")
        return out_mx if out_mx is not None else out
    args = (codes.data_ptr(), codes.stride(0), scales.data_ptr(), *wargs, out.data_ptr(), out.stride(0), *tail)
    if lora_t is not None:
        _req(lora_t, torch.bfloat16, "gemm_fp8.lora_t")
        _req(lora_B, torch.bfloat16, "gemm_fp8.lora_B")
        assert lora_t.dim() == 2 and lora_B.dim() == 2 and lora_t.stride(1) == 1 and lora_B.stride(1) == 1
        Rp = lora_t.shape[1]
        assert lora_t.shape[0] == M and tuple(lora_B.shape) == (N, Rp)
        rc = _l.load().apexmi_gemm_fp8_lora(*args, lora_t.data_ptr(), lora_t.stride(0), lora_B.data_ptr(), lora_B.stride(0), Rp, _stream())
        _l.check(rc, "gemm_fp8_lora")
        return out
    _l.check(_l.load().apexmi_gemm_fp8(*args, _stream()), "gemm_fp8")
    return out


# ---- opt-in MXFP4 / MXFP6 compute: packed e2m1 / e2m3 codes, one e8m0 scale byte per 32 consecutive k --------------
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)      # the magnitudes of the low three code bits; bit 3 is the sign
# the magnitudes of the low five code bits (exp << 3 | man, bias 1; exp = 0 is man / 8); bit 5 is the sign
E2M3_VALUES = tuple(m / 8 if e == 0 else (1 + m / 8) * 2.0 ** (e - 1) for e in range(4) for m in range(8))


@dataclasses.dataclass(frozen=True)
class _MxFormat:
    """What differs, on the host side, between the MX formats whose two block scales the MFMA applies: one row per format, read
    by the one quantiser body, pair check, weight record, route rule, activation scratch and GEMM wrapper below and by the loop
    in `gemm`.  A new format is one row, its kernel and a record subclass."""
    mode: str                    # the `compute` word of a record that routes
    slot: str                    # the attribute of a weight tensor that carries its record
    bits: int                    # of a code: a row of K codes (whole blocks of 32) is K bits / 8 bytes
    k_mult: int                  # the K multiple of the GEMM route = the codes of one K-tile
    mx_n_mult: Optional[int]     # the N multiple of an MX output (`out_mx`), or None: the GEMM has no MX-output entry point
    values: tuple                # the magnitudes of the codes below the sign bit, which is the top one
    quant: str                   # the public quantiser and GEMM wrapper.  `gemm` calls them by these names, as its callers do;
    gemm: str                    # the library's entry points are "apexmi_" + name, the MX-output one + "_mx"
    name: str                    # the words of the messages: the format,
    record: str                  # its weight record
    cols: str                    # and the bytes of a code row

    def row_bytes(self, K: int) -> int:
        return K * self.bits // 8

    def k_of(self, nbytes: int) -> int:
        return nbytes * 8 // self.bits


_MXFP4 = _MxFormat("fp4", "_fp4", 4, 256, 128, E2M1_VALUES, "quant_blocks_mxfp4", "gemm_mxfp4", "MXFP4", "Mxfp4Weight", "K / 2")
_MXFP6 = _MxFormat("fp6", "_fp6", 6, 128, None, E2M3_VALUES, "quant_blocks_mxfp6", "gemm_mxfp6", "MXFP6", "Mxfp6Weight", "3 K / 4")
_MX_FORMATS = (_MXFP4, _MXFP6)      # the order `gemm` asks them in
_MX_SLOTS = tuple((f.slot, f) for f in _MX_FORMATS)      # what `gemm` walks on every call: no attribute loads for a plain weight


def _empty_mx_codes(fmt: _MxFormat, M: int, K: int, device) -> torch.Tensor:
    """An unwritten codes buffer [M, K bits / 8] whose rows are padded to 16 bytes, the alignment the GEMMs ask of a code row"""
    kb = fmt.row_bytes(K)
    return torch.empty((M, (kb + 15) // 16 * 16), dtype=torch.uint8, device=device)[:, :kb]


def _quant_blocks_mx(fmt: _MxFormat, a, out, scale_out) -> Tuple[torch.Tensor, torch.Tensor]:
    """`quant_blocks_mxfp4` / `quant_blocks_mxfp6`: the argument check, the default `out` (rows padded to 16 bytes), the pair check
    and the launch."""
    who = fmt.quant
    if not isinstance(a, torch.Tensor) or a.dtype != torch.bfloat16:
        raise _l.ApexMIError(f"{who}.a: expected a torch.bfloat16 tensor, got {getattr(a, 'dtype', type(a).__name__)}")
    if a.dim() != 2 or a.stride(1) != 1 or a.shape[1] % 32 != 0 or a.shape[1] < 32 or a.shape[0] < 1:
        raise _l.ApexMIError(f"{who}.a: expected [M >= 1, K % 32 == 0] with contiguous rows, got {tuple(a.shape)}")
    M, K = a.shape
    if out is None:
        out = _empty_mx_codes(fmt, M, K, a.device)
    if scale_out is None:
        scale_out = torch.empty((M, K // 32), dtype=torch.uint8, device=a.device)
    _check_mx_codes(fmt, who + ".out", out, scale_out, M, K)
    _req(a, torch.bfloat16, who + ".a")
    _l.check(getattr(_l.load(), "apexmi_" + who)(a.data_ptr(), a.stride(0), M, K, out.data_ptr(), out.stride(0), scale_out.data_ptr(),
                                                 scale_out.stride(0), _stream()), who)
    return out, scale_out


def quant_blocks_mxfp4(a: torch.Tensor, out: Optional[torch.Tensor] = None,
                       scale_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MXFP4 block quantisation of bf16 `a` [M, K] (row stride free, K % 32 == 0) -> (codes uint8 [M, K / 2]: OCP e2m1, byte j of a
    row = code[2 j] | code[2 j + 1] << 4 as torch's float4_e2m1fn_x2 packs them; scales uint8 [M, K / 32] = e8m0 exponents; row
    strides free, code rows 16-byte aligned).  Per block of 32 consecutive columns:
        amax = max |a| with unbiased f32 exponent E and mantissa bits man;  e = clamp(E - 2 + (man > 0x400000), -126, 127)
        (0 for a zero block);  scale byte = e + 127;  code = e2m1_rne(clamp(a * 2^-e, -6, 6))
    2^e is the smallest power of two with amax / 2^e <= 6, so the clamp clips nothing; ties go to the even code (0.25 -> 0,
    0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4) and the sign bit of `a` is kept, also where the magnitude
    rounds to zero.  Inputs must be finite.  One launch; what `gemm_mxfp4` reads on both sides."""
    return _quant_blocks_mx(_MXFP4, a, out, scale_out)


def quant_blocks_mxfp6(a: torch.Tensor, out: Optional[torch.Tensor] = None,
                       scale_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """MXFP6 block quantisation of bf16 `a` [M, K] (row stride free, K % 32 == 0) -> (codes uint8 [M, 3 K / 4]: OCP e2m3, block b of a
    row = bytes 24 b .. 24 b + 23, code j of the block = bits 6 j .. 6 j + 5 of those bytes as one little-endian integer; scales uint8
    [M, K / 32] = e8m0 exponents; row strides free, code rows 8-byte aligned — 16 for `gemm_mxfp6`, which the default `out` has).  Per
    block of 32 consecutive columns:
        amax = max |a| with unbiased f32 exponent E and mantissa bits man;  e = clamp(E - 2 + (man > 0x700000), -126, 127)
        (0 for a zero block);  scale byte = e + 127;  code = e2m3_rne(clamp(a * 2^-e, -7.5, 7.5))
    2^e is the smallest power of two with amax / 2^e <= 7.5, so the clamp clips nothing; ties go to the even code and the sign bit of
    `a` is kept, also where the magnitude rounds to zero.  Inputs must be finite.  One launch; what `gemm_mxfp6` reads on both sides."""
    return _quant_blocks_mx(_MXFP6, a, out, scale_out)


def _check_mx_codes(fmt: _MxFormat, who: str, q, s, M: int, K: int, on_device: bool = True) -> None:
    """A (codes [M, K bits / 8], scales [M, K / 32]) pair of `fmt`, both uint8 tensors with contiguous rows: type and shape first,
    then (what every launch asks) the device"""
    for name, t, cols in (("codes", q, fmt.row_bytes(K)), ("scales", s, K // 32)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise _l.ApexMIError(f"{who}: the {name} must be a torch.uint8 tensor, got {getattr(t, 'dtype', type(t).__name__)}")
        if t.dim() != 2 or tuple(t.shape) != (M, cols) or t.stride(1) != 1:
            raise _l.ApexMIError(f"{who}: the {name} must be [{M}, {cols}] with contiguous rows (K = {K}), got {tuple(t.shape)}")
        if on_device:
            _req(t, torch.uint8, f"{who} ({name})")


def _unpack_codes(fmt: _MxFormat, q: torch.Tensor) -> torch.Tensor:
    """uint8 [R, K bits / 8] -> the codes int64 [R, K]: bit fields of one little-endian integer, in the smallest groups of whole
    bytes that hold whole codes (e2m1: 2 codes a byte, e2m3: 4 codes per 3 bytes)"""
    g = fmt.bits // math.gcd(fmt.bits, 8)
    b = q.long().view(q.shape[0], -1, g)
    v = sum(b[..., i] << 8 * i for i in range(g))
    return torch.stack([(v >> sh) & ((1 << fmt.bits) - 1) for sh in range(0, 8 * g, fmt.bits)], dim=-1).view(q.shape[0], -1)


class _MxWeight:
    """An MX copy of a bf16 weight [N, K] in the format `fmt` of the subclass: `q` uint8 [N, K bits / 8] codes, `s` uint8 [N, K / 32]
    e8m0 scale bytes, as the format's quantiser writes them.  NOT a ResidentWeight: the bf16 weight stays where it is and the
    record sits beside it, on the weight tensor's `fmt.slot`, where `ops.gemm` looks.  `compute`: `fmt.mode` (routed) or anything
    else (ignored)."""
    fmt: _MxFormat

    def __init__(self, q: torch.Tensor, s: torch.Tensor):
        fmt = self.fmt
        N, K = q.shape[0], fmt.k_of(q.shape[1])
        _check_mx_codes(fmt, fmt.record, q, s, N, K, on_device=False)      # a CPU record can still be asked for its route
        self.q, self.s, self.shape, self.compute = q, s, (N, K), fmt.mode

    @classmethod
    def from_bf16(cls, w: torch.Tensor):
        return cls(*globals()[cls.fmt.quant](w))

    @property
    def device(self):
        return self.q.device

    def nbytes(self) -> int:
        return self.q.numel() + self.s.numel()

    def dequant(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bf16 [N, K] = value(code) x 2^(scale byte - 127): exact in bf16 (at most four significant bits times a power of two) unless
        it overflows, which only a block holding values above 2^127 produces.  Plain torch: test and tool support, not a hot path."""
        fmt, (N, K) = self.fmt, self.shape
        lut = torch.tensor(fmt.values + tuple(-v for v in fmt.values), dtype=torch.float32, device=self.q.device)
        v = lut[_unpack_codes(fmt, self.q)].view(N, K // 32, 32)
        v = (v * torch.exp2(self.s.float() - 127.0).unsqueeze(-1)).view(N, K).to(torch.bfloat16)
        if out is None:
            return v
        _req(out, torch.bfloat16, fmt.record + ".dequant.out")
        out.copy_(v)
        return out


class Mxfp4Weight(_MxWeight):
    """An MXFP4 copy of a bf16 weight [N, K] for the opt-in fp4 compute: `q` uint8 [N, K / 2] e2m1 codes, `s` uint8 [N, K / 32]
    e8m0 scale bytes, as `quant_blocks_mxfp4` writes them.  NOT a ResidentWeight: the bf16 weight stays where it is and this record
    sits beside it (on the weight tensor's `_fp4` slot, where `ops.gemm` looks); 0.53 bytes per weight element.  `compute`: "fp4"
    (routed by `mxfp4_route`) or anything else (ignored)."""
    fmt = _MXFP4


class Mxfp6Weight(_MxWeight):
    """An MXFP6 copy of a bf16 weight [N, K] for the opt-in fp6 compute: `q` uint8 [N, 3 K / 4] e2m3 codes, `s` uint8 [N, K / 32]
    e8m0 scale bytes, as `quant_blocks_mxfp6` writes them.  NOT a ResidentWeight: the bf16 weight stays where it is and this record
    sits beside it (on the weight tensor's `_fp6` slot, where `ops.gemm` looks); 0.78 bytes per weight element.  `compute`: "fp6"
    (routed by `mxfp6_route`) or anything else (ignored)."""
    fmt = _MXFP6

    def __init__(self, q: torch.Tensor, s: torch.Tensor):
        if not isinstance(q, torch.Tensor) or q.dim() != 2 or q.shape[1] % 24 != 0:
            raise _l.ApexMIError(f"Mxfp6Weight: the codes must be a uint8 [N, 3 K / 4] tensor of whole 24-byte blocks, got "
                                 f"{tuple(getattr(q, 'shape', ()))}")
        super().__init__(q, s)


def _mx_of(fmt: _MxFormat, w):
    """The record of `fmt` behind `w` (the record itself, or a weight tensor carrying one in `fmt.slot`), or None."""
    return w if isinstance(w, _MxWeight) and w.fmt is fmt else getattr(w, fmt.slot, None)


def _mxfp4_of(w):
    return _mx_of(_MXFP4, w)


def _mx_route(fmt: _MxFormat, a: torch.Tensor, w, out: Optional[torch.Tensor], epilogue: str) -> bool:
    """`mxfp4_route` / `mxfp6_route`: a record of `fmt` that is switched on, and the shared shape rules with the format's K-tile."""
    f = _mx_of(fmt, w)
    if not isinstance(f, _MxWeight) or f.fmt is not fmt or f.compute != fmt.mode:
        return False
    return _block_gemm_route(a, f.shape, out, epilogue, fmt.k_mult)


def mxfp4_route(a: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias") -> bool:
    """Whether `gemm(a, w, out=out, epilogue=epilogue)` goes out as `quant_blocks_mxfp4` + `gemm_mxfp4`.  Pure: reads dtypes, shapes
    and strides only (CPU tensors are fine).  True only when ALL of these hold:
      * `w` is (or carries in `_fp4`) an `Mxfp4Weight` with `compute == "fp4"`;
      * `a` is bf16 and `out` is bf16 or None (float activations = the f32-storage mode and a float `out` = the f32 residual
        stream keep the bf16 path);
      * the shape is eligible: M >= 1, K % 256 == 0, N % 16 == 0, 16-byte rows of `a`, and the epilogue is one of bias / gelu /
        gate_res."""
    return _mx_route(_MXFP4, a, w, out, epilogue)


def mxfp6_route(a: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias") -> bool:
    """Whether `gemm(a, w, out=out, epilogue=epilogue)` goes out as `quant_blocks_mxfp6` + `gemm_mxfp6`.  Pure: reads dtypes, shapes
    and strides only (CPU and meta tensors are fine).  True only when ALL of these hold:
      * `w` is (or carries in `_fp6`) an `Mxfp6Weight` with `compute == "fp6"`;
      * `a` is bf16 and `out` is bf16 or None (float activations = the f32-storage mode and a float `out` = the f32 residual
        stream keep the bf16 path);
      * the shape is eligible: M >= 1, K % 128 == 0, N % 16 == 0, 16-byte rows of `a`, and the epilogue is one of bias / gelu /
        gate_res."""
    return _mx_route(_MXFP6, a, w, out, epilogue)


_mx_act_scratch: dict = {}      # fmt.mode -> a store of `_stream_scratch`: the formats do not overwrite each other


def _act_scratch_mx(fmt: _MxFormat, dev, M: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-stream home of the activation's codes [M, K bits / 8] and scale bytes [M, K / 32] in `fmt` (as `_act_scratch`)."""
    kb, nb = fmt.row_bytes(K), K // 32
    q, s = _stream_scratch(_mx_act_scratch.setdefault(fmt.mode, {}), dev, (M * kb, torch.uint8), (M * nb, torch.uint8))
    return q[:M * kb].view(M, kb), s[:M * nb].view(M, nb)


def _mx_out_mx(fmt: _MxFormat, who: str, out_mx, M: int, N: int, epilogue: str):
    """The `out_mx` pair of one [M, N] problem of `gemm_mxfp4` / `gemm_mxfp4_grouped(_qkv)`: (codes uint8 [M, N bits / 8], scales
    uint8 [M, N / 32]), bias or gelu, N a multiple of `fmt.mx_n_mult`.  Returns the pair."""
    try:
        mq, ms = out_mx
    except (TypeError, ValueError):
        raise _l.ApexMIError(f"{who}: out_mx: expected a (codes, scales) pair") from None
    if epilogue not in ("bias", "gelu"):
        raise _l.ApexMIError(f"{who}: out_mx exists for the bias and gelu epilogues, not '{epilogue}'")
    if N % fmt.mx_n_mult != 0:
        raise _l.ApexMIError(f"{who}: out_mx needs N % {fmt.mx_n_mult} == 0, got N={N}")
    _check_mx_codes(fmt, who + ".out_mx", mq, ms, M, N)
    return mq, ms


def _gemm_mx(fmt: _MxFormat, codes, scales, w, bias, out, epilogue: str, gate, residual, out_mx=None):
    """`gemm_mxfp4` / `gemm_mxfp6`: one launch of the format's GEMM, or of its MX-output entry point with `out_mx`."""
    who = fmt.gemm
    if out_mx is not None and fmt.mx_n_mult is None:
        raise _l.ApexMIError(f"{who}: out_mx: the {fmt.name} GEMM has no epilogue that quantises its own output (there is no "
                             f"apexmi_{who}_mx entry point)")
    if not isinstance(w, _MxWeight) or w.fmt is not fmt:
        raise _l.ApexMIError(f"{who}: expected an {fmt.record}, got {type(w).__name__}")
    if epilogue not in _FP8_EPI:
        raise _l.ApexMIError(f"{who}: epilogue '{epilogue}' is not one of {_FP8_EPI}")
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2:
        raise _l.ApexMIError(f"{who}: null operand: `codes` must be a uint8 [M, {fmt.cols}] tensor, got {type(codes).__name__}")
    M, (N, K) = codes.shape[0], w.shape
    _check_mx_codes(fmt, who, codes, scales, M, K)
    if out_mx is not None:
        mq, ms = _mx_out_mx(fmt, who, out_mx, M, N, epilogue)
        _epilogue_operands(who, M, N, codes.device, bias, None, epilogue, None, None, fused=True, told=True)
    else:
        out, flag = _epilogue_operands(who, M, N, codes.device, bias, out, epilogue, gate, residual, alloc=True, told=True)
    operands = (codes.data_ptr(), codes.stride(0), scales.data_ptr(), scales.stride(0), w.q.data_ptr(), w.q.stride(0), w.s.data_ptr(),
                w.s.stride(0), _ptr(bias))
    if out_mx is not None:
        rc = getattr(_l.load(), f"apexmi_{who}_mx")(*operands, None, 0, mq.data_ptr(), mq.stride(0), ms.data_ptr(), ms.stride(0), M, N, K,
                                                    _EPI[epilogue], None, None, 0, _stream())
        _l.check(rc, who + "_mx")
        return mq, ms
    rc = getattr(_l.load(), "apexmi_" + who)(*operands, out.data_ptr(), out.stride(0), M, N, K, _EPI[epilogue] | flag, _ptr(gate),
                                             _ptr(residual), residual.stride(0) if epilogue == "gate_res" else 0, _stream())
    _l.check(rc, who)
    return out


def gemm_mxfp4(codes: torch.Tensor, scales: torch.Tensor, w: "Mxfp4Weight", bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, epilogue: str = "bias", gate: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None, out_mx=None):
    """out[M, N] (bf16) = epi(sum_k value(codes[m, k]) 2^(scales[m, k / 32] - 127) value(w.q[n, k]) 2^(w.s[n, k / 32] - 127) + bias):
    e2m1 x e2m1 on the block-scaled MFMA, which applies both scale bytes; f32 accumulation, one bf16 rounding.  `codes` /
    `scales` as `quant_blocks_mxfp4` returns them; `w` an `Mxfp4Weight`; epilogue bias / gelu / gate_res (`residual` may be `out`).
    K % 256 == 0, N % 16 == 0.

    `out_mx=(codes_out uint8 [M, N / 2], scales_out uint8 [M, N / 32])` (bias / gelu, N % 128 == 0; row strides free, multiples of
    4): the launch quantises its own output in the epilogue and writes those instead of `out` (which is ignored); bit-identical
    to the bf16 launch followed by `quant_blocks_mxfp4`.  Returns the pair."""
    return _gemm_mx(_MXFP4, codes, scales, w, bias, out, epilogue, gate, residual, out_mx)


def gemm_mxfp6(codes: torch.Tensor, scales: torch.Tensor, w: "Mxfp6Weight", bias: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, epilogue: str = "bias", gate: Optional[torch.Tensor] = None,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, N] (bf16) = epi(sum_k value(codes[m, k]) 2^(scales[m, k / 32] - 127) value(w.q[n, k]) 2^(w.s[n, k / 32] - 127) + bias):
    e2m3 x e2m3 on the block-scaled MFMA, which applies both scale bytes; f32 accumulation, one bf16 rounding.  `codes` /
    `scales` as `quant_blocks_mxfp6` returns them; `w` an `Mxfp6Weight`; epilogue bias / gelu / gate_res (`residual` may be `out`).
    K % 128 == 0, N % 16 == 0."""
    return _gemm_mx(_MXFP6, codes, scales, w, bias, out, epilogue, gate, residual)


def mxfp4_norm_quant_route(x: torch.Tensor, xn: torch.Tensor, w, out: Optional[torch.Tensor] = None, epilogue: str = "bias") -> bool:
    """Whether the pair `ln_modulate(x, ..., out=xn)` -> `gemm(xn, w, out=out, epilogue=epilogue)` may go out as
    `ln_modulate_quant_mxfp4` -> `gemm(..., quantised_mxfp4=)`: the norm writes the e2m1 codes and scale bytes itself and the
    GEMM's own `quant_blocks_mxfp4` launch disappears.  Pure, like `mxfp4_route` (dtypes, shapes and strides only; CPU tensors
    are fine).  True only when the GEMM takes `mxfp4_route` on `xn` AND the fused norm accepts the pair (`fp8_norm_quant_rows`:
    `x` bf16 or float32 [M, C] with 16-byte rows, `xn` bf16 of the same shape, C % 128 == 0 and C <= 8192).  The fp4 mode has no
    adapter tail, so nothing but the GEMM reads `xn`: the caller stores no bf16 row unless something of its own reads it."""
    return fp8_norm_quant_rows(x, xn) and mxfp4_route(xn, w, out, epilogue)


def mxfp4_mx_route(a_or_shape, w_up, w_down, epilogue_up: str = "gelu", epilogue_down: str = "gate_res",
                   out: Optional[torch.Tensor] = None) -> bool:
    """Whether the pair `h = gemm(a, w_up, epilogue=epilogue_up)` -> `gemm(h, w_down, out=out, epilogue=epilogue_down)` may keep
    `h` in MXFP4 between the two launches: `gemm_mxfp4(out_mx=)` -> `gemm_mxfp4` on that pair.  Pure, like `mxfp4_route`
    (dtypes, shapes and strides; CPU tensors are fine).  `a_or_shape`: the bf16 input [M, K] of the up projection, or its shape.
    True only when BOTH weights carry fp4 records and take `mxfp4_route`, the up epilogue is bias or gelu, N_up % 256 == 0 (the
    down launch's K-tile rule, which includes the MX output's N % 128 == 0), and `out` (the down projection's output and, for
    gate_res, its residual) is bf16 or None."""
    return _updown_route(mxfp4_route, _mxfp4_of, 256, a_or_shape, w_up, w_down, epilogue_up, epilogue_down, out)


def ln_modulate_quant_mxfp4(x: torch.Tensor, scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
                            gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None, eps: float = 1e-6,
                            rms: bool = False, split: int = 0, scale2: Optional[torch.Tensor] = None,
                            shift2: Optional[torch.Tensor] = None, codes: Optional[torch.Tensor] = None,
                            scale_out: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`ln_modulate(x, ...)` into bf16 followed by `quant_blocks_mxfp4` on its output, as ONE launch: -> (codes uint8 [M, C / 2],
    scales uint8 [M, C / 32]), bit-identical to the two launches.  `x` bf16, or float32 (the f32 residual stream); C % 128 == 0.
    `out` (optional, bf16 [M, C], row stride free): also receives the normalised rows, bit-identical to `ln_modulate(x, ...,
    out=out)`; None = the bf16 rows are never stored.  `codes` / `scale_out` (row strides free, code rows 16-byte aligned) default
    to the per-stream activation scratch of `gemm`'s fp4 route, valid until that stream's next fp4 GEMM or fused norm."""
    who = "ln_modulate_quant_mxfp4"
    M, Cc = _norm_quant_operands(who, x, out, scale, shift, scale2, shift2, gamma, beta, told=True)
    if codes is None and scale_out is None:
        codes, scale_out = _act_scratch_mx(_MXFP4, x.device, M, Cc)
    if codes is None:
        codes = _empty_mx_codes(_MXFP4, M, Cc, x.device)
    if scale_out is None:
        scale_out = torch.empty((M, Cc // 32), dtype=torch.uint8, device=x.device)
    _check_mx_codes(_MXFP4, who + ".codes", codes, scale_out, M, Cc)
    rc = _l.load().apexmi_ln_modulate_quant_mxfp4(
        x.data_ptr(), x.stride(0), _l.F32 if x.dtype == torch.float32 else _l.BF16, _ptr(out), 0 if out is None else out.stride(0),
        codes.data_ptr(), codes.stride(0), scale_out.data_ptr(), scale_out.stride(0), M, Cc, _ptr(scale), _ptr(shift), _ptr(gamma),
        _ptr(beta), float(eps), 1 if rms else 0, int(split), _ptr(scale2), _ptr(shift2), _stream())
    _l.check(rc, who)
    return codes, scale_out


FP8_MAX_GROUPS = 4


def _grouped_problems(a_list, w_list, out_list, epilogues):
    """The problems (a, w, out, epilogue) of a grouped launch as its route predicates read them, or None where the lists do not
    describe one: 1 to 4 problems, one weight each, `epilogues` one name or one per problem, `out_list` None or one tensor (or
    None) per problem, and every `a` of the same K."""
    n = len(a_list)
    if not 1 <= n <= FP8_MAX_GROUPS or len(w_list) != n:
        return None
    epis = [epilogues] * n if isinstance(epilogues, str) else list(epilogues)
    outs = [None] * n if out_list is None else list(out_list)
    if len(epis) != n or len(outs) != n or len({a.shape[-1] for a in a_list}) != 1:
        return None
    return list(zip(a_list, w_list, outs, epis))


def fp8_grouped_route(a_list, w_list, out_list=None, epilogues="bias") -> bool:
    """Whether a grouped launch over these problems may go out as quantise + `gemm_fp8_grouped`.  Pure, like `fp8_compute_route`
    (dtypes, shapes and strides only; CPU tensors are fine): true only when EVERY problem satisfies `fp8_compute_route` — a
    launch is all fp8 or all today's path, never mixed — and there are 1 to 4 of them sharing K.  `epilogues`: one name or one
    per problem; `out_list`: None, or one tensor (or None) per problem."""
    problems = _grouped_problems(a_list, w_list, out_list, epilogues)
    return problems is not None and all(fp8_compute_route(a, w, o, e) for a, w, o, e in problems)


def mxfp4_grouped_route(a_list, w_list, out_list=None, epilogues="bias") -> bool:
    """Whether a grouped launch over these problems may go out as ONE `quant_blocks_mxfp4` + `gemm_mxfp4_grouped`.  Pure, like
    `mxfp4_route` (dtypes, shapes and strides only; CPU and meta tensors are fine): true only when EVERY problem satisfies
    `mxfp4_route` — a launch is all fp4 or not routed, never mixed — and there are 1 to 4 of them sharing K.  `epilogues`: one
    name or one per problem; `out_list`: None, or one tensor (or None) per problem.  `gemm_grouped` itself never routes: the
    model asks this predicate, as it asks `fp8_grouped_route`."""
    problems = _grouped_problems(a_list, w_list, out_list, epilogues)
    return problems is not None and all(mxfp4_route(a, w, o, e) for a, w, o, e in problems)


def mxfp4_grouped_mx_route(a_list, w_up_list, w_down_list, epilogues_up="gelu", epilogues_down="gate_res", out_list=None) -> bool:
    """Whether the pair of grouped launches h_i = epi_up(a_i w_up_i^T) -> epi_down(h_i w_down_i^T) may keep every h_i in MXFP4
    between them: `gemm_mxfp4_grouped(out_mx_list=)` -> `gemm_mxfp4_grouped` on those pairs.  Pure, like `mxfp4_grouped_route`.
    True only when both launches take `mxfp4_grouped_route` and every problem takes `mxfp4_mx_route`."""
    n = len(a_list)
    eu = [epilogues_up] * n if isinstance(epilogues_up, str) else list(epilogues_up)
    ed = [epilogues_down] * n if isinstance(epilogues_down, str) else list(epilogues_down)
    outs = list(out_list) if out_list is not None else [None] * n
    if not (len(w_up_list) == len(w_down_list) == len(eu) == len(ed) == len(outs) == n) or not mxfp4_grouped_route(a_list, w_up_list, None, eu):
        return False
    if not all(mxfp4_mx_route(a, wu, wd, e1, e2, o) for a, wu, wd, e1, e2, o in zip(a_list, w_up_list, w_down_list, eu, ed, outs)):
        return False
    hs = [torch.empty((a.shape[0], _mxfp4_of(wu).shape[0]), dtype=torch.bfloat16, device="meta") for a, wu in zip(a_list, w_up_list)]
    return mxfp4_grouped_route(hs, w_down_list, outs, ed)


def fp8_grouped_lora_route(a_list, w_list, out_list=None, epilogues="bias") -> bool:
    """Whether a grouped launch over these problems, some of whose records carry run-time LoRA factors, may go out as skinny
    `gemm_grouped` + quantise + `gemm_fp8_grouped(lora_t_list=, lora_B_list=)`.  Pure, like `fp8_compute_route` (dtypes, shapes and
    strides only; CPU tensors are fine).  True only when EVERY problem satisfies either `fp8_compute_route` (a record without
    factors) or the rules of `fp8_lora_route` without its `lora_buf` condition (an e4m3 record with `compute == "fp8"` AND
    `lora_compute == "fp8"` that carries factors; t lives in a tensor of its own, so no padded activation buffer is needed), AT
    LEAST ONE problem carries factors (otherwise `fp8_grouped_route` is the question), and there are 1 to 4 problems sharing K.  A
    launch is all fp8 or not routed, never mixed."""
    problems = _grouped_problems(a_list, w_list, out_list, epilogues)
    if problems is None:
        return False
    any_lora = False
    for a, w, o, e in problems:
        f8 = _fp8_of(w)
        if isinstance(f8, Fp8Weight) and f8.lora_A is not None:
            any_lora = True
            if not _fp8_lora_problem_route(a, f8, o, e):
                return False
        elif not fp8_compute_route(a, w, o, e):
            return False
    return any_lora


def fp8_mx_route(a_or_shape, w_up, w_down, epilogue_up: str = "gelu", epilogue_down: str = "gate_res",
                 out: Optional[torch.Tensor] = None) -> bool:
    """Whether the pair `h = gemm(a, w_up, epilogue=epilogue_up)` -> `gemm(h, w_down, out=out, epilogue=epilogue_down)` may keep
    `h` in MX fp8 between the two launches: `gemm_fp8(out_mx=)` -> `gemm_fp8(block_scales=)`.  Pure, like `fp8_compute_route`
    (dtypes, shapes and strides; CPU tensors are fine).  `a_or_shape`: the bf16 input [M, K] of the up projection, or its shape.
    True only when BOTH Linears take `fp8_compute_route` (so neither record carries run-time LoRA factors), N_up % 128 == 0, the
    up epilogue is bias or gelu, and `out` (the down projection's output and, for gate_res, its residual) is bf16 or None."""
    return _updown_route(fp8_compute_route, _fp8_of, 128, a_or_shape, w_up, w_down, epilogue_up, epilogue_down, out)


def fp8_grouped_tiles(shapes):
    """The tile each workgroup of a `gemm_fp8_grouped` or `gemm_mxfp4_grouped` launch (the walk does not depend on the operand
    format) over problems `shapes` = [(M, N), ...] computes, restated from the kernels (fp8_group_entry and fp8_tile_origin in
    csrc/fp8_gemm_tile.h): a list over block ids of (problem, tile row, tile column).  The XCD remap runs over the launch's total tile count, the problem is found by the prefix sums of the tile
    counts, and inside a problem bands of 8 tile rows are walked column by column."""
    tm = [(m + 127) // 128 for m, _ in shapes]
    tn = [(n + 127) // 128 for _, n in shapes]
    tile0 = [sum(a * b for a, b in zip(tm[:i], tn[:i])) for i in range(len(shapes))]
    total = sum(a * b for a, b in zip(tm, tn))
    q, r = total >> 3, total & 7
    out = []
    for bid in range(total):
        xcd, idx = bid & 7, bid >> 3
        t = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx
        pi = 0
        for i in range(1, len(shapes)):
            if t >= tile0[i]:
                pi = i
        t -= tile0[pi]
        band = 8 * tn[pi]
        first_m = (t // band) * 8
        gsz = min(tm[pi] - first_m, 8)
        out.append((pi, first_m + (t % band) % gsz, (t % band) // gsz))
    return out


def _fp8_grouped_args(who, codes_list, scales_list, w_list, bias_list, out_list, epilogue, gate_list, residual_list, fused=None,
                      block_scales_list=None, out_mx_list=None):
    """ctypes arrays of a grouped fp8 launch after the per-problem checks (`_fp8_problem`); `fused[i]`: problem i writes no `out`.
    Counts above 4, e5m2 records and float outputs are refused by the entry point with its own message."""
    import ctypes as C
    n = len(codes_list)
    epis = [epilogue] * n if isinstance(epilogue, str) else list(epilogue)
    none = [None] * n
    bias_list, gate_list, residual_list = bias_list or none, gate_list or none, residual_list or none
    fused = fused or [0] * n
    bsl, oml = block_scales_list or none, out_mx_list or none
    fused = [1 if (f or om is not None) else 0 for f, om in zip(fused, oml)]
    K = codes_list[0].shape[1]
    flags = [_fp8_problem(who, qa, sa, w, b, o, e, g, r, K=K, fused=bool(f), block_scales=bs, out_mx=om)[1]
             for qa, sa, w, b, o, e, g, r, f, bs, om in zip(codes_list, scales_list, w_list, bias_list, out_list, epis, gate_list,
                                                            residual_list, fused, bsl, oml)]
    VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
    return (n, VP(*[t.data_ptr() for t in codes_list]), I64(*[t.stride(0) for t in codes_list]),
            VP(*[_ptr(t) for t in scales_list]), VP(*[w.q.data_ptr() for w in w_list]), I64(*[w.q.stride(0) for w in w_list]),
            INT(*[0 if w.q.dtype == torch.float8_e4m3fn else 1 for w in w_list]), VP(*[w.scale.data_ptr() for w in w_list]),
            I64(*[w.scale.numel() for w in w_list]), VP(*[_ptr(b) for b in bias_list]),
            VP(*[None if f else o.data_ptr() for o, f in zip(out_list, fused)]),
            I64(*[0 if f else o.stride(0) for o, f in zip(out_list, fused)]), INT(*[t.shape[0] for t in codes_list]),
            INT(*[w.shape[0] for w in w_list]), K, INT(*[_EPI[e] | fl for e, fl in zip(epis, flags)]),
            VP(*[_ptr(g) if e == "gate_res" else None for g, e in zip(gate_list, epis)]),
            VP(*[_ptr(r) if e == "gate_res" else None for r, e in zip(residual_list, epis)]),
            I64(*[(r.stride(0) if (r is not None and e == "gate_res") else 0) for r, e in zip(residual_list, epis)]))


def _fp8_grouped_lora_args(who, codes_list, w_list, lora_t_list, lora_B_list):
    """ctypes arrays (t, ldt, lb, ldb, Rp) of the grouped LoRA entry points; None entries = no adapter on that problem."""
    import ctypes as C
    n = len(codes_list)
    tl, bl = list(lora_t_list or [None] * n), list(lora_B_list or [None] * n)
    if len(tl) != n or len(bl) != n:
        raise _l.ApexMIError(f"{who}: lora_t_list / lora_B_list must have one entry (or None) per problem")
    rp = []
    for i, (t, b) in enumerate(zip(tl, bl)):
        if (t is None) != (b is None):
            raise _l.ApexMIError(f"{who}: lora_t_list[{i}] and lora_B_list[{i}] go together (both or neither)")
        if t is None:
            rp.append(0)
            continue
        _req(t, torch.bfloat16, f"{who}.lora_t_list[{i}]")
        _req(b, torch.bfloat16, f"{who}.lora_B_list[{i}]")
        assert t.dim() == 2 and b.dim() == 2 and t.stride(1) == 1 and b.stride(1) == 1
        assert t.shape[0] == codes_list[i].shape[0] and tuple(b.shape) == (w_list[i].shape[0], t.shape[1])
        rp.append(int(t.shape[1]))
    VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
    st = lambda ts: I64(*[0 if t is None else t.stride(0) for t in ts])  # noqa: E731
    return VP(*[_ptr(t) for t in tl]), st(tl), VP(*[_ptr(b) for b in bl]), st(bl), INT(*rp)


def gemm_fp8_grouped(codes_list, scales_list, w_list, bias_list, out_list, epilogue="bias", gate_list=None,
                     residual_list=None, block_scales_list=None, out_mx_list=None, lora_t_list=None, lora_B_list=None) -> None:
    """Up to 4 `gemm_fp8` problems sharing K in ONE launch (img / txt streams; QKV + MLP-up of a single block): out_list[i] =
    epi_i((codes_i . w_i.q^T) * scales_i[m] * w_i.scale[n] + bias_i), bit for bit what `gemm_fp8` leaves for that problem alone.
    `epilogue` is one name or one per problem (bias / gelu / gate_res, freely mixed); a gate_res problem may have
    residual_list[i] is out_list[i] (in place).  Several problems may share one (codes, scales) pair or row slices of it.

    `block_scales_list[i]` (then scales_list[i] is None) / `out_mx_list[i]` (then out_list[i] is ignored and may be None): the MX
    forms of `gemm_fp8`, per problem; None entries are ordinary problems, so a launch may mix MX and bf16 outputs.

    `lora_t_list[i]` [M_i, Rp_i] / `lora_B_list[i]` [N_i, Rp_i] (bf16, both or neither per problem, Rp_i a multiple of 64, row strides
    free; not with the MX lists): the run-time LoRA form of `gemm_fp8`, per problem.  None entries are problems without an adapter:
    every problem leaves the bits of its own single launch, `gemm_fp8(lora_t=, lora_B=)` or plain `gemm_fp8`.  At least one
    problem must carry an adapter; with both lists None the call is the plain launch."""
    if lora_t_list is not None or lora_B_list is not None:
        if block_scales_list is not None or out_mx_list is not None:
            raise _l.ApexMIError("gemm_fp8_grouped: the run-time LoRA form (lora_t_list / lora_B_list) takes per-row scales and writes "
                                 "bf16: block_scales_list / out_mx_list are not supported with it")
        args = _fp8_grouped_args("gemm_fp8_grouped", codes_list, scales_list, w_list, bias_list, out_list, epilogue, gate_list,
                                 residual_list)
        largs = _fp8_grouped_lora_args("gemm_fp8_grouped", codes_list, w_list, lora_t_list, lora_B_list)
        _l.check(_l.load().apexmi_gemm_fp8_grouped_lora(*args, *largs, _stream()), "gemm_fp8_grouped_lora")
        return
    args = _fp8_grouped_args("gemm_fp8_grouped", codes_list, scales_list, w_list, bias_list, out_list, epilogue, gate_list,
                             residual_list, block_scales_list=block_scales_list, out_mx_list=out_mx_list)
    n = len(codes_list)
    bsl, oml = list(block_scales_list or [None] * n), list(out_mx_list or [None] * n)
    if any(t is not None for t in bsl + oml):
        import ctypes as C
        VP, I64 = C.c_void_p * n, C.c_int64 * n
        mq, ms = [None if o is None else o[0] for o in oml], [None if o is None else o[1] for o in oml]
        st = lambda ts: I64(*[0 if t is None else t.stride(0) for t in ts])  # noqa: E731
        rc = _l.load().apexmi_gemm_fp8_grouped_mx(*args, VP(*[_ptr(t) for t in bsl]), st(bsl), VP(*[_ptr(t) for t in mq]), st(mq),
                                                  VP(*[_ptr(t) for t in ms]), st(ms), _stream())
        _l.check(rc, "gemm_fp8_grouped_mx")
        return
    _l.check(_l.load().apexmi_gemm_fp8_grouped(*args, _stream()), "gemm_fp8_grouped")


def _qkv_tail_args(who: str, n: int, is_qkv, norm_q, norm_k, row0, H: int, eps: float, rope, qo, ko, vt, told: bool = False) -> tuple:
    """The fused-q/k/v tail of the arguments of `gemm_fp8_grouped_qkv` / `gemm_mxfp4_grouped_qkv` (n problems) after its checks:
    contiguous bf16 qo / ko [H, S_out, 128] and vt [H, 128, Skp], the float32 rope table [2, S_out, 128], bf16 norm weights of 128.
    `told`: a missing output or table and wrong shapes raise ApexMIError with a reason (what the fp4 form does) instead of failing
    an assertion."""
    import ctypes as C
    for name, t_ in (("qo", qo), ("ko", ko), ("vt", vt)):
        if told and not isinstance(t_, torch.Tensor):
            raise _l.ApexMIError(f"{who}: null q/k/v output `{name}`")
        _req(t_, torch.bfloat16, f"{who} output {name}" if told else f"{who} output")
    if told and not isinstance(rope, torch.Tensor):
        raise _l.ApexMIError(f"{who}: null rope table")
    _req(rope, torch.float32, f"{who}.rope")
    S_out = qo.shape[1]
    fits = qo.is_contiguous() and ko.is_contiguous() and vt.is_contiguous() and rope.is_contiguous() \
        and tuple(qo.shape) == tuple(ko.shape) == (H, S_out, 128) and vt.dim() == 3 and tuple(vt.shape[:2]) == (H, 128) \
        and tuple(rope.shape) == (2, S_out, 128)
    if told and not fits:
        raise _l.ApexMIError(f"{who}: expected contiguous qo / ko [{H}, S_out, 128], vt [{H}, 128, Skp] and rope [2, S_out, 128], got "
                             f"{tuple(qo.shape)}, {tuple(ko.shape)}, {tuple(vt.shape)}, {tuple(rope.shape)}")
    assert fits
    none = [None] * n
    for t_ in list(norm_q or none) + list(norm_k or none):
        if t_ is not None:
            _req(t_, torch.bfloat16, f"{who} norm weight")
            assert t_.is_contiguous() and t_.numel() == 128
    VP, INT = C.c_void_p * n, C.c_int * n
    return (INT(*[1 if f else 0 for f in is_qkv]), VP(*[_ptr(t_) for t_ in (norm_q or none)]),
            VP(*[_ptr(t_) for t_ in (norm_k or none)]), INT(*[int(r) for r in row0]), int(H), float(eps), rope.data_ptr(), qo.data_ptr(),
            ko.data_ptr(), vt.data_ptr(), S_out, vt.shape[2])


def gemm_fp8_grouped_qkv(codes_list, scales_list, w_list, bias_list, out_list, epilogue, is_qkv, norm_q, norm_k, row0, H: int,
                         eps: float, rope: torch.Tensor, qo: torch.Tensor, ko: torch.Tensor, vt: torch.Tensor,
                         block_scales_list=None, out_mx_list=None, lora_t_list=None, lora_B_list=None) -> None:
    """`gemm_fp8_grouped` with `qkv_prepare` fused into the epilogue of the problems flagged in `is_qkv` (fused QKV projections,
    N = 3 H 128), mirroring `gemm_grouped_qkv`: q / k leave normalised per head, rotated and laid out [H, S_out, 128], v leaves
    transposed [H, 128, Skp]; bit-identical to gemm_fp8_grouped + qkv_prepare on the same codes (columns >= S_out of `vt` are not
    written).  out_list[i] of a fused problem is ignored (may be None).  Any row count and head count.

    `lora_t_list` / `lora_B_list`: as in `gemm_fp8_grouped` (a fused problem takes the block-diagonal B' of its q | k | v parts);
    bit-identical to gemm_fp8_grouped(lora_t_list=, lora_B_list=) + qkv_prepare."""
    lora = lora_t_list is not None or lora_B_list is not None
    if block_scales_list is not None or out_mx_list is not None:
        raise _l.ApexMIError("gemm_fp8_grouped_qkv: the fused q/k/v epilogue takes per-row scales and writes bf16: "
                             "block_scales_list / out_mx_list are not supported with it")
    n = len(codes_list)
    args = _fp8_grouped_args("gemm_fp8_grouped_qkv", codes_list, scales_list, w_list, bias_list, out_list, epilogue, None, None,
                             fused=[1 if f else 0 for f in is_qkv])
    qargs = _qkv_tail_args("gemm_fp8_grouped_qkv", n, is_qkv, norm_q, norm_k, row0, H, eps, rope, qo, ko, vt)
    if lora:
        largs = _fp8_grouped_lora_args("gemm_fp8_grouped_qkv", codes_list, w_list, lora_t_list, lora_B_list)
        _l.check(_l.load().apexmi_gemm_fp8_grouped_qkv_lora(*args, *qargs, *largs, _stream()), "gemm_fp8_grouped_qkv_lora")
        return
    rc = _l.load().apexmi_gemm_fp8_grouped_qkv(*args, *qargs, _stream())
    _l.check(rc, "gemm_fp8_grouped_qkv")


def _mxfp4_grouped_args(who, codes_list, scales_list, w_list, bias_list, out_list, epilogue, gate_list, residual_list, fused=None,
                        out_mx_list=None):
    """ctypes arrays of a grouped fp4 launch after the per-problem checks (`_check_mx_codes`, `_epilogue_operands`); `fused[i]`:
    problem i writes no `out`.  Every refusal raises ApexMIError with a reason before the library is asked; a float `out` is left
    to the entry point, which rejects it with its own message.  `out_mx_list` (one pair or None per problem): the arrays of the
    _mx entry points, with the four MX arrays behind ldc; a problem with a pair writes no `out`."""
    import ctypes as C
    lists = (codes_list, scales_list, w_list, out_list)
    n = len(codes_list)
    if not 1 <= n <= FP8_MAX_GROUPS or any(len(x) != n for x in lists):
        raise _l.ApexMIError(f"{who}: a launch holds 1 to {FP8_MAX_GROUPS} problems with one codes / scales / weight / out entry each, "
                             f"got {[len(x) for x in lists]}")
    epis = [epilogue] * n if isinstance(epilogue, str) else list(epilogue)
    none = [None] * n
    bias_list, gate_list, residual_list = list(bias_list or none), list(gate_list or none), list(residual_list or none)
    fused = list(fused or [0] * n)
    if any(len(x) != n for x in (epis, bias_list, gate_list, residual_list, fused)):
        raise _l.ApexMIError(f"{who}: one epilogue name, or one per problem, and one bias / gate / residual entry (or None) per problem")
    mx = none
    if out_mx_list is not None:
        mx = list(out_mx_list)
        if len(mx) != n:
            raise _l.ApexMIError(f"{who}: out_mx_list takes one (codes, scales) pair or None per problem")
        for i, (om, f) in enumerate(zip(mx, fused)):
            if om is not None and f:
                raise _l.ApexMIError(f"{who}: problem {i}: a fused q/k/v problem writes q / k / V^T and takes no out_mx")
        fused = [1 if (f or om is not None) else 0 for f, om in zip(fused, mx)]
    for i, (w, e) in enumerate(zip(w_list, epis)):
        if not isinstance(w, Mxfp4Weight):
            raise _l.ApexMIError(f"{who}: problem {i}: expected an Mxfp4Weight, got {type(w).__name__}")
        if e not in _FP8_EPI:
            raise _l.ApexMIError(f"{who}: problem {i}: epilogue '{e}' is not one of {_FP8_EPI}")
    K = w_list[0].shape[1]
    if any(w.shape[1] != K for w in w_list):
        raise _l.ApexMIError(f"{who}: the problems of a launch share K, got {[w.shape[1] for w in w_list]}")
    flags = []
    for i, (q, s, w, b, o, e, g, r, f) in enumerate(zip(codes_list, scales_list, w_list, bias_list, out_list, epis, gate_list,
                                                        residual_list, fused)):
        at = f"{who} (problem {i})"
        if not isinstance(q, torch.Tensor) or q.dim() != 2:
            raise _l.ApexMIError(f"{at}: null operand: `codes` must be a uint8 [M, K / 2] tensor, got {type(q).__name__}")
        _check_mx_codes(_MXFP4, at, q, s, q.shape[0], K)
        if mx[i] is not None:
            mx[i] = _mx_out_mx(_MXFP4, at, mx[i], q.shape[0], w.shape[0], e)
        flags.append(_epilogue_operands(at, q.shape[0], w.shape[0], q.device, b, o, e, g, r, fused=bool(f), told=True)[1])
    VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
    mx_args = ()
    if out_mx_list is not None:
        mx_args = (VP(*[None if om is None else om[0].data_ptr() for om in mx]), I64(*[0 if om is None else om[0].stride(0) for om in mx]),
                   VP(*[None if om is None else om[1].data_ptr() for om in mx]), I64(*[0 if om is None else om[1].stride(0) for om in mx]))
    return (n, VP(*[t.data_ptr() for t in codes_list]), I64(*[t.stride(0) for t in codes_list]),
            VP(*[t.data_ptr() for t in scales_list]), I64(*[t.stride(0) for t in scales_list]),
            VP(*[w.q.data_ptr() for w in w_list]), I64(*[w.q.stride(0) for w in w_list]),
            VP(*[w.s.data_ptr() for w in w_list]), I64(*[w.s.stride(0) for w in w_list]), VP(*[_ptr(b) for b in bias_list]),
            VP(*[None if f else o.data_ptr() for o, f in zip(out_list, fused)]),
            I64(*[0 if f else o.stride(0) for o, f in zip(out_list, fused)]), *mx_args, INT(*[t.shape[0] for t in codes_list]),
            INT(*[w.shape[0] for w in w_list]), K, INT(*[_EPI[e] | fl for e, fl in zip(epis, flags)]),
            VP(*[_ptr(g) if e == "gate_res" else None for g, e in zip(gate_list, epis)]),
            VP(*[_ptr(r) if e == "gate_res" else None for r, e in zip(residual_list, epis)]),
            I64(*[(r.stride(0) if e == "gate_res" else 0) for r, e in zip(residual_list, epis)]))


def gemm_mxfp4_grouped(codes_list, scales_list, w_list, bias_list, out_list, epilogue="bias", gate_list=None,
                       residual_list=None, out_mx_list=None) -> None:
    """Up to 4 `gemm_mxfp4` problems sharing K in ONE launch (img / txt streams; QKV + MLP-up of a single block): out_list[i] =
    epi_i(codes_i x w_list[i] + bias_i) with both block scales applied by the MFMA, bit for bit what `gemm_mxfp4` leaves for that
    problem alone.  `w_list` holds `Mxfp4Weight`s; `epilogue` is one name or one per problem (bias / gelu / gate_res, freely
    mixed); a gate_res problem may have residual_list[i] is out_list[i] (in place).  Several problems may share one (codes,
    scales) pair or row slices of it.  Refusals raise ApexMIError with a reason and write nothing.
    `out_mx_list` (one `gemm_mxfp4(out_mx=)` pair or None per problem): a problem with a pair leaves as MXFP4 codes and scale
    bytes instead of out_list[i] (ignored, may be None), bit for bit `gemm_mxfp4(out_mx=)` alone; MX and bf16 outputs may be
    mixed in one launch."""
    who = "gemm_mxfp4_grouped"
    args = _mxfp4_grouped_args(who, codes_list, scales_list, w_list, bias_list, out_list, epilogue, gate_list, residual_list,
                               out_mx_list=out_mx_list)
    if out_mx_list is not None:
        _l.check(_l.load().apexmi_gemm_mxfp4_grouped_mx(*args, _stream()), who + "_mx")
        return
    _l.check(_l.load().apexmi_gemm_mxfp4_grouped(*args, _stream()), who)


def gemm_mxfp4_grouped_qkv(codes_list, scales_list, w_list, bias_list, out_list, epilogue, is_qkv, norm_q, norm_k, row0, H: int,
                           eps: float, rope: torch.Tensor, qo: torch.Tensor, ko: torch.Tensor, vt: torch.Tensor,
                           out_mx_list=None) -> None:
    """`gemm_mxfp4_grouped` with `qkv_prepare` fused into the epilogue of the problems flagged in `is_qkv` (fused QKV projections,
    N = 3 H 128), mirroring `gemm_fp8_grouped_qkv`: q / k leave normalised per head, rotated and laid out [H, S_out, 128], v leaves
    transposed [H, 128, Skp]; bit-identical to gemm_mxfp4_grouped + qkv_prepare on the same codes (columns >= S_out of `vt` are not
    written).  out_list[i] of a fused problem is ignored (may be None).  Any row count and head count.  `out_mx_list`: as
    `gemm_mxfp4_grouped`, for the problems that are not fused q/k/v (a fused problem with a pair raises)."""
    who = "gemm_mxfp4_grouped_qkv"
    n = len(codes_list)
    if len(is_qkv) != n or len(row0) != n:
        raise _l.ApexMIError(f"{who}: is_qkv and row0 take one entry per problem")
    args = _mxfp4_grouped_args(who, codes_list, scales_list, w_list, bias_list, out_list, epilogue, None, None,
                               fused=[1 if f else 0 for f in is_qkv], out_mx_list=out_mx_list)
    qargs = _qkv_tail_args(who, n, is_qkv, norm_q, norm_k, row0, H, eps, rope, qo, ko, vt, told=True)
    if out_mx_list is not None:
        _l.check(_l.load().apexmi_gemm_mxfp4_grouped_qkv_mx(*args, *qargs, _stream()), who + "_mx")
        return
    _l.check(_l.load().apexmi_gemm_mxfp4_grouped_qkv(*args, *qargs, _stream()), who)


_EPI = {"bias": _l.EPI_BIAS, "gelu": _l.EPI_BIAS_GELU, "gate_res": _l.EPI_BIAS_GATE_RES,
        "gelu_erf": _l.EPI_BIAS_GELU_ERF, "silu": _l.EPI_BIAS_SILU, "quick_gelu": _l.EPI_BIAS_QUICK_GELU}


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, epilogue: str = "bias",
         gate: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
         lora_buf: Optional[torch.Tensor] = None,
         quantised: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, out_mx=None,
         quantised_mxfp4: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, out_mxfp4=None) -> torch.Tensor:
    """out[M,N] = epi(a[M,K] @ w[N,K]^T + bias).  2-D operands, last dim contiguous; a / out / residual bf16, or float32
    in the f32-storage verification mode (w and bias stay bf16).  A bf16 `a` with a float32 `out` (and `residual`) is the
    f32 RESIDUAL STREAM: the same launch with the float epilogue, no split of `a`.  `lora_buf`: see _gemm_fp8_lora (ignored
    unless `w` is a resident-fp8 weight with run-time LoRA factors).

    OPT-IN FP8 COMPUTE: a resident e4m3 `Fp8Weight` with `compute == "fp8"` takes `quant_rows_fp8` (codes and
    scales in a per-stream scratch) + `gemm_fp8` instead of dequantise + bf16 GEMM when `fp8_compute_route` says so.  Today's
    path, unchanged, is taken by everything else: `compute == "bf16"` (the default), run-time LoRA factors attached (unless the
    record also has `lora_compute == "fp8"` and `fp8_lora_route` says so: then the fp8 GEMM runs with the adapter tail), e5m2
    weights, GGUF records, float activations (the f32-storage mode), a float `out` (the f32 residual stream), K not a multiple
    of 128 or N not a multiple of 16, and epilogues other than bias / gelu / gate_res.  `gemm_grouped` never routes.

    `quantised=(codes, scales)`: the activations of the fp8 route ALREADY quantised — what `quant_rows_fp8(a)` would return, as
    `ln_modulate_quant_fp8` produces it in the norm's own launch — so the route skips its quantise launch.  With
    `fp8_compute_route` only the shape and dtype of `a` are read (the norm may not have stored its rows at all); with
    `fp8_lora_route` the skinny GEMM still reads the bf16 `a`.  The caller decides BEFOREHAND with `fp8_norm_quant_route`: a call
    whose GEMM takes neither route raises instead of quietly multiplying an `a` that may never have been written.

    `out_mx=(codes, block_scales)`: the fp8 route writes its output as MX codes and block scales (`gemm_fp8(out_mx=)`) instead of
    `out`, and returns the pair.  The caller decides beforehand with `fp8_mx_route`; any other route raises.

    OPT-IN MXFP4 COMPUTE: a bf16 weight that carries an `Mxfp4Weight` with `compute == "fp4"` in its `_fp4` slot
    (`set_fp4_compute` of the model attaches it) takes `quant_blocks_mxfp4` (codes and scale bytes in a per-stream scratch) +
    `gemm_mxfp4` when `mxfp4_route` says so, asked before everything above.  A weight without the slot never reaches that code.
    `quantised_mxfp4=(codes, scales)`: the activations of that route ALREADY quantised — what `quant_blocks_mxfp4(a)` would
    return, as `ln_modulate_quant_mxfp4` or an `out_mxfp4` launch produces it — so the route skips its quantise launch and reads
    only the shape and dtype of `a`.  `out_mxfp4=(codes, scales)`: the route writes its output as MXFP4 (`gemm_mxfp4(out_mx=)`)
    instead of `out`, and returns the pair.  The caller decides beforehand with `mxfp4_norm_quant_route` / `mxfp4_mx_route`; a
    call that passes either and does not take the fp4 route raises.

    OPT-IN MXFP6 COMPUTE: the same with an `Mxfp6Weight` (`compute == "fp6"`) in the weight's `_fp6` slot
    (`set_fp6_compute`), `quant_blocks_mxfp6` + `gemm_mxfp6` and `mxfp6_route`.  A weight carries at most one of the two slots
    (the models' switches see to it); `gemm_grouped` routes neither."""
    _req_act(a, "gemm.a")
    fmt = None
    for slot, f in _MX_SLOTS:
        if getattr(w, slot, None) is not None and _mx_route(f, a, w, out, epilogue):
            fmt = f
            break
    if (quantised_mxfp4 is not None or out_mxfp4 is not None) and fmt is not _MXFP4:
        raise _l.ApexMIError("gemm: `quantised_mxfp4` / `out_mxfp4` were passed but this call does not take the MXFP4 route "
                             "(mxfp4_route is False): decide with mxfp4_norm_quant_route / mxfp4_mx_route first")
    if fmt is not None:
        if quantised is not None or out_mx is not None:
            raise _l.ApexMIError(f"gemm: `quantised` / `out_mx` belong to the fp8 route, and this call takes the {fmt.name} route (the "
                                 f"weight carries an {fmt.record}): e4m3 codes are not {fmt.mode} operands")
        public = globals()      # the wrappers by their public names, as a caller (or a test that counts calls) sees them
        if quantised_mxfp4 is not None:
            qa, sa = quantised_mxfp4
            _check_mx_codes(fmt, "gemm.quantised_mxfp4", qa, sa, a.shape[0], a.shape[1])
        else:
            qa, sa = _act_scratch_mx(fmt, a.device, a.shape[0], a.shape[1])
            public[fmt.quant](a, out=qa, scale_out=sa)
        if out_mxfp4 is not None:
            return public[fmt.gemm](qa, sa, getattr(w, fmt.slot), bias, epilogue=epilogue, out_mx=out_mxfp4)
        return public[fmt.gemm](qa, sa, getattr(w, fmt.slot), bias, out=out, epilogue=epilogue, gate=gate, residual=residual)
    f8 = _fp8_of(w)
    if f8 is not None and getattr(f8, "compute", "bf16") == "fp8" and fp8_compute_route(a, f8, out, epilogue):
        qa, sa = _fp8_acts(a, quantised)
        if out_mx is not None:
            return gemm_fp8(qa, sa, f8, bias, epilogue=epilogue, out_mx=out_mx)
        return gemm_fp8(qa, sa, f8, bias, out=out, epilogue=epilogue, gate=gate, residual=residual)
    if out_mx is not None:
        raise _l.ApexMIError("gemm: `out_mx` was passed but this call does not take the fp8 route (fp8_compute_route is False): "
                             "decide with fp8_mx_route first")
    if quantised is not None and not (f8 is not None and f8.lora_A is not None and fp8_lora_route(a, f8, out, epilogue, lora_buf)):
        raise _l.ApexMIError("gemm: `quantised` activations were passed but this call does not take the fp8 route "
                             "(fp8_compute_route / fp8_lora_route are both False): decide with fp8_norm_quant_route first")
    if f8 is not None and f8.lora_A is not None:
        if fp8_lora_route(a, f8, out, epilogue, lora_buf):
            K, Rp = a.shape[1], f8.lora_A.shape[0]
            t = lora_buf[:, K:K + Rp]
            gemm(a, f8.lora_A, None, out=t)                      # t = a A^T in bf16, as _gemm_fp8_lora produces it
            qa, sa = _fp8_acts(a, quantised)
            return gemm_fp8(qa, sa, f8, bias, out=out, epilogue=epilogue, gate=gate, residual=residual, lora_t=t, lora_B=f8.lora_B)
        return _gemm_fp8_lora(a, f8, bias, out, epilogue, gate, residual, lora_buf)
    w = _bf16_weight(w, a.dtype == torch.float32)
    _req(w, torch.bfloat16, "gemm.w")
    assert a.dim() == 2 and w.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K
    act = a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=act, device=a.device)
    else:
        assert out.shape == (M, N) and out.stride(1) == 1
    f32_out = act == torch.bfloat16 and out.dtype == torch.float32      # f32 residual stream: bf16 operand, float C / R
    if not f32_out:
        _req(out, act, "gemm.out")
    if bias is not None:
        _req(bias, torch.bfloat16, "gemm.bias")
        assert bias.is_contiguous() and bias.numel() == N
    ldr = 0
    if epilogue == "gate_res":
        _req(gate, torch.float32, "gemm.gate")
        _req(residual, out.dtype, "gemm.residual")
        assert gate.is_contiguous() and gate.numel() == N
        assert residual.shape == (M, N) and residual.stride(1) == 1
        ldr = residual.stride(0)
    epi = _EPI[epilogue]
    if f32_out:
        epi |= _l.EPI_F32_IO
    elif act == torch.float32:     # exact bf16 split of the activations against [w | w | w]: same kernel, float epilogue
        a, w, K, epi = split3(a), _w3(w), 3 * K, epi | _l.EPI_F32_IO
    rc = _l.load().apexmi_gemm_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), _ptr(bias),
                                    out.data_ptr(), out.stride(0), M, N, K, epi,
                                    _ptr(gate), _ptr(residual), ldr, _stream())
    _l.check(rc, "gemm_bf16")
    return out


def gemm_grouped(a_list, w_list, bias_list, out_list, epilogue="bias", gate_list=None,
                 residual_list=None) -> None:
    """Several gemm() problems sharing K in one launch (img/txt streams; QKV + MLP-up of a single
    block).  `epilogue` is one name or a list with one name per problem."""
    import ctypes as C
    n = len(a_list)
    K = w_list[0].shape[1]
    epis = [epilogue] * n if isinstance(epilogue, str) else list(epilogue)
    act = a_list[0].dtype
    # resident fp8 weights: the problems of one launch need their dequantised operands side by side — carved out of ONE per-stream
    # scratch (stream order makes the reuse safe, see _bf16_weight); a weight with run-time LoRA factors has no grouped form
    f8s = [_fp8_of(w) for w in w_list]
    if any(f is not None for f in f8s):
        if any(f is not None and f.lora_A is not None for f in f8s):
            raise _l.ApexMIError("gemm_grouped: a resident-fp8 weight carries run-time LoRA factors: only gemm(..., lora_buf=) applies them")
        if act == torch.float32:     # verification mode caches on (data_ptr, version): never hand it a recycled buffer
            w_list = [w if f is None else f.dequant() for w, f in zip(w_list, f8s)]
        else:
            sizes = [0 if f is None else (f.shape[0] * f.shape[1] + 7) // 8 * 8 for f in f8s]
            dev = next(f for f in f8s if f is not None).device
            buf, off, ws = _scratch(dev, sum(sizes)), 0, []
            for w, f, sz in zip(w_list, f8s, sizes):      # (not `n`: that is the problem count the launch below takes)
                ws.append(w if f is None else f.dequant(out=buf[off:off + f.shape[0] * f.shape[1]].view(f.shape[0], f.shape[1])))
                off += sz
            w_list = ws
    # bf16 operands with float outputs (and residuals): the f32 residual stream (see gemm)
    f32_out = act == torch.bfloat16 and out_list[0].dtype == torch.float32
    odt = torch.float32 if f32_out else act
    for a, w, o in zip(a_list, w_list, out_list):
        _req_act(a, "gemm_grouped.a")
        _req(a, act, "gemm_grouped.a")
        _req(w, torch.bfloat16, "gemm_grouped.w")
        _req(o, odt, "gemm_grouped.out")
        assert a.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and o.stride(1) == 1
        assert w.shape[1] == K and a.shape[1] == K and o.shape == (a.shape[0], w.shape[0])
    VP = C.c_void_p * n
    I64 = C.c_int64 * n
    INT = C.c_int * n
    none = [None] * n
    bias_list = bias_list or none
    gate_list = gate_list or none
    residual_list = residual_list or none
    for e, g, r, o, w in zip(epis, gate_list, residual_list, out_list, w_list):
        if e == "gate_res":
            _req(g, torch.float32, "gemm_grouped.gate")
            _req(r, odt, "gemm_grouped.residual")
            assert g.is_contiguous() and g.numel() == w.shape[0] and r.shape == o.shape and r.stride(1) == 1
    flag = _l.EPI_F32_IO if f32_out else 0
    if act == torch.float32:     # f32-storage verification mode (see gemm)
        done: dict = {}
        sp = []
        for a in a_list:         # problems that read the same activations share one split
            k_ = (a.data_ptr(), tuple(a.shape), a.stride(0))
            if k_ not in done:
                done[k_] = split3(a)
            sp.append(done[k_])
        a_list, w_list, K, flag = sp, [_w3(w) for w in w_list], 3 * K, _l.EPI_F32_IO
    rc = _l.load().apexmi_gemm_bf16_grouped(
        n, VP(*[a.data_ptr() for a in a_list]), I64(*[a.stride(0) for a in a_list]),
        VP(*[w.data_ptr() for w in w_list]), I64(*[w.stride(0) for w in w_list]),
        VP(*[_ptr(b) for b in bias_list]), VP(*[o.data_ptr() for o in out_list]),
        I64(*[o.stride(0) for o in out_list]), INT(*[a.shape[0] for a in a_list]),
        INT(*[w.shape[0] for w in w_list]), K, INT(*[_EPI[e] | flag for e in epis]),
        VP(*[_ptr(g) for g in gate_list]), VP(*[_ptr(r) for r in residual_list]),
        I64(*[(r.stride(0) if r is not None else 0) for r in residual_list]), _stream())
    _l.check(rc, "gemm_bf16_grouped")


def qkv_fusable(a_list, w_list, row0, H: int) -> bool:
    """Would gemm_grouped_qkv() take this launch?  (bf16 storage, an even head count, the 256x256 16x16x32 tiling.)"""
    if H % 2 or any(a.dtype != torch.bfloat16 and not (_shipped_verify and a.dtype == torch.float32) for a in a_list):
        return False
    return bool(_l.load().apexmi_gemm_qkv_fusable(sum(a.shape[0] for a in a_list), max(w.shape[0] for w in w_list),
                                                  w_list[0].shape[1]))


def gemm_grouped_qkv(a_list, w_list, bias_list, out_list, epilogue, is_qkv, norm_q, norm_k, row0, H: int, eps: float,
                     rope: torch.Tensor, qo: torch.Tensor, ko: torch.Tensor, vt: torch.Tensor) -> None:
    """gemm_grouped() with qkv_prepare() fused into the epilogue of the problems flagged in `is_qkv` (fused QKV projections,
    N = 3 H 128): q / k leave normalised per head, rotated and laid out [H, S_out, 128], v leaves transposed [H, 128, Skp];
    bit-identical to gemm_grouped + qkv_prepare.  out_list[i] of a fused problem is ignored (may be None).  bf16 storage only;
    raises (apexmi error) when the launch would not run on the 256x256 16x16x32 tiling — callers keep the two-pass path then."""
    import ctypes as C
    n = len(a_list)
    K = w_list[0].shape[1]
    epis = [epilogue] * n if isinstance(epilogue, str) else list(epilogue)
    if _shipped_verify and any(a.dtype == torch.float32 for a in a_list):
        # verification through the shipped kernels: the fused problems take the bf16 rounding of their float operand (the value
        # production stores there) and leave bf16 q / k / v^T; problems that ride along (the single block's MLP-up) keep the
        # float path, as their own launch
        none_ = [None] * n
        bl, nq_, nk_ = bias_list or none_, norm_q or none_, norm_k or none_
        keep = [i for i in range(n) if is_qkv[i]]
        for i in range(n):
            if not is_qkv[i]:
                gemm(a_list[i], w_list[i], bl[i], out=out_list[i], epilogue=epis[i])
        sel = lambda lst: [lst[i] for i in keep]          # noqa: E731
        return gemm_grouped_qkv([to_bf16(a.contiguous()) if a.dtype == torch.float32 else a for a in sel(a_list)], sel(w_list),
                                sel(bl), [None] * len(keep), sel(epis), [1] * len(keep), sel(nq_), sel(nk_), sel(list(row0)), H, eps,
                                rope, qo, ko, vt)
    for a, w, o, f in zip(a_list, w_list, out_list, is_qkv):
        _req(a, torch.bfloat16, "gemm_grouped_qkv.a")
        _req(w, torch.bfloat16, "gemm_grouped_qkv.w")
        assert a.dim() == 2 and a.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K and a.shape[1] == K
        if not f:
            _req(o, torch.bfloat16, "gemm_grouped_qkv.out")
            assert o.stride(1) == 1 and o.shape == (a.shape[0], w.shape[0])
    for t_ in (qo, ko, vt):
        _req(t_, torch.bfloat16, "gemm_grouped_qkv output")
        assert t_.is_contiguous()
    _req(rope, torch.float32, "gemm_grouped_qkv.rope")
    S_out = qo.shape[1]
    assert qo.shape == ko.shape == (H, S_out, 128) and vt.shape[:2] == (H, 128) and rope.is_contiguous()
    assert rope.shape == (2, S_out, 128)
    VP = C.c_void_p * n
    I64 = C.c_int64 * n
    INT = C.c_int * n
    none = [None] * n
    bias_list = bias_list or none
    pairs = rope_pairs(rope)
    rc = _l.load().apexmi_gemm_bf16_grouped_qkv_pairs(
        n, VP(*[a.data_ptr() for a in a_list]), I64(*[a.stride(0) for a in a_list]),
        VP(*[w.data_ptr() for w in w_list]), I64(*[w.stride(0) for w in w_list]), VP(*[_ptr(b) for b in bias_list]),
        VP(*[_ptr(o) if not f else None for o, f in zip(out_list, is_qkv)]),
        I64(*[(o.stride(0) if (o is not None and not f) else 0) for o, f in zip(out_list, is_qkv)]),
        INT(*[a.shape[0] for a in a_list]), INT(*[w.shape[0] for w in w_list]), K, INT(*[_EPI[e] for e in epis]),
        INT(*[1 if f else 0 for f in is_qkv]), VP(*[_ptr(t_) for t_ in (norm_q or none)]), VP(*[_ptr(t_) for t_ in (norm_k or none)]),
        INT(*[int(r) for r in row0]), int(H), float(eps), rope.data_ptr(), _ptr(pairs), qo.data_ptr(), ko.data_ptr(), vt.data_ptr(),
        S_out, vt.shape[2], _stream())
    _l.check(rc, "gemm_bf16_grouped_qkv")


rope_pairs_enabled = True      # A/B switch (tests, tools): False = the fused epilogue reads the full [2, S, 128] table


def rope_pairs(rope: torch.Tensor, trusted: bool = False) -> Optional[torch.Tensor]:
    """The compact copy [2, S, D / 2] of a rotary table whose entries come in equal pairs (apexmi_rope_table_axes writes every
    cos / sin twice), made ONCE per table (cached on the tensor; tables are cached per geometry by the models) — the fused q/k/v
    epilogue prefetches its rows from it.  None for a table that is not pair-duplicated (checked on the device, one host read per
    table).  `trusted`: the caller made the table with `rope_table_axes` (pairs by construction): no check, no host read — the
    models pass it, so a table rebuilt per call (ids that are inference tensors) costs one more small launch, not a sync."""
    if not rope_pairs_enabled:
        return None
    key = (rope.data_ptr(), tensor_version(rope))
    hit = getattr(rope, "_apex_pairs", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    _req(rope, torch.float32, "rope_pairs.rope")
    assert rope.dim() == 3 and rope.shape[0] == 2 and rope.is_contiguous() and rope.shape[2] % 2 == 0
    S, D = rope.shape[1], rope.shape[2]
    out = torch.empty((2, S, D // 2), dtype=torch.float32, device=rope.device)
    bad = torch.zeros((), dtype=torch.int32, device=rope.device)
    _l.check(_l.load().apexmi_rope_pairs(rope.data_ptr(), S, D, out.data_ptr(), bad.data_ptr(), _stream()), "rope_pairs")
    res = out if (trusted or int(bad.item()) == 0) else None
    try:
        rope._apex_pairs = (key, res)
    except Exception:
        pass
    return res


def gemv(w: torch.Tensor, x: torch.Tensor, bias: Optional[torch.Tensor] = None,
         out: Optional[torch.Tensor] = None, pre_silu: bool = False, post: Optional[str] = None,
         accum: bool = False) -> torch.Tensor:
    """y[M,N] (f32) = post(pre(x[M,K] f32) @ w[N,K]^T (bf16) + bias)."""
    _req(w, torch.bfloat16, "gemv.w")
    _req(x, torch.float32, "gemv.x")
    assert w.dim() == 2 and w.stride(1) == 1 and x.dim() == 2 and x.stride(1) == 1
    M, K = x.shape
    N = w.shape[0]
    assert w.shape[1] == K
    if out is None:
        assert not accum
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    else:
        _req(out, torch.float32, "gemv.out")
        assert out.shape == (M, N) and out.stride(1) == 1
    if bias is not None:
        _req(bias, torch.bfloat16, "gemv.bias")
    flags = 0
    if pre_silu:
        flags |= _l.GEMV_PRE_SILU
    if post == "silu":
        flags |= _l.GEMV_POST_SILU
    elif post == "gelu":
        flags |= _l.GEMV_POST_GELU
    elif post is not None:
        raise ValueError(post)
    if accum:
        flags |= _l.GEMV_ACCUM
    rc = _l.load().apexmi_gemv(w.data_ptr(), w.stride(0), _ptr(bias), x.data_ptr(), x.stride(0),
                               out.data_ptr(), out.stride(0), M, N, K, flags, _stream())
    _l.check(rc, "gemv")
    return out


def ln_modulate(x: torch.Tensor, scale: Optional[torch.Tensor] = None,
                shift: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                gamma: Optional[torch.Tensor] = None, beta: Optional[torch.Tensor] = None,
                eps: float = 1e-6, rms: bool = False, split: int = 0,
                scale2: Optional[torch.Tensor] = None, shift2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = LayerNorm(x) [*gamma + beta] * (1 + scale) + shift, or RMSNorm(x) * gamma.
    Rows [0, split) use (scale2, shift2) instead (text rows of a joint buffer).  `out` has x's dtype, or is bf16 for a
    float32 x (the f32 residual stream feeding a bf16 GEMM operand: apexmi_ln_modulate2_f32in)."""
    _req_act(x, "ln_modulate.x")
    assert x.dim() == 2 and x.stride(1) == 1
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=x.dtype, device=x.device)
    else:
        assert out.shape == (M, Cc) and out.stride(1) == 1
    f32in = x.dtype == torch.float32 and out.dtype == torch.bfloat16
    if not f32in:
        _req(out, x.dtype, "ln_modulate.out")
    for t, nm in ((scale, "scale"), (shift, "shift"), (scale2, "scale2"), (shift2, "shift2")):
        if t is not None:
            _req(t, torch.float32, "ln_modulate." + nm)
            assert t.is_contiguous() and t.numel() == Cc
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        if t is not None:
            _req(t, torch.bfloat16, "ln_modulate." + nm)
            assert t.is_contiguous() and t.numel() == Cc
    fn = _l.load().apexmi_ln_modulate2_f32in if f32in else _fn("apexmi_ln_modulate2", x)
    rc = fn(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), M, Cc,
            _ptr(scale), _ptr(shift), _ptr(gamma), _ptr(beta), float(eps),
            1 if rms else 0, int(split), _ptr(scale2), _ptr(shift2), _stream())
    _l.check(rc, "ln_modulate")
    return out


def qkv_prepare(q: torch.Tensor, k: torch.Tensor, v: Optional[torch.Tensor], H: int,
                qo: torch.Tensor, ko: torch.Tensor, vt: Optional[torch.Tensor],
                wq: Optional[torch.Tensor] = None, wk: Optional[torch.Tensor] = None,
                wq2: Optional[torch.Tensor] = None, wk2: Optional[torch.Tensor] = None,
                split: int = 0, eps: float = 1e-6, rope: Optional[torch.Tensor] = None,
                rope_mode: int = _l.ROPE_NONE, row0: int = 0) -> None:
    """q,k,v: [S, H*128] row views sharing one row stride; qo,ko: [H, S_out, 128]; vt: [H,128,Skp]."""
    _req_act(q, "qkv_prepare.q")
    for t_ in (k, v, qo, ko, vt):
        if t_ is not None:
            _req(t_, q.dtype, "qkv_prepare operand")
    S = q.shape[0]
    D = q.shape[1] // H
    ld = q.stride(0)
    assert (k is None or k.stride(0) == ld) and (v is None or v.stride(0) == ld)
    assert qo.is_contiguous() and qo.shape[0] == H
    assert k is None or (ko.is_contiguous() and qo.shape == ko.shape)
    S_out = qo.shape[1]
    Skp = 0
    if vt is not None:
        assert vt.is_contiguous() and vt.shape[0] == H and vt.shape[1] == D
        Skp = vt.shape[2]
    if rope is not None:
        _req(rope, torch.float32, "qkv_prepare.rope")
        assert rope.is_contiguous()
    rc = _fn("apexmi_qkv_prepare", q)(q.data_ptr(), _ptr(k), _ptr(v), ld, S, H, D, split,
                                       _ptr(wq), _ptr(wk), _ptr(wq2), _ptr(wk2), float(eps),
                                       _ptr(rope), rope_mode, qo.data_ptr(), _ptr(ko), _ptr(vt),
                                       S_out, Skp, row0, _stream())
    _l.check(rc, "qkv_prepare")


def qk_rms_rope_rows(q: torch.Tensor, k: Optional[torch.Tensor], v: Optional[torch.Tensor], H: int, qo: torch.Tensor,
                     ko: Optional[torch.Tensor], vt: Optional[torch.Tensor], wq: Optional[torch.Tensor] = None,
                     wk: Optional[torch.Tensor] = None, eps: float = 1e-6, rope: Optional[torch.Tensor] = None,
                     rope_mode: int = _l.ROPE_NONE, row0: int = 0) -> None:
    """Wan's q / k preparation in one pass: RMSNorm over all H * 128 channels of every q (and k) row (weights wq / wk of that
    width), rounded to the storage type where the in-place norm of the reference writes it, RoPE, [H, S_out, 128] layout; v
    (optional) transposed to [H, 128, Skp].  Bit-identical to ln_modulate(rms) on q, on k, then qkv_prepare."""
    _req_act(q, "qk_rms_rope_rows.q")
    for t_ in (k, v, qo, ko, vt):
        if t_ is not None:
            _req(t_, q.dtype, "qk_rms_rope_rows operand")
    S, ld = q.shape[0], q.stride(0)
    assert q.shape[1] == H * 128 and (k is None or k.stride(0) == ld) and (v is None or v.stride(0) == ld)
    assert qo.is_contiguous() and qo.shape[0] == H and (k is None) == (ko is None) and (v is None) == (vt is None)
    assert ko is None or (ko.is_contiguous() and ko.shape == qo.shape)
    Skp = 0
    if vt is not None:
        assert vt.is_contiguous() and vt.shape[0] == H and vt.shape[1] == 128
        Skp = vt.shape[2]
    for w_ in (wq, wk):
        if w_ is not None:
            _req(w_, torch.bfloat16, "qk_rms_rope_rows weight")
            assert w_.is_contiguous() and w_.numel() == H * 128
    if rope is not None:
        _req(rope, torch.float32, "qk_rms_rope_rows.rope")
        assert rope.is_contiguous()
    rc = _fn("apexmi_qk_rms_rope_rows", q)(q.data_ptr(), _ptr(k), _ptr(v), ld, S, H, _ptr(wq), _ptr(wk), float(eps), _ptr(rope),
                                           rope_mode, qo.data_ptr(), _ptr(ko), _ptr(vt), qo.shape[1], Skp, row0, _stream())
    _l.check(rc, "qk_rms_rope_rows")


def v_transpose(v: torch.Tensor, vt: torch.Tensor) -> None:
    """v: [S, H, 128] view (any row/head stride) -> vt [H, 128, Skp] zero padded."""
    _req(v, torch.bfloat16, "v_transpose.v")
    S, H, D = v.shape
    assert v.stride(2) == 1 and vt.is_contiguous()
    rc = _l.load().apexmi_v_transpose(v.data_ptr(), v.stride(1), v.stride(0), S, H, D, vt.data_ptr(),
                                      vt.shape[2], 0, _stream())
    _l.check(rc, "v_transpose")


def attention_prepared(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor,
                       Sk: int, scale: Optional[float] = None) -> torch.Tensor:
    """q [B,H,Sq,128], k [B,H,Sk,128], vt [B,H,128,Skp] packed; out [B,Sq,H,128] (strided ok)."""
    _req_act(q, "attention.q")
    B, H, Sq, D = q.shape
    assert D == 128 and q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    assert out.shape == (B, Sq, H, D) and out.stride(3) == 1
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    lib = _l.load()
    if _shipped_verify and (q.dtype == torch.float32 or out.dtype == torch.float32):
        # verification through the shipped flash kernels: bf16 roundings of q / k / v^T in (or the fused epilogue's bf16
        # outputs as they are), the kernel's bf16 result widened into the float buffer
        qb, kb, vb = (to_bf16(t_) if t_.dtype == torch.float32 else t_ for t_ in (q, k, vt))
        ob = torch.empty((B, Sq, H, D), dtype=torch.bfloat16, device=q.device)
        attention_prepared(qb, kb, vb, ob, Sk, scale)
        out.copy_(ob)
        return out
    if q.dtype == torch.float32:     # f32-storage verification mode: f32 arithmetic, no bf16 probabilities
        for t_ in (k, vt, out):
            _req(t_, torch.float32, "attention operand")
        rc = lib.apexmi_attn_fwd_prepared_f32(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B, H, Sq, Sk,
                                              vt.shape[3], _st(out),
                                              float(scale), _stream())
        _l.check(rc, "attn_fwd_prepared_f32")
        return out
    need = lib.apexmi_attn_prepared_workspace_bytes(B, H, Sq, Sk)     # scratch of the tail split, usually 0
    ws = _workspace(("prep", q.device.index, _stream()), q.device, need) if need else None
    rc = lib.apexmi_attn_fwd_prepared_ws(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B, H, Sq, Sk,
                                         vt.shape[3], _st(out),
                                         float(scale), _ptr(ws), need, _stream())
    _l.check(rc, "attn_fwd_prepared")
    return out


def attention_prepared_window(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, Sk: int,
                              plan: "WindowPlan", scale: Optional[float] = None) -> torch.Tensor:
    """attention_prepared restricted to the coordinate window of `plan` (window_plan): q [B,H,Sq,128], k [B,H,Sk,128],
    vt [B,H,128,Skp] packed bf16; out [B,Sq,H,128] (strided ok).  Bit-identical to attention_masked on the window's dense bool
    mask; the f32-storage verification mode has no window kernel."""
    _req(q, None, "attention_window.q")
    if q.dtype != torch.bfloat16:
        raise _l.ApexMIError(f"attention_prepared_window: bf16 operands only, got {q.dtype} (the f32-storage verification mode "
                             "has no window attention)")
    for t_ in (k, vt, out):
        _req(t_, torch.bfloat16, "attention_window operand")
    B, H, Sq, D = q.shape
    assert D == 128 and q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    assert k.shape == (B, H, Sk, D) and vt.shape[:3] == (B, H, D) and vt.shape[3] >= (Sk + 63) // 64 * 64
    assert out.shape == (B, Sq, H, D) and out.stride(3) == 1
    plan.check(Sq, Sk, q.device, "attention_prepared_window")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    rc = _l.load().apexmi_attn_fwd_prepared_window(
        q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B, H, Sq, Sk, vt.shape[3],
        _st(out), plan.q_coords.data_ptr(), plan.k_coords.data_ptr(),
        *plan.radius, plan.block_map.data_ptr(), float(scale), _stream())
    _l.check(rc, "attn_fwd_prepared_window")
    return out


def attention_prepared_band(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, out: torch.Tensor, Sk: int,
                            plan: "BandPlan", scale: Optional[float] = None) -> torch.Tensor:
    """attention_prepared restricted to the per-block key bands of `plan` (band_plan / frame_band_plan): q [B,H,Sq,128],
    k [B,H,Sk,128], vt [B,H,128,Skp] packed bf16; out [B,Sq,H,128] (strided ok).  Every 256-row query block attends the keys
    [lo, hi) of its band; bit-identical, block by block, to attention_prepared on the large-attention kernel over that block's
    rows and the key slice.  bf16 only (the f32-storage verification mode has no band kernel).  No host synchronisation."""
    _req(q, None, "attention_band.q")
    if q.dtype != torch.bfloat16:
        raise _l.ApexMIError(f"attention_prepared_band: bf16 operands only, got {q.dtype} (the f32-storage verification mode "
                             "has no band attention)")
    for t_ in (k, vt, out):
        _req(t_, torch.bfloat16, "attention_band operand")
    B, H, Sq, D = q.shape
    assert D == 128 and q.is_contiguous() and k.is_contiguous() and vt.is_contiguous()
    assert k.shape == (B, H, Sk, D) and vt.shape[:3] == (B, H, D) and vt.shape[3] >= (Sk + 63) // 64 * 64
    assert out.shape == (B, Sq, H, D) and out.stride(3) == 1
    if not isinstance(plan, BandPlan):
        raise _l.ApexMIError(f"attention_prepared_band: plan must be an ops.BandPlan (ops.band_plan), got {type(plan).__name__}")
    plan.check(Sq, Sk, H, q.device, "attention_prepared_band")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    rc = _l.load().apexmi_attn_fwd_prepared_band(q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr(), B, H, Sq, Sk,
                                                 vt.shape[3], _st(out), plan.bands.data_ptr(), plan.Hb, float(scale), _stream())
    _l.check(rc, "attn_fwd_prepared_band")
    return out


def attention_prepared_dual(q: torch.Tensor, k_t: torch.Tensor, vt_t: torch.Tensor, Sk_t: int,
                            k_i: Optional[torch.Tensor], vt_i: Optional[torch.Tensor], Sk_i: int, out: torch.Tensor,
                            scale: Optional[float] = None) -> torch.Tensor:
    """Two-context cross-attention in one launch: out = bf16(bf16(attn(q, text)) + bf16(attn(q, image))), each key set with its
    own softmax.  Operands as attention_prepared: q [B,H,Sq,128], k_* [B,H,>=Sk_*,128], vt_* [B,H,128,Skp_*] zero padded;
    out [B,Sq,H,128] (strided ok).  Sk_i = 0 (k_i / vt_i may be None) is the text attention alone."""
    _req_act(q, "attention_dual.q")
    if q.dtype != torch.bfloat16:
        raise _l.ApexMIError("attention_prepared_dual: bf16 operands only (the f32-storage verification mode has no dual "
                             "cross-attention)")
    B, H, Sq, D = q.shape
    assert D == 128 and q.is_contiguous() and out.shape == (B, Sq, H, D) and out.stride(3) == 1
    _req(out, torch.bfloat16, "attention_dual.out")
    ops_ = [(k_t, vt_t, Sk_t)] + ([(k_i, vt_i, Sk_i)] if Sk_i else [])
    for k_, vt_, sk in ops_:
        _req(k_, torch.bfloat16, "attention_dual.k")
        _req(vt_, torch.bfloat16, "attention_dual.vt")
        assert k_.is_contiguous() and vt_.is_contiguous() and k_.shape[:2] == (B, H) and k_.shape[3] == D
        assert vt_.shape[:3] == (B, H, D) and vt_.shape[3] >= (sk + 63) // 64 * 64
        # the kernel addresses head (b, h) at (b H + h) Sk rows: k must hold exactly Sk rows per head
        assert k_.shape[2] == sk, f"attention_prepared_dual: k has {k_.shape[2]} rows per head, Sk = {sk}"
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    rc = _l.load().apexmi_attn_fwd_prepared_dual(
        q.data_ptr(), k_t.data_ptr(), vt_t.data_ptr(), int(Sk_t), vt_t.shape[3],
        _ptr(k_i) if Sk_i else None, _ptr(vt_i) if Sk_i else None, int(Sk_i), vt_i.shape[3] if Sk_i else 0,
        out.data_ptr(), B, H, Sq, _st(out), float(scale), _stream())
    _l.check(rc, "attn_fwd_prepared_dual")
    return out


_DT ={torch.bfloat16: _l.BF16, torch.float16: _l.F16, torch.float32: _l.F32}


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              softmax_scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q k^T scale) v for q:[B,H,Sq,D], k,v:[B,H,Sk,D] (permuted views welcome).
    Returns a [B,H,Sq,D] view of a [B,Sq,H,D] buffer, i.e. `.permute(0,2,1,3)` by the caller
    (flux/base/attention.py:95) is a no-copy view and `.flatten(2,3)` stays a view."""
    _req(q, None, "attention.q")
    if q.dtype not in _DT or k.dtype != q.dtype or v.dtype != q.dtype:
        raise _l.ApexMIError(f"attention: unsupported dtypes {q.dtype}/{k.dtype}/{v.dtype}")
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if q.stride(3) != 1:
        q = q.contiguous()
    if k.stride(3) != 1:
        k = k.contiguous()
    if v.stride(3) != 1:
        v = v.contiguous()
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    need = lib.apexmi_attn_workspace_bytes(B, H, Sq, Sk, D, _DT[q.dtype])
    ws = _workspace((q.device.index, _stream()), q.device, need) if need else None
    rc = lib.apexmi_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Sq, Sk, D,
                             _st(q), _st(k), _st(v), _st(out),
                             float(softmax_scale), _DT[q.dtype], _ptr(ws), need, _stream())
    _l.check(rc, "attn_fwd")
    return out.permute(0, 2, 1, 3)


_MASK_CODES = {torch.bool: _l.MASK_BOOL, torch.float32: _l.F32, torch.bfloat16: _l.BF16, torch.float16: _l.F16}


def _mask_operand(attn_mask: Optional[torch.Tensor], B: int, Hq: int, Sq: int, Sk: int, q_dtype=None):
    """attn_mask -> (tensor, dtype code, element strides (b, h, q, k) of its broadcast to [B, Hq, Sq, Sk]), or (None, -1,
    (0, 0, 0, 0)).  torch's rule: right-aligned broadcasting (expand), bool (True = attend) or additive f32 / q's dtype.
    Broadcast dims get stride 0, so the mask is read in place and never materialised at [B, Hq, Sq, Sk].  A key dimension whose
    stride is neither 0 nor 1 costs one contiguous copy of the mask's own elements."""
    if attn_mask is None:
        return None, -1, (0, 0, 0, 0)
    m = attn_mask
    if m.dtype not in _MASK_CODES:
        raise _l.ApexMIError(f"attention_masked: attn_mask dtype {m.dtype} unsupported (bool, float32 or q's dtype)")
    if m.dtype in (torch.bfloat16, torch.float16) and q_dtype is not None and m.dtype != q_dtype:
        raise _l.ApexMIError(f"attention_masked: additive attn_mask of dtype {m.dtype} does not match q's dtype {q_dtype}")
    if m.dim() > 4:
        raise _l.ApexMIError(f"attention_masked: attn_mask of shape {tuple(m.shape)} has more than 4 dims")
    shape = (B, Hq, Sq, Sk)
    try:
        e = m.expand(shape)
    except RuntimeError as err:
        raise _l.ApexMIError(f"attention_masked: attn_mask of shape {tuple(m.shape)} does not broadcast to {shape}") from err
    if e.stride(3) not in (0, 1) and Sk > 1:
        e = m.contiguous().expand(shape)
    strides = tuple(0 if n == 1 else st for n, st in zip(shape, e.stride()))
    return e, _MASK_CODES[m.dtype], strides


def attention_masked(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_mask: Optional[torch.Tensor] = None,
                     is_causal: bool = False, softmax_scale: Optional[float] = None,
                     enable_gqa: bool = False, return_lse: bool = False):
    """F.scaled_dot_product_attention without dropout (the reference's "sdpa", R/src/attention/functions.py:338-377):
    q [B,Hq,Sq,D], k / v [B,Hkv,Sk,D] bf16 or f16 (permuted views welcome), D = 64 or 128; attn_mask bool or additive,
    broadcastable to [B,Hq,Sq,Sk]; is_causal top-left aligned, AND-ed with the mask; grouped-query heads with enable_gqa (or
    Hkv == 1).  A row without any allowed key is zero.  Returns a [B,Hq,Sq,D] view of a [B,Sq,Hq,D] buffer.  Shapes alone
    size every launch: no host synchronisation.

    return_lse=True returns (out, lse): lse [B,Hq,Sq] float32, contiguous, the natural-log row normaliser
    ln sum_j exp(scale q_i k_j + mask_ij) over the allowed keys (causal rule included; -inf for a row without an allowed key),
    flash-attn's softmax_lse.  It is what attention_merge needs to combine calls over separate key sets.  `out` is bit-identical
    to the call without it."""
    _req(q, None, "attention_masked.q")
    _req(k, None, "attention_masked.k")
    _req(v, None, "attention_masked.v")
    Hq, Hkv, Sq, Sk, D = _flash_qkv("attention_masked", q, k, v, 4, (64, 128), bool(enable_gqa))
    B = q.shape[0]
    m, mcode, mst = _mask_operand(attn_mask, B, Hq, Sq, Sk, q.dtype)
    if m is not None and m.device != q.device:
        raise _l.ApexMIError(f"attention_masked: attn_mask is on {m.device}, q on {q.device}")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    need = lib.apexmi_attn_masked_workspace_bytes(B, Hq, Hkv, Sq, Sk, D)
    ws = _workspace(("masked", q.device.index, _stream()), q.device, need)
    # the two entry points differ by the lse pointer behind `out` and its strides behind out's
    ptrs = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr())
    shape = (B, Hq, Hkv, Sq, Sk, D, _st(q), _st(k), _st(v), _st(out))
    rest = (_ptr(m), mcode, _l.i64x4(mst), 1 if is_causal else 0, float(softmax_scale), _DT[q.dtype], ws.data_ptr(), need, _stream())
    if return_lse:
        lse = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device)
        _l.check(lib.apexmi_attn_fwd_masked_lse(*ptrs, lse.data_ptr(), *shape, _st(lse), *rest), "attn_fwd_masked_lse")
        return out.permute(0, 2, 1, 3), lse
    _l.check(lib.apexmi_attn_fwd_masked(*ptrs, *shape, *rest), "attn_fwd_masked")
    return out.permute(0, 2, 1, 3)


MERGE_MAX = 8


def attention_merge(outs, lses, out: Optional[torch.Tensor] = None):
    """Merge 1..8 partial attention results over disjoint key sets into the attention over their union.  outs[p] [B,H,Sq,D] and
    lses[p] [B,H,Sq] float32 are what attention_masked(..., return_lse=True) returns ([B,H,Sq,D] views of [B,Sq,H,D] buffers; any
    other layout costs a copy), bf16 or f16, D a multiple of 8.  In f32, with m = max_p lse_p and w_p = exp(lse_p - m) (0 for
    lse_p = -inf):  out = sum_p w_p out_p / sum_p w_p rounded once,  lse = m + ln sum_p w_p.  A row whose lse_p are all -inf gives
    out = 0 and lse = -inf.  `out` (optional, the layout of the partials) may be outs[0].  Returns (out, lse); one launch, no
    host synchronisation."""
    outs, lses = list(outs), list(lses)
    n = len(outs)
    if not 1 <= n <= MERGE_MAX or len(lses) != n:
        raise _l.ApexMIError(f"attention_merge: {n} partial outs and {len(lses)} lses (1 to {MERGE_MAX} of each, equally many)")
    o0 = outs[0]
    if o0.dtype not in (torch.bfloat16, torch.float16):
        raise _l.ApexMIError(f"attention_merge: dtype {o0.dtype} unsupported (bf16 or f16)")
    if o0.dim() != 4 or o0.shape[3] % 8 != 0 or o0.numel() == 0:
        raise _l.ApexMIError(f"attention_merge: outs must be non-empty [B, H, Sq, D] with D a multiple of 8, got {tuple(o0.shape)}")
    B, H, Sq, D = o0.shape
    for i, (o, l) in enumerate(zip(outs, lses)):
        if tuple(o.shape) != (B, H, Sq, D) or o.dtype != o0.dtype or o.device != o0.device:
            raise _l.ApexMIError(f"attention_merge: outs[{i}] {tuple(o.shape)} {o.dtype} on {o.device} does not match outs[0] "
                                 f"{tuple(o0.shape)} {o0.dtype} on {o0.device}")
        if tuple(l.shape) != (B, H, Sq) or l.dtype != torch.float32 or l.device != o0.device:
            raise _l.ApexMIError(f"attention_merge: lses[{i}] {tuple(l.shape)} {l.dtype} on {l.device} does not match [B, H, Sq] = "
                                 f"{(B, H, Sq)} float32 on {o0.device}")
    for i, (o, l) in enumerate(zip(outs, lses)):
        _req(o, None, f"attention_merge.outs[{i}]")
        _req(l, None, f"attention_merge.lses[{i}]")

    def bshd(t):   # the return layout of attention_masked: a [B,H,Sq,D] view of a contiguous [B,Sq,H,D] buffer
        return t if t.permute(0, 2, 1, 3).is_contiguous() else t.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)

    if out is None:
        out = torch.empty((B, Sq, H, D), dtype=o0.dtype, device=o0.device).permute(0, 2, 1, 3)
    else:
        _req(out, o0.dtype, "attention_merge.out")
        if tuple(out.shape) != (B, H, Sq, D) or out.device != o0.device or not out.permute(0, 2, 1, 3).is_contiguous():
            raise _l.ApexMIError(f"attention_merge: out must be a [B, H, Sq, D] = {(B, H, Sq, D)} view of a contiguous "
                                 f"[B, Sq, H, D] buffer on {o0.device}")
    outs = [bshd(o) for o in outs]
    lses = [l.contiguous() for l in lses]
    lse = torch.empty((B, H, Sq), dtype=torch.float32, device=o0.device)
    optr = (_l.vp * n)(*[o.data_ptr() for o in outs])
    lptr = (_l.vp * n)(*[l.data_ptr() for l in lses])
    rc = _l.load().apexmi_attn_merge(n, optr, lptr, out.data_ptr(), lse.data_ptr(), B, H, Sq, D,
                                     _l.i64x3((out.stride(0), out.stride(2), out.stride(1))), _st(lse),
                                     _DT[o0.dtype], _stream())
    _l.check(rc, "attn_merge")
    return out, lse


def attention_chunked(q: torch.Tensor, ks, vs, attn_masks=None, softmax_scale: Optional[float] = None,
                      enable_gqa: bool = False):
    """Attention of q over the union of 1..8 key/value chunks that live in separate buffers, without concatenating them:
    ks[p] / vs[p] [B,Hkv,Sk_p,D] (the Sk_p may differ), attn_masks (optional) one mask or None per chunk, each broadcastable
    to [B,Hq,Sq,Sk_p] as in attention_masked.  One attention_masked(..., return_lse=True) launch per chunk and one
    attention_merge.  Returns (out, lse) of the whole key set, out as attention_masked returns it.  Wide heads (D = 256, 384 or
    512) go through attention_wide(..., return_lse=True) per chunk instead; that kernel has neither masks nor grouped-query
    heads, so both are refused there.

    is_causal is not offered: the causal rule of a chunk depends on the offset of its keys in the whole sequence, which a chunk
    does not carry.  A causal caller passes per-chunk masks (the chunk's columns of the causal mask)."""
    ks, vs = list(ks), list(vs)
    n = len(ks)
    if not 1 <= n <= MERGE_MAX or len(vs) != n:
        raise _l.ApexMIError(f"attention_chunked: {n} key and {len(vs)} value chunks (1 to {MERGE_MAX} of each, equally many)")
    masks = [None] * n if attn_masks is None else list(attn_masks)
    if len(masks) != n:
        raise _l.ApexMIError(f"attention_chunked: {len(masks)} masks for {n} chunks (one per chunk, None for no mask)")
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    if q.dim() == 4 and q.shape[-1] in WIDE_HEAD_DIMS:
        if any(m is not None for m in masks):
            raise _l.ApexMIError(f"attention_chunked: head dim {q.shape[-1]} runs on the wide-head kernel, which takes no masks")
        if enable_gqa or any(kk.dim() != 4 or kk.shape[1] != q.shape[1] for kk in ks):
            raise _l.ApexMIError(f"attention_chunked: head dim {q.shape[-1]} runs on the wide-head kernel, which has no "
                                 "grouped-query heads (every chunk needs q's head count, enable_gqa=False)")
        parts = [attention_wide(q, k, v, softmax_scale=softmax_scale, return_lse=True) for k, v in zip(ks, vs)]
        return attention_merge([p[0] for p in parts], [p[1] for p in parts], out=parts[0][0])
    parts = [attention_masked(q, k, v, m, softmax_scale=softmax_scale, enable_gqa=enable_gqa, return_lse=True)
             for k, v, m in zip(ks, vs, masks)]
    return attention_merge([p[0] for p in parts], [p[1] for p in parts], out=parts[0][0])


def attention_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: torch.Tensor,
                     max_seqlen_q: int, max_seqlen_k: int, softmax_scale: Optional[float] = None, is_causal: bool = False,
                     enable_gqa: bool = False, return_lse: bool = False):
    """Attention over a PACKED variable-length batch in one launch (the reference's "sdpa_varlen" / "flash_varlen",
    R/src/attention/functions.py:580-745, :932-1089): q [Tq,Hq,D], k / v [Tk,Hkv,D] bf16 or f16 (strided views welcome), D = 64
    or 128; cu_seqlens_q / cu_seqlens_k int32 [n + 1] on q's device; sequence i owns query rows cu_seqlens_q[i] ..
    cu_seqlens_q[i+1] - 1 and attends keys cu_seqlens_k[i] .. cu_seqlens_k[i+1] - 1 only.  max_seqlen_q / max_seqlen_k (host
    integers, at least the longest sequence) size the launch; the cu arrays are read on the device only: no host
    synchronisation, and a wrong cu array or a too-small max_seqlen truncates the result without reading or writing out of
    range.  Grouped-query heads with enable_gqa (or Hkv == 1).

    is_causal is top-left aligned per sequence (local key j <= local query i), as attention_masked and the reference's
    sdpa_varlen (per-sequence F.scaled_dot_product_attention(is_causal=True)); flash-attn >= 2.1 aligns bottom-right instead,
    which differs whenever a sequence has different query and key lengths.

    Returns out [Tq,Hq,D] (contiguous), or (out, lse) with return_lse=True: lse [Hq,Tq] float32, the natural-log row
    normaliser (flash-attn's varlen layout).  A sequence with queries and no keys gives zero rows and lse = -inf; rows at or past
    cu_seqlens_q[n] are not written.  A sequence's rows are bit-identical to attention_masked on that sequence alone, and `out`
    is bit-identical with and without return_lse.  out[None].permute(0, 2, 1, 3) and lse[None] are what attention_merge accepts
    (no copy), so varlen partials over separate key sets merge like any others."""
    # shapes and types first, the device last: every refusal below is reachable without a device
    Hq, Hkv, Tq, Tk, D = _flash_qkv("attention_varlen", q, k, v, 3, (64, 128), bool(enable_gqa))
    if k.device != q.device or v.device != q.device:
        raise _l.ApexMIError(f"attention_varlen: k / v are on {k.device} / {v.device}, q on {q.device}")
    for name, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
        if not isinstance(cu, torch.Tensor) or cu.dtype != torch.int32 or cu.dim() != 1 or not cu.is_contiguous():
            raise _l.ApexMIError(f"attention_varlen: {name} must be a contiguous 1-D int32 tensor")
        if cu.device != q.device:
            raise _l.ApexMIError(f"attention_varlen: {name} is on {cu.device}, q on {q.device}")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel() or cu_seqlens_q.numel() < 2:
        raise _l.ApexMIError(f"attention_varlen: cu_seqlens_q has {cu_seqlens_q.numel()} entries, cu_seqlens_k "
                             f"{cu_seqlens_k.numel()} (n + 1 of each, n >= 1)")
    max_seqlen_q, max_seqlen_k = int(max_seqlen_q), int(max_seqlen_k)
    if max_seqlen_q < 1 or max_seqlen_k < 1:
        raise _l.ApexMIError(f"attention_varlen: max_seqlen_q={max_seqlen_q} / max_seqlen_k={max_seqlen_k} must be at least 1")
    n = cu_seqlens_q.numel() - 1
    _req(q, None, "attention_varlen.q")
    max_seqlen_q, max_seqlen_k = min(max_seqlen_q, Tq), min(max_seqlen_k, Tk)   # a sequence is never longer than its array
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((Tq, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((Hq, Tq), dtype=torch.float32, device=q.device) if return_lse else None
    lib = _l.load()
    need = lib.apexmi_attn_varlen_workspace_bytes(Tk, n, Hkv, D)
    ws = _workspace(("varlen", q.device.index, _stream()), q.device, need)
    rc = lib.apexmi_attn_fwd_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), _ptr(lse), cu_seqlens_q.data_ptr(),
                                    cu_seqlens_k.data_ptr(), n, Tq, Tk, Hq, Hkv, D, max_seqlen_q, max_seqlen_k, _st(q, 2), _st(k, 2),
                                    _st(v, 2), _st(out, 2), _st(lse, 2) if return_lse else None, 1 if is_causal else 0,
                                    float(softmax_scale), _DT[q.dtype], ws.data_ptr(), need, _stream())
    _l.check(rc, "attn_fwd_varlen")
    return (out, lse) if return_lse else out


class WindowPlan:
    """A coordinate window, ready to launch (window_plan): the packed coordinates `q_coords` [Sq, 4] / `k_coords` [Sk, 4] int16
    ({c0, c1, c2, 0} per token; one tensor for self-attention), the clamped `radius` and the `block_map` uint8 [ceil(Sq / 128),
    ceil(Sk / 64)] (0 SKIP, 1 DENSE, 2 PARTIAL) the kernel walks.  Built once; every launch only reads it."""

    def __init__(self, q_coords: torch.Tensor, k_coords: torch.Tensor, radius: Tuple[int, int, int], block_map: torch.Tensor):
        self.q_coords, self.k_coords, self.radius, self.block_map = q_coords, k_coords, radius, block_map
        self.Sq, self.Sk = int(q_coords.shape[0]), int(k_coords.shape[0])

    @property
    def device(self):
        return self.block_map.device

    def check(self, Sq: int, Sk: int, device, who: str) -> None:
        if (Sq, Sk) != (self.Sq, self.Sk):
            raise _l.ApexMIError(f"{who}: the window plan is for (Sq, Sk) = ({self.Sq}, {self.Sk}), the operands have ({Sq}, {Sk})")
        if device != self.device:
            raise _l.ApexMIError(f"{who}: the window plan is on {self.device}, the operands on {device}")

    def tile_counts(self) -> Tuple[int, int, int]:
        """(SKIP, DENSE, PARTIAL) tiles of the block map (synchronises: diagnostics, not part of a step)."""
        c = torch.bincount(self.block_map.flatten().long(), minlength=3).tolist()
        return int(c[0]), int(c[1]), int(c[2])


_I16 = (-32768, 32767)
_INT_DTYPES = (torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64)


def _check_window_coords(c, name: str) -> None:
    if not isinstance(c, torch.Tensor) or c.dtype not in _INT_DTYPES:
        raise _l.ApexMIError(f"window_plan: {name} must be an integer tensor, got {getattr(c, 'dtype', type(c))}")
    if c.dim() != 2 or c.shape[1] != 3 or c.shape[0] == 0:
        raise _l.ApexMIError(f"window_plan: {name} must be [S, 3] with S >= 1, got shape {tuple(c.shape)}")
    lo, hi = int(c.min()), int(c.max())      # plan build time only
    if lo < _I16[0] or hi > _I16[1]:
        raise _l.ApexMIError(f"window_plan: {name} values span [{lo}, {hi}], outside int16 (the kernel's 8-byte token record)")


def _pack_window_coords(c: torch.Tensor, name: str, device) -> torch.Tensor:
    """integer [S, 3] (CPU tensors are moved once) -> int16 [S, 4] records {c0, c1, c2, 0} on `device`"""
    packed = torch.zeros((c.shape[0], 4), dtype=torch.int16, device=device)
    packed[:, :3] = c.to(device=device, dtype=torch.int16)
    return packed


def window_plan(q_coords: torch.Tensor, k_coords: Optional[torch.Tensor] = None, radius: Sequence[int] = (0, 0, 0),
                device=None) -> WindowPlan:
    """Plan of a coordinate window for attention_window / attention_prepared_window: key j is allowed for query i iff
    |q_coords[i][a] - k_coords[j][a]| <= radius[a] on the three axes (one window for all batches and heads).  q_coords [Sq, 3],
    k_coords [Sk, 3] integer tensors on the device (CPU tensors are moved once, to `device` or the other operand's device);
    k_coords=None is self-attention.  The block map is written here, once, by a HIP pre-pass over the two coordinate arrays;
    nothing of size Sq x Sk is ever allocated."""
    try:
        r = tuple(int(x) for x in radius)
    except TypeError as err:
        raise _l.ApexMIError(f"window_plan: radius must be three integers, got {radius!r}") from err
    if len(r) != 3 or any(x < 0 for x in r):
        raise _l.ApexMIError(f"window_plan: radius must be three non-negative integers, got {radius!r}")
    for c, name in ((q_coords, "q_coords"), (k_coords, "k_coords")):
        if c is not None or name == "q_coords":
            _check_window_coords(c, name)
    tensors = [t for t in (q_coords, k_coords) if isinstance(t, torch.Tensor)]
    tensors = [t for t in (q_coords, k_coords) if isinstance(t, torch.Tensor)]
    devs = {t.device for t in tensors if t.is_cuda}
    if len(devs) > 1:
        raise _l.ApexMIError(f"window_plan: q_coords and k_coords are on different devices ({sorted(map(str, devs))})")
    if devs:
        dev = devs.pop()
        if device is not None and torch.device(device) != dev:
            raise _l.ApexMIError(f"window_plan: coordinates are on {dev}, device={device} was asked for")
    elif device is not None:
        dev = torch.device(device)
    else:
        if not torch.cuda.is_available():
            raise _l.ApexMIError("window_plan: no ROCm device to build the plan on (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _l.ApexMIError(f"window_plan: expected a ROCm device, got {dev} (no CPU fallback)")
    qc = _pack_window_coords(q_coords, "q_coords", dev)
    kc = qc if k_coords is None else _pack_window_coords(k_coords, "k_coords", dev)
    r = tuple(min(x, 65535) for x in r)     # two int16 coordinates differ by at most 65535
    Sq, Sk = qc.shape[0], kc.shape[0]
    lib = _l.load()
    nbytes = lib.apexmi_attn_window_map_bytes(Sq, Sk)
    bmap = torch.empty(((Sq + 127) // 128, (Sk + 63) // 64), dtype=torch.uint8, device=dev)
    assert bmap.numel() == nbytes
    with torch.cuda.device(dev):
        rc = lib.apexmi_attn_window_map(qc.data_ptr(), kc.data_ptr(), Sq, Sk, *r, bmap.data_ptr(), nbytes, _stream())
    _l.check(rc, "attn_window_map")
    return WindowPlan(qc, kc, r, bmap)


def attention_window(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, plan: WindowPlan, softmax_scale: Optional[float] = None,
                     enable_gqa: bool = False) -> torch.Tensor:
    """softmax(q k^T scale over the keys inside the coordinate window of `plan`) v: attention_masked with the bool mask given as
    the rule of window_plan, bit-identical to it on the equivalent dense mask, without that mask.  q [B,Hq,Sq,D], k / v
    [B,Hkv,Sk,D] bf16 or f16 (permuted views welcome), D = 64 or 128; a row without any allowed key is zero.  Returns a
    [B,Hq,Sq,D] view of a [B,Sq,Hq,D] buffer.  No host synchronisation."""
    _req(q, None, "attention_window.q")
    _req(k, None, "attention_window.k")
    _req(v, None, "attention_window.v")
    if not isinstance(plan, WindowPlan):
        raise _l.ApexMIError(f"attention_window: plan must be an ops.WindowPlan (ops.window_plan), got {type(plan).__name__}")
    Hq, Hkv, Sq, Sk, D = _flash_qkv("attention_window", q, k, v, 4, (64, 128), bool(enable_gqa))
    B = q.shape[0]
    plan.check(Sq, Sk, q.device, "attention_window")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, Sq, Hq, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    need = lib.apexmi_attn_masked_workspace_bytes(B, Hq, Hkv, Sq, Sk, D)
    ws = _workspace(("masked", q.device.index, _stream()), q.device, need)
    rc = lib.apexmi_attn_fwd_window(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Hq, Hkv, Sq, Sk, D,
                                    _st(q), _st(k), _st(v), _st(out),
                                    plan.q_coords.data_ptr(), plan.k_coords.data_ptr(), *plan.radius,
                                    plan.block_map.data_ptr(), float(softmax_scale), _DT[q.dtype], ws.data_ptr(), need, _stream())
    _l.check(rc, "attn_fwd_window")
    return out.permute(0, 2, 1, 3)


class BandPlan:
    """Per-block key bands, ready to launch (band_plan / frame_band_plan): query rows in blocks of 256 counted from row 0 of each
    (batch, head), block b attends the keys [lo[b], hi[b]).  `bands` is the device copy, int32 [Hb, nqb, 2] ({lo, hi} pairs),
    uploaded once; `lo` / `hi` are the host copies [Hb, nqb] (lists of lists) behind dense_mask() and kept_fraction.  Hb = 1:
    every head shares the bands; Hb = H: one set per head.  Batches share the plan."""

    def __init__(self, lo, hi, Sq: int, Sk: int, bands: torch.Tensor):
        self.lo, self.hi, self.Sq, self.Sk, self.bands = lo, hi, int(Sq), int(Sk), bands
        self.Hb, self.nqb = len(lo), len(lo[0])

    @property
    def device(self):
        return self.bands.device

    @property
    def kept_fraction(self) -> float:
        """attended (query, key) pairs over Sq * Sk, mean over the plan's heads (host arithmetic)"""
        kept = 0
        for lo_h, hi_h in zip(self.lo, self.hi):
            for b, (lo, hi) in enumerate(zip(lo_h, hi_h)):
                kept += (min(256, self.Sq - 256 * b)) * (hi - lo)
        return kept / (self.Hb * self.Sq * self.Sk)

    def dense_mask(self) -> torch.Tensor:
        """the bool mask [Hb, Sq, Sk] of the plan (True = attended), on the CPU: tests and small sizes only"""
        m = torch.zeros((self.Hb, self.Sq, self.Sk), dtype=torch.bool)
        for h, (lo_h, hi_h) in enumerate(zip(self.lo, self.hi)):
            for b, (lo, hi) in enumerate(zip(lo_h, hi_h)):
                m[h, 256 * b:256 * b + 256, lo:hi] = True
        return m

    def check(self, Sq: int, Sk: int, H: int, device, who: str) -> None:
        if (Sq, Sk) != (self.Sq, self.Sk):
            raise _l.ApexMIError(f"{who}: the band plan is for (Sq, Sk) = ({self.Sq}, {self.Sk}), the operands have ({Sq}, {Sk})")
        if self.Hb not in (1, H):
            raise _l.ApexMIError(f"{who}: the band plan has bands for {self.Hb} heads, the operands have {H} (1 or H)")
        if device != self.device:
            raise _l.ApexMIError(f"{who}: the band plan is on {self.device}, the operands on {device}")


def _band_rows(x, name: str):
    """host integers [nqb] or [H, nqb] (list, tuple, numpy array, CPU integer tensor) -> list of lists of int"""
    if isinstance(x, torch.Tensor):
        if x.dtype not in _INT_DTYPES:
            raise _l.ApexMIError(f"band_plan: {name} must hold integers, got {x.dtype}")
        if x.is_cuda:
            raise _l.ApexMIError(f"band_plan: {name} must be a host array (the plan is validated on the host and uploaded once)")
    x = x.tolist() if hasattr(x, "tolist") else x
    try:
        rows = [list(r) for r in x] if len(x) and hasattr(x[0], "__len__") else [list(x)]
        return [[operator.index(v) for v in r] for r in rows]
    except TypeError as err:
        raise _l.ApexMIError(f"band_plan: {name} must be [nqb] or [H, nqb] integers, got {x!r}") from err


def band_plan(lo, hi, Sq: int, Sk: int, device=None) -> BandPlan:
    """Plan of per-block key bands for attention_band / attention_prepared_band: `lo`, `hi` are host integer arrays [nqb] (every
    head shares the bands) or [H, nqb] (one set per head), nqb = ceil(Sq / 256); every row of query block b (rows 256 b ...) attends
    exactly the keys lo[b] <= j < hi[b].  Rules, checked here on the host: 0 <= lo < hi <= Sk (no band is empty), lo a multiple of
    64, hi a multiple of 64 or Sk.  The pairs are uploaded once; every launch only reads them."""
    Sq, Sk = int(Sq), int(Sk)
    if Sq < 1 or Sk < 1:
        raise _l.ApexMIError(f"band_plan: empty problem (Sq={Sq} Sk={Sk})")
    lo_r, hi_r = _band_rows(lo, "lo"), _band_rows(hi, "hi")
    nqb = (Sq + 255) // 256
    if len(lo_r) != len(hi_r) or any(len(a) != len(b) for a, b in zip(lo_r, hi_r)):
        raise _l.ApexMIError(f"band_plan: lo and hi differ in shape ({len(lo_r)} x {[len(r) for r in lo_r]} against "
                             f"{len(hi_r)} x {[len(r) for r in hi_r]})")
    for r in lo_r:
        if len(r) != nqb:
            raise _l.ApexMIError(f"band_plan: {len(r)} bands for {nqb} query blocks of 256 rows (Sq={Sq})")
    for h, (lo_h, hi_h) in enumerate(zip(lo_r, hi_r)):
        for b, (a, e) in enumerate(zip(lo_h, hi_h)):
            if a % 64 != 0:
                raise _l.ApexMIError(f"band_plan: lo={a} of block {b} (head row {h}) is not a multiple of 64")
            if e % 64 != 0 and e != Sk:
                raise _l.ApexMIError(f"band_plan: hi={e} of block {b} (head row {h}) is neither a multiple of 64 nor Sk={Sk}")
            if not 0 <= a < e <= Sk:
                raise _l.ApexMIError(f"band_plan: band [{a}, {e}) of block {b} (head row {h}) is empty or outside [0, {Sk})")
    if device is None:
        if not torch.cuda.is_available():
            raise _l.ApexMIError("band_plan: no ROCm device to put the plan on (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    else:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise _l.ApexMIError(f"band_plan: expected a ROCm device, got {dev} (no CPU fallback)")
    pairs = torch.tensor([[[a, e] for a, e in zip(lo_h, hi_h)] for lo_h, hi_h in zip(lo_r, hi_r)], dtype=torch.int32)
    return BandPlan(lo_r, hi_r, Sq, Sk, pairs.to(dev))


def frame_bands(frames: int, tokens_per_frame: int, radius: int):
    """the (lo, hi) lists of frame_band_plan, host arithmetic only"""
    frames, tpf, radius = int(frames), int(tokens_per_frame), int(radius)
    if frames < 1 or tpf < 1:
        raise _l.ApexMIError(f"frame_band_plan: frames={frames} and tokens_per_frame={tpf} must be at least 1")
    if radius < 0:
        raise _l.ApexMIError(f"frame_band_plan: radius={radius} must not be negative")
    S = frames * tpf
    lo, hi = [], []
    for b in range((S + 255) // 256):
        f0, f1 = (256 * b) // tpf, (min(256 * b + 256, S) - 1) // tpf
        lo.append(max(0, f0 - radius) * tpf // 64 * 64)
        hi.append(min(S, ((f1 + radius + 1) * tpf + 63) // 64 * 64))
    return lo, hi


def frame_band_plan(frames: int, tokens_per_frame: int, radius: int, device=None) -> BandPlan:
    """Band plan of a temporal window over FRAME-MAJOR tokens (self-attention, S = frames * tokens_per_frame, token i belongs to
    frame i // tokens_per_frame; all heads share it).  For the block b that holds rows of the frames f0 ... f1:
        lo = floor64(max(0, f0 - radius) * tokens_per_frame)
        hi = min(S, ceil64((f1 + radius + 1) * tokens_per_frame)).
    This is a SUPERSET of the exact +-radius frame window |frame(i) - frame(j)| <= radius, never less: a band is one range for all
    256 rows of its block, so it is coarser than the exact window by at most the frames one block straddles (a row of frame f1
    also sees the frames f0 - radius ... and a row of frame f0 the frames ... f1 + radius) plus less than one 64-key tile at each
    end (the rounding of lo and hi)."""
    lo, hi = frame_bands(frames, tokens_per_frame, radius)
    S = int(frames) * int(tokens_per_frame)
    return band_plan(lo, hi, S, S, device)


def attention_band(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, plan: BandPlan,
                   softmax_scale: Optional[float] = None) -> torch.Tensor:
    """softmax(q k^T scale over the keys of the query block's band) v: q [B,H,Sq,128], k / v [B,H,Sk,128] bf16 (permuted views
    welcome), `plan` an ops.BandPlan (band_plan / frame_band_plan).  Equal to F.scaled_dot_product_attention with
    plan.dense_mask() as the bool mask; block by block bit-identical to the large-attention kernel on the key slice.  Returns a
    [B,H,Sq,128] view of a [B,Sq,H,128] buffer, as `attention` does.  No host synchronisation."""
    _req(q, None, "attention_band.q")
    _req(k, None, "attention_band.k")
    _req(v, None, "attention_band.v")
    if not isinstance(plan, BandPlan):
        raise _l.ApexMIError(f"attention_band: plan must be an ops.BandPlan (ops.band_plan), got {type(plan).__name__}")
    if q.dtype != torch.bfloat16 or k.dtype != q.dtype or v.dtype != q.dtype:
        raise _l.ApexMIError(f"attention_band: dtypes {q.dtype}/{k.dtype}/{v.dtype} unsupported (bf16 only)")
    if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
        raise _l.ApexMIError("attention_band: q, k, v must be 4-D [B, H, S, D]")
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    if D != 128:
        raise _l.ApexMIError(f"attention_band: head dim {D} unsupported (128 only)")
    if k.shape != (B, H, Sk, D) or v.shape != k.shape:
        raise _l.ApexMIError(f"attention_band: shapes q {tuple(q.shape)} k {tuple(k.shape)} v {tuple(v.shape)} do not match")
    if q.numel() == 0 or k.numel() == 0:
        raise _l.ApexMIError("attention_band: empty problem")
    plan.check(Sq, Sk, H, q.device, "attention_band")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    need = lib.apexmi_attn_band_workspace_bytes(B, H, Sq, Sk)
    ws = _workspace(("band", q.device.index, _stream()), q.device, need)
    rc = lib.apexmi_attn_fwd_band(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Sq, Sk, D, _st(q), _st(k), _st(v),
                                  _st(out), plan.bands.data_ptr(), plan.Hb, float(softmax_scale), _DT[q.dtype], ws.data_ptr(), need,
                                  _stream())
    _l.check(rc, "attn_fwd_band")
    return out.permute(0, 2, 1, 3)


def attention_framecausal(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, tokens_per_frame: int,
                          softmax_scale: Optional[float] = None) -> torch.Tensor:
    """Frame-causal attention of the HunyuanVideo-1.5 VAE mid block: q, k, v [B,H,S,D] bf16 (D a multiple of 128 up to
    1024, any S), token i attends the keys of frames <= its own.  Same return convention as `attention`."""
    _req(q, torch.bfloat16, "attention_framecausal.q")
    B, H, S, D = q.shape
    q, k, v = (t if t.stride(3) == 1 else t.contiguous() for t in (q, k, v))
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, S, H, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    need = lib.apexmi_attn_framecausal_workspace_bytes(S, D)
    ws = _workspace((q.device.index, _stream()), q.device, need, at_least=1)
    rc = lib.apexmi_attn_fwd_framecausal(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, S, D,
                                         int(tokens_per_frame),
                                         _st(q), _st(k), _st(v), _st(out),
                                         float(softmax_scale), ws.data_ptr(), need, _stream())
    _l.check(rc, "attn_fwd_framecausal")
    return out.permute(0, 2, 1, 3)


WIDE_HEAD_DIMS = (256, 384, 512)


WIDE_SPLITS_MAX = 8


def _wide_key_splits(key_splits, who: str):
    """1 .. 8 or "auto" (returned as 0, the C ABI's code), anything else refused"""
    if isinstance(key_splits, str):
        if key_splits != "auto":
            raise _l.ApexMIError(f"{who}: key_splits={key_splits!r} unsupported (an int 1 to {WIDE_SPLITS_MAX}, or \"auto\")")
        return 0
    if isinstance(key_splits, bool) or not isinstance(key_splits, int) or not 1 <= key_splits <= WIDE_SPLITS_MAX:
        raise _l.ApexMIError(f"{who}: key_splits={key_splits!r} unsupported (an int 1 to {WIDE_SPLITS_MAX}, or \"auto\")")
    return key_splits


def attention_wide(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, softmax_scale: Optional[float] = None,
                   frame_tokens: int = 0, key_splits=1, return_lse: bool = False):
    """softmax(q k^T scale) v for wide heads in one launch: q [B,H,Sq,D], k / v [B,H,Sk,D] bf16 or f16 views, D = 256, 384 or
    512, read in place (column slices of one fused buffer welcome; rows that are not 16-byte aligned cost a copy).
    frame_tokens > 0: key j is allowed for query i iff j // frame_tokens <= i // frame_tokens (Sq == Sk, whole frames).
    Same return convention as `attention`: a [B,H,Sq,D] view of a [B,Sq,H,D] buffer.  The workspace is V^T only, linear in Sk.
    It rounds as the flash kernels do (oracle.layers.sdpa's storage policy), not as `attention`'s materialised path for these
    head sizes does, so the two differ in the last bits.

    key_splits (an int 1 .. 8, or "auto"): n > 1 launches n workgroups per 128-row query block, each over a share of the key
    tiles, and merges their f32 partial results in a second launch (a short sequence fills more compute units; the workspace
    grows by the partials, n B Sq H (D + 1) 4 bytes).  "auto" picks n from the shape and the device's compute-unit count
    (apexmi_attn_wide_auto_splits), without a host synchronisation.  return_lse=True returns (out, lse): lse [B,H,Sq] float32,
    contiguous, the natural-log row normaliser, -inf for a row without an allowed key: attention_masked's convention, what
    attention_merge takes.  With key_splits=1 `out` is bit-identical with and without the lse, and the defaults make the call
    this function always made."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        _req(t, None, f"attention_wide.{name}")
    H, _, Sq, Sk, D = _flash_qkv("attention_wide", q, k, v, 4, WIDE_HEAD_DIMS, None)      # None: no grouped-query heads
    B = q.shape[0]
    frame_tokens = int(frame_tokens)
    if frame_tokens < 0 or (frame_tokens and (Sq != Sk or Sq % frame_tokens)):
        raise _l.ApexMIError(f"attention_wide: frame_tokens={frame_tokens} needs Sq == Sk and a whole number of frames "
                             f"(Sq={Sq}, Sk={Sk})")
    n = _wide_key_splits(key_splits, "attention_wide")
    q, k, v = _rows16(q), _rows16(k), _rows16(v)
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(D)
    out = torch.empty((B, Sq, H, D), dtype=q.dtype, device=q.device)
    lib = _l.load()
    # the workspace of the split count that runs: "auto" is the library's rule on this device's compute-unit count, here as there
    n_ws = n or lib.apexmi_attn_wide_auto_splits(B * H * ((Sq + 127) // 128), (Sk + 63) // 64,
                                                 torch.cuda.get_device_properties(q.device).multi_processor_count)
    need = lib.apexmi_attn_wide_split_workspace_bytes(B, H, Sq, Sk, D, n_ws)
    ws = _workspace(("wide", q.device.index, _stream()), q.device, need)
    common = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, Sq, Sk, D, _st(q), _st(k), _st(v), _st(out),
              float(softmax_scale), _DT[q.dtype], frame_tokens)
    if n != 1 or return_lse:
        lse = torch.empty((B, H, Sq), dtype=torch.float32, device=q.device) if return_lse else None
        with torch.cuda.device(q.device):      # "auto" reads the current device's compute-unit count
            rc = lib.apexmi_attn_fwd_wide_split(*common, _ptr(lse), _st(lse) if return_lse else None, n, ws.data_ptr(), need,
                                                _stream())
        _l.check(rc, "attn_fwd_wide_split")
        return (out.permute(0, 2, 1, 3), lse) if return_lse else out.permute(0, 2, 1, 3)
    _l.check(lib.apexmi_attn_fwd_wide(*common, ws.data_ptr(), need, _stream()), "attn_fwd_wide")
    return out.permute(0, 2, 1, 3)


def attention_bias(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, softmax_scale: float,
                   bias: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                   causal: bool = False, out: Optional[torch.Tensor] = None, kv_heads: Optional[int] = None,
                   seg: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Text-encoder self-attention over packed projections: q [Sq, H*D], k, v [Sk, Hkv*D] bf16 (row-strided views of a
    fused QKV buffer welcome), bias f32 [H, Sq, Sk] (T5 relative-position bias), keep uint8 [Sk] (0 = padded key), seg
    int32 [S] (block-diagonal attention: segment id per token).  Returns [Sq, H*D]."""
    _req_act(q, "attention_bias.q")
    _req(k, q.dtype, "attention_bias.k")
    _req(v, q.dtype, "attention_bias.v")
    assert q.dim() == 2 and q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1
    Sq, inner = q.shape
    Sk = k.shape[0]
    D = inner // heads
    if out is None:
        out = torch.empty((Sq, inner), dtype=q.dtype, device=q.device)
    if bias is not None:
        _req(bias, torch.float32, "attention_bias.bias")
        assert bias.is_contiguous() and bias.shape == (heads, Sq, Sk)
    if keep is not None:
        _req(keep, torch.uint8, "attention_bias.keep")
        assert keep.is_contiguous() and keep.numel() == Sk
    if seg is not None:
        _req(seg, torch.int32, "attention_bias.seg")
        assert seg.is_contiguous() and seg.numel() == Sq == Sk
    hkv = heads if kv_heads is None else int(kv_heads)
    assert k.shape[1] == hkv * D and v.shape[1] == hkv * D
    lib = _l.load()
    if q.dtype == torch.float32:           # f32-storage verification mode: one f32 pass per (row, head), no bf16 probabilities
        _req(out, torch.float32, "attention_bias.out")
        rc = lib.apexmi_attn_fwd_bias_f32(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                          out.data_ptr(), out.stride(0), heads, hkv, Sq, Sk, D, float(softmax_scale), _ptr(bias),
                                          _ptr(keep), _ptr(seg), 1 if causal else 0, _stream())
        _l.check(rc, "attn_fwd_bias_f32")
        return out
    need = lib.apexmi_attn_bias_workspace_bytes(heads, Sq, Sk, D)
    ws = _workspace((q.device.index, _stream()), q.device, need)
    rc = lib.apexmi_attn_fwd_bias(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
                                  out.data_ptr(), out.stride(0), heads, hkv, Sq, Sk, D, float(softmax_scale), _ptr(bias),
                                  _ptr(keep), _ptr(seg), 1 if causal else 0, ws.data_ptr(), need, _stream())
    _l.check(rc, "attn_fwd_bias")
    return out


def rope_half_(x: torch.Tensor, heads: int, head_stride: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """In place: every head of x [rows, >= heads * head_stride] (bf16, row-strided view welcome) rotates its first D =
    cos.shape[1] columns, x <- x cos + rotate_half(x) sin with f32 tables [rows, D]."""
    _req_act(x, "rope_half.x")
    _req(cos, torch.float32, "rope_half.cos")
    _req(sin, torch.float32, "rope_half.sin")
    assert x.dim() == 2 and x.stride(1) == 1 and cos.shape == sin.shape == (x.shape[0], cos.shape[1])
    assert cos.is_contiguous() and sin.is_contiguous() and x.shape[1] >= heads * head_stride
    _l.check(_fn("apexmi_rope_half", x)(x.data_ptr(), x.stride(0), x.shape[0], heads, head_stride, cos.shape[1],
                                        cos.data_ptr(), sin.data_ptr(), _stream()), "rope_half")
    return x


def relpos_bias(weight: torch.Tensor, bucket: torch.Tensor, Sq: int, Sk: int) -> torch.Tensor:
    """weight bf16 [num_buckets, H], bucket int32 [Sq + Sk - 1] (device) -> f32 [H, Sq, Sk]."""
    _req(weight, torch.bfloat16, "relpos_bias.weight")
    _req(bucket, torch.int32, "relpos_bias.bucket")
    assert weight.is_contiguous() and bucket.is_contiguous() and bucket.numel() == Sq + Sk - 1
    nb, H = weight.shape
    out = torch.empty((H, Sq, Sk), dtype=torch.float32, device=weight.device)
    _l.check(_l.load().apexmi_relpos_bias(weight.data_ptr(), nb, H, bucket.data_ptr(), Sq, Sk, out.data_ptr(), _stream()),
             "relpos_bias")
    return out


def gather_rows(table: torch.Tensor, ids: torch.Tensor, pos: Optional[torch.Tensor] = None,
                out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """table[ids] (+ pos[row % len(pos)]): bf16 [vocab, C], ids int64 [rows] on the device -> [rows, C] (`out_dtype` float32: the
    f32-storage verification mode, the position sum unrounded)."""
    _req(table, torch.bfloat16, "gather_rows.table")
    _req(ids, torch.int64, "gather_rows.ids")
    assert table.dim() == 2 and table.stride(1) == 1 and ids.dim() == 1 and ids.is_contiguous()
    rows, Cc = ids.numel(), table.shape[1]
    out = torch.empty((rows, Cc), dtype=out_dtype, device=table.device)
    period = 1
    if pos is not None:
        _req(pos, torch.bfloat16, "gather_rows.pos")
        assert pos.dim() == 2 and pos.stride(1) == 1 and pos.shape[1] == Cc
        period = pos.shape[0]
    if out_dtype == torch.float32:
        rc = _l.load().apexmi_gather_rows_f32(table.data_ptr(), table.stride(0), table.shape[0], ids.data_ptr(), _ptr(pos),
                                              pos.stride(0) if pos is not None else 0, period, out.data_ptr(), out.stride(0),
                                              rows, Cc, _stream())
        _l.check(rc, "gather_rows_f32")
        return out
    rc = _l.load().apexmi_gather_rows_bf16(table.data_ptr(), table.stride(0), table.shape[0], ids.data_ptr(), _ptr(pos),
                                           pos.stride(0) if pos is not None else 0, period, out.data_ptr(), out.stride(0),
                                           rows, Cc, _stream())
    _l.check(rc, "gather_rows_bf16")
    return out


def frames_to_u8(video: torch.Tensor) -> torch.Tensor:
    """bf16 video [C, T, H, W] (any strides) in [-1, 1] -> uint8 frames [T, H, W, C]."""
    _req_act(video, "frames_to_u8.video")
    assert video.dim() == 4
    Cc, T, H, W = video.shape
    out = torch.empty((T, H, W, Cc), dtype=torch.uint8, device=video.device)
    rc = _fn("apexmi_frames_to_u8", video)(video.data_ptr(), video.stride(0), video.stride(1), video.stride(2), video.stride(3),
                                       Cc, T, H, W, out.data_ptr(), _stream())
    _l.check(rc, "frames_to_u8")
    return out


def mul(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a * b for contiguous bf16 tensors of equal shape (numel a multiple of 8); float tensors in the f32-storage mode."""
    _req_act(a, "mul.a")
    _req(b, a.dtype, "mul.b")
    assert a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty_like(a)
    if a.dtype == torch.float32:
        _l.check(_l.load().apexmi_mul_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "mul_f32")
        return out
    _l.check(_l.load().apexmi_mul_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "mul_bf16")
    return out


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a + b for contiguous tensors of equal shape (bf16; float in the f32-storage mode; numel a multiple of 8).
    A float32 a with a bf16 b (a float residual stream taking a bf16 term) is a + 1.0 * b in f32: the euler_step kernel."""
    _req_act(a, "add.a")
    if a.dtype == torch.float32 and b.dtype == torch.bfloat16:
        assert a.shape == b.shape
        return euler_step(a, b, 1.0, out=out)
    _req(b, a.dtype, "add.b")
    assert a.shape == b.shape and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty_like(a)
    fn = getattr(_l.load(), "apexmi_add_f32" if a.dtype == torch.float32 else "apexmi_add_bf16")
    _l.check(fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "add")
    return out


def group_mean(x: torch.Tensor, out_channels: int) -> torch.Tensor:
    """Mean over consecutive channel groups of a channels-last tensor: [..., C * gs] -> [..., C] (f32 sum; bf16, or float in the
    f32-storage mode)."""
    _req_act(x, "group_mean.x")
    assert x.is_contiguous() and x.shape[-1] % out_channels == 0
    gs = x.shape[-1] // out_channels
    out = torch.empty(*x.shape[:-1], out_channels, dtype=x.dtype, device=x.device)
    P = x.numel() // x.shape[-1]
    fn = getattr(_l.load(), "apexmi_group_mean_f32" if x.dtype == torch.float32 else "apexmi_group_mean_bf16")
    _l.check(fn(x.data_ptr(), out.data_ptr(), P, out_channels, gs, _stream()), "group_mean")
    return out


_freq_tables: dict = {}


def _timestep_freqs(dim: int, shift: float, device) -> torch.Tensor:
    """The layer constant exp(-ln(10000) * i / (dim/2 - shift)), i < dim/2, built ONCE per (dim, shift, device) on the
    host with the f32 operation sequence of diffusers' `get_timestep_embedding` (in-tree copy: reference
    transformer/qwenimage/base/model.py:46-97), so the kernel's sin / cos arguments equal the reference's bit for bit."""
    key = (dim, float(shift), str(device))
    f = _freq_tables.get(key)
    if f is None:
        half = dim // 2
        exponent = -math.log(10000) * torch.arange(0, half, dtype=torch.float32)
        f = torch.exp(exponent / (half - shift)).to(device)
        _freq_tables[key] = f
    return f


def timestep_embedding(t: torch.Tensor, dim: int, scale: float = 1.0, flip_sin_to_cos: bool = True,
                       downscale_freq_shift: float = 0.0) -> torch.Tensor:
    _req(t, torch.float32, "timestep_embedding.t")
    t = t.contiguous()
    M = t.numel()
    out = torch.empty((M, dim), dtype=torch.float32, device=t.device)
    freqs = _timestep_freqs(dim, downscale_freq_shift, t.device)
    rc = _l.load().apexmi_timestep_embedding(t.data_ptr(), out.data_ptr(), M, dim, float(scale),
                                             1 if flip_sin_to_cos else 0, float(downscale_freq_shift),
                                             freqs.data_ptr(), _stream())
    _l.check(rc, "timestep_embedding")
    return out


def rope_table_axes(ids: torch.Tensor, axes_dim, theta: float = 10000.0) -> torch.Tensor:
    """ids f32 [S, n_axes] -> f32 [2, S, sum(axes_dim)] (cos plane, sin plane)."""
    import ctypes as C
    _req(ids, torch.float32, "rope_table_axes.ids")
    ids = ids.contiguous()
    S, n = ids.shape
    D = int(sum(axes_dim))
    out = torch.empty((2, S, D), dtype=torch.float32, device=ids.device)
    arr = (C.c_int * n)(*[int(a) for a in axes_dim])
    rc = _l.load().apexmi_rope_table_axes(ids.data_ptr(), S, n, arr, float(theta), out.data_ptr(), _stream())
    _l.check(rc, "rope_table_axes")
    return out


def add_bcast(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[l, :] = a[l, :] + b  (f32; a [L, n] contiguous, b [n])."""
    _req(a, torch.float32, "add_bcast.a")
    _req(b, torch.float32, "add_bcast.b")
    assert a.is_contiguous() and b.is_contiguous() and a.shape[-1] == b.numel()
    if out is None:
        out = torch.empty_like(a)
    rows = a.numel() // b.numel()
    _l.check(_l.load().apexmi_add_bcast_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), rows, b.numel(),
                                            _stream()), "add_bcast_f32")
    return out


def add_rowvec(x: torch.Tensor, v: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r, :] = x[r, :] + v  (bf16 [rows, cols] + bf16 [cols], f32 add; x / out float in the f32-storage mode)."""
    _req_act(x, "add_rowvec.x")
    _req(v, torch.bfloat16, "add_rowvec.v")
    assert x.dim() == 2 and x.stride(1) == 1 and v.is_contiguous() and v.numel() == x.shape[1]
    if out is None:
        out = torch.empty((x.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    else:
        _req(out, x.dtype, "add_rowvec.out")
        assert out.shape == x.shape and out.stride(1) == 1
    fn = getattr(_l.load(), "apexmi_add_rowvec_f32" if x.dtype == torch.float32 else "apexmi_add_rowvec_bf16")
    _l.check(fn(x.data_ptr(), x.stride(0), v.data_ptr(), out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], _stream()),
             "add_rowvec")
    return out


def to_bf16(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.float32, "to_bf16.x")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _l.check(_l.load().apexmi_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), _stream()))
    return out


def dequant_fp8_scaled(w: torch.Tensor, scale: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[rows, cols] (bf16) = w (float8_e4m3fn | float8_e5m2, [rows, cols]).to(bf16) * scale.to(bf16); `scale` is
    a scalar or one value per row.  `out` may be a row-range view of a packed weight matrix."""
    fmt = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}.get(w.dtype)
    if fmt is None:
        raise TypeError(f"dequant_fp8_scaled: weight dtype {w.dtype} is not an fp8 format")
    if not w.is_cuda:
        raise RuntimeError("dequant_fp8_scaled: tensors must be on the GPU (there is no CPU path)")
    w2 = w.reshape(w.shape[0], -1).contiguous()
    rows, cols = w2.shape
    s = scale.to(w.device).to(torch.bfloat16).reshape(-1).contiguous()
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.bfloat16, device=w.device)
    else:
        _req(out, torch.bfloat16, "dequant_fp8_scaled.out")
        assert out.shape == (rows, cols) and out.stride(1) == 1
    _l.check(_l.load().apexmi_dequant_fp8_scaled(w2.data_ptr(), fmt, s.data_ptr(), s.numel(), rows, cols,
                                                 out.data_ptr(), out.stride(0), _stream()), "dequant_fp8_scaled")
    return out


def dequant_gguf(blocks: torch.Tensor, ggml_type: int, shape: Sequence[int], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[rows, K] (bf16) = the GGUF block bytes `blocks` (uint8, device) of a weight of `shape` = (rows, ..., K) dequantised by
    ggml's definition in f32 (gguf_file.dequantize is the bit-exact restatement).  `out` may be a row-range view of a packed weight
    matrix or of a wider scratch (row stride >= K)."""
    if blocks.dtype != torch.uint8:
        raise TypeError(f"dequant_gguf: block bytes must be uint8, got {blocks.dtype}")
    _req(blocks, torch.uint8, "dequant_gguf.blocks")
    rows = int(shape[0])
    K = int(math.prod(int(d) for d in shape[1:])) if len(shape) > 1 else 1
    b = blocks.reshape(-1).contiguous()
    from .gguf_file import TYPES
    if ggml_type in TYPES and rows * K // TYPES[ggml_type][1] * TYPES[ggml_type][2] != b.numel() and K % TYPES[ggml_type][1] == 0:
        raise _l.ApexMIError(f"dequant_gguf: {b.numel()} bytes do not hold a {tuple(shape)} tensor of ggml type {ggml_type}")
    if out is None:
        out = torch.empty((rows, K), dtype=torch.bfloat16, device=blocks.device)
    else:
        _req(out, torch.bfloat16, "dequant_gguf.out")
        if out.dim() != 2 or tuple(out.shape) != (rows, K) or out.stride(1) != 1:
            raise _l.ApexMIError(f"dequant_gguf.out: expected a [{rows}, {K}] view with contiguous rows, got {tuple(out.shape)}")
    ldo = out.stride(0) if rows > 1 else max(out.stride(0), K)
    _l.check(_l.load().apexmi_dequant_gguf(b.data_ptr(), int(ggml_type), rows, K, out.data_ptr(), ldo, _stream()), "dequant_gguf")
    return out


def to_f32(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.bfloat16, "to_f32.x")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _l.check(_l.load().apexmi_cast_bf16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream()))
    return out


def euler_step(sample: torch.Tensor, model_output: torch.Tensor, dt: float,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """prev = sample + dt * model_output in f32, stored in sample's dtype (bf16 or f32)."""
    _req(model_output, torch.bfloat16, "euler_step.model_output")
    _req(sample, None, "euler_step.sample")
    assert sample.is_contiguous() and model_output.is_contiguous()
    assert sample.numel() == model_output.numel()
    if out is None:
        out = torch.empty_like(sample)
    rc = _l.load().apexmi_euler_step(sample.data_ptr(), model_output.data_ptr(), out.data_ptr(),
                                     sample.numel(), float(dt), _DT[sample.dtype], _stream())
    _l.check(rc, "euler_step")
    return out


# ---- channels-last VAE ops ---------------------------------------------------------------------
_zero_lines: dict = {}


def _zeros16(device) -> torch.Tensor:
    z = _zero_lines.get(device)
    if z is None:
        z = torch.zeros(64, dtype=torch.bfloat16, device=device)
        _zero_lines[device] = z
    return z


def pack_conv_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, (kT,) kH, kW] -> [Cout4, Kpad] with k = tap*Cin + ci, zero padded (K to 64, Cout to 4)."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    cout, cin = w.shape[:2]
    k = w.shape[2] * w.shape[3] * w.shape[4] * cin
    kpad = (k + 63) // 64 * 64
    if w.shape[2] > 1:     # room to address the last temporal slice on its own (single-frame / independent-frame launches)
        spatial = w.shape[3] * w.shape[4] * cin
        kpad = (max(kpad, (w.shape[2] - 1) * spatial + (spatial + 63) // 64 * 64) + 63) // 64 * 64
    cout4 = (cout + 3) // 4 * 4
    out = torch.zeros(cout4, kpad, dtype=w.dtype, device=w.device)
    out[:cout, :k] = w.permute(0, 2, 3, 4, 1).reshape(cout, k)
    return out


_w3c_cache: dict = {}


def _conv_w3(w_packed: torch.Tensor, ksize, cin: int) -> torch.Tensor:
    """Packed conv weight [Cout4, Kpad] (k = tap * cin + ci) -> the packing of the same weight with every tap's channel run
    repeated three times (k = tap * 3 cin + j cin + ci): the partner of the [hi | mid | lo] channel split."""
    ver = tensor_version(w_packed)
    key = (w_packed.data_ptr(), ver, tuple(w_packed.shape), tuple(ksize), cin)
    hit = None if ver is None else _w3c_cache.get(key)   # (source, repeated): the source reference pins the address in the key
    t = None if hit is None else hit[1]
    if t is None:
        kT, kH, kW = (int(v) for v in ksize)
        taps = kT * kH * kW
        cout4 = w_packed.shape[0]
        k3 = taps * 3 * cin
        kpad = (k3 + 63) // 64 * 64
        if kT > 1:
            spatial = kH * kW * 3 * cin
            kpad = (max(kpad, (kT - 1) * spatial + (spatial + 63) // 64 * 64) + 63) // 64 * 64
        t = torch.zeros(cout4, kpad, dtype=w_packed.dtype, device=w_packed.device)
        t[:, :k3] = w_packed[:, :taps * cin].reshape(cout4, taps, 1, cin).expand(cout4, taps, 3, cin).reshape(cout4, k3)
        if len(_w3c_cache) > 512:
            _w3c_cache.clear()
        if ver is not None:
            _w3c_cache[key] = (w_packed, t)
    return t


def _conv_operands(who: str, x, w_packed, bias, residual=None, out=None, up: int = 1):
    """The operand refusals the channels-last convolution wrappers share; returns (T, H, W, cin, cout, kpad).  residual and a
    given out must have the output's shape [T, up H, up W, cout] (up = 2: the convolution reads x through the 2x upsample)."""
    _req_act(x, f"{who}.x")
    _req(w_packed, torch.bfloat16, f"{who}.w")
    assert x.dim() == 4 and x.is_contiguous() and w_packed.is_contiguous()
    T, H, W, cin = x.shape
    cout, kpad = w_packed.shape
    if bias is not None:
        assert bias.numel() == cout and bias.is_contiguous()
    if residual is not None:
        assert tuple(residual.shape) == (T, up * H, up * W, cout) and residual.is_contiguous()
    if out is not None:
        assert tuple(out.shape) == (T, up * H, up * W, cout) and out.is_contiguous()
    return T, H, W, cin, cout, kpad


def _conv_prefix(x, w_packed, bias, residual, out, dims, ksize) -> tuple:
    """The 15 leading arguments of every apexmi_conv3d_cl* entry point; dims = (T, H, W, cin, cout, kpad) as _conv_operands
    returns them."""
    return (x.data_ptr(), w_packed.data_ptr(), _ptr(bias), _ptr(residual), _ptr(out), _zeros16(x.device).data_ptr(), *dims,
            int(ksize[0]), int(ksize[1]), int(ksize[2]))


def _conv_f32(x, w_packed, bias, ksize, out_shape, residual=None, out=None, replicate=False, independent_frames=False,
              upsample2x=False, stride=(1, 1), pad=(-1, -1), out_hw=(0, 0), tstride=(1, 0, 0), slope=None):
    """The f32-storage verification form of every conv3d_cl* wrapper below: float activations in, float out / residual.  The
    wrappers have run _conv_operands; what is checked here is the float storage."""
    _req(x, torch.float32, "conv3d_cl.x")
    T, H, W, cin = x.shape
    x3 = split3(x.view(T * H * W, cin)).view(T, H, W, 3 * cin)
    w3 = _conv_w3(w_packed, ksize, cin)
    cout = w_packed.shape[0]
    if out is None:
        out = torch.empty(out_shape, dtype=torch.float32, device=x.device)
    assert out.is_contiguous() and tuple(out.shape) == tuple(out_shape) and out.dtype == torch.float32
    if residual is not None:
        _req(residual, torch.float32, "conv3d_cl.residual")
        assert residual.shape == out.shape and residual.is_contiguous()
    flags = (1 if replicate else 0) | (2 if independent_frames else 0) | (4 if upsample2x else 0)
    rc = _l.load().apexmi_conv3d_cl_f32(*_conv_prefix(x3, w3, bias, residual, out, (T, H, W, 3 * cin, cout, w3.shape[1]), ksize),
                                        flags, int(stride[0]), int(stride[1]), int(pad[0]),
                                        int(pad[1]), int(out_hw[0]), int(out_hw[1]), int(tstride[0]), int(tstride[1]),
                                        int(tstride[2]), 0 if slope is None else 1, 0.0 if slope is None else float(slope),
                                        _stream())
    _l.check(rc, "conv3d_cl_f32")
    return out


def conv3d_cl(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ksize,
              residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              replicate: bool = False, independent_frames: bool = False, upsample2x: bool = False,
              clip_frames: int = 0) -> torch.Tensor:
    """x [T,H,W,Cin] bf16 contiguous -> [T,H,W,Cout4]; causal in time, "same" padding in space: zeros, or (replicate)
    clamped coordinates as HunyuanVideo15CausalConv3d pads.  upsample2x: the convolution reads x through a nearest 2x
    spatial upsample (output [T,2H,2W,Cout4]) without materialising it.  clip_frames: the T frames are T / clip_frames
    independent clips stacked along T (the tiles of a tiled decode in one launch, `apexmi_conv3d_cl_clips`)."""
    up = 2 if upsample2x else 1
    dims = _conv_operands("conv3d_cl", x, w_packed, bias, residual, out, up)
    T, H, W, cin, cout, kpad = dims
    shape = (T, up * H, up * W, cout)
    if x.dtype == torch.float32 and _shipped_verify and not (clip_frames and clip_frames != T):
        # verification through the shipped convolution tiles (slab / conv-shaped / 128x128, whichever production picks for this
        # shape): bf16 rounding of the float input, the kernel's bf16 result widened; the residual is added in float
        y = to_f32(conv3d_cl(to_bf16(x), w_packed, bias, ksize, replicate=replicate, independent_frames=independent_frames,
                             upsample2x=upsample2x))
        if residual is not None:
            y = add(y, residual)
        if out is not None:
            out.copy_(y)
            return out
        return y
    if x.dtype == torch.float32:
        assert not (replicate and independent_frames) and not (replicate and upsample2x)
        if clip_frames and clip_frames != T:
            raise _l.ApexMIError("conv3d_cl: stacked clips are not part of the f32-storage verification mode")
        return _conv_f32(x, w_packed, bias, ksize, shape, residual=residual, out=out, replicate=replicate,
                         independent_frames=independent_frames, upsample2x=upsample2x)
    if out is None:
        out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    assert not (replicate and independent_frames) and not (replicate and upsample2x)
    args, lib = _conv_prefix(x, w_packed, bias, residual, out, dims, ksize), _l.load()
    if upsample2x:
        _l.check(lib.apexmi_conv3d_cl_up2(*args, 1 if independent_frames else 0, _stream()), "conv3d_cl_up2")
        return out
    if clip_frames and clip_frames != T:
        assert not independent_frames and T % int(clip_frames) == 0
        _l.check(lib.apexmi_conv3d_cl_clips(*args, 1 if replicate else 0, int(clip_frames), _stream()), "conv3d_cl_clips")
        return out
    fn = lib.apexmi_conv3d_cl_replicate if replicate else lib.apexmi_conv3d_cl_frames if independent_frames else lib.apexmi_conv3d_cl
    _l.check(fn(*args, _stream()), "conv3d_cl")
    return out


def conv3d_cl_act(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ksize,
                  residual: Optional[torch.Tensor] = None, slope: Optional[float] = None, upsample2x: bool = False,
                  independent_frames: bool = False) -> torch.Tensor:
    """act(conv(x) + bias (+ residual)) with act = leaky ReLU(slope) (slope None: no activation), zero padding, causal in
    time; upsample2x / independent_frames as conv3d_cl.  The TAEHV blocks (reference vae/tae/model.py:20-45)."""
    up = 2 if upsample2x else 1
    dims = _conv_operands("conv3d_cl_act", x, w_packed, bias, residual, None, up)
    T, H, W, cin, cout, kpad = dims
    shape = (T, up * H, up * W, cout)
    if x.dtype == torch.float32:
        return _conv_f32(x, w_packed, bias, ksize, shape, residual=residual, independent_frames=independent_frames,
                         upsample2x=upsample2x, slope=slope)
    out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
    rc = _l.load().apexmi_conv3d_cl_act(*_conv_prefix(x, w_packed, bias, residual, out, dims, ksize),
                                        1 if independent_frames else 0, 1 if upsample2x else 0,
                                        0 if slope is None else 1, 0.0 if slope is None else float(slope), _stream())
    _l.check(rc, "conv3d_cl_act")
    return out


def tanh_clamp(x: torch.Tensor, inv_scale: float = 1.0) -> torch.Tensor:
    """3 tanh(x * inv_scale / 3) (TAEHV `Clamp`, reference vae/tae/model.py:24-26)."""
    _req_act(x, "tanh_clamp.x")
    assert x.is_contiguous() and (x.dtype == torch.float32 or x.numel() % 8 == 0)
    out = torch.empty_like(x)
    _l.check(_fn("apexmi_tanh_clamp", x)(x.data_ptr(), out.data_ptr(), x.numel(), float(inv_scale), _stream()), "tanh_clamp")
    return out


def pixel_shuffle_clamp(x: torch.Tensor, channels: int, r: int, trim: int = 0, lo: float = -1.0, hi: float = 1.0) -> torch.Tensor:
    """x [T, H, W, Cs] channels-last -> [channels, T - trim, H r, W r]: clamp, F.pixel_shuffle(r), drop `trim` leading frames
    (reference vae/tae/model.py:318-333)."""
    _req_act(x, "pixel_shuffle_clamp.x")
    assert x.dim() == 4 and x.is_contiguous()
    T, H, W, cs = x.shape
    out = torch.empty((channels, T - trim, H * r, W * r), dtype=x.dtype, device=x.device)
    _l.check(_fn("apexmi_pixel_shuffle_clamp", x)(x.data_ptr(), out.data_ptr(), T, H, W, cs, channels, r, trim, float(lo),
                                                  float(hi), _stream()), "pixel_shuffle_clamp")
    return out


def conv3d_cl_norm_fusable(x: torch.Tensor, cout: int, upsample2x: bool = False) -> bool:
    T, H, W, cin = x.shape
    return bool(_l.load().apexmi_conv3d_cl_norm_fusable(T, H, W, cin, cout, 1 if upsample2x else 0))


CONV_FAMILIES = ("128x128", "v2", "slab48", "slab64", "slab96")


def conv3d_cl_family(x_shape, w_packed_shape, ksize, replicate: bool = False, independent_frames: bool = False,
                     upsample2x: bool = False, norm: bool = False, clip_frames: int = 0, stride=(1, 1), pad=(-1, -1),
                     out_hw=(0, 0), tstride=(1, 0, 0)) -> Tuple[str, int]:
    """Which tile family a bf16 convolution call of these shapes takes under the current `conv.*` tune settings, from the
    launch's own decision function (`apexmi_conv3d_cl_family`; nothing runs): (one of CONV_FAMILIES, N extent of the v2 tile
    or 0).  x_shape [T, H, W, Cin] as stored, w_packed_shape [Cout4, Kpad]; the keywords as conv3d_cl / conv3d_cl_norm
    (norm) / conv2d_cl_strided (stride, pad, out_hw) / conv3d_cl_tstrided (tstride = (stride_t, t_first, out_frames))."""
    import ctypes
    T, H, W, cin = (int(v) for v in x_shape)
    cout, kpad = (int(v) for v in w_packed_shape)
    if clip_frames == T:
        clip_frames = 0
    n = ctypes.c_int(0)
    fam = _l.load().apexmi_conv3d_cl_family(T, H, W, cin, cout, kpad, int(ksize[0]), int(ksize[1]), int(ksize[2]),
                                            1 if replicate else 0, 1 if independent_frames else 0, 1 if upsample2x else 0,
                                            1 if norm else 0, int(clip_frames), int(stride[0]), int(stride[1]), int(pad[0]),
                                            int(pad[1]), int(out_hw[0]), int(out_hw[1]), int(tstride[0]), int(tstride[1]),
                                            int(tstride[2]), ctypes.addressof(n))
    _l.check(0 if fam >= 0 else 1, "conv3d_cl_family")
    return CONV_FAMILIES[fam], n.value


def conv3d_cl_norm(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ksize, gamma: torch.Tensor,
                   silu: bool = True, residual: Optional[torch.Tensor] = None, want_raw: bool = True,
                   upsample2x: bool = False, independent_frames: bool = False):
    """conv3d_cl with the RMS norm (+ SiLU) of its output fused into the epilogue: returns (y or None, norm(y)).
    Shapes the fused tiles do not cover (`conv3d_cl_norm_fusable`) run as conv3d_cl + rmsnorm_cl — same values."""
    up = 2 if upsample2x else 1
    dims = _conv_operands("conv3d_cl_norm", x, w_packed, bias, residual, None, up)
    _req(gamma, torch.bfloat16, "conv3d_cl_norm.gamma")
    T, H, W, cin, cout, kpad = dims
    if (x.dtype == torch.float32 and _shipped_verify and gamma.numel() == cout and conv3d_cl_norm_fusable(x, cout, upsample2x)):
        # verification through the shipped FUSED tile: conv + bias (+ bf16-rounded residual, as production holds it) + RMS norm
        # (+ SiLU) in one epilogue on the bf16 rounding of the float input; both results widened
        y, yn = conv3d_cl_norm(to_bf16(x), w_packed, bias, ksize, gamma, silu=silu,
                               residual=None if residual is None else to_bf16(residual), want_raw=want_raw,
                               upsample2x=upsample2x, independent_frames=independent_frames)
        return (None if y is None else to_f32(y)), to_f32(yn)
    # (float activations — the verification mode — otherwise take the two-launch form: same values, no fused tile)
    if x.dtype == torch.float32 or gamma.numel() != cout or not conv3d_cl_norm_fusable(x, cout, upsample2x):
        if gamma.numel() != cout:
            # the RMS norm divides by sqrt(channel count): a gamma shorter than the packed Cout (a Cout that is not a multiple
            # of 4 gets zero rows in the packed weight) would silently normalise over the padded width
            raise _l.ApexMIError(f"conv3d_cl_norm: gamma has {gamma.numel()} entries for {cout} (packed) output channels; the "
                                 f"fused / separate RMS norm needs the layer's channel count to equal the packed one")
        y = conv3d_cl(x, w_packed, bias, ksize, residual=residual, upsample2x=upsample2x, independent_frames=independent_frames)
        return (y if want_raw else None), rmsnorm_cl(y, gamma, silu=silu)
    assert gamma.is_contiguous()
    y = torch.empty((T, up * H, up * W, cout), dtype=torch.bfloat16, device=x.device) if want_raw else None
    yn = torch.empty((T, up * H, up * W, cout), dtype=torch.bfloat16, device=x.device)
    args = _conv_prefix(x, w_packed, bias, residual, y, dims, ksize)
    rc = _l.load().apexmi_conv3d_cl_norm(*args[:5], yn.data_ptr(), gamma.data_ptr(), 1 if silu else 0, *args[5:],
                                         1 if independent_frames else 0, 1 if upsample2x else 0, _stream())
    _l.check(rc, "conv3d_cl_norm")
    return y, yn


def conv3d_cl_tstrided(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], ksize, stride_t: int,
                       t_first: int, out_frames: int) -> torch.Tensor:
    """Causal conv3d evaluated only at input frames t_first, t_first + stride_t, ...: x [T,H,W,Cin] -> [out_frames,H,W,Cout4]
    (WanResample "downsample3d" time_conv, reference vae/wan/model.py:340-365)."""
    dims = _conv_operands("conv3d_cl_tstrided", x, w_packed, bias)
    T, H, W, cin, cout, kpad = dims
    if x.dtype == torch.float32:
        return _conv_f32(x, w_packed, bias, ksize, (out_frames, H, W, cout), tstride=(stride_t, t_first, out_frames))
    out = torch.empty((out_frames, H, W, cout), dtype=torch.bfloat16, device=x.device)
    rc = _l.load().apexmi_conv3d_cl_tstrided(*_conv_prefix(x, w_packed, bias, None, out, dims, ksize), int(stride_t), int(t_first),
                                             int(out_frames), _stream())
    _l.check(rc, "conv3d_cl_tstrided")
    return out


def _conv2d_cl_strided(who: str, x, w_packed, bias, stride: int, pad: int, extent) -> torch.Tensor:
    """The one body of conv2d_cl_down2 / conv2d_cl_strided: a 3x3 per-frame convolution with `pad` zero rows / columns above /
    left, `stride` both ways; extent: input height / width -> the output's (each wrapper's own formula)."""
    dims = _conv_operands(who, x, w_packed, bias)
    T, H, W, cin, cout, kpad = dims
    Ho, Wo = extent(H), extent(W)
    if x.dtype == torch.float32:
        return _conv_f32(x, w_packed, bias, (1, 3, 3), (T, Ho, Wo, cout), stride=(stride, stride), pad=(pad, pad), out_hw=(Ho, Wo))
    out = torch.empty((T, Ho, Wo, cout), dtype=torch.bfloat16, device=x.device)
    rc = _l.load().apexmi_conv3d_cl_strided(*_conv_prefix(x, w_packed, bias, None, out, dims, (1, 3, 3)), stride, stride, pad, pad,
                                            Ho, Wo, _stream())
    _l.check(rc, "conv3d_cl_strided")
    return out


def conv2d_cl_down2(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """ZeroPad2d((0, 1, 0, 1)) + Conv2d(3x3, stride 2) per frame: x [T, H, W, Cin] -> [T, Ho, Wo, Cout4] with
    Ho = (H - 2) // 2 + 1 (= H / 2 for even H); w_packed from pack_conv_weight of the [Cout, Cin, 3, 3] weight."""
    return _conv2d_cl_strided("conv2d_cl_down2", x, w_packed, bias, 2, 0, lambda n: (n - 2) // 2 + 1)


def conv2d_cl_strided(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], stride: int = 2, pad: int = 1) -> torch.Tensor:
    """nn.Conv2d(3x3, stride, padding=pad) per frame: x [T, H, W, Cin] -> [T, Ho, Wo, Cout4], Ho = (H + 2 pad - 3) // stride + 1
    (the TAEHV encoder's downsampling convolutions, reference vae/tae/model.py:218, :223, :228)."""
    return _conv2d_cl_strided("conv2d_cl_strided", x, w_packed, bias, stride, pad, lambda n: (n + 2 * pad - 3) // stride + 1)


def rmsnorm_cl(x: torch.Tensor, gamma: torch.Tensor, silu: bool = False,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _req_act(x, "rmsnorm_cl.x")
    _req(gamma, torch.bfloat16, "rmsnorm_cl.gamma")      # bf16 weights in both storage modes: a float gamma would be read as bf16
    assert x.is_contiguous() and gamma.is_contiguous() and gamma.numel() == x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    P = x.numel() // x.shape[-1]
    _l.check(_fn("apexmi_rmsnorm_cl", x)(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), P, x.shape[-1],
                                         1 if silu else 0, _stream()), "rmsnorm_cl")
    return out


def upsample2x_cl(x: torch.Tensor) -> torch.Tensor:
    _req(x, torch.bfloat16, "upsample2x_cl.x")
    assert x.dim() == 4 and x.is_contiguous()
    T, H, W, Cc = x.shape
    out = torch.empty((T, 2 * H, 2 * W, Cc), dtype=torch.bfloat16, device=x.device)
    _l.check(_l.load().apexmi_upsample2x_cl(x.data_ptr(), out.data_ptr(), T, H, W, Cc, _stream()), "upsample2x_cl")
    return out


def time_interleave_cl(x: torch.Tensor) -> torch.Tensor:
    """[T,H,W,2C] -> [2T,H,W,C]."""
    _req_act(x, "time_interleave_cl.x")
    assert x.dim() == 4 and x.is_contiguous() and x.shape[3] % 16 == 0
    T, H, W, C2 = x.shape
    out = torch.empty((2 * T, H, W, C2 // 2), dtype=x.dtype, device=x.device)
    _l.check(_fn("apexmi_time_interleave_cl", x)(x.data_ptr(), out.data_ptr(), T, H * W, C2 // 2, _stream()),
             "time_interleave_cl")
    return out


def crossfade_(a: torch.Tensor, b: torch.Tensor, dim: int) -> torch.Tensor:
    """In place on b: b[.., e, ..] = a[.., e, ..] (1 - e/E) + b[.., e, ..] e/E along `dim` (E = size of dim).
    a, b: same-shape bf16 views of [T, H, W, C] tensors (blend_v: dim=1, blend_h: dim=2)."""
    _req_act(a, "crossfade.a")
    _req(b, a.dtype, "crossfade.b")
    assert a.shape == b.shape and a.dim() == 4 and a.stride(3) == 1 and b.stride(3) == 1
    T, H, W, Cc = b.shape
    E = b.shape[dim]
    fade = _fn("apexmi_crossfade", a)
    if dim == 1:    # rows: outer = T, e = H rows, inner = W*C (needs contiguous rows in both)
        assert a.stride(2) == Cc and b.stride(2) == Cc
        rc = fade(a.data_ptr(), b.data_ptr(), T, E, W * Cc, a.stride(0), a.stride(1),
                                  b.stride(0), b.stride(1), _stream())
        _l.check(rc, "crossfade")
    else:           # columns: one call per frame, outer = H, e = W columns, inner = C
        for t in range(T):
            rc = fade(a[t].data_ptr(), b[t].data_ptr(), H, E, Cc, a.stride(1), a.stride(2),
                                      b.stride(1), b.stride(2), _stream())
            _l.check(rc, "crossfade")
    return b


_gn_ws: dict = {}


def groupnorm_cl(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int = 32, eps: float = 1e-6,
                 silu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm (+ SiLU) over ONE channels-last sample [..., C]: every leading dimension is a position of that sample, so the
    statistics of a group run over all of them (a batch is normalised sample by sample, as AutoencoderKL.decode does).
    gamma, beta: bf16 [C] on x's device.  The sums of x and x^2 are taken in float64, so the result is accurate relative to the
    spread of a group however far its mean is from zero (the envelope is in tests/vae_pass_probes.py)."""
    _req_act(x, "groupnorm_cl.x")
    _req(gamma, torch.bfloat16, "groupnorm_cl.gamma")
    _req(beta, torch.bfloat16, "groupnorm_cl.beta")
    Cc = x.shape[-1]
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t.numel() != Cc or t.device != x.device:
            raise _l.ApexMIError(f"groupnorm_cl.{name}: expected {Cc} values on {x.device}, got {t.numel()} on {t.device}")
    assert x.is_contiguous() and gamma.is_contiguous() and beta.is_contiguous()
    P = x.numel() // Cc
    if out is None:
        out = torch.empty_like(x)
    lib = _l.load()
    need = lib.apexmi_groupnorm_workspace_bytes(P, Cc)
    key = (x.device, _stream())
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _gn_ws[key] = ws
    rc = _fn("apexmi_groupnorm_cl", x)(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), P, Cc, groups,
                                 float(eps), 1 if silu else 0, ws.data_ptr(), need, _stream())
    _l.check(rc, "groupnorm_cl")
    return out


# ---- independent items on side streams ----------------------------------------------------------------------------
def run_on_streams(streams: list, ns: int, n_items: int, fn, device):
    """`fn(i)` for i in range(n_items) — independent pieces of one call (the images of a batch) — side by side on `ns` HIP
    streams forked from the calling stream and joined back into it; `streams` is the caller's pool (grown on demand).  Each
    result is marked as used by the calling stream (the caching allocator keys blocks on the stream that allocated them).  The
    callee's scratch must be per stream (the models key their workspaces on the stream; the op workspaces above already do)."""
    main = torch.cuda.current_stream()
    if len(streams) < ns:
        streams += [torch.cuda.Stream(device=device) for _ in range(ns - len(streams))]
    for s_ in streams[:ns]:
        s_.wait_stream(main)
    outs = []
    for i in range(n_items):
        st = streams[i % ns]
        with torch.cuda.stream(st):
            y = fn(i)
            y.record_stream(main)
            outs.append(y)
    for s_ in streams[:ns]:
        main.wait_stream(s_)
    return outs


# ---- device guard ------------------------------------------------------------------------------------------------
# Every wrapper above enqueues on `torch.cuda.current_stream()` of the CURRENT device.  A model living on cuda:1
# while the caller's current device is cuda:0 would otherwise launch on device 0's stream with device-1 pointers.
# Each public op therefore runs with its first device operand's device current; model entry points (forward /
# decode / encode) do the same with `on_model_device`, which also covers their own stream / event objects.
def _first_device(args, kwargs):
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                return a.device
        elif isinstance(a, (list, tuple)) and a and isinstance(a[0], torch.Tensor) and a[0].is_cuda:
            return a[0].device
    return None


def _guarded(fn):
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = _first_device(args, kwargs)
        if dev is None or dev.index is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


def on_model_device(method):
    """Decorator for model entry points: run with `self.device` as the current device."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        dev = self.device
        if dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
            return method(self, *args, **kwargs)
        with torch.cuda.device(dev):
            return method(self, *args, **kwargs)
    return wrapper


def _install_guards():
    import types
    g = globals()
    for name, obj in list(g.items()):
        if isinstance(obj, types.FunctionType) and not name.startswith("_") and obj.__module__ == __name__ \
                and name not in ("on_model_device",):
            g[name] = _guarded(obj)


_install_guards()
