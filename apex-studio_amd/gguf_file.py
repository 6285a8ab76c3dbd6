"""The GGUF container and ggml block formats on the host: reader, writer, numpy reference dequantisers, test quantisers.

Pure Python + numpy (`np.memmap`); no dependency on the `gguf` package.  The reference reads these files with `load_gguf`
(R/src/quantize/load.py:364) and keeps the tensors as `GGMLTensor`s that `GGMLLinear` dequantises per forward
(R/src/quantize/ggml_layer.py:220).  Here the block bytes go to the GPU as they are and `apexmi_dequant_gguf` expands them
(`ops.dequant_gguf`); the dequantisers below restate ggml's public `dequantize_row_*` definitions in float32 with every
multiply / add / subtract rounded separately and are the yardstick the kernels are held to bit for bit.

File (little-endian): u32 magic "GGUF", u32 version (2 | 3), u64 n_tensors, u64 n_kv; n_kv x {string key, u32 value type, value};
n_tensors x {string name, u32 n_dims, u64 ne[n_dims] (ne[0] = innermost), u32 ggml type, u64 offset}; the data section starts at
the next multiple of `general.alignment` (default 32); offsets are relative to it.  A tensor's torch shape is ne[] REVERSED.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .lib import ApexMIError

MAGIC = 0x46554747
DEFAULT_ALIGNMENT = 32

# metadata value types
U8, I8, U16, I16, U32, I32, F32V, BOOL, STRING, ARRAY, U64, I64, F64 = range(13)
_SCALAR_FMT = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", F32V: "<f", BOOL: "<?", U64: "<Q", I64: "<q",
               F64: "<d"}

# ggml tensor types
F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K, Q5_K, Q6_K, BF16 = 0, 1, 2, 3, 6, 7, 8, 12, 13, 14, 30
# id -> (name, elements per block, bytes per block): the types this package reads
TYPES: Dict[int, Tuple[str, int, int]] = {
    F32: ("F32", 1, 4), F16: ("F16", 1, 2), BF16: ("BF16", 1, 2),
    Q4_0: ("Q4_0", 32, 18), Q4_1: ("Q4_1", 32, 20), Q5_0: ("Q5_0", 32, 22), Q5_1: ("Q5_1", 32, 24), Q8_0: ("Q8_0", 32, 34),
    Q4_K: ("Q4_K", 256, 144), Q5_K: ("Q5_K", 256, 176), Q6_K: ("Q6_K", 256, 210),
}
QUANTIZED = tuple(t for t, (_, blk, _) in TYPES.items() if blk > 1)
# ids ggml defines that are NOT read here (named in the error only)
UNSUPPORTED_NAMES = {9: "Q8_1", 10: "Q2_K", 11: "Q3_K", 15: "Q8_K", 16: "IQ2_XXS", 17: "IQ2_XS", 18: "IQ3_XXS", 19: "IQ1_S",
                     20: "IQ4_NL", 21: "IQ3_S", 22: "IQ2_S", 23: "IQ4_XS", 24: "I8", 25: "I16", 26: "I32", 27: "I64", 28: "F64",
                     29: "IQ1_M", 34: "TQ1_0", 35: "TQ2_0", 39: "MXFP4"}
ORIG_SHAPE_PREFIX = "comfy.gguf.orig_shape."


def type_name(t: int) -> str:
    return TYPES[t][0] if t in TYPES else UNSUPPORTED_NAMES.get(t, "unknown")


def _unsupported(name: str, t: int) -> ApexMIError:
    return ApexMIError(f"GGUF tensor '{name}': ggml type id {t} ({type_name(t)}) is not supported "
                       f"(supported: {', '.join(n for n, _, _ in TYPES.values())})")


# ---- quantised data on the host ---------------------------------------------------------------------------------------------------
class Quantized:
    """Rows of a quantised weight as the file stores them: `shape` (torch order; rows = dim 0) and `segments`, a list of
    (ggml type, rows, uint8 bytes).  One segment for a tensor or a row range of it; several after a half swap or when rows of
    different tensors are stacked."""

    def __init__(self, shape: Sequence[int], segments: List[Tuple[int, int, np.ndarray]], name: str = ""):
        self.shape = tuple(int(s) for s in shape)
        self.segments = segments
        self.name = name
        if sum(n for _, n, _ in segments) != self.shape[0]:
            raise ValueError(f"{name}: segments hold {sum(n for _, n, _ in segments)} rows, shape says {self.shape[0]}")

    dtype = "gguf"

    def numel(self) -> int:
        return int(np.prod(self.shape, dtype=np.int64))

    @property
    def row_elems(self) -> int:
        return self.numel() // self.shape[0]

    def rows(self, a: int, b: int) -> "Quantized":
        if not 0 <= a < b <= self.shape[0]:
            raise IndexError(f"{self.name}: rows [{a}, {b}) of {self.shape[0]}")
        out, r0 = [], 0
        for t, n, data in self.segments:
            lo, hi = max(a, r0), min(b, r0 + n)
            if lo < hi:
                rb = data.size // n
                out.append((t, hi - lo, data[(lo - r0) * rb:(hi - r0) * rb]))
            r0 += n
        return Quantized((b - a,) + self.shape[1:], out, self.name)

    def swap_halves(self) -> "Quantized":
        h = self.shape[0] // 2
        if 2 * h != self.shape[0]:
            raise ValueError(f"{self.name}: half swap of {self.shape[0]} rows")
        a, b = self.rows(0, h), self.rows(h, 2 * h)
        return Quantized(self.shape, b.segments + a.segments, self.name)

    def dequantize(self) -> np.ndarray:
        """float32, by the reference dequantisers below."""
        k = self.row_elems
        return np.concatenate([dequantize(t, np.asarray(d)).reshape(n, k) for t, n, d in self.segments]).reshape(self.shape)


# ---- reader ---------------------------------------------------------------------------------------------------------------------
@dataclass
class GGUFTensor:
    """One tensor of a file, lazily: nothing is read until `data` / `rows()` / `read()` touch the memory map."""
    name: str
    ggml_type: int
    shape: Tuple[int, ...]            # torch order (ne[] reversed; `comfy.gguf.orig_shape.<name>` when the file carries it)
    file_shape: Tuple[int, ...]       # ne[] reversed, as stored
    offset: int                       # absolute byte offset in the file
    nbytes: Optional[int]             # None: unsupported type (size unknown)
    _map: Any = None

    @property
    def quantized(self) -> bool:
        return self.ggml_type in QUANTIZED

    def _check(self):
        if self.ggml_type not in TYPES:
            raise _unsupported(self.name, self.ggml_type)

    @property
    def data(self) -> np.ndarray:
        """uint8 view of the tensor's bytes."""
        self._check()
        return self._map[self.offset:self.offset + self.nbytes]

    def rows(self, a: int, b: int) -> np.ndarray:
        """Bytes of rows [a, b) of dim 0 — blocks run along the innermost dim, so whole rows are one contiguous range."""
        self._check()
        if not 0 <= a <= b <= self.shape[0]:
            raise IndexError(f"{self.name}: rows [{a}, {b}) of {self.shape[0]}")
        rb = self.nbytes // self.shape[0]
        return self._map[self.offset + a * rb:self.offset + b * rb]

    def read(self, a: Optional[int] = None, b: Optional[int] = None):
        """The tensor (or rows [a, b) of it) for the loader: a torch tensor for F32 / F16 / BF16, a `Quantized` otherwise."""
        import torch
        self._check()
        a, b = (0, self.shape[0]) if a is None else (a, b)
        raw = np.array(self.rows(a, b))                       # one host copy of the (small) bytes, detached from the map
        shape = (b - a,) + tuple(self.shape[1:])
        if self.quantized:
            return Quantized(shape, [(self.ggml_type, b - a, raw)], self.name)
        if self.ggml_type == F32:
            return torch.from_numpy(raw.view(np.float32)).reshape(shape)
        if self.ggml_type == F16:
            return torch.from_numpy(raw.view(np.float16)).reshape(shape)
        return torch.from_numpy(raw.view(np.int16)).view(torch.bfloat16).reshape(shape)


class _Cursor:
    def __init__(self, buf, path):
        self.buf, self.pos, self.path = buf, 0, path

    def take(self, n: int) -> bytes:
        if n < 0 or self.pos + n > len(self.buf):
            raise ApexMIError(f"{self.path}: truncated GGUF file (header wants {n} bytes at offset {self.pos}, "
                              f"file has {len(self.buf)})")
        b = bytes(self.buf[self.pos:self.pos + n])
        self.pos += n
        return b

    def scalar(self, vt: int):
        fmt = _SCALAR_FMT[vt]
        return struct.unpack(fmt, self.take(struct.calcsize(fmt)))[0]

    def string(self) -> str:
        return self.take(self.scalar(U64)).decode("utf-8")

    def value(self, vt: int):
        if vt == STRING:
            return self.string()
        if vt == ARRAY:
            et, n = self.scalar(U32), self.scalar(U64)
            if et == ARRAY or et not in range(13):
                raise ApexMIError(f"{self.path}: GGUF array of element type {et}")
            return [self.value(et) for _ in range(n)]
        if vt not in _SCALAR_FMT:
            raise ApexMIError(f"{self.path}: unknown GGUF metadata value type {vt}")
        return self.scalar(vt)


class GGUFReader:
    """`metadata` (key -> value), `metadata_types` (key -> value type, arrays as (ARRAY, element type)), `tensors`
    (name -> GGUFTensor, file order), `version`, `alignment`."""

    def __init__(self, path: str):
        self.path = path
        m = np.memmap(path, dtype=np.uint8, mode="r")
        self._map = m
        c = _Cursor(m, path)
        if len(m) < 8 or c.scalar(U32) != MAGIC:
            raise ApexMIError(f"{path}: not a GGUF file (bad magic)")
        version = c.scalar(U32)
        if version not in (2, 3):
            if version & 0xFFFF == 0 and (version >> 24) in (2, 3):
                raise ApexMIError(f"{path}: big-endian GGUF files are not supported")
            raise ApexMIError(f"{path}: GGUF version {version} is not supported (2 and 3 are)")
        self.version = version
        n_tensors, n_kv = c.scalar(U64), c.scalar(U64)
        self.metadata: Dict[str, Any] = {}
        self.metadata_types: Dict[str, Any] = {}
        for _ in range(n_kv):
            key, vt = c.string(), c.scalar(U32)
            if vt == ARRAY:
                et = struct.unpack("<I", bytes(m[c.pos:c.pos + 4]))[0] if c.pos + 4 <= len(m) else -1
                self.metadata_types[key] = (ARRAY, et)
            else:
                self.metadata_types[key] = vt
            self.metadata[key] = c.value(vt)
        self.alignment = int(self.metadata.get("general.alignment", DEFAULT_ALIGNMENT))
        if self.alignment <= 0:
            raise ApexMIError(f"{path}: general.alignment = {self.alignment}")
        infos = []
        for _ in range(n_tensors):
            name, nd = c.string(), c.scalar(U32)
            if nd > 8:
                raise ApexMIError(f"{path}: tensor '{name}' has {nd} dimensions")
            ne = [c.scalar(U64) for _ in range(nd)]
            infos.append((name, ne, c.scalar(U32), c.scalar(U64)))
        data0 = (c.pos + self.alignment - 1) // self.alignment * self.alignment
        self.data_offset = data0
        self.tensors: Dict[str, GGUFTensor] = {}
        for name, ne, t, off in infos:
            fshape = tuple(int(n) for n in reversed(ne)) or (1,)
            numel = int(np.prod(fshape, dtype=np.int64))
            nbytes = None
            if t in TYPES:
                _, blk, bs = TYPES[t]
                if fshape[-1] % blk:
                    raise ApexMIError(f"{path}: tensor '{name}' ({type_name(t)}): innermost dim {fshape[-1]} is not a multiple of "
                                      f"the block length {blk}")
                nbytes = numel // blk * bs
            if off % self.alignment:
                raise ApexMIError(f"{path}: tensor '{name}': offset {off} is not aligned to {self.alignment}")
            if data0 + off + (nbytes or 0) > len(m):
                raise ApexMIError(f"{path}: tensor '{name}' runs past the end of the file ({data0 + off + (nbytes or 0)} > {len(m)})")
            shape = fshape
            orig = self.metadata.get(ORIG_SHAPE_PREFIX + name)
            if orig is not None:
                orig = tuple(int(v) for v in orig)
                if int(np.prod(orig, dtype=np.int64)) != numel:
                    raise ApexMIError(f"{path}: tensor '{name}': {ORIG_SHAPE_PREFIX}* = {orig} does not hold {numel} elements")
                if t in TYPES and orig[-1] % TYPES[t][1]:
                    raise ApexMIError(f"{path}: tensor '{name}': original shape {orig} cuts a {type_name(t)} block")
                shape = orig
            self.tensors[name] = GGUFTensor(name, int(t), shape, fshape, data0 + int(off), nbytes, m)

    def keys(self):
        return self.tensors.keys()

    def __getitem__(self, name: str) -> GGUFTensor:
        return self.tensors[name]


# ---- writer ---------------------------------------------------------------------------------------------------------------------
class GGUFWriter:
    """Writes already-encoded tensors: `add_tensor(name, torch_shape, ggml_type, data)` with `data` the block bytes (or a numpy
    array of the matching float type); `add_meta(key, value, vtype)`, arrays as `vtype=(ARRAY, element type)`."""

    def __init__(self, path: str, version: int = 3, alignment: int = DEFAULT_ALIGNMENT):
        if version not in (2, 3):
            raise ValueError(f"GGUF version {version}")
        self.path, self.version, self.alignment = path, version, int(alignment)
        self._kv: List[Tuple[str, Any, Any]] = []
        self._tensors: List[Tuple[str, Tuple[int, ...], int, bytes]] = []
        if self.alignment != DEFAULT_ALIGNMENT:
            self.add_meta("general.alignment", self.alignment, U32)

    def add_meta(self, key: str, value, vtype) -> None:
        self._kv.append((key, value, vtype))

    def add_tensor(self, name: str, shape: Sequence[int], ggml_type: int, data, orig_shape: Optional[Sequence[int]] = None) -> None:
        if ggml_type not in TYPES:
            raise _unsupported(name, ggml_type)
        _, blk, bs = TYPES[ggml_type]
        shape = tuple(int(s) for s in shape)
        raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1).tobytes()
        numel = int(np.prod(shape, dtype=np.int64))
        if shape[-1] % blk or len(raw) != numel // blk * bs:
            raise ValueError(f"{name}: {len(raw)} bytes do not encode shape {shape} as {type_name(ggml_type)}")
        if orig_shape is not None:
            self.add_meta(ORIG_SHAPE_PREFIX + name, [int(s) for s in orig_shape], (ARRAY, I32))
        self._tensors.append((name, shape, int(ggml_type), raw))

    @staticmethod
    def _string(s: str) -> bytes:
        b = s.encode("utf-8")
        return struct.pack("<Q", len(b)) + b

    @classmethod
    def _value(cls, value, vtype) -> bytes:
        if isinstance(vtype, tuple):
            et = vtype[1]
            return struct.pack("<IQ", et, len(value)) + b"".join(cls._value(v, et) for v in value)
        if vtype == STRING:
            return cls._string(value)
        return struct.pack(_SCALAR_FMT[vtype], value)

    def write(self) -> str:
        pad = lambda n: (-n) % self.alignment      # noqa: E731
        head = struct.pack("<IIQQ", MAGIC, self.version, len(self._tensors), len(self._kv))
        for key, value, vtype in self._kv:
            head += self._string(key) + struct.pack("<I", ARRAY if isinstance(vtype, tuple) else vtype) + self._value(value, vtype)
        off = 0
        for name, shape, t, raw in self._tensors:
            head += self._string(name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", n) for n in reversed(shape))
            head += struct.pack("<IQ", t, off)
            off += len(raw) + pad(len(raw))
        with open(self.path, "wb") as f:
            f.write(head + b"\0" * pad(len(head)))
            for _, _, _, raw in self._tensors:
                f.write(raw + b"\0" * pad(len(raw)))
        return self.path


# ---- reference dequantisers (float32, every operation rounded separately) --------------------------------------------------------
def _f16(b: np.ndarray) -> np.ndarray:
    """[n, 2] bytes -> [n, 1] float32 (exact)."""
    return np.ascontiguousarray(b).view(np.float16).astype(np.float32).reshape(-1, 1)


def _f32(a) -> np.ndarray:
    return np.asarray(a).astype(np.float32)


def _scale_min_k4(s: np.ndarray):
    """[n, 12] bytes -> (sc [n, 8], mn [n, 8]) float32: ggml's get_scale_min_k4 for j = 0..7."""
    s = s.astype(np.int32)
    sc = np.concatenate([s[:, 0:4] & 63, (s[:, 8:12] & 15) | ((s[:, 0:4] >> 6) << 4)], axis=1)
    mn = np.concatenate([s[:, 4:8] & 63, (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)], axis=1)
    return _f32(sc), _f32(mn)


def dequantize(ggml_type: int, data: np.ndarray) -> np.ndarray:
    """Block bytes (uint8, a whole number of blocks) -> flat float32 values."""
    if ggml_type not in TYPES:
        raise _unsupported("<bytes>", ggml_type)
    _, blk, bs = TYPES[ggml_type]
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    if data.size % bs:
        raise ValueError(f"{data.size} bytes are not a whole number of {type_name(ggml_type)} blocks ({bs} bytes)")
    if ggml_type == F32:
        return data.view(np.float32).copy()
    if ggml_type == F16:
        return data.view(np.float16).astype(np.float32)
    if ggml_type == BF16:
        return (data.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    b = data.reshape(-1, bs)
    if ggml_type in (Q4_0, Q4_1):
        o = 2 if ggml_type == Q4_0 else 4
        d = _f16(b[:, 0:2])
        qs = b[:, o:o + 16].astype(np.int32)
        q = np.concatenate([qs & 15, qs >> 4], axis=1)
        y = _f32(q - 8) * d if ggml_type == Q4_0 else _f32(q) * d + _f16(b[:, 2:4])
    elif ggml_type in (Q5_0, Q5_1):
        o = 2 if ggml_type == Q5_0 else 4
        d = _f16(b[:, 0:2])
        qh = np.ascontiguousarray(b[:, o:o + 4]).view("<u4").astype(np.int64)                     # [n, 1]
        qs = b[:, o + 4:o + 20].astype(np.int32)
        bit = ((qh >> np.arange(32, dtype=np.int64)[None, :]) & 1).astype(np.int32)               # bit e = fifth bit of element e
        q = np.concatenate([qs & 15, qs >> 4], axis=1) | (bit << 4)
        y = _f32(q - 16) * d if ggml_type == Q5_0 else _f32(q) * d + _f16(b[:, 2:4])
    elif ggml_type == Q8_0:
        y = _f32(b[:, 2:34].view(np.int8)) * _f16(b[:, 0:2])
    elif ggml_type in (Q4_K, Q5_K):
        d, dmin = _f16(b[:, 0:2]), _f16(b[:, 2:4])
        sc, mn = _scale_min_k4(b[:, 4:16])
        d1, n1 = d * sc, dmin * mn                                                                # [n, 8] per sub-block of 32
        o = 16 if ggml_type == Q4_K else 48
        qs = b[:, o:o + 128].astype(np.int32).reshape(-1, 4, 32)
        q = np.stack([qs & 15, qs >> 4], axis=2)                                                  # [n, 4 groups, 2 halves, 32]
        if ggml_type == Q5_K:
            qh = b[:, 16:48].astype(np.int32)[:, None, None, :]
            j = (2 * np.arange(4)[:, None] + np.arange(2)[None, :])[None, :, :, None]
            q = q + (((qh >> j) & 1) << 4)
        y = d1.reshape(-1, 4, 2, 1) * _f32(q) - n1.reshape(-1, 4, 2, 1)
    else:     # Q6_K
        ql = b[:, 0:128].astype(np.int32).reshape(-1, 2, 2, 32)                                   # [n, half, l / l + 32, 32]
        qh = b[:, 128:192].astype(np.int32).reshape(-1, 2, 1, 32)
        sc = _f32(b[:, 192:208].view(np.int8)).reshape(-1, 2, 4, 2)                               # [n, half, quarter, is]
        d = _f16(b[:, 208:210]).reshape(-1, 1, 1, 1)
        lo4 = np.concatenate([ql & 15, ql >> 4], axis=2)                                          # quarters q1 q2 q3 q4
        hi2 = (qh >> (2 * np.arange(4))[None, None, :, None]) & 3
        q = (lo4 | (hi2 << 4)) - 32                                                               # [n, 2, 4, 32]
        y = (d * sc)[..., None] * _f32(q).reshape(-1, 2, 4, 2, 16)
    return np.ascontiguousarray(y, dtype=np.float32).reshape(-1)


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> the uint16 bit patterns of round-to-nearest-even bf16 (finite inputs and infinities)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dequantize_bf16(ggml_type: int, data: np.ndarray):
    """The reference result as a flat torch.bfloat16 tensor."""
    import torch
    return torch.from_numpy(bf16_bits(dequantize(ggml_type, data)).view(np.int16)).view(torch.bfloat16)


# ---- round-to-nearest quantisers (test files and the bench tool; NOT ggml's search-based ones) -----------------------------------
def _f16_up(v: np.ndarray) -> np.ndarray:
    """Smallest float16 >= v (v >= 0), so a scale never rounds below what the block's range needs."""
    v = np.asarray(v, dtype=np.float64)
    h = v.astype(np.float16)
    low = h.astype(np.float64) < v
    return np.where(low, np.nextafter(h, np.float16(np.inf)), h).astype(np.float16)


def quantize(ggml_type: int, x: np.ndarray) -> np.ndarray:
    """Flat values (a whole number of blocks) -> block bytes.  Every value lands within half a step d (d * sc for Q4_K) of
    its code: scales are rounded UP so nothing clips."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    _, blk, bs = TYPES[ggml_type]
    if x.size % blk:
        raise ValueError(f"{x.size} values are not a whole number of {type_name(ggml_type)} blocks")
    xb = x.reshape(-1, blk)
    out = np.zeros((xb.shape[0], bs), dtype=np.uint8)
    if ggml_type == Q8_0:
        d = _f16_up(np.abs(xb).max(axis=1) / 127.0)
        df = d.astype(np.float64)[:, None]
        q = np.where(df > 0, np.rint(xb / np.where(df > 0, df, 1.0)), 0.0)
        out[:, 0:2] = d.reshape(-1, 1).view(np.uint8)
        out[:, 2:34] = np.clip(q, -127, 127).astype(np.int8).view(np.uint8)
    elif ggml_type == Q4_0:
        d = _f16_up(np.maximum(-xb.min(axis=1) / 8.0, xb.max(axis=1) / 7.0).clip(min=0.0))
        df = d.astype(np.float64)[:, None]
        q = np.clip(np.where(df > 0, np.rint(xb / np.where(df > 0, df, 1.0)), 0.0) + 8, 0, 15).astype(np.uint8)
        out[:, 0:2] = d.reshape(-1, 1).view(np.uint8)
        out[:, 2:18] = q[:, :16] | (q[:, 16:] << 4)
    elif ggml_type == Q4_K:
        sub = xb.reshape(-1, 8, 32)
        neg = np.maximum(-sub.min(axis=2), 0.0)                                     # [n, 8] offset each sub-block needs
        dmin = _f16_up(neg.max(axis=1) / 63.0)
        dm = dmin.astype(np.float64)[:, None]
        mn = np.where(dm > 0, np.ceil(neg / np.where(dm > 0, dm, 1.0)), 0.0).clip(0, 63)
        top = np.maximum(sub.max(axis=2) + dm * mn, 0.0)                            # code 15 must reach this
        d = _f16_up(top.max(axis=1) / (15.0 * 63.0))
        dd = d.astype(np.float64)[:, None]
        sc = np.where(dd > 0, np.ceil(top / np.where(dd > 0, 15.0 * dd, 1.0)), 0.0).clip(0, 63)
        step = (dd * sc)[:, :, None]
        q = np.where(step > 0, np.rint((sub + (dm * mn)[:, :, None]) / np.where(step > 0, step, 1.0)), 0.0).clip(0, 15).astype(np.uint8)
        sc, mn = sc.astype(np.uint8), mn.astype(np.uint8)
        out[:, 0:2] = d.reshape(-1, 1).view(np.uint8)
        out[:, 2:4] = dmin.reshape(-1, 1).view(np.uint8)
        s = out[:, 4:16]
        s[:, 0:4] = (sc[:, 0:4] & 63) | ((sc[:, 4:8] >> 4) << 6)
        s[:, 4:8] = (mn[:, 0:4] & 63) | ((mn[:, 4:8] >> 4) << 6)
        s[:, 8:12] = (sc[:, 4:8] & 15) | ((mn[:, 4:8] & 15) << 4)
        q = q.reshape(-1, 4, 2, 32)
        out[:, 16:144] = (q[:, :, 0, :] | (q[:, :, 1, :] << 4)).reshape(-1, 128)
    else:
        raise NotImplementedError(f"quantize: {type_name(ggml_type)} (Q8_0, Q4_0 and Q4_K have test quantisers)")
    return out.reshape(-1)
