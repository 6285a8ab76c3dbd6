"""Per-element probes of the HBM-bound passes between the GEMMs and the attention calls (csrc/elementwise.hip): ln_modulate,
qkv_prepare, qk_rms_rope_rows, v_transpose, rope_half and the f32 / bf16 casts.  Operands, float64 references and the verdict,
written from the docstrings of ops.ln_modulate / qkv_prepare / qk_rms_rope_rows / rope_half_ and the comment headers of
include/apexmi.h and elementwise.hip, never from a kernel.  Pure torch on the CPU; the GPU tests feed the operands to the kernels,
the host tests prove the two conditions below for every GPU case and that the verdict rejects single wrong decisions the older
two-number bar (rel-L2 < 3e-3, max-abs within 2 bf16 ulps of the largest magnitude) lets through.

(a) EXACT, torch.equal.  Everything without a reciprocal square root: RoPE (three table layouts), the [H, S_out, 128] layout, V^T,
rope_half, the casts.  x is an integer in [-32, 32] times 2^-3, every cos / sin entry an integer in [-16, 16] times 2^-4, both
formulas of (row, column) in which one step along either axis changes the value (linear forms with steps that are units of the
modulus), and in which the two entries of a pair (interleaved mode) and the entries at c and c + D/2 (rope_half) differ.  Every
product is a multiple of 2^-7 of magnitude <= 4, every sum of two of them a multiple of 2^-7 <= 8: exact in f32 with or without
FMA contraction.  The one inexact step is the bf16 store, so the expected output is ref64.float().to(bf16) bit for bit (ties
included) and ref64.float() for the f32-storage forms.  Every output buffer is pre-filled with SENTINEL (bf16-exact, outside every
reference's range) and compared WHOLE: rows outside [row0, row0 + S), V^T columns before row0 and from row0 + round_up(S, 64),
the columns [C, ldo) of a strided ln_modulate and [D, head_stride) of rope_half must still hold it.

(b) INTERVAL, for the norms.  rsqrtf is accurate to 1 ulp, not exact, so each element gets the float64 reference `ref` and an
a-priori envelope `env` of an f32 evaluation in the documented order.  u = 2^-24 (unit roundoff), n = max(1, C / 64).
  statistics.  A lane sums L terms in sequence (L = C / 64 in the wave kernel, 8 ceil(C / 2048) <= n + 7 in the block kernel, 8 for
    the per-head norm of qkv_prepare), then 6 butterfly steps, then up to 3 LDS adds, then one division: the computed mean is off by
    at most (L + 9) u mean|x| <= (n + 16) u mean|x|.  The deviations d = x - mean carry that plus u |d|; in the sum of their squares
    the mean's error cancels to first order (sum d = 0), so the variance is off by a factor 1 + (2 + 1 + L + 9) u, the eps add and
    the division add 2 u, rsqrtf halves the lot and adds its own 2 u: rstd is off by a factor 1 + (L / 2 + 9) u.
  normalised value.  (x - mean) rstd: one subtraction, one product:
        |err| <= (L / 2 + 11) u |d| rstd + (L + 9) u mean|x| rstd <= e_n := (n + 24) u (|d| + mean|x|) rstd
    (RMSNorm: no mean, the mean|x| term is absent).  The slack, at least 9 u (|d| + mean|x|) rstd, covers the second-order terms.
  affine steps.  N = normalised * gamma * (1 + scale) passes 5 roundings (gamma product, beta add, 1 + scale, its product, shift
    add), B = beta (1 + scale) passes 4, shift 1:
        env = e_n |gamma (1 + scale)| + u (5 |N| + 4 |B| + |shift|)
    (a function of the operands and C only; this restates the `4 u (|ref| + |B| + |shift|)` form without assuming |N| <= |ref|).
  per-head norm + RoPE (qkv_prepare with weights).  a = x r w with r = rsqrt(mean(x^2) + eps) over 128 columns, L = 8:
        env_a = 32 u |x| r |w| + 2 u |a|,      env_out = |c| env_a + |s| env_b + 2 u (|a c| + |b s|)
    for out = a c -/+ b s: one product p is rounded on its own, then the sum or the fma rounds once more, so the error is at most
    u (2 + u) |p| + u |other product|; the kernels differ in which product that is, and the bound (with its factor 1 + u, left out
    above) holds for either and is attained.  The third pass of the path qk_rms_rope_rows is documented to equal is the RoPE of stored norms, which
    carry no error of their own (env_a = env_b = 0): float values fall under this envelope; bf16 values times 5-bit table entries
    are 13-bit products, exact in f32, and their sum is rounded once with or without FMA, so there the output must equal
    ref64.float().to(bf16) bit for bit, as in (a).
  verdict.  A bf16 output is accepted iff bf16(ref - env) <= out <= bf16(ref + env) (rounding is monotone, so any f32 value
    within env of ref lands there); where the two ends coincide the element is DECIDED and must match bit for bit.  A float output
    must lie within env of ref.  Non-finite outputs always fail.
  Two conditions, asserted by the host tests for every case the GPU tests run, not measurements: (1) at most UNDECIDED_CAP of a
  case's elements are undecided; (2) the reference evaluated in f32 on the CPU in three summation orders (each lane's terms in
  sequence then the butterfly, as documented; chunks of 8 then a pairwise tree; torch's own) and rounded to the output type is
  accepted everywhere.  (One sequence over the WHOLE row is not among them: its C - 1 roundings are outside the documented order
  the envelope is derived from, and on the RMS form of the offset row, whose squares all round the same way, it lands two
  envelopes out at C = 1536.)

Norm operands: bf16-exact random rows x ~ 3 N(0, 1) + 0.5, except: row 1 is a unit-variance row scaled by 2^-10 (mean square ~
eps: a dropped or doubled eps moves it by tens of percent); row 2 is all zero (output exactly beta (1 + scale) + shift); row 3 is
a random row scaled by 2^-7 (eps is a 1e-3 effect: inside the old bar, outside the envelope); row 5 is 8 + k / 16 with small
integers k (mean >> spread: RMS and LN differ grossly, a one-pass variance cancels; its outputs take 2 K + 1 values, so its
undecided share moves in steps of 1 / (2 K + 1): it sits past the M = 5 cases).  gamma, beta, scale, shift, scale2
and shift2 are formulas of the column whose step over one column and over one 8-column chunk is never zero."""
import functools
import itertools
from typing import NamedTuple

import torch

from tests.conv_probes import BF, mismatches, ulp_distance  # noqa: F401  (re-exported for the two test files)
from tests.gemm_probes import old_bar_accepts  # noqa: F401

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24
EPS = float(torch.tensor(1e-6, dtype=F32))      # the float the kernels receive
SENTINEL = 24576.0                              # 1.5 * 2^14: bf16-exact, outside every reference's range (asserted per case)
UNDECIDED_CAP = 0.03
ROPE_INTERLEAVED, ROPE_COMPLEX, ROPE_NONE = 0, 1, 2      # include/apexmi.h (the host tests compare with lib's)
D = 128


def round_up(a, b):
    return (a + b - 1) // b * b


def store(ref64, dtype):
    """the one rounding of the store: float64 -> f32 is exact on every reference here that is compared bit for bit"""
    return ref64.float().to(dtype)


def truncate_bf16(y32):
    """MUTATION helper: the bf16 store by truncation instead of round-to-nearest-even"""
    return (y32.contiguous().view(torch.int32) & -65536).view(F32).to(BF)


# ------------------------------------------------------------------------------------------------------------ exact operands
def grid_x(S, W, salt=0):
    """float64 [S, W]: integers in [-32, 32] times 2^-3; one step along a row or a column changes the value"""
    s, c = torch.arange(S).view(-1, 1), torch.arange(W).view(1, -1)
    return ((s * 7 + c * 5 + salt * 11 + (s // 3) * 2) % 65 - 32).double() / 8


def _cos_grid(r, c):
    return ((r * 7 + c * 5) % 33 - 16).float() / 16


def _sin_grid(r, c):
    return ((r * 4 + c * 7 + 3) % 33 - 16).float() / 16


def rope_table(S_out, mode):
    """f32 table of `mode` for S_out rows: [2, S_out, 128] (cos plane, sin plane) | [S_out, 64, 2] (cos, sin) | None"""
    r = torch.arange(S_out).view(-1, 1)
    if mode == ROPE_INTERLEAVED:
        c = torch.arange(D).view(1, -1)
        return torch.stack([_cos_grid(r, c), _sin_grid(r, c)]).contiguous()
    if mode == ROPE_COMPLEX:
        c = torch.arange(D // 2).view(1, -1)
        return torch.stack([_cos_grid(r, c), _sin_grid(r, c)], dim=-1).contiguous()
    return None


def half_tables(rows, Dh):
    """(cos, sin) f32 [rows, Dh] of rope_half"""
    r, c = torch.arange(rows).view(-1, 1), torch.arange(Dh).view(1, -1)
    return _cos_grid(r, c).contiguous(), _sin_grid(r, c).contiguous()


def check_grid(x64=None, table=None):
    """the conditions of an exact probe: operands on their grids and bf16-exact"""
    if x64 is not None:
        assert torch.equal(x64 * 8, (x64 * 8).round()) and float(x64.abs().max()) <= 4 and torch.equal(x64.float().to(BF).double(), x64)
    if table is not None:
        t = table.double()
        assert torch.equal(t * 16, (t * 16).round()) and float(t.abs().max()) <= 1 and torch.equal(table.to(BF).float(), table)


# ------------------------------------------------------------------------------------------------------------- RoPE references
def rope_ref(a, table, mode, rows, env=None, mut=None):
    """float64 RoPE of a [S, H, 128] (row s of `a` uses table row rows[s]) and, with env (same shape), the propagated envelope.
    interleaved: out[2i] = a[2i] cos[2i] - a[2i+1] sin[2i], out[2i+1] = a[2i+1] cos[2i+1] + a[2i] sin[2i+1]
    complex:     (out[2i] + i out[2i+1]) = (a[2i] + i a[2i+1]) (cos[i] + i sin[i])
    mut (host tests): 'other_entry' reads the table entry of the pair's other element."""
    if mode == ROPE_NONE:
        return (a, env) if env is not None else a
    ev, od = a[..., 0::2], a[..., 1::2]
    if mode == ROPE_INTERLEAVED:
        cos, sin = table[0][rows].double().unsqueeze(1), table[1][rows].double().unsqueeze(1)
        ce, co, se, so = cos[..., 0::2], cos[..., 1::2], sin[..., 0::2], sin[..., 1::2]
        if mut == "other_entry":
            ce, co, se, so = co, ce, so, se
    else:
        t = table[rows].double().unsqueeze(1)
        ce = co = t[..., 0]
        se = so = t[..., 1]
    ye, yo = ev * ce - od * se, od * co + ev * so
    out = torch.stack([ye, yo], dim=-1).flatten(-2)
    if env is None:
        return out
    ee, eo = env[..., 0::2], env[..., 1::2]
    ve = ce.abs() * ee + se.abs() * eo + 2 * U * (1 + U) * ((ev * ce).abs() + (od * se).abs())
    vo = co.abs() * eo + so.abs() * ee + 2 * U * (1 + U) * ((od * co).abs() + (ev * so).abs())
    return out, torch.stack([ve, vo], dim=-1).flatten(-2)


def rope_half_ref(x64, heads, head_stride, cos, sin):
    """x <- x cos + rotate_half(x) sin on the first Dh columns of every head of x64 [rows, >= heads * head_stride]; the rest kept"""
    Dh, h = cos.shape[1], cos.shape[1] // 2
    out = x64.clone()
    c, s = cos.double(), sin.double()
    for hd in range(heads):
        a, b = x64[:, hd * head_stride: hd * head_stride + h], x64[:, hd * head_stride + h: hd * head_stride + Dh]
        out[:, hd * head_stride: hd * head_stride + h] = a * c[:, :h] - b * s[:, :h]
        out[:, hd * head_stride + h: hd * head_stride + Dh] = b * c[:, h:] + a * s[:, h:]
    return out


ROPE_HALF_CASES = [(Dh, heads, f32) for Dh in (80, 128) for heads in (1, 5) for f32 in (False, True)]
ROPE_HALF_ROWS = 7


def rope_half_case(Dh, heads):
    """(buffer float64 [rows, heads * 128 + 8] with SENTINEL outside the rotated columns, cos, sin, expected float64 buffer)"""
    rows, hs = ROPE_HALF_ROWS, D
    buf = torch.full((rows, heads * hs + 8), SENTINEL, dtype=F64)
    for hd in range(heads):
        buf[:, hd * hs: hd * hs + Dh] = grid_x(rows, Dh, salt=hd + 1)
    cos, sin = half_tables(rows, Dh)
    return buf, cos, sin, rope_half_ref(buf, heads, hs, cos, sin)


# ------------------------------------------------------------------------------------------------------------- V^T and its tiling
def vt_written_columns(S, row0):
    """The documented tiling of the V transpose: whole 64-key tiles, every tile written in full.  Columns [row0, row0 + S) hold
    data, [row0 + S, hi) zeros; returns (row0, hi)."""
    return row0, row0 + round_up(S, 64)


def vt_call_fits(S, Skp, row0):
    """True iff those writes stay inside their own row of [.., Skp] and every 64-key tile starts on a tile boundary"""
    lo, hi = vt_written_columns(S, row0)
    return hi <= Skp and lo % 64 == 0 and Skp % 64 == 0


def vt_expected(v64, H, Skp, row0, dtype, pad=0.0):
    """the whole [H, 128, Skp] buffer after the call on a SENTINEL-filled one: v64 [S, H * 128].  pad != 0: MUTATION"""
    S = v64.shape[0]
    lo, hi = vt_written_columns(S, row0)
    assert vt_call_fits(S, Skp, row0)
    out = torch.full((H, D, Skp), SENTINEL, dtype=F64)
    out[:, :, lo + S:hi] = pad
    out[:, :, lo:lo + S] = v64.reshape(S, H, D).permute(1, 2, 0)
    return store(out, dtype)


V_TRANSPOSE_CASES = [(5, 3), (100, 3), (131, 2)]       # (S, H): the stand-alone transpose on a strided [S, H, 128] view


# ---------------------------------------------------------------------------------------------------------------- the verdict
class Verdict(NamedTuple):
    ok: torch.Tensor           # per element: accepted
    decided: torch.Tensor      # per element: the interval holds one value (bf16) / always (float)
    ratio: float               # float out: max |out - ref| / env.  bf16 out: the least pre-rounding error consistent with out,
    #                            max(0, |out - ref| - half an ulp of out) / env

    @property
    def passed(self):
        return bool(self.ok.all())

    @property
    def undecided(self):
        return 1.0 - float(self.decided.double().mean())

    def rejects_decided(self):
        return bool((~self.ok & self.decided).any())


def verdict(out, ref, env):
    ref, env = ref.double(), env.double()
    o = out.double()
    fin = torch.isfinite(o)
    tiny = 1e-300
    if out.dtype == BF:
        lo, hi = (ref - env).float().to(BF), (ref + env).float().to(BF)
        ok = fin & (o >= lo.double()) & (o <= hi.double())
        decided = lo == hi
        _, e = torch.frexp(o.abs().float())
        half = torch.ldexp(torch.ones_like(o, dtype=F32), e - 9).double()
        err = ((o - ref).abs() - half).clamp_min(0)
    else:
        ok = fin & ((o - ref).abs() <= env)
        decided = torch.ones_like(ok)
        err = (o - ref).abs()
    r = torch.where(fin, err / (env + tiny), torch.full_like(err, float("inf")))
    r = torch.where((err == 0) & fin, torch.zeros_like(r), r)
    return Verdict(ok, decided, float(r.max()))


def describe(v, out, ref, env, n=4):
    """'count: (index) got g want [lo, hi]' of the first n rejected elements"""
    bad = (~v.ok).nonzero()
    items = [f"{tuple(int(i) for i in ix)} got {float(out[tuple(ix)])!r} ref {float(ref[tuple(ix)])!r} env {float(env[tuple(ix)]):.3e}"
             for ix in bad[:n]]
    return f"{bad.shape[0]} of {out.numel()} outside the envelope ({int((~v.ok & v.decided).sum())} decided); first: " + "; ".join(items)


# -------------------------------------------------------------------------------------------------------------- ln_modulate
LN_ROWS = 13
LN_MS = (1, 5, 13)
BLOCK_C = (8, 256, 1536, 2048, 2056, 4096, 4104, 6144, 6152, 8192)     # one per decision of nit = ceil(C / 2048), full and part-filled
WAVE_C = (3072, 3584, 5120)                                             # NCH 6 / 7 / 10
STORAGES = ("bf16", "f32", "f32in")                                     # bf16 -> bf16, f32 -> f32, f32 -> bf16
ROW_TINY, ROW_ZERO, ROW_SMALL, ROW_OFFSET = 1, 2, 3, 5


def storage_dtypes(storage):
    return {"bf16": (BF, BF), "f32": (F32, F32), "f32in": (F32, BF)}[storage]


def offset_row(C, K):
    """8 + k / 16 with k in [-K, K] a formula of the column (bf16-exact).  The envelope of this row grows with (n + 24) mean / spread,
    so ln_rows lets the spread K grow with C: mean / spread runs from 90 (K = 2) to 9 (K = 25 at C = 8192)."""
    c = torch.arange(C)
    return 8 + ((c * 2 + c // 8 + c // 64) % (2 * K + 1) - K).double() / 16


@functools.lru_cache(maxsize=None)
def ln_rows(C, f32):
    """float64 [13, C], exact in the storage type of x (bf16, or float when f32): the rows of the module docstring"""
    g = torch.Generator().manual_seed(7000 + C)
    x = torch.randn(LN_ROWS, C, generator=g) * 3 + 0.5
    x = (x if f32 else x.to(BF)).double()
    c = torch.arange(C)
    x[ROW_TINY] = torch.randn(C, generator=g).to(BF).double() * 2.0 ** -10
    x[ROW_ZERO] = 0.0
    x[ROW_OFFSET] = offset_row(C, max(2, (max(1, C // 64) + 24) // 6))
    x[ROW_SMALL] = x[ROW_SMALL] * 2.0 ** -7
    assert torch.equal(x.to(F32 if f32 else BF).double(), x)
    return x


OFFGRID = 3 * 2.0 ** -14     # takes beta (1 + scale) + shift (multiples of 2^-9: the all-zero row's output) off the bf16 ties


@functools.lru_cache(maxsize=None)
def mod_vectors(C):
    """gamma, beta (bf16), scale, shift, scale2, shift2 (f32) [C]: steps over one column and over 8 columns are non-zero mod each
    period, and the two sets differ"""
    c = torch.arange(C)
    return dict(gamma=(0.5 + ((c * 7) % 13).float() / 8).to(BF), beta=(((c * 5 + 3) % 17 - 8).float() / 16).to(BF),
                scale=((c * 3 + 1) % 23 - 11).float() / 32, shift=((c * 11 + 5) % 19 - 9).float() / 16 + OFFGRID,
                scale2=((c * 5 + 2) % 29 - 14).float() / 32, shift2=((c * 7 + 1) % 31 - 15).float() / 16 + OFFGRID)


# form -> the operands ln_modulate gets (besides x); "split" takes both modulation sets
FORMS = {"plain": (), "rms": ("gamma", "rms"), "affine": ("gamma", "beta"), "scale": ("scale",), "shift": ("shift",),
         "mod": ("scale", "shift"), "affine_mod": ("gamma", "beta", "scale", "shift"),
         "split": ("scale", "shift", "scale2", "shift2")}


class LnCase(NamedTuple):
    C: int
    M: int
    storage: str
    form: str
    split: int = 0
    layout: str = "packed"          # packed | strided (ld = C + 16 bytes, sentinel columns) | inplace (out = x)

    @property
    def id(self):
        return f"C{self.C}.M{self.M}.{self.storage}.{self.form}{self.split if self.form == 'split' else ''}.{self.layout}"


def splits_of(M):
    return sorted({s for s in (0, 1, 3, M - 1, M) if 0 <= s <= M})


def ln_cases(C):
    """every ln_modulate case of one width"""
    out = []
    for M, storage in itertools.product(LN_MS, STORAGES):
        for form in FORMS:
            if form == "split":
                out += [LnCase(C, M, storage, form, s) for s in splits_of(M)]
            else:
                out.append(LnCase(C, M, storage, form))
        out.append(LnCase(C, M, storage, "split", min(3, M), "strided"))
        out.append(LnCase(C, M, storage, "affine_mod", 0, "strided"))
        if storage != "f32in":
            out.append(LnCase(C, M, storage, "split", M - 1, "inplace"))
    return out


def ln_pad(storage):
    """(extra x columns, extra out columns) of the strided layout: 16 bytes each"""
    xd, od = storage_dtypes(storage)
    return (8 if xd == BF else 4), (8 if od == BF else 4)


def ln_operands(case, x=None):
    """(x float64 [M, C], dict of the modulation operands of the case's form); x: rows of the caller's instead of ln_rows'"""
    x = ln_rows(case.C, case.storage != "bf16")[:case.M] if x is None else x
    mv = mod_vectors(case.C)
    return x, {k: mv[k] for k in FORMS[case.form] if k != "rms"}


def _row_mod(M, C, split, a, a2):
    """[M, C] float64 of a per-row modulation vector: rows < split take the second set"""
    rows = torch.arange(M).view(-1, 1)
    first = a.double().expand(M, C) if a is not None else None
    if split > 0 and a2 is not None:
        return torch.where(rows < split, a2.double().expand(M, C), first if first is not None else torch.zeros(M, C, dtype=F64))
    return first


def ln_ref(x, C, rms=False, gamma=None, beta=None, scale=None, shift=None, scale2=None, shift2=None, split=0, eps=EPS):
    """(ref, env) float64 [M, C] of out = LayerNorm(x) [* gamma + beta] * (1 + scale) + shift, or RMSNorm(x) * gamma; rows
    [0, split) use (scale2, shift2).  The envelope is the one derived in the module docstring."""
    M = x.shape[0]
    n = max(1, C // 64)
    mean = torch.zeros(M, 1, dtype=F64) if rms else x.mean(-1, keepdim=True)
    d = x - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    spread = d.abs() if rms else d.abs() + x.abs().mean(-1, keepdim=True)
    e_n = (n + 24) * U * spread * rstd
    one = torch.ones(M, C, dtype=F64)
    g = gamma.double().expand(M, C) if gamma is not None else one
    b = beta.double().expand(M, C) if beta is not None else torch.zeros(M, C, dtype=F64)
    sc, sh = _row_mod(M, C, split, scale, scale2), _row_mod(M, C, split, shift, shift2)
    k = (1 + sc) if sc is not None else one
    sh = sh if sh is not None else torch.zeros(M, C, dtype=F64)
    N, B = d * rstd * g * k, b * k
    ref = N + B + sh
    env = e_n * (g * k).abs() + U * (5 * N.abs() + 4 * B.abs() + sh.abs())
    assert float(ref.abs().max()) < SENTINEL / 4
    return ref, env


def ln_case_ref(case, x=None):
    x, mods = ln_operands(case, x)
    return ln_ref(x, case.C, rms="rms" in FORMS[case.form], split=case.split, **mods)


# f32 emulation on the CPU: the reference itself in three summation orders, and the single wrong decisions of the host tests
ORDERS = ("seq", "chunk8", "torch")


def sum32(v, order):
    """f32 sum over the last axis of v [M, C] (C a multiple of 8) in one of ORDERS -> [M, 1]"""
    M, C = v.shape
    if order == "torch":
        return v.sum(-1, keepdim=True)
    if order == "seq":          # lane l owns the 8-column chunks l, l + 64, ..: its terms in sequence, then the butterfly over 64 lanes
        L = round_up(C, 512) // 512
        t = torch.cat([v, torch.zeros(M, L * 512 - C, dtype=F32)], dim=1).view(M, L, 64, 8)
        acc = torch.zeros(M, 64, dtype=F32)
        for it in range(L):
            for j in range(8):
                acc = acc + t[:, it, :, j]
        w = 32
        while w >= 1:
            acc = acc[:, :w] + acc[:, w:2 * w]
            w //= 2
        return acc
    t = v.view(M, C // 8, 8)
    acc = t[..., 0]
    for j in range(1, 8):
        acc = acc + t[..., j]
    while acc.shape[1] > 1:
        if acc.shape[1] % 2:
            acc = torch.cat([acc, torch.zeros(M, 1, dtype=F32)], dim=1)
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc


def ln_stats32(x32, rms, order, eps=EPS, mut=None):
    """(mean, rstd) f32 [M, 1], two-pass.  mut: 'cm1' variance over C - 1 | 'noeps' | 'onepass' E[x^2] - mean^2"""
    C = x32.shape[1]
    Cf = torch.tensor(float(C), dtype=F32)
    mean = torch.zeros(x32.shape[0], 1, dtype=F32) if rms else sum32(x32, order) / Cf
    if mut == "onepass":
        var = sum32(x32 * x32, order) / Cf - mean * mean
    else:
        d = x32 - mean
        var = sum32(d * d, order) / (Cf - 1 if mut == "cm1" else Cf)
    return mean, torch.rsqrt(var if mut == "noeps" else var + torch.tensor(eps, dtype=F32))


def ln_emulate(case, order="chunk8", mut=None, x=None):
    """The case's output from an f32 evaluation on the CPU in the documented order of operations, rounded once at the store.
    mut plants ONE wrong decision: the three of ln_stats32, 'round_twice' (a bf16 rounding before the modulation), 'chunk_off'
    (scale / shift read one 8-column chunk off), 'split_off' (split + 1), 'prev_row' (the last row of an odd M computed from the
    previous row's data), 'trunc' (truncation at the store)."""
    own = x is not None
    x, mods = ln_operands(case, x)
    M, C = x.shape
    x32 = x.float()
    if mut == "prev_row":
        assert M % 2 == 1 and M > 1
        x32 = x32.clone()
        x32[M - 1] = x32[M - 2]
    rms = "rms" in FORMS[case.form]
    if own or mut in ("cm1", "noeps", "onepass", "prev_row"):
        mean, rstd = ln_stats32(x32, rms, order, mut=mut if mut in ("cm1", "noeps", "onepass") else None)
    else:
        mean, rstd = (t[:M] for t in _stats_cached(case.C, case.storage != "bf16", rms, order))
    y = (x32 - mean) * rstd
    if mut == "round_twice":
        y = y.to(BF).float()
    if "gamma" in mods:
        y = y * mods["gamma"].float()
    if "beta" in mods:
        y = y + mods["beta"].float()
    split = case.split + (1 if mut == "split_off" else 0)
    roll = (lambda t: torch.roll(t, -8)) if mut == "chunk_off" else (lambda t: t)
    sc = _row_mod(M, C, split, mods.get("scale"), mods.get("scale2"))
    sh = _row_mod(M, C, split, mods.get("shift"), mods.get("shift2"))
    if sc is not None:
        y = y * (1.0 + roll(sc.float()))
    if sh is not None:
        y = y + roll(sh.float())
    od = storage_dtypes(case.storage)[1]
    if mut == "trunc":
        assert od == BF
        return truncate_bf16(y)
    return y.to(od)


@functools.lru_cache(maxsize=None)
def _stats_cached(C, f32, rms, order):
    return ln_stats32(ln_rows(C, f32).float(), rms, order)


# ------------------------------------------------------------------------------------------------------------ qkv_prepare
class QkvCase(NamedTuple):
    H: int
    S: int
    row0: int
    mode: int                 # ROPE_*
    norm: str                 # none | one (wq, wk) | split (rows < split use wq2, wk2)
    kv: str                   # qkv | qv (k = None) | qk (v = None) | q
    f32: bool = False
    skp_extra: int = 0        # whole tiles of V^T beyond what the call needs

    @property
    def id(self):
        return (f"H{self.H}.S{self.S}.r{self.row0}.{('inter', 'complex', 'none')[self.mode]}.{self.norm}.{self.kv}."
                f"{'f32' if self.f32 else 'bf16'}.x{self.skp_extra}")

    @property
    def S_out(self):
        return self.row0 + self.S + 7

    @property
    def Skp(self):
        return self.row0 + round_up(self.S, 64) + self.skp_extra

    @property
    def split(self):
        return 0 if self.norm != "split" else (3 if self.S < 40 else 37)


QKV_H, QKV_S, QKV_ROW0 = (3, 4, 8), (5, 64, 100, 131), (0, 64)
_KVS = ("qkv", "qv", "qk", "q")


def qkv_cases(H):
    """the qkv_prepare cases of one head count: every (S, row0, rope mode, norm, storage), the k / v presence and the spare V^T
    tiles rotating so that each value meets each S and each mode"""
    out = []
    i = 0
    for S, row0, mode, norm in itertools.product(QKV_S, QKV_ROW0, (ROPE_INTERLEAVED, ROPE_COMPLEX, ROPE_NONE), ("none", "one", "split")):
        for f32 in (False, True):
            if f32 and norm == "one":
                continue
            out.append(QkvCase(H, S, row0, mode, norm, _KVS[(i + i // 4) % 4], f32, 64 * ((i // 3) % 2)))
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def qkv_operands(case):
    """dict: q, k, v float64 [S, H * 128] exact in the storage type (None where absent), wq, wk, wq2, wk2 bf16 [128] or None, table"""
    H, S = case.H, case.S
    W = H * D
    if case.norm == "none":
        q, k = grid_x(S, W, 1), grid_x(S, W, 2)
    else:
        g = torch.Generator().manual_seed(9000 + 131 * H + S)
        q, k = (torch.randn(S, W, generator=g) * 2 for _ in range(2))
        q, k = ((t if case.f32 else t.to(BF)).double() for t in (q, k))
    c = torch.arange(D)
    w = [(0.5 + ((c * m + a) % p).float() / 8).to(BF) for m, a, p in ((7, 0, 13), (5, 2, 11), (3, 1, 13), (9, 4, 11))]
    ops = dict(q=q, k=k if "k" in case.kv else None, v=grid_x(S, W, 3) if "v" in case.kv else None,
               wq=None, wk=None, wq2=None, wk2=None, table=rope_table(case.S_out, case.mode))
    if case.norm != "none":
        ops.update(wq=w[0], wk=w[1])
    if case.norm == "split":
        ops.update(wq2=w[2], wk2=w[3])
    return ops


def head_rms_ref(x, w, w2, split, eps=EPS):
    """(a, env_a) float64 [S, H, 128]: per-head RMSNorm of x [S, H, 128] times the weight of the row's stream"""
    if w is None:
        return x, torch.zeros_like(x)
    r = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    rows = torch.arange(x.shape[0]).view(-1, 1, 1)
    ws = w.double().view(1, 1, D)
    if split > 0:
        ws = torch.where(rows < split, w2.double().view(1, 1, D), ws)
    a = x * r * ws
    return a, 32 * U * x.abs() * r * ws.abs() + 2 * U * a.abs()


def qk_expected(x, H, w, w2, split, table, mode, row0, mut=None):
    """(ref, env) float64 [H, S, 128] of one of q / k [S, H * 128]: norm, RoPE with table row row0 + s, head-major layout.
    mut: 'other_entry' (rope_ref) | 'row_s' (table row s instead of row0 + s)"""
    S = x.shape[0]
    a, ea = head_rms_ref(x.reshape(S, H, D), w, w2, split)
    rows = torch.arange(S) + (0 if mut == "row_s" else row0)
    y, ey = rope_ref(a, table, mode, rows, env=ea, mut=mut)
    return y.permute(1, 0, 2).contiguous(), ey.permute(1, 0, 2).contiguous()


def qkv_expected(case, mut=None):
    """{'q': (ref, env), 'k': (ref, env) or None, 'vt': the whole expected buffer or None}.  Without norm weights the operands sit
    on the grid and the caller compares store(ref) bit for bit; env is then only the (unused) bound of the RoPE roundings."""
    o = qkv_operands(case)
    res = {"q": qk_expected(o["q"], case.H, o["wq"], o["wq2"], case.split, o["table"], case.mode, case.row0, mut), "k": None, "vt": None}
    if o["k"] is not None:
        res["k"] = qk_expected(o["k"], case.H, o["wk"], o["wk2"], case.split, o["table"], case.mode, case.row0, mut)
    if o["v"] is not None:
        res["vt"] = vt_expected(o["v"], case.H, case.Skp, case.row0, F32 if case.f32 else BF)
    return res


def placed(ref_store, S_out, row0):
    """the whole [H, S_out, 128] buffer after a call on a SENTINEL-filled one, from the stored rows [H, S, 128]"""
    H, S, _ = ref_store.shape
    out = torch.full((H, S_out, D), SENTINEL, dtype=ref_store.dtype)
    out[:, row0:row0 + S] = ref_store
    return out


def qk_emulate(x, H, w, w2, split, table, mode, row0, order, dtype):
    """f32 evaluation on the CPU of one of q / k, stored as `dtype`: [H, S, 128]"""
    S = x.shape[0]
    x32 = x.float().reshape(S * H, D)
    if w is not None:
        r = torch.rsqrt(sum32(x32 * x32, order) * torch.tensor(1.0 / D, dtype=F32) + torch.tensor(EPS, dtype=F32))
        ws = w.float().view(1, 1, D).expand(S, H, D)
        if split > 0:
            ws = torch.where(torch.arange(S).view(-1, 1, 1) < split, w2.float().view(1, 1, D), ws)
        x32 = x32 * r * ws.reshape(S * H, D)
    a = x32.view(S, H, D)
    if mode != ROPE_NONE:
        rows = torch.arange(S) + row0
        ev, od = a[..., 0::2], a[..., 1::2]
        if mode == ROPE_INTERLEAVED:
            cos, sin = table[0][rows].unsqueeze(1), table[1][rows].unsqueeze(1)
            ce, co, se, so = cos[..., 0::2], cos[..., 1::2], sin[..., 0::2], sin[..., 1::2]
        else:
            t = table[rows].unsqueeze(1)
            ce = co = t[..., 0]
            se = so = t[..., 1]
        a = torch.stack([ev * ce - od * se, od * co + ev * so], dim=-1).flatten(-2)
    return a.permute(1, 0, 2).contiguous().to(dtype)


# ------------------------------------------------------------------------------------------------------- qk_rms_rope_rows
class RowsCase(NamedTuple):
    H: int
    S: int
    row0: int
    mode: int
    kv: str                   # qkv | q
    f32: bool

    @property
    def id(self):
        return f"H{self.H}.S{self.S}.r{self.row0}.{('inter', 'complex', 'none')[self.mode]}.{self.kv}.{'f32' if self.f32 else 'bf16'}"

    @property
    def S_out(self):
        return self.row0 + self.S + 7

    @property
    def Skp(self):
        return self.row0 + round_up(self.S, 64)


def rows_cases():
    out = []
    for i, (H, S, row0, kv, f32) in enumerate(itertools.product((24, 40), (5, 100), (0, 64), ("qkv", "q"), (False, True))):
        out.append(RowsCase(H, S, row0, (ROPE_COMPLEX, ROPE_INTERLEAVED, ROPE_NONE)[(i + i // 3) % 3], kv, f32))
    return out


@functools.lru_cache(maxsize=None)
def rows_operands(H, S, f32):
    """q, k float64 [S, H * 128] random (rows 1 / 2 / 3: tiny, zero, small), v on the grid, wq / wk bf16 [H * 128]"""
    W = H * D
    g = torch.Generator().manual_seed(11000 + H * 7 + S)
    q, k = (torch.randn(S, W, generator=g) * 2 for _ in range(2))
    q, k = ((t if f32 else t.to(BF)).double() for t in (q, k))
    q[1] *= 2.0 ** -10
    q[2] = 0.0
    k[3] *= 2.0 ** -7
    c = torch.arange(W)
    return dict(q=q, k=k, v=grid_x(S, W, 5), wq=(0.5 + ((c * 7) % 13).float() / 8).to(BF), wk=(0.5 + ((c * 5 + 2) % 11).float() / 8).to(BF))


def rope_only_expected(a, H, table, mode, row0):
    """(ref, env) [H, S, 128] of the RoPE + layout pass on storage values a [S, H * 128] that carry no error of their own"""
    return qk_expected(a, H, None, None, 0, table, mode, row0)


# --------------------------------------------------------------------------------------------------------------------- casts
def _i32(v):
    """int64 bit patterns -> int32 tensor with the same low 32 bits"""
    return torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)


def normal_bf16_codes():
    b = torch.arange(65536, dtype=torch.int64)
    e = (b >> 7) & 0xFF
    return b[(e >= 1) & (e <= 254)]


def cast_probe_inputs():
    """f32 [3 x 65024 + 8]: for every normal bf16 code point the f32 midpoint to the next code point away from zero and its two
    f32 neighbours; then +-0, +-inf, +-the largest float, +-the first float above the largest bf16.  No subnormal results."""
    b = normal_bf16_codes() << 16
    bits = torch.cat([b + 0x7FFF, b + 0x8000, b + 0x8001,
                      torch.tensor([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0001, 0xFF7F0001])])
    return _i32(bits).view(F32).clone()


def cast_nan_inputs():
    return _i32(torch.tensor([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFF812345])).view(F32).clone()


def all_bf16_codes():
    """bf16 [65536]: every code point"""
    return torch.arange(65536, dtype=torch.int64).sub(32768).to(torch.int16).view(BF).clone()
