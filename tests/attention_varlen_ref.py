"""Float64 yardsticks of attention over a packed variable-length batch (ops.attention_varlen).  Pure torch on
the CPU; tests/test_attention_varlen_host.py proves them against each other before tests/test_gpu_attention_varlen.py holds the
kernel to them.  Two statements of the same rule:
  * varlen_weights: the DENSE weight array [Tq, Tk] over the packed tokens, block-diagonal (query row cu_q[i] + r sees keys
    cu_k[i] .. cu_k[i+1] - 1 only), AND-ed with the local causal rule (local key j <= local query r, top-left per sequence);
  * varlen_ref: one attention_lse_ref.attention_ref call per sequence on that sequence's rows alone.
Packed layouts: q / out [Tq, Hq, D], k / v [Tk, Hkv, D], lse [Hq, Tq]."""
import torch

from tests import attention_probes as P
from tests.attention_lse_ref import NEG_INF, attention_ref

HQ, HKV = 4, 2
FORMATS = ((P.BF, 128), (P.F16, 64), (P.BF, 64), (P.F16, 128))
# name -> (query lengths, key lengths).  cross: a tail in the 128-row block (200) and in the 64-key tile (333, 5, 129), a one-row
# sequence, an empty query sequence, a sequence without keys, exact multiples (128, 64) and cu offsets that are no multiples of 8
GEOMETRIES = {"cross": ((200, 1, 0, 128, 77), (333, 64, 5, 0, 129)),
              "self": ((200, 1, 128, 77), (200, 1, 128, 77))}
MAX_SEQLENS = ("exact", (256, 384))          # the second leaves idle query blocks and idle V^T tiles in every sequence


def cu_of(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0).tolist()), dtype=torch.int32)


def max_seqlens(q_lens, k_lens, setting):
    return (max(q_lens), max(k_lens)) if setting == "exact" else setting


def varlen_weights(q_lens, k_lens, causal=False):
    """w [Tq, Tk] float64 in {0, 1}"""
    w = torch.zeros(sum(q_lens), sum(k_lens), dtype=torch.float64)
    q0 = k0 = 0
    for lq, lk in zip(q_lens, k_lens):
        blk = torch.ones(lq, lk, dtype=torch.float64)
        if causal:
            blk = blk * P.causal_rule(lq, lk).to(torch.float64)
        w[q0:q0 + lq, k0:k0 + lk] = blk
        q0, k0 = q0 + lq, k0 + lk
    return w


def _bhsd(t):
    """packed [T, H, D] -> [1, H, T, D]"""
    return t.permute(1, 0, 2)[None]


def dense_ref(q, k, v, q_lens, k_lens, causal, scale):
    """(out [Tq, Hq, D], lse [Hq, Tq]) float64: ONE attention over the packed tokens under the dense weight array"""
    w = varlen_weights(q_lens, k_lens, causal)[None, None].expand(1, q.shape[1], -1, -1)
    o, l = attention_ref(_bhsd(q), _bhsd(k), _bhsd(v), w, scale)
    return o[0].permute(1, 0, 2).contiguous(), l[0]


def varlen_ref(q, k, v, q_lens, k_lens, causal, scale):
    """(out [Tq, Hq, D], lse [Hq, Tq]) float64: attention_ref per sequence; a sequence without keys gives zero rows and -inf"""
    Tq, Hq, D = q.shape
    out = torch.zeros(Tq, Hq, D, dtype=torch.float64)
    lse = torch.full((Hq, Tq), NEG_INF, dtype=torch.float64)
    q0 = k0 = 0
    for lq, lk in zip(q_lens, k_lens):
        if lq and lk:
            w = P.weights_of(None, 1, Hq, lq, lk, causal)
            o, l = attention_ref(_bhsd(q[q0:q0 + lq]), _bhsd(k[k0:k0 + lk]), _bhsd(v[k0:k0 + lk]), w, scale)
            out[q0:q0 + lq] = o[0].permute(1, 0, 2)
            lse[:, q0:q0 + lq] = l[0]
        q0, k0 = q0 + lq, k0 + lk
    return out, lse


def boundary_flips(q_lens, k_lens):
    """(packed row, packed key) decisions at every sequence's key boundaries, for its first and last row: the neighbouring
    sequences' nearest keys (a flip admits them) and the sequence's own first and last key (a flip drops them: the boundary moved
    by one key)"""
    Tk = sum(k_lens)
    pos = set()
    q0 = k0 = 0
    for lq, lk in zip(q_lens, k_lens):
        for r in {q0, q0 + lq - 1} if lq else ():
            pos |= {(r, j) for j in (k0 - 1, k0, k0 + lk - 1, k0 + lk) if 0 <= j < Tk}
        q0, k0 = q0 + lq, k0 + lk
    return sorted(pos)


def vt_slots(k_lens):
    """(first column of every sequence's V^T slot, pitch): slot i starts at align64(cu_k[i]) + 64 i, pitch = align64(Tk) + 64 n"""
    a64 = lambda x: (x + 63) // 64 * 64   # noqa: E731
    cu = cu_of(k_lens).tolist()
    return [a64(cu[i]) + 64 * i for i in range(len(k_lens))], a64(cu[-1]) + 64 * len(k_lens)
