"""Float64 yardsticks of the log-sum-exp output and of the merge over key chunks.  Pure torch on the CPU;
tests/test_attention_lse_host.py proves them against each other before tests/test_gpu_attention_lse.py holds the kernels to them.
The rule of a call is the weight array of attention_probes.weights_of: w = 0 excluded, 1 allowed, exp(additive mask)."""
import torch

NEG_INF = float("-inf")


def scores_of(q, k, scale):
    """scale q k^T in float64, [B, Hq, Sq, Sk] (grouped-query heads: query head h reads kv head h / group)"""
    kk = k.to(torch.float64).repeat_interleave(q.shape[1] // k.shape[1], dim=1)
    return (q.to(torch.float64) @ kk.transpose(2, 3)) * scale


def lse_ref(q, k, w, scale):
    """lse[b, h, i] = ln sum_j w_ij exp(scale q_i k_j); -inf for a row whose weights are all 0"""
    s = scores_of(q, k, scale) + torch.log(w)
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)                 # a dead row: exp(-inf - 0) = 0, ln 0 = -inf
    return (m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))).squeeze(-1)


def attention_ref(q, k, v, w, scale):
    """(out [B, Hq, Sq, D], lse [B, Hq, Sq]) in float64; a row without an allowed key is zero"""
    lse = lse_ref(q, k, w, scale)
    safe = torch.where(torch.isinf(lse), torch.zeros_like(lse), lse)
    p = torch.exp(scores_of(q, k, scale) + torch.log(w) - safe[..., None])   # dead rows: exp(-inf) = 0
    vv = v.to(torch.float64).repeat_interleave(q.shape[1] // v.shape[1], dim=1)
    return p @ vv, lse


def merge_ref(outs, lses):
    """m = max_p lse_p, w_p = exp(lse_p - m) (0 for lse_p = -inf), out = sum_p w_p out_p / sum_p w_p, lse = m + ln sum_p w_p; a
    row whose lse_p are all -inf gives out = 0 and lse = -inf.  A partial of weight 0 contributes nothing whatever it holds."""
    L = torch.stack([l.to(torch.float64) for l in lses])                    # [n, B, H, Sq]
    O = torch.stack([o.to(torch.float64) for o in outs])                    # [n, B, H, Sq, D]
    m = L.max(0).values
    dead = torch.isinf(m) & (m < 0)
    wgt = torch.where(torch.isinf(L) & (L < 0), torch.zeros_like(L), torch.exp(L - torch.where(dead, torch.zeros_like(m), m)))
    den = wgt.sum(0)
    num = torch.where(wgt[..., None] > 0, wgt[..., None] * O, torch.zeros_like(O)).sum(0)
    out = torch.where(dead[..., None], torch.zeros_like(num), num / den.clamp_min(1e-300)[..., None])
    lse = torch.where(dead, torch.full_like(m, NEG_INF), m + torch.log(den.clamp_min(1e-300)))
    return out, lse
