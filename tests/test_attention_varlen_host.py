"""Host side (no GPU) of attention over a packed variable-length batch: the two float64 statements of the rule
(tests/attention_varlen_ref.py) agree, the comparisons tests/test_gpu_attention_varlen.py uses reject a boundary moved by one key
and a neighbouring sequence's key, the V^T slot layout is aligned, disjoint and inside its pitch, and apexmi_attn_fwd_varlen,
ops.attention_varlen and the "hip_mfma_varlen" backend refuse every invalid argument before any device call."""
import math

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from apex_studio_amd.attention_backend import KEY_VARLEN, hip_mfma_varlen
from apex_studio_amd.lib import ApexMIError
from tests import attention_probes as P
from tests import attention_varlen_ref as R

BF, F16 = torch.bfloat16, torch.float16


# ------------------------------------------------------------------------------------------------- the yardsticks, on the CPU
def test_geometries_cover_the_edges():
    ql, kl = R.GEOMETRIES["cross"]
    assert (sum(ql), sum(kl)) == (406, 531) and len(ql) == len(kl)
    assert 0 in ql and 0 in kl and 1 in ql                                   # empty query sequence, no keys, one row
    assert any(l % 128 == 0 and l for l in ql) and any(l % 64 == 0 and l for l in kl)
    assert any(l % 128 for l in ql) and any(l % 64 for l in kl) and any(l > 128 for l in ql) and any(l > 64 for l in kl)
    assert any(c % 8 for c in R.cu_of(ql).tolist()) and any(c % 8 for c in R.cu_of(kl).tolist())
    assert any(lq and not lk for lq, lk in zip(ql, kl))                      # queries without keys
    for name, (ql, kl) in R.GEOMETRIES.items():
        for setting in R.MAX_SEQLENS:
            mq, mk = R.max_seqlens(ql, kl, setting)
            assert mq >= max(ql) and mk >= max(kl)
    assert R.GEOMETRIES["self"][0] == R.GEOMETRIES["self"][1]


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("geometry", list(R.GEOMETRIES))
def test_dense_weights_and_per_sequence_reference_agree(geometry, causal):
    ql, kl = R.GEOMETRIES[geometry]
    g = torch.Generator().manual_seed(3)
    q = torch.randn(sum(ql), R.HQ, 16, generator=g, dtype=torch.float64)
    k = torch.randn(sum(kl), R.HKV, 16, generator=g, dtype=torch.float64)
    v = torch.randn(sum(kl), R.HKV, 16, generator=g, dtype=torch.float64)
    w = R.varlen_weights(ql, kl, causal)
    # the weight array: as many allowed keys per row as the rule says, none outside the row's own sequence
    cq, ck = R.cu_of(ql).tolist(), R.cu_of(kl).tolist()
    for i, (lq, lk) in enumerate(zip(ql, kl)):
        rows = w[cq[i]:cq[i + 1]]
        want = torch.arange(1, lq + 1).clamp(max=lk).double() if causal else torch.full((lq,), float(lk), dtype=torch.float64)
        assert torch.equal(rows.sum(-1), want) and torch.equal(rows[:, ck[i]:ck[i + 1]].sum(-1), want)
    o1, l1 = R.dense_ref(q, k, v, ql, kl, causal, 0.7)
    o2, l2 = R.varlen_ref(q, k, v, ql, kl, causal, 0.7)
    dead = w.sum(-1) == 0
    assert bool(dead.any()) == (geometry == "cross")
    assert torch.equal(torch.isinf(l1), dead[None].expand_as(l1)) and torch.equal(torch.isinf(l2), torch.isinf(l1))
    assert torch.equal(o1[dead], torch.zeros_like(o1[dead])) and torch.equal(o2[dead], torch.zeros_like(o2[dead]))
    assert (o1 - o2).abs().max() < 1e-12
    assert (l1 - l2)[~torch.isinf(l1)].abs().max() < 1e-12


@pytest.mark.parametrize("dtype,D", R.FORMATS)
@pytest.mark.parametrize("causal", [False, True])
def test_membership_check_rejects_a_moved_boundary_and_a_neighbours_key(dtype, D, causal):
    """the probe of the GPU test: V codes the GLOBAL packed key index, so a key of the wrong sequence is a wrong code"""
    ql, kl = R.GEOMETRIES["cross"]
    Tk = sum(kl)
    assert Tk <= 1024                                                          # one key more or less moves a column by >= 1 / 33
    w = R.varlen_weights(ql, kl, causal)[None, None].expand(1, R.HQ, -1, -1).contiguous()
    v = P.code_values(1, R.HKV, Tk, D, dtype)
    ref = P.membership_expected(w, v)
    assert P.membership_ok(ref.to(dtype), ref, dtype)
    flips = [(i, j) for i, j in R.boundary_flips(ql, kl)]
    assert len(flips) >= 20
    admitted = [(i, j) for i, j in flips if w[0, 0, i, j] == 0]
    dropped = [(i, j) for i, j in flips if w[0, 0, i, j] > 0]
    assert admitted and dropped
    for h in (0, R.HQ - 1):
        assert P.membership_mutants(w, v, ref, dtype, flips, (0, h)) == []
    # the counting probe: one key more or less moves ln n by more than a hundred bars
    n = w.sum(-1)
    assert float(n.max()) <= 1024 and math.log(1025 / 1024) > 90 * 1e-5


def test_vt_slots_are_aligned_disjoint_and_inside_the_pitch():
    g = torch.Generator().manual_seed(5)
    lists = [list(kl) for _, kl in R.GEOMETRIES.values()] + [[0], [1], [64], [0, 0, 1], [63, 1, 64, 65]]
    for _ in range(2000):
        n = int(torch.randint(1, 9, (1,), generator=g))
        lists.append([int(x) * int(torch.randint(0, 2, (1,), generator=g)) for x in torch.randint(0, 300, (n,), generator=g)])
    for kl in lists:
        starts, pitch = R.vt_slots(kl)
        end_prev = 0
        for s, l in zip(starts, kl):
            assert s % 64 == 0 and s >= end_prev
            end_prev = s + (l + 63) // 64 * 64                                  # the padded tail tile belongs to the slot
        assert end_prev <= pitch
        if sum(kl):
            need = lib.load().apexmi_attn_varlen_workspace_bytes(sum(kl), len(kl), R.HKV, 128)
            assert need >= R.HKV * 128 * pitch * 2 and need % 256 == 0 and need < R.HKV * 128 * pitch * 2 + 256


# -------------------------------------------------------------------------------------------------------- the C entry refuses
def _bad(L, rc, needle):
    msg = L.apexmi_last_error().decode()
    assert rc != 0 and needle in msg and msg.startswith("attn_fwd_varlen:"), (rc, msg)


def test_cabi_argument_checks():
    L = lib.load()
    Pn = 0x100000
    s2 = lib.i64x2((4 * 128, 128))
    l2 = lib.i64x2((406, 1))
    big = 1 << 30

    def call(q=Pn, out=Pn, lse=Pn, cu_q=Pn, cu_k=Pn, n=5, Tq=406, Tk=531, Hq=4, Hkv=2, D=128, mq=200, mk=333, st=s2, ost=s2, lst=l2,
             dtype=lib.BF16, ws=Pn, wsb=big):
        return L.apexmi_attn_fwd_varlen(q, Pn, Pn, out, lse, cu_q, cu_k, n, Tq, Tk, Hq, Hkv, D, mq, mk, st, st, st, ost, lst, 0, 0.1,
                                        dtype, ws, wsb, None)

    _bad(L, call(q=None), "null operand")
    _bad(L, call(out=None), "null operand")
    _bad(L, call(st=None), "null operand")
    _bad(L, call(cu_q=None), "cu_seqlens")
    _bad(L, call(cu_k=Pn + 2), "cu_seqlens")
    _bad(L, call(lse=Pn + 2), "lse")
    _bad(L, call(lst=None), "lse")
    _bad(L, call(n=0), "empty problem")
    _bad(L, call(Tq=0), "empty problem")
    _bad(L, call(Tk=0), "empty problem")
    _bad(L, call(Hkv=0), "empty problem")
    _bad(L, call(mq=0), "max_seqlen_q=0")
    _bad(L, call(mk=-3), "max_seqlen_k=-3")
    _bad(L, call(D=80), "head dim 80")
    _bad(L, call(dtype=lib.F32), "dtype 2")
    _bad(L, call(Hkv=3), "head ratio")
    _bad(L, call(n=70000), "grid too large")
    _bad(L, call(n=60000, Hq=60000, Hkv=60000, Tq=1 << 20, mq=1 << 20), "grid too large")
    _bad(L, call(st=lib.i64x2((4 * 128, 100))), "16-byte aligned")
    _bad(L, call(q=Pn + 8), "16-byte aligned")
    _bad(L, call(wsb=16), "workspace too small")
    _bad(L, call(ws=None), "workspace too small")
    assert L.apexmi_attn_varlen_workspace_bytes(531, 5, 2, 64) == 2 * 64 * (576 + 320) * 2
    for args in ((0, 5, 2, 64), (531, 0, 2, 64), (531, 5, 0, 64), (531, 5, 2, 80)):
        assert L.apexmi_attn_varlen_workspace_bytes(*args) == 0


# ------------------------------------------------------------------------------------------------ the Python operators refuse
def _operands(Tq=12, Tk=20, Hq=4, Hkv=2, D=64, dtype=BF):
    q = torch.zeros(Tq, Hq, D, dtype=dtype)
    k = torch.zeros(Tk, Hkv, D, dtype=dtype)
    cu_q, cu_k = torch.tensor([0, 5, Tq], dtype=torch.int32), torch.tensor([0, 9, Tk], dtype=torch.int32)
    return q, k, k.clone(), cu_q, cu_k


def test_ops_attention_varlen_refuses_each_invalid_argument():
    q, k, v, cu_q, cu_k = _operands()

    def refuses(needle, *args, **kw):
        with pytest.raises(ApexMIError, match=needle) as e:
            ops.attention_varlen(*args, **kw)
        assert str(e.value).startswith("attention_varlen"), str(e.value)

    ok = dict(enable_gqa=True)
    refuses("dtypes", q.float(), k.float(), v.float(), cu_q, cu_k, 7, 11, **ok)
    refuses("dtypes", q, k.half(), v, cu_q, cu_k, 7, 11, **ok)
    refuses("3-D packed", q[None], k[None], v[None], cu_q, cu_k, 7, 11, **ok)
    refuses("3-D packed", q, k, v[0], cu_q, cu_k, 7, 11, **ok)
    refuses("head dim 80", q[..., :0].new_zeros(12, 4, 80), k.new_zeros(20, 2, 80), k.new_zeros(20, 2, 80), cu_q, cu_k, 7, 11, **ok)
    refuses("do not match", q, k, v[:10], cu_q, cu_k, 7, 11, **ok)
    refuses("do not match", q, k.new_zeros(20, 2, 128), k.new_zeros(20, 2, 128), cu_q, cu_k, 7, 11, **ok)
    refuses("empty problem", q[:0], k, v, cu_q, cu_k, 7, 11, **ok)
    refuses("empty problem", q, k[:0], v[:0], cu_q, cu_k, 7, 11, **ok)
    refuses("enable_gqa", q, k, v, cu_q, cu_k, 7, 11)                                        # 4 heads over 2 without the keyword
    refuses("whole ratio", q, k.new_zeros(20, 3, 64), k.new_zeros(20, 3, 64), cu_q, cu_k, 7, 11, **ok)
    refuses("cu_seqlens_q must be", q, k, v, cu_q.long(), cu_k, 7, 11, **ok)
    refuses("cu_seqlens_k must be", q, k, v, cu_q, cu_k.float(), 7, 11, **ok)
    refuses("cu_seqlens_q must be", q, k, v, [0, 5, 12], cu_k, 7, 11, **ok)
    refuses("cu_seqlens_k must be", q, k, v, cu_q, cu_k[None], 7, 11, **ok)
    refuses("cu_seqlens_k must be", q, k, v, cu_q, torch.tensor([0, 0, 9, 0, 20, 0], dtype=torch.int32)[::2], 7, 11, **ok)
    refuses("entries", q, k, v, cu_q, cu_k[:2], 7, 11, **ok)
    refuses("entries", q, k, v, cu_q[:1], cu_k[:1], 7, 11, **ok)
    refuses("max_seqlen_q=0", q, k, v, cu_q, cu_k, 0, 11, **ok)
    refuses("max_seqlen_k=-1", q, k, v, cu_q, cu_k, 7, -1, **ok)
    refuses("no CPU fallback", q, k, v, cu_q, cu_k, 7, 11, **ok)                             # everything valid but the device
    refuses("no CPU fallback", q, k[:, :1], v[:, :1], cu_q, cu_k, 7, 11)                     # Hkv == 1 needs no keyword
    if torch.cuda.is_available():
        refuses("is on", q.cuda(), k.cuda(), v.cuda(), cu_q, cu_k.cuda(), 7, 11, **ok)
        refuses("are on", q.cuda(), k, v, cu_q.cuda(), cu_k.cuda(), 7, 11, **ok)


def test_backend_refuses_each_invalid_argument():
    q, k, v, cu_q, cu_k = _operands()
    kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_seqlen_q=7, max_seqlen_k=11, enable_gqa=True)

    def refuses(needle, *args, **kwargs):
        with pytest.raises(ApexMIError, match=needle) as e:
            hip_mfma_varlen(*args, **kwargs)
        return str(e.value)

    assert refuses("dropout", q, k, v, dropout_p=0.1, **kw).startswith("hip_mfma_varlen")
    assert refuses("attn_mask", q, k, v, attn_mask=torch.ones(12, 20, dtype=torch.bool), **kw).startswith("hip_mfma_varlen")
    for missing in ("cu_seqlens_q", "cu_seqlens_k", "max_seqlen_q", "max_seqlen_k"):
        assert refuses("required", q, k, v, **{n: x for n, x in kw.items() if n != missing}).startswith("hip_mfma_varlen")
    q4, k4, v4 = (t.permute(1, 0, 2)[None] for t in (q, k, v))
    assert refuses("batch dimension 1", q4.expand(2, -1, -1, -1), k4.expand(2, -1, -1, -1), v4.expand(2, -1, -1, -1),
                   **kw).startswith("hip_mfma_varlen")
    assert refuses("all be packed", q4, k, v, **kw).startswith("hip_mfma_varlen")
    assert refuses("all be packed", q[0], k[0], v[0], **kw).startswith("hip_mfma_varlen")
    # valid but for the device: both layouts reach the operator, which refuses CPU tensors; nothing falls back
    assert refuses("no CPU fallback", q, k, v, **kw).startswith("attention_varlen")
    assert refuses("no CPU fallback", q4, k4, v4, is_causal=True, return_lse=True, **kw).startswith("attention_varlen")
    assert refuses("enable_gqa", q4, k4, v4, **{**kw, "enable_gqa": False}).startswith("attention_varlen")


def test_the_key_is_registered_on_request_and_disturbs_nothing():
    from apex_studio_amd.register import FunctionRegister
    reg = FunctionRegister()
    ab.register(reg, set_default=True, varlen=True)
    assert KEY_VARLEN == ab.KEY_VARLEN == "hip_mfma_varlen" and reg.get(KEY_VARLEN) is hip_mfma_varlen
    assert reg.get(ab.KEY) is ab.hip_mfma and reg.get(ab.KEY_SDPA) is ab.hip_mfma_sdpa and reg.get(ab.KEY_WINDOW) is ab.hip_mfma_window
    assert reg.get_default() == ab.KEY
    assert reg.is_available(ab.KEY_VARLEN) == reg.is_available(ab.KEY)
    assert sorted(reg) == sorted((ab.KEY, ab.KEY_SDPA, ab.KEY_WINDOW, ab.KEY_VARLEN))
    reg2 = FunctionRegister()
    ab.register(reg2)
    assert ab.KEY_VARLEN not in reg2
