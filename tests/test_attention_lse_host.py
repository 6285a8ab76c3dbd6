"""Host side (no GPU) of the log-sum-exp output and the merge over key chunks: the C-ABI argument checks of
apexmi_attn_fwd_masked_lse and apexmi_attn_merge, the refusals of the Python operators, and the proof of the float64 yardsticks
(tests/attention_lse_ref.py) that tests/test_gpu_attention_lse.py holds the kernels to: merge_ref over uneven chunks of the keys
reproduces the one-piece reference."""
import ctypes

import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError
from tests import attention_probes as P
from tests.attention_lse_ref import attention_ref, lse_ref, merge_ref


def _bad(L, rc, needle):
    msg = L.apexmi_last_error().decode()
    assert rc != 0 and needle in msg, (rc, msg)


def test_cabi_argument_checks_lse():
    L = lib.load()
    Pn = 0x100000
    s3 = lib.i64x3((8 * 128 * 64, 8 * 128, 128))
    l3 = lib.i64x3((8 * 64, 64, 1))
    m4 = lib.i64x4((0, 0, 64, 1))
    big = 1 << 30

    def call(q=Pn, lse=Pn, B=1, Hq=8, Hkv=8, Sq=64, Sk=64, D=128, mask=None, mcode=lib.MASK_BOOL, mst=m4, dtype=lib.BF16, ws=Pn,
             wsb=big, st=s3, lst=l3):
        return L.apexmi_attn_fwd_masked_lse(q, Pn, Pn, Pn, lse, B, Hq, Hkv, Sq, Sk, D, st, st, st, st, lst, mask, mcode, mst, 0,
                                            0.1, dtype, ws, wsb, None)

    _bad(L, call(lse=None), "lse")
    _bad(L, call(lst=None), "lse")
    _bad(L, call(lse=Pn + 2), "lse")
    _bad(L, call(q=None), "null operand")
    _bad(L, call(Sq=0), "empty problem")
    _bad(L, call(D=96), "head dim 96")
    _bad(L, call(dtype=lib.F32), "dtype")
    _bad(L, call(dtype=7), "dtype 7")
    _bad(L, call(Hkv=3), "head ratio")
    _bad(L, call(mask=Pn, mcode=7), "mask dtype code 7")
    _bad(L, call(mask=Pn, mst=lib.i64x4((0, 0, 64, 2))), "mask key stride")
    _bad(L, call(st=lib.i64x3((8 * 128 * 64, 8 * 128, 100))), "16-byte aligned")
    _bad(L, call(wsb=16), "workspace too small")
    # the messages name the entry that was called
    call(D=96)
    assert L.apexmi_last_error().decode().startswith("attn_fwd_masked_lse:")


def test_cabi_argument_checks_merge():
    L = lib.load()
    Pn = 0x100000
    o3 = lib.i64x3((64 * 8 * 128, 8 * 128, 128))
    l3 = lib.i64x3((8 * 64, 64, 1))

    def call(n=2, outs=None, lses=None, out=Pn, lse_out=None, B=1, H=8, Sq=64, D=128, ost=o3, lst=l3, dtype=lib.BF16):
        optr = (ctypes.c_void_p * 9)(*([Pn] * 9 if outs is None else outs))
        lptr = (ctypes.c_void_p * 9)(*([Pn] * 9 if lses is None else lses))
        return L.apexmi_attn_merge(n, optr, lptr, out, lse_out, B, H, Sq, D, ost, lst, dtype, None)

    _bad(L, call(n=0), "n=0")
    _bad(L, call(n=9), "n=9")
    _bad(L, call(n=-1), "n=-1")
    _bad(L, call(D=100), "head dim 100")
    _bad(L, call(D=0), "empty problem")
    _bad(L, call(Sq=0), "empty problem")
    _bad(L, call(dtype=lib.F32), "dtype 2")
    _bad(L, call(dtype=9), "dtype 9")
    _bad(L, call(out=None), "null operand")
    _bad(L, call(ost=None), "null operand")
    _bad(L, call(n=3, outs=[Pn, Pn, None] + [Pn] * 6), "null partial 2")
    _bad(L, call(n=2, lses=[Pn, None] + [Pn] * 7), "null partial 1")
    _bad(L, call(n=2, lses=[Pn, Pn + 64] + [Pn] * 7, lse_out=Pn + 64), "lse_out must not be lses[1]")
    _bad(L, call(outs=[Pn + 8] + [Pn] * 8), "16-byte aligned")
    _bad(L, call(ost=lib.i64x3((64 * 8 * 128, 8 * 128, 100))), "16-byte aligned")
    _bad(L, L.apexmi_attn_merge(1, None, None, Pn, None, 1, 8, 64, 128, o3, l3, lib.BF16, None), "null operand")


# ------------------------------------------------------------------------------------------------- the yardstick, on the CPU
def _problem(seed=0, B=2, Hq=4, Hkv=2, Sq=37, Sk=90, D=16):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Hq, Sq, D, generator=g, dtype=torch.float64)
    k = torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64)
    v = torch.randn(B, Hkv, Sk, D, generator=g, dtype=torch.float64)
    return q, k, v


def _chunks(Sk, cuts):
    edges = [0] + list(cuts) + [Sk]
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("kind", ["none", "bool", "additive", "causal & bool"])
def test_merge_ref_over_uneven_chunks_is_the_one_piece_reference(kind):
    B, Hq, Hkv, Sq, Sk, D = 2, 4, 2, 37, 90, 16
    q, k, v = _problem()
    mask, causal = None, False
    if kind in ("bool", "causal & bool"):
        mask = P._rand_bool((B, 1, Sq, Sk), 1, 0.5)
        mask[:, :, 3] = False                                   # a row without any allowed key
        mask[:, :, 5, 20:] = False                              # rows whose keys all sit in one chunk: the first ...
        mask[:, :, 6] = False
        mask[:, :, 6, 20] = True                                # ... the one-key chunk ...
        mask[:, :, 7, :21] = False                              # ... the last
        causal = kind == "causal & bool"
    elif kind == "additive":
        mask = P._additive((1, Hq, Sq, Sk), 2, torch.float32, dead_rows=(0, 36))
        mask[..., 9, :21] = float("-inf")
    w = P.weights_of(mask, B, Hq, Sq, Sk, causal)
    scale = 0.7
    ref_o, ref_l = attention_ref(q, k, v, w, scale)
    dead = w.sum(-1) == 0
    assert torch.equal(torch.isinf(ref_l) & (ref_l < 0), dead) and (kind == "none" or bool(dead.any()))
    assert torch.equal(ref_o[dead], torch.zeros_like(ref_o[dead]))
    # torch's own logsumexp and softmax agree with the restatement on the live rows
    s = (q @ k.repeat_interleave(2, 1).transpose(2, 3)) * scale + torch.log(w)
    assert (torch.logsumexp(s, -1)[~dead] - ref_l[~dead]).abs().max() < 1e-12
    assert ((torch.softmax(s, -1).nan_to_num(0.0) @ v.repeat_interleave(2, 1)) - ref_o).abs().max() < 1e-12

    for cuts in ((20, 21), (64,), (1, 2, 3, 50, 51, 70, 89)):   # a one-key chunk, a tile boundary, 8 chunks
        parts = [attention_ref(q, k[:, :, a:b], v[:, :, a:b], w[..., a:b], scale) for a, b in _chunks(Sk, cuts)]
        if kind != "none" and cuts == (20, 21):
            assert any(bool((torch.isinf(l) & ~dead).any()) for _, l in parts)          # a live row that is dead in some chunk
        out, lse = merge_ref([p[0] for p in parts], [p[1] for p in parts])
        assert torch.isfinite(out).all() and not torch.isnan(lse).any()
        assert torch.equal(torch.isinf(lse), dead) and torch.equal(out[dead], torch.zeros_like(out[dead]))
        assert (out - ref_o).abs().max() < 1e-12
        assert (lse[~dead] - ref_l[~dead]).abs().max() < 1e-12


def test_merge_ref_ignores_a_partial_of_weight_zero_and_keeps_one_partial():
    g = torch.Generator().manual_seed(3)
    o = torch.randn(1, 2, 5, 8, generator=g, dtype=torch.float64)
    l = torch.randn(1, 2, 5, generator=g, dtype=torch.float64) * 30
    out, lse = merge_ref([o], [l])
    assert torch.equal(out, o) and torch.equal(lse, l)
    junk = torch.full_like(o, float("nan"))
    out, lse = merge_ref([junk, o], [torch.full_like(l, float("-inf")), l])
    assert torch.equal(out, o) and torch.equal(lse, l)


def test_lse_ref_counts_keys_when_q_is_zero():
    c = P.masked_cases()["gqa 4/2 causal & bool 129x333 bf16 D128"]
    w = P.case_weights(c)
    q = torch.zeros(c["B"], c["Hq"], c["Sq"], c["D"])
    k = torch.randn(c["B"], c["Hkv"], c["Sk"], c["D"])
    n = w.sum(-1)
    lse = lse_ref(q, k, w, 0.3)
    assert torch.equal(torch.isinf(lse), n == 0)
    assert (lse[n > 0] - torch.log(n[n > 0])).abs().max() < 1e-12


# ------------------------------------------------------------------------------------------------- the Python operators refuse
def test_ops_refuse_cpu_tensors_and_mismatched_shapes():
    q = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(ApexMIError):
        ops.attention_masked(q, q, q, return_lse=True)
    with pytest.raises(ApexMIError):
        ab.hip_mfma_sdpa(q, q, q, return_lse=True)
    with pytest.raises(ApexMIError):
        ops.attention_chunked(q, [q, q], [q, q])
    lse = torch.zeros(1, 2, 8)
    with pytest.raises(ApexMIError, match="device"):
        ops.attention_merge([q], [lse])
    with pytest.raises(ApexMIError, match="1 to 8"):
        ops.attention_merge([], [])
    with pytest.raises(ApexMIError, match="1 to 8"):
        ops.attention_merge([q] * 9, [lse] * 9)
    with pytest.raises(ApexMIError, match="equally many"):
        ops.attention_merge([q, q], [lse])
    with pytest.raises(ApexMIError, match="1 to 8"):
        ops.attention_chunked(q, [], [])
    with pytest.raises(ApexMIError, match="1 to 8"):
        ops.attention_chunked(q, [q] * 9, [q] * 9)
    with pytest.raises(ApexMIError, match="masks"):
        ops.attention_chunked(q, [q, q], [q, q], attn_masks=[None])


def test_merge_refuses_mismatched_operands():
    o = torch.zeros(2, 8, 3, 64, dtype=torch.bfloat16).permute(0, 2, 1, 3)          # [B, H, Sq, D] = [2, 3, 8, 64]
    l = torch.zeros(2, 3, 8)
    for outs, lses in (([o, o[:, :, :4]], [l, l]), ([o, o.half()], [l, l]), ([o, o], [l, l[:, :, :4]]), ([o[..., :60]], [l]),
                       ([o[0]], [l[0]])):
        with pytest.raises(ApexMIError, match="match|multiple of 8"):
            ops.attention_merge(outs, lses)
    with pytest.raises(ApexMIError, match="dtype"):
        ops.attention_merge([o.float()], [l])
    with pytest.raises(ApexMIError, match="float32"):
        ops.attention_merge([o], [l.double()])
