"""The Python refusals of the flash wrappers that refuse a CPU tensor first (ops.attention_masked, attention_window,
attention_wide, attention_chunked), as complete messages on tiny device tensors, and the keys of the workspace cache.  The
literals and the key set are what the wrappers gave before they shared their front end (ops._flash_qkv, ops._workspace): the
reference, not the code under test.  The refusal rows launch nothing."""
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import lib, ops
from apex_studio_amd.lib import ApexMIError

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def T(*shape, dtype=BF):
    return torch.zeros(shape, dtype=dtype, device=DEV)


def _plan(Sq=8, Sk=8):
    """a window plan put together by hand: nothing is launched"""
    return ops.WindowPlan(torch.zeros(Sq, 4, dtype=torch.int16, device=DEV), torch.zeros(Sk, 4, dtype=torch.int16, device=DEV),
                          (0, 0, 0), torch.ones((Sq + 127) // 128, (Sk + 63) // 64, dtype=torch.uint8, device=DEV))


def _sdpa_rows():
    """(fault, q, k, v, kwargs) rows shared by attention_masked and attention_window"""
    q, k = (1, 2, 8, 64), (1, 2, 8, 64)
    return [
        ("f32", T(*q, dtype=F32), T(*k, dtype=F32), T(*k, dtype=F32), {}),
        ("k of another dtype", T(*q), T(*k, dtype=F16), T(*k), {}),
        ("3-D q", T(2, 8, 64), T(*k), T(*k), {}),
        ("5-D v", T(*q), T(*k), T(1, *k), {}),
        ("head dim 80", T(1, 2, 8, 80), T(1, 2, 8, 80), T(1, 2, 8, 80), {}),
        ("head dim 256", T(1, 2, 8, 256), T(1, 2, 8, 256), T(1, 2, 8, 256), {}),
        ("k of another batch", T(*q), T(2, 2, 8, 64), T(2, 2, 8, 64), {}),
        ("k of another head dim", T(*q), T(1, 2, 8, 128), T(1, 2, 8, 128), {}),
        ("v shorter than k", T(*q), T(*k), T(1, 2, 7, 64), {}),
        ("4 heads over 3", T(1, 4, 8, 64), T(1, 3, 8, 64), T(1, 3, 8, 64), dict(enable_gqa=True)),
        ("4 heads over 2 without enable_gqa", T(1, 4, 8, 64), T(*k), T(*k), {}),
        ("no queries", T(1, 2, 0, 64), T(*k), T(*k), {}),
        ("no keys", T(*q), T(1, 2, 0, 64), T(1, 2, 0, 64), {}),
        ("no batch", T(0, 2, 8, 64), T(0, 2, 8, 64), T(0, 2, 8, 64), {}),
        # two faults: the order of the checks
        ("f32, then 3-D", T(2, 8, 64, dtype=F32), T(2, 8, 64, dtype=F32), T(2, 8, 64, dtype=F32), {}),
        ("3-D, then head dim 80", T(2, 8, 80), T(2, 8, 80), T(2, 8, 80), {}),
        ("head dim 80, then v shorter than k", T(1, 2, 8, 80), T(1, 2, 8, 80), T(1, 2, 7, 80), {}),
        ("v shorter than k, then 4 heads over 3", T(1, 4, 8, 64), T(1, 3, 8, 64), T(1, 3, 7, 64), dict(enable_gqa=True)),
        ("4 heads over 3, then no queries", T(1, 4, 0, 64), T(1, 3, 8, 64), T(1, 3, 8, 64), dict(enable_gqa=True)),
    ]


def _rows():
    rows = []
    for fault, q, k, v, kw in _sdpa_rows():
        rows.append(("attention_masked", fault, lambda q=q, k=k, v=v, kw=kw: ops.attention_masked(q, k, v, **kw)))
    q = T(1, 2, 8, 64)
    masked = lambda m, **kw: (lambda: ops.attention_masked(q, q, q, m, **kw))     # noqa: E731
    rows += [
        ("attention_masked", "int32 mask", masked(T(8, 8, dtype=torch.int32))),
        ("attention_masked", "f16 mask for bf16 q", masked(T(8, 8, dtype=F16))),
        ("attention_masked", "5-D mask", masked(T(1, 1, 1, 8, 8, dtype=torch.bool))),
        ("attention_masked", "mask of 7 keys", masked(T(8, 7, dtype=torch.bool))),
        ("attention_masked", "mask on the CPU", masked(torch.ones(8, 8, dtype=torch.bool))),
        ("attention_masked", "no keys, then int32 mask",
         lambda: ops.attention_masked(q, T(1, 2, 0, 64), T(1, 2, 0, 64), T(8, 8, dtype=torch.int32))),
    ]
    for fault, q_, k_, v_, kw in _sdpa_rows():
        rows.append(("attention_window", fault, lambda q=q_, k=k_, v=v_, kw=kw: ops.attention_window(q, k, v, _plan(), **kw)))
    rows += [
        ("attention_window", "a plan that is none", lambda: ops.attention_window(q, q, q, None)),
        ("attention_window", "a plan that is none, then f32", lambda: ops.attention_window(T(2, 8, 64, dtype=F32), q, q, (1, 1, 1))),
        ("attention_window", "a plan for other lengths", lambda: ops.attention_window(q, q, q, _plan(8, 16))),
        ("attention_window", "no keys, then a plan for other lengths",
         lambda: ops.attention_window(q, T(1, 2, 0, 64), T(1, 2, 0, 64), _plan(8, 16))),
    ]
    w, w2 = T(1, 2, 8, 256), T(1, 1, 8, 256)
    wide = lambda q_, k_, v_, **kw: (lambda: ops.attention_wide(q_, k_, v_, **kw))     # noqa: E731
    rows += [
        ("attention_wide", "f32", wide(*(T(1, 2, 8, 256, dtype=F32),) * 3)),
        ("attention_wide", "v of another dtype", wide(w, w, T(1, 2, 8, 256, dtype=F16))),
        ("attention_wide", "3-D q", wide(T(2, 8, 256), w, w)),
        ("attention_wide", "head dim 128", wide(T(1, 2, 8, 128), T(1, 2, 8, 128), T(1, 2, 8, 128))),
        ("attention_wide", "head dim 320", wide(T(1, 2, 8, 320), T(1, 2, 8, 320), T(1, 2, 8, 320))),
        ("attention_wide", "k of another head count", wide(w, w2, w2)),
        ("attention_wide", "k of another batch", wide(w, T(2, 2, 8, 256), T(2, 2, 8, 256))),
        ("attention_wide", "k of another head dim", wide(w, T(1, 2, 8, 384), T(1, 2, 8, 384))),
        ("attention_wide", "v shorter than k", wide(w, w, T(1, 2, 7, 256))),
        ("attention_wide", "no queries", wide(T(1, 2, 0, 256), w, w)),
        ("attention_wide", "no keys", wide(w, T(1, 2, 0, 256), T(1, 2, 0, 256))),
        ("attention_wide", "frames of 3 in 8", wide(w, w, w, frame_tokens=3)),
        ("attention_wide", "frames with Sq != Sk", wide(w, T(1, 2, 16, 256), T(1, 2, 16, 256), frame_tokens=4)),
        ("attention_wide", "frame_tokens -2", wide(w, w, w, frame_tokens=-2)),
        ("attention_wide", "key_splits 9", wide(w, w, w, key_splits=9)),
        ("attention_wide", "key_splits Auto", wide(w, w, w, key_splits="Auto")),
        ("attention_wide", "f32, then 3-D", wide(*(T(2, 8, 256, dtype=F32),) * 3)),
        ("attention_wide", "3-D, then head dim 128", wide(T(2, 8, 128), T(2, 8, 128), T(2, 8, 128))),
        ("attention_wide", "head dim 128, then k of another head count", wide(T(1, 2, 8, 128), T(1, 1, 8, 128), T(1, 1, 8, 128))),
        ("attention_wide", "k of another head count, then no queries", wide(T(1, 2, 0, 256), w2, w2)),
        ("attention_wide", "no keys, then frame_tokens -2", wide(w, T(1, 2, 0, 256), T(1, 2, 0, 256), frame_tokens=-2)),
        ("attention_wide", "frames of 3 in 8, then key_splits 9", wide(w, w, w, frame_tokens=3, key_splits=9)),
    ]
    chunked = lambda q_, ks, vs, *a, **kw: (lambda: ops.attention_chunked(q_, ks, vs, *a, **kw))     # noqa: E731
    kv, g = T(1, 2, 8, 64), T(1, 4, 8, 64)
    rows += [
        ("attention_chunked", "no chunks", chunked(q, [], [])),
        ("attention_chunked", "9 chunks", chunked(q, [kv] * 9, [kv] * 9)),
        ("attention_chunked", "2 key and 1 value chunks", chunked(q, [kv, kv], [kv])),
        ("attention_chunked", "1 mask for 2 chunks", chunked(q, [kv, kv], [kv, kv], [None])),
        ("attention_chunked", "wide heads with a mask", chunked(w, [w], [w], [T(8, 8, dtype=torch.bool)])),
        ("attention_chunked", "wide heads with enable_gqa", chunked(w, [w], [w], enable_gqa=True)),
        ("attention_chunked", "wide heads over fewer key heads", chunked(w, [w2], [w2])),
        ("attention_chunked", "f32", chunked(T(1, 2, 8, 64, dtype=F32), [T(1, 2, 8, 64, dtype=F32)], [T(1, 2, 8, 64, dtype=F32)])),
        ("attention_chunked", "head dim 80", chunked(T(1, 2, 8, 80), [T(1, 2, 8, 80)], [T(1, 2, 8, 80)])),
        ("attention_chunked", "a chunk of another batch", chunked(q, [T(2, 2, 8, 64)], [T(2, 2, 8, 64)])),
        ("attention_chunked", "4 heads over 2 without enable_gqa", chunked(g, [kv], [kv])),
        ("attention_chunked", "4 heads over 3", chunked(g, [T(1, 3, 8, 64)], [T(1, 3, 8, 64)], enable_gqa=True)),
        ("attention_chunked", "a chunk without keys", chunked(q, [T(1, 2, 0, 64)], [T(1, 2, 0, 64)])),
        ("attention_chunked", "wide heads, v of another dtype", chunked(w, [w], [T(1, 2, 8, 256, dtype=F16)])),
        ("attention_chunked", "9 chunks, then f32", chunked(T(1, 2, 8, 64, dtype=F32), [kv] * 9, [kv] * 9)),
        ("attention_chunked", "wide heads with a mask, then enable_gqa", chunked(w, [w], [w], [T(8, 8, dtype=torch.bool)], enable_gqa=True)),
    ]
    return rows


# (wrapper, fault) -> the complete message
MESSAGES = {
    ('attention_masked', 'f32'):
        "attention_masked: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_masked', 'k of another dtype'):
        "attention_masked: dtypes torch.bfloat16/torch.float16/torch.bfloat16 unsupported (bf16 or f16, all equal)",
    ('attention_masked', '3-D q'):
        "attention_masked: q, k, v must be 4-D [B, H, S, D]",
    ('attention_masked', '5-D v'):
        "attention_masked: q, k, v must be 4-D [B, H, S, D]",
    ('attention_masked', 'head dim 80'):
        "attention_masked: head dim 80 unsupported (64 or 128)",
    ('attention_masked', 'head dim 256'):
        "attention_masked: head dim 256 unsupported (64 or 128)",
    ('attention_masked', 'k of another batch'):
        "attention_masked: shapes q (1, 2, 8, 64) k (2, 2, 8, 64) v (2, 2, 8, 64) do not match",
    ('attention_masked', 'k of another head dim'):
        "attention_masked: shapes q (1, 2, 8, 64) k (1, 2, 8, 128) v (1, 2, 8, 128) do not match",
    ('attention_masked', 'v shorter than k'):
        "attention_masked: shapes q (1, 2, 8, 64) k (1, 2, 8, 64) v (1, 2, 7, 64) do not match",
    ('attention_masked', '4 heads over 3'):
        "attention_masked: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_masked', '4 heads over 2 without enable_gqa'):
        "attention_masked: 4 query heads over 2 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_masked', 'no queries'):
        "attention_masked: empty problem",
    ('attention_masked', 'no keys'):
        "attention_masked: empty problem",
    ('attention_masked', 'no batch'):
        "attention_masked: empty problem",
    ('attention_masked', 'f32, then 3-D'):
        "attention_masked: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_masked', '3-D, then head dim 80'):
        "attention_masked: q, k, v must be 4-D [B, H, S, D]",
    ('attention_masked', 'head dim 80, then v shorter than k'):
        "attention_masked: head dim 80 unsupported (64 or 128)",
    ('attention_masked', 'v shorter than k, then 4 heads over 3'):
        "attention_masked: shapes q (1, 4, 8, 64) k (1, 3, 8, 64) v (1, 3, 7, 64) do not match",
    ('attention_masked', '4 heads over 3, then no queries'):
        "attention_masked: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_masked', 'int32 mask'):
        "attention_masked: attn_mask dtype torch.int32 unsupported (bool, float32 or q's dtype)",
    ('attention_masked', 'f16 mask for bf16 q'):
        "attention_masked: additive attn_mask of dtype torch.float16 does not match q's dtype torch.bfloat16",
    ('attention_masked', '5-D mask'):
        "attention_masked: attn_mask of shape (1, 1, 1, 8, 8) has more than 4 dims",
    ('attention_masked', 'mask of 7 keys'):
        "attention_masked: attn_mask of shape (8, 7) does not broadcast to (1, 2, 8, 8)",
    ('attention_masked', 'mask on the CPU'):
        "attention_masked: attn_mask is on cpu, q on cuda:0",
    ('attention_masked', 'no keys, then int32 mask'):
        "attention_masked: empty problem",
    ('attention_window', 'f32'):
        "attention_window: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_window', 'k of another dtype'):
        "attention_window: dtypes torch.bfloat16/torch.float16/torch.bfloat16 unsupported (bf16 or f16, all equal)",
    ('attention_window', '3-D q'):
        "attention_window: q, k, v must be 4-D [B, H, S, D]",
    ('attention_window', '5-D v'):
        "attention_window: q, k, v must be 4-D [B, H, S, D]",
    ('attention_window', 'head dim 80'):
        "attention_window: head dim 80 unsupported (64 or 128)",
    ('attention_window', 'head dim 256'):
        "attention_window: head dim 256 unsupported (64 or 128)",
    ('attention_window', 'k of another batch'):
        "attention_window: shapes q (1, 2, 8, 64) k (2, 2, 8, 64) v (2, 2, 8, 64) do not match",
    ('attention_window', 'k of another head dim'):
        "attention_window: shapes q (1, 2, 8, 64) k (1, 2, 8, 128) v (1, 2, 8, 128) do not match",
    ('attention_window', 'v shorter than k'):
        "attention_window: shapes q (1, 2, 8, 64) k (1, 2, 8, 64) v (1, 2, 7, 64) do not match",
    ('attention_window', '4 heads over 3'):
        "attention_window: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_window', '4 heads over 2 without enable_gqa'):
        "attention_window: 4 query heads over 2 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_window', 'no queries'):
        "attention_window: empty problem",
    ('attention_window', 'no keys'):
        "attention_window: empty problem",
    ('attention_window', 'no batch'):
        "attention_window: empty problem",
    ('attention_window', 'f32, then 3-D'):
        "attention_window: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_window', '3-D, then head dim 80'):
        "attention_window: q, k, v must be 4-D [B, H, S, D]",
    ('attention_window', 'head dim 80, then v shorter than k'):
        "attention_window: head dim 80 unsupported (64 or 128)",
    ('attention_window', 'v shorter than k, then 4 heads over 3'):
        "attention_window: shapes q (1, 4, 8, 64) k (1, 3, 8, 64) v (1, 3, 7, 64) do not match",
    ('attention_window', '4 heads over 3, then no queries'):
        "attention_window: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_window', 'a plan that is none'):
        "attention_window: plan must be an ops.WindowPlan (ops.window_plan), got NoneType",
    ('attention_window', 'a plan that is none, then f32'):
        "attention_window: plan must be an ops.WindowPlan (ops.window_plan), got tuple",
    ('attention_window', 'a plan for other lengths'):
        "attention_window: the window plan is for (Sq, Sk) = (8, 16), the operands have (8, 8)",
    ('attention_window', 'no keys, then a plan for other lengths'):
        "attention_window: empty problem",
    ('attention_wide', 'f32'):
        "attention_wide: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_wide', 'v of another dtype'):
        "attention_wide: dtypes torch.bfloat16/torch.bfloat16/torch.float16 unsupported (bf16 or f16, all equal)",
    ('attention_wide', '3-D q'):
        "attention_wide: q, k, v must be 4-D [B, H, S, D]",
    ('attention_wide', 'head dim 128'):
        "attention_wide: head dim 128 unsupported (256, 384, 512); other head sizes go through `attention`",
    ('attention_wide', 'head dim 320'):
        "attention_wide: head dim 320 unsupported (256, 384, 512); other head sizes go through `attention`",
    ('attention_wide', 'k of another head count'):
        "attention_wide: shapes q (1, 2, 8, 256) k (1, 1, 8, 256) v (1, 1, 8, 256) do not match",
    ('attention_wide', 'k of another batch'):
        "attention_wide: shapes q (1, 2, 8, 256) k (2, 2, 8, 256) v (2, 2, 8, 256) do not match",
    ('attention_wide', 'k of another head dim'):
        "attention_wide: shapes q (1, 2, 8, 256) k (1, 2, 8, 384) v (1, 2, 8, 384) do not match",
    ('attention_wide', 'v shorter than k'):
        "attention_wide: shapes q (1, 2, 8, 256) k (1, 2, 8, 256) v (1, 2, 7, 256) do not match",
    ('attention_wide', 'no queries'):
        "attention_wide: empty problem",
    ('attention_wide', 'no keys'):
        "attention_wide: empty problem",
    ('attention_wide', 'frames of 3 in 8'):
        "attention_wide: frame_tokens=3 needs Sq == Sk and a whole number of frames (Sq=8, Sk=8)",
    ('attention_wide', 'frames with Sq != Sk'):
        "attention_wide: frame_tokens=4 needs Sq == Sk and a whole number of frames (Sq=8, Sk=16)",
    ('attention_wide', 'frame_tokens -2'):
        "attention_wide: frame_tokens=-2 needs Sq == Sk and a whole number of frames (Sq=8, Sk=8)",
    ('attention_wide', 'key_splits 9'):
        "attention_wide: key_splits=9 unsupported (an int 1 to 8, or \"auto\")",
    ('attention_wide', 'key_splits Auto'):
        "attention_wide: key_splits='Auto' unsupported (an int 1 to 8, or \"auto\")",
    ('attention_wide', 'f32, then 3-D'):
        "attention_wide: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_wide', '3-D, then head dim 128'):
        "attention_wide: q, k, v must be 4-D [B, H, S, D]",
    ('attention_wide', 'head dim 128, then k of another head count'):
        "attention_wide: head dim 128 unsupported (256, 384, 512); other head sizes go through `attention`",
    ('attention_wide', 'k of another head count, then no queries'):
        "attention_wide: shapes q (1, 2, 0, 256) k (1, 1, 8, 256) v (1, 1, 8, 256) do not match",
    ('attention_wide', 'no keys, then frame_tokens -2'):
        "attention_wide: empty problem",
    ('attention_wide', 'frames of 3 in 8, then key_splits 9'):
        "attention_wide: frame_tokens=3 needs Sq == Sk and a whole number of frames (Sq=8, Sk=8)",
    ('attention_chunked', 'no chunks'):
        "attention_chunked: 0 key and 0 value chunks (1 to 8 of each, equally many)",
    ('attention_chunked', '9 chunks'):
        "attention_chunked: 9 key and 9 value chunks (1 to 8 of each, equally many)",
    ('attention_chunked', '2 key and 1 value chunks'):
        "attention_chunked: 2 key and 1 value chunks (1 to 8 of each, equally many)",
    ('attention_chunked', '1 mask for 2 chunks'):
        "attention_chunked: 1 masks for 2 chunks (one per chunk, None for no mask)",
    ('attention_chunked', 'wide heads with a mask'):
        "attention_chunked: head dim 256 runs on the wide-head kernel, which takes no masks",
    ('attention_chunked', 'wide heads with enable_gqa'):
        "attention_chunked: head dim 256 runs on the wide-head kernel, which has no grouped-query heads (every chunk needs q's head count, enable_gqa=False)",
    ('attention_chunked', 'wide heads over fewer key heads'):
        "attention_chunked: head dim 256 runs on the wide-head kernel, which has no grouped-query heads (every chunk needs q's head count, enable_gqa=False)",
    ('attention_chunked', 'f32'):
        "attention_masked: dtypes torch.float32/torch.float32/torch.float32 unsupported (bf16 or f16, all equal)",
    ('attention_chunked', 'head dim 80'):
        "attention_masked: head dim 80 unsupported (64 or 128)",
    ('attention_chunked', 'a chunk of another batch'):
        "attention_masked: shapes q (1, 2, 8, 64) k (2, 2, 8, 64) v (2, 2, 8, 64) do not match",
    ('attention_chunked', '4 heads over 2 without enable_gqa'):
        "attention_masked: 4 query heads over 2 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_chunked', '4 heads over 3'):
        "attention_masked: 4 query heads over 3 key/value heads needs enable_gqa=True and a whole ratio",
    ('attention_chunked', 'a chunk without keys'):
        "attention_masked: empty problem",
    ('attention_chunked', 'wide heads, v of another dtype'):
        "attention_wide: dtypes torch.bfloat16/torch.bfloat16/torch.float16 unsupported (bf16 or f16, all equal)",
    ('attention_chunked', '9 chunks, then f32'):
        "attention_chunked: 9 key and 9 value chunks (1 to 8 of each, equally many)",
    ('attention_chunked', 'wide heads with a mask, then enable_gqa'):
        "attention_chunked: head dim 256 runs on the wide-head kernel, which takes no masks",
}


def test_wrappers_refuse_with_the_exact_messages():
    rows = _rows()
    assert len({(r[0], r[1]) for r in rows}) == len(rows) == len(MESSAGES)
    before = list(ops._ws_cache.items())
    for who, fault, run in rows:
        with pytest.raises(ApexMIError) as e:
            run()
        assert str(e.value) == MESSAGES[who, fault], (who, fault)
    assert [(k, id(w)) for k, w in ops._ws_cache.items()] == [(k, id(w)) for k, w in before]      # no workspace was asked for


def test_workspace_keys_and_which_wrappers_share_a_buffer():
    """One call of each wrapper at the smallest shape that launches (two query blocks and a key tail), then the exact key set:
    masked and window share ("masked", ...), attention / attention_framecausal / attention_bias the untagged key, varlen and wide
    own theirs; a buffer is kept while it is large enough and replaced when it is not."""
    saved = dict(ops._ws_cache)
    ops._ws_cache.clear()
    try:
        g = torch.Generator().manual_seed(11)
        R = lambda *shape: torch.randn(shape, generator=g).to(device=DEV, dtype=BF)     # noqa: E731
        q, k, v = R(1, 2, 129, 64), R(1, 2, 65, 64), R(1, 2, 65, 64)
        dev, stream = q.device.index, torch.cuda.current_stream().cuda_stream
        masked_key = ("masked", dev, stream)
        ops.attention(q, k, v)
        ops.attention_masked(q, k, v)
        ws_masked = ops._ws_cache[masked_key]
        plan = ops.window_plan(torch.arange(129 * 3).reshape(129, 3) % 7, torch.arange(65 * 3).reshape(65, 3) % 7, (2, 2, 2), device=DEV)
        ops.attention_window(q, k, v, plan)
        assert ops._ws_cache[masked_key] is ws_masked                                   # one buffer for the two wrappers
        cu_q, cu_k = (torch.tensor(c, dtype=torch.int32, device=DEV) for c in ([0, 100, 129], [0, 30, 65]))
        ops.attention_varlen(R(129, 2, 64), R(65, 2, 64), R(65, 2, 64), cu_q, cu_k, 100, 35)
        ops.attention_wide(R(1, 1, 129, 256), R(1, 1, 65, 256), R(1, 1, 65, 256))
        f = R(1, 1, 256, 128)
        ops.attention_framecausal(f, f, f, 64)
        ops.attention_bias(R(129, 128), R(65, 128), R(65, 128), 2, 0.125)
        assert set(ops._ws_cache) == {(dev, stream), masked_key, ("varlen", dev, stream), ("wide", dev, stream)}
        assert all(w.dtype == torch.uint8 and w.device == q.device for w in ops._ws_cache.values())
        ops.attention_masked(q, k[:, :, :33], v[:, :, :33])
        assert ops._ws_cache[masked_key] is ws_masked                                   # smaller: kept
        long = R(1, 2, 4096, 64)
        ops.attention_masked(q, long, long)
        grown = ops._ws_cache[masked_key]
        assert grown is not ws_masked and grown.numel() > ws_masked.numel()             # larger: replaced
        assert grown.numel() == lib.load().apexmi_attn_masked_workspace_bytes(1, 2, 2, 129, 4096, 64)
        torch.cuda.synchronize()
    finally:
        ops._ws_cache.clear()
        ops._ws_cache.update(saved)
