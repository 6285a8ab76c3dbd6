"""The host side of the grouped MXFP4 GEMM (csrc/gemm_mxfp4.hip: apexmi_gemm_mxfp4_grouped, apexmi_gemm_mxfp4_grouped_qkv;
ops.mxfp4_grouped_route; FluxTransformer2DModel.set_fp4_compute's name validation) without a GPU: the route predicate on CPU / meta
tensors, the entry points' refusals with dummy (never dereferenced) pointers, and the names a model accepts."""
import ctypes as C

import pytest
import torch

BF = torch.bfloat16


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _rec(N, K):
    return _ops().Mxfp4Weight(torch.zeros(N, K // 2, dtype=torch.uint8), torch.full((N, K // 32), 127, dtype=torch.uint8))


def _a(M, K, dtype=BF):
    return torch.empty(M, K, dtype=dtype, device="meta")


# ------------------------------------------------------------------------------------------------------------------ route
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_route_holds_for_one_to_four_routed_problems_sharing_k(n):
    ops = _ops()
    K = 512
    shapes = [(130, 144), (72, 272), (300, 128), (1, 16)][:n]
    a = [_a(M, K) for M, _ in shapes]
    w = [_rec(N, K) for _, N in shapes]
    assert ops.mxfp4_grouped_route(a, w)
    assert ops.mxfp4_grouped_route(a, w, [_a(M, N) for M, N in shapes], ["bias", "gelu", "gate_res", "bias"][:n])
    carried = []
    for r in w:                                   # a bf16 weight carrying the record on its `_fp4` slot, as the models attach it
        t = torch.empty(r.shape, dtype=BF, device="meta")
        t._fp4 = r
        carried.append(t)
    assert ops.mxfp4_grouped_route(a, carried)


def test_route_refuses():
    ops = _ops()
    K = 256
    a2, w2 = [_a(8, K), _a(9, K)], [_rec(32, K), _rec(48, K)]
    assert ops.mxfp4_grouped_route(a2, w2)
    assert not ops.mxfp4_grouped_route([], [])
    assert not ops.mxfp4_grouped_route([_a(8, K)] * 5, [_rec(32, K)] * 5)
    assert not ops.mxfp4_grouped_route([_a(8, K), _a(9, 512)], [_rec(32, K), _rec(48, 512)]), "unequal K"
    assert not ops.mxfp4_grouped_route(a2, [w2[0], torch.empty(48, K, dtype=BF, device="meta")]), "one weight without a record"
    off = _rec(48, K)
    off.compute = "bf16"
    assert not ops.mxfp4_grouped_route(a2, [w2[0], off]), "one record that is switched off"
    assert not ops.mxfp4_grouped_route(a2, w2, [None, torch.empty(9, 48, dtype=torch.float32, device="meta")]), "a float out"
    assert not ops.mxfp4_grouped_route(a2, w2, None, ["bias", "silu"]), "an epilogue outside the three"
    assert not ops.mxfp4_grouped_route([_a(8, 384), _a(9, 384)], [_rec(32, 384), _rec(48, 384)]), "K % 256 != 0"
    assert not ops.mxfp4_grouped_route([_a(8, K, torch.float32), _a(9, K)], w2), "float activations"
    assert not ops.mxfp4_grouped_route(a2, w2, None, ["bias"]), "one epilogue name per problem"


def test_the_grouped_tile_walk_is_the_format_independent_one():
    """no second restatement of the walk: the fp4 launch is described by ops.fp8_grouped_tiles, and every tile occurs once"""
    ops = _ops()
    shapes = [(130, 144), (72, 272), (300, 128), (1, 16)]
    tiles = ops.fp8_grouped_tiles(shapes)
    want = {(i, r, c) for i, (M, N) in enumerate(shapes) for r in range((M + 127) // 128) for c in range((N + 127) // 128)}
    assert len(tiles) == len(want) == 11 and set(tiles) == want and len(tiles) % 8 != 0
    assert not hasattr(ops, "mxfp4_grouped_tiles")


# ------------------------------------------------------------------------------------------------------------ entry points
def _arrays(n, P, K=256, **over):
    """the 18 arguments between `count` and the stream of apexmi_gemm_mxfp4_grouped for n problems of 8 x 32 x K on the dummy
    address P; `over` replaces whole arrays (or K)"""
    VP, I64, INT = C.c_void_p * n, C.c_int64 * n, C.c_int * n
    d = dict(qa=VP(*[P] * n), lda=I64(*[K // 2] * n), sa=VP(*[P] * n), ldsa=I64(*[K // 32] * n), qw=VP(*[P] * n), ldw=I64(*[K // 2] * n),
             sw=VP(*[P] * n), ldsw=I64(*[K // 32] * n), bias=VP(*[None] * n), C=VP(*[P] * n), ldc=I64(*[32] * n), M=INT(*[8] * n),
             N=INT(*[32] * n), K=K, epi=INT(*[0] * n), gate=VP(*[None] * n), R=VP(*[None] * n), ldr=I64(*[0] * n))
    d.update(over)
    return [d[k] for k in ("qa", "lda", "sa", "ldsa", "qw", "ldw", "sw", "ldsw", "bias", "C", "ldc", "M", "N", "K", "epi", "gate", "R", "ldr")]


def test_entry_points_refuse_bad_arguments_with_a_reason():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000                      # 16-byte aligned dummy address, never dereferenced

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    VP2, I2 = C.c_void_p * 2, C.c_int * 2
    g = L.apexmi_gemm_mxfp4_grouped
    bad(g(0, *_arrays(1, P), None), "count=0 not in [1,4]")
    bad(g(5, *_arrays(5, P), None), "count=5 not in [1,4]")
    bad(g(2, *_arrays(2, P, K=384), None), "K=384 must be a multiple of 256")
    bad(g(2, *_arrays(2, P, N=I2(32, 24)), None), "N=24 of problem 1 must be a multiple of 16")
    bad(g(2, *_arrays(2, P, M=I2(8, 0)), None), "M=0 of problem 1")
    bad(g(2, *_arrays(2, P, sa=VP2(P, None)), None), "null operand (problem 1)")
    bad(g(2, *_arrays(2, P, C=VP2(None, P)), None), "null operand (problem 0)")
    bad(g(2, *_arrays(2, P, qa=None), None), "null argument array")
    bad(g(2, *_arrays(2, P, epi=I2(0, lib.EPI_BIAS_GATE_RES)), None), "gate/residual epilogue needs gate and R (problem 1)")
    bad(g(2, *_arrays(2, P, epi=I2(0, lib.EPI_BIAS | lib.EPI_F32_IO)), None), "f32 output")
    bad(g(2, *_arrays(2, P, epi=I2(0, lib.EPI_BIAS_SILU)), None), "is not one of bias")
    bad(g(2, *_arrays(2, P, ldsa=(C.c_int64 * 2)(8, 4)), None), "block scales of problem 1 must be 4-byte aligned rows of at least K / 32 = 8")
    bad(g(2, *_arrays(2, P, lda=(C.c_int64 * 2)(128, 64)), None), "code rows at least K / 2 = 128 bytes")

    q = L.apexmi_gemm_mxfp4_grouped_qkv
    H, S = 2, 16

    def tail(is_qkv=(1, 0), rope=P, qo=P, ko=P, vt=P, row0=(0, 0), S_out=S, Skp=S):
        return (I2(*is_qkv), VP2(None, None), VP2(None, None), I2(*row0), H, 1e-6, rope, qo, ko, vt, S_out, Skp, None)

    fused = dict(N=I2(768, 32), C=VP2(None, P))        # C of the fused problem may be null
    bad(q(2, *_arrays(2, P, **fused), *tail(rope=None)), "null argument")
    bad(q(2, *_arrays(2, P, **fused), *tail(qo=None)), "null argument")
    bad(q(2, *_arrays(2, P, **fused), *tail(ko=None)), "null argument")
    bad(q(2, *_arrays(2, P, **fused), *tail(vt=None)), "null argument")
    bad(q(2, *_arrays(2, P, N=I2(512, 32), C=VP2(None, P)), *tail()), "a fused problem has N = 3 H 128 = 768 (got 512)")
    bad(q(2, *_arrays(2, P, **fused), *tail(row0=(9, 0))), "rows [9, 17) must lie inside S_out=16")
    bad(q(2, *_arrays(2, P, **fused), *tail(Skp=12)), "Skp=12 must be a multiple of 8 >= S_out=16")
    bad(q(2, *_arrays(2, P, N=I2(768, 32), C=VP2(None, None)), *tail()), "null operand (problem 1)")
    bad(q(5, *_arrays(5, P), *tail()), "gemm_mxfp4_grouped_qkv: count=5 not in [1,4]")


def test_python_wrappers_refuse_before_the_library_is_asked():
    ops = _ops()
    from apex_studio_amd.lib import ApexMIError
    K = 256
    q, s = torch.zeros(8, K // 2, dtype=torch.uint8), torch.full((8, K // 32), 127, dtype=torch.uint8)
    out = torch.zeros(8, 32, dtype=BF)
    with pytest.raises(ApexMIError, match="1 to 4 problems"):
        ops.gemm_mxfp4_grouped([], [], [], [], [])
    with pytest.raises(ApexMIError, match="1 to 4 problems"):
        ops.gemm_mxfp4_grouped([q] * 5, [s] * 5, [_rec(32, K)] * 5, None, [out] * 5)
    with pytest.raises(ApexMIError, match="expected an Mxfp4Weight"):
        ops.gemm_mxfp4_grouped([q], [s], [torch.zeros(32, K, dtype=BF)], None, [out])
    with pytest.raises(ApexMIError, match="share K"):
        ops.gemm_mxfp4_grouped([q, q], [s, s], [_rec(32, K), _rec(32, 512)], None, [out, out])
    with pytest.raises(ApexMIError, match="epilogue 'silu'"):
        ops.gemm_mxfp4_grouped([q], [s], [_rec(32, K)], None, [out], epilogue="silu")
    with pytest.raises(ApexMIError, match="one epilogue"):
        ops.gemm_mxfp4_grouped([q, q], [s, s], [_rec(32, K), _rec(32, K)], None, [out, out], epilogue=["bias"])
    with pytest.raises(ApexMIError, match=r"codes must be \[8, 128\]"):
        ops.gemm_mxfp4_grouped([q[:, :64]], [s], [_rec(32, K)], None, [out])
    with pytest.raises(ApexMIError, match=r"problem 0.*no CPU fallback"):           # CPU tensors: the product ops never fall back
        ops.gemm_mxfp4_grouped([q], [s], [_rec(32, K)], None, [out])


# ------------------------------------------------------------------------------------------------------------------ model
def test_set_fp4_compute_checks_the_names_before_anything_else():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.lib import ApexMIError
    m = FluxTransformer2DModel(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128,
                               num_attention_heads=2, joint_attention_dim=256, pooled_projection_dim=64, device="meta", dtype=BF)
    assert m._FP4_LINEARS == ("qkv", "attn_out", "ffn_up", "ffn_down", "single_in", "single_out")
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*unknown Linear name\(s\) \['cross_q'\]"):
        m.set_fp4_compute(True, linears=("qkv", "cross_q"))
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: .*takes names out of"):
        m.set_fp4_compute(True, linears=3)
    with pytest.raises(ApexMIError, match=r"^flux\.mi355: set_fp4_compute\(False\) takes no `linears`"):
        m.set_fp4_compute(False, linears=("qkv",))
    assert m.set_fp4_compute(False) is m and m._fp4_bytes == 0
