"""The opt-in FP8 GEMM on the GPU: the per-row quantiser bit for bit against its documented formula, the operand
lane map of the block-scaled MFMA with exact integer data, random operands under every epilogue against the f32 product of the
dequantised codes, the routing of `ops.gemm`, and graph capture."""
import pytest
import torch

from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F8 = torch.bfloat16, torch.float8_e4m3fn


def quant_reference(a: torch.Tensor):
    """The formula of `apexmi_quant_rows_fp8`, restated with torch on the CPU: IEEE float32, every operation rounded on its own."""
    x = a.float()
    amax = x.abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))      # tensor / tensor: true division
    y = torch.minimum(torch.maximum(x / scale, torch.full_like(x, -448.0)), torch.full_like(x, 448.0))
    return y.to(F8).view(torch.uint8), scale.reshape(-1)


def codes_of(x: torch.Tensor) -> torch.Tensor:
    """float values that e4m3 holds exactly -> their code bytes"""
    q = x.to(F8)
    assert torch.equal(q.float(), x.float())
    return q.view(torch.uint8)


def weight_of(codes_cpu: torch.Tensor, scale: torch.Tensor):
    from apex_studio_amd import ops
    return ops.Fp8Weight(codes_cpu.view(F8).to(DEV), scale.to(DEV))


# ---------------------------------------------------------------- quantiser
@pytest.mark.parametrize("K", [128, 640])
@pytest.mark.parametrize("M", [1, 3, 130])
def test_quantiser_is_the_documented_formula_bit_for_bit(M, K):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    g = torch.Generator().manual_seed(100 * M + K)
    rows = M + 3
    a = torch.randn(rows, K, generator=g) * 10.0 ** (torch.rand(rows, 1, generator=g) * 6 - 3)
    a[M] = 0.0                                                   # all-zero row
    a[M + 1] = torch.randn(K, generator=g) * 2e-39               # absmax is a bf16 subnormal
    a[M + 2, 5], a[M + 2, K - 3] = 3.39e38, -3.39e38             # the largest bf16 magnitudes
    a = a.to(BF)
    assert 0 < float(a[M + 1].float().abs().max()) < 2.0 ** -126 and float(a[M + 2].float().abs().max()) > 3.38e38
    for lo in range(0, rows, M):                                 # the special rows travel in M-row launches too
        part = a[lo:lo + M]
        want_q, want_s = quant_reference(part)
        pad = torch.zeros(part.shape[0], K + 64, dtype=BF, device=DEV)       # padded row stride
        pad[:, :K] = part.to(DEV)
        q, s = ops.quant_rows_fp8(pad[:, :K])
        torch.cuda.synchronize()
        assert torch.equal(s.cpu(), want_s), (lo, s.cpu(), want_s)
        assert torch.equal(q.cpu(), want_q), (lo, int((q.cpu() != want_q).sum()))
        assert not bool(((q.cpu() & 0x7f) == 0x7f).any()), "no NaN code"
    zq, zs = quant_reference(a[M:M + 1])
    assert float(zs[0]) == 1.0 and int(zq.max()) == 0


# ---------------------------------------------------------------- lane map, exact
def _int_operands(M, N, K):
    m, n, k = torch.arange(M).view(-1, 1), torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    A = ((m * 7 + k * 3 + (m * k) % 5) % 17 - 8).float()          # depends on (row, k)
    W = ((n * 5 + k * 11 + (n + 2 * k) % 7) % 17 - 8).float()      # depends on (col, k), no symmetry with A
    return A, W


@pytest.mark.parametrize("K", [128, 384, 1152])
def test_lane_map_with_exact_integer_operands(K):
    """Integers in [-8, 8] are exact in e4m3 and every partial sum stays below 2^24, so the f32 accumulation is exact in any
    order: the output must equal the integer matmul after the bf16 rounding of both sides.  K = 384 is an odd number of K-tiles."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    for M in (1, 33, 129, 257):
        for N in (16, 144, 272):
            A, W = _int_operands(M, N, K)
            want = (A.double() @ W.double().T)
            assert float(want.abs().max()) < 2 ** 24
            out = ops.gemm_fp8(codes_of(A).to(DEV), torch.ones(M, device=DEV), weight_of(codes_of(W), torch.ones(1)))
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), want.float().to(BF)), (M, N, K, int((out.cpu() != want.float().to(BF)).sum()))


def test_identity_against_an_asymmetric_weight():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    K, N = 256, 144
    _, W = _int_operands(1, N, K)
    out = ops.gemm_fp8(codes_of(torch.eye(K)).to(DEV), torch.ones(K, device=DEV), weight_of(codes_of(W), torch.ones(1)))
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().float(), W.T)


# ---------------------------------------------------------------- random operands
_CASES = {}


def _case(M, N, K, per_row):
    key = (M, N, K, per_row)
    if key not in _CASES:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K + per_row)
        qa, sa = quant_reference((torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)).to(BF))
        w = torch.randn(N, K, generator=g) * 0.02
        sw = ((w.abs().amax(dim=1) if per_row else w.abs().max().reshape(1)) / 448.0).to(BF)
        qw = (w / sw.float().view(-1, 1)).clamp(-448, 448).to(F8)
        bias = torch.randn(N, generator=g).to(BF) * 0.5
        gate = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(BF)
        y = (qa.view(F8).float() @ qw.float().T) * sa.view(-1, 1) * sw.float().view(1, -1) + bias.float()
        # the tanh GELU is evaluated in float64 on the f32 pre-activation: in float32 torch's 0.5 x (1 + tanh(u)) cancels for
        # negative x and is itself more than 1 bf16 ulp off the true value on 1 % of these elements
        gelu = torch.nn.functional.gelu(y.double(), approximate="tanh").float()
        ref = {"bias": y, "gelu": gelu, "gate_res": res.float() + gate * y}
        _CASES[key] = dict(qa=qa, sa=sa, qw=qw.view(torch.uint8), sw=sw, bias=bias, gate=gate, res=res, ref=ref)
    return _CASES[key]


def _ordered(t: torch.Tensor) -> torch.Tensor:
    """bf16 bit patterns as integers in value order (ulp distances)"""
    b = t.view(torch.int16).int()
    return torch.where(b < 0, -(b & 0x7fff), b)


# rel-L2 against the f32 reference = accumulation order + the final bf16 rounding.  Measured on the MI355X over the two shapes
# and both scale kinds (profiles/gemm_fp8_measured.jsonl): bias 1.647e-3 .. 1.669e-3, gelu 1.655e-3 .. 1.671e-3, gate_res
# 1.661e-3 .. 1.674e-3 (a uniform bf16 rounding alone is 2^-9 / sqrt(3) x ~1.5 = 1.7e-3); bars at 2x the largest
_BARS = {"bias": 3.3e-3, "gelu": 3.3e-3, "gate_res": 3.3e-3}


@pytest.mark.parametrize("epilogue", ["bias", "gelu", "gate_res"])
@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("shape", [(200, 272, 512), (129, 5120, 256)])
def test_random_operands_under_every_epilogue(shape, per_row, epilogue):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    M, N, K = shape
    c = _case(M, N, K, per_row)
    w = weight_of(c["qw"], c["sw"])
    qa = torch.zeros(M, K + 128, dtype=torch.uint8, device=DEV)               # a padded row stride
    qa[:, :K] = c["qa"].to(DEV)
    big = torch.full((M, N + 32), 7.0, dtype=BF, device=DEV)                  # out is a column slice
    kw = dict(gate=c["gate"].to(DEV), residual=c["res"].to(DEV)) if epilogue == "gate_res" else {}
    out = ops.gemm_fp8(qa[:, :K], c["sa"].to(DEV), w, c["bias"].to(DEV), out=big[:, 16:16 + N], epilogue=epilogue, **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == big[:, 16:].data_ptr()
    assert float((big[:, :16].float() - 7).abs().max()) == 0 and float((big[:, 16 + N:].float() - 7).abs().max()) == 0
    got, ref = out.cpu(), c["ref"][epilogue]
    rel = float((got.float() - ref).norm() / ref.norm())
    ulp = (_ordered(got) - _ordered(ref.to(BF))).abs()
    within = float((ulp <= 1).float().mean())
    print(f"[gemm_fp8 {M}x{N}x{K} {'row' if per_row else 'one'} {epilogue}] rel-L2 {rel:.3e}, within 1 bf16 ulp {within:.5f}, "
          f"max ulp {int(ulp.max())}")
    measured(f"gemm_fp8.{epilogue}.{M}x{N}x{K}.{'row' if per_row else 'one'}", rel, _BARS[epilogue])
    assert within >= 0.99, within


# ---------------------------------------------------------------- routing through ops.gemm
def _routed_pair(M=200, N=272, K=512, Rp=64):
    c = _case(M, N, K, True)
    g = torch.Generator().manual_seed(5)
    buf = torch.zeros(M, K + Rp, dtype=BF, device=DEV)
    buf[:, :K] = torch.randn(M, K, generator=g).to(BF).to(DEV)
    return c, buf, weight_of(c["qw"], c["sw"])


def test_ops_gemm_routes_to_the_fp8_pair_bit_for_bit():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    c, buf, w = _routed_pair()
    a, bias = buf[:, :512], c["bias"].to(DEV)
    base = ops.gemm(a, w, bias).clone()                         # compute = "bf16": dequantise + bf16 GEMM
    w.compute = "fp8"
    assert ops.fp8_compute_route(a, w)
    routed = ops.gemm(a, w, bias, epilogue="gelu").clone()
    q, s = ops.quant_rows_fp8(a)
    manual = ops.gemm_fp8(q, s, w, bias, epilogue="gelu")
    plain = ops.gemm(a, w, bias).clone()
    w.compute = "bf16"
    again = ops.gemm(a, w, bias)
    torch.cuda.synchronize()
    assert torch.equal(routed, manual)
    assert not torch.equal(plain, base) and float((plain.float() - base.float()).norm() / base.float().norm()) < 0.1
    assert torch.equal(again, base), "switching back restores the bf16 path bit for bit"


def test_a_weight_with_lora_factors_keeps_the_bf16_path():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    c, buf, w = _routed_pair()
    g = torch.Generator().manual_seed(6)
    w.parts = [("lin", 0, 272)]
    w.set_lora([("lin", torch.randn(4, 512, generator=g) * 0.1, torch.randn(272, 4, generator=g) * 0.1, 1.0)])
    a, bias = buf[:, :512], c["bias"].to(DEV)
    want = ops.gemm(a, w, bias, lora_buf=buf).clone()
    w.compute = "fp8"
    assert not ops.fp8_compute_route(a, w)
    got = ops.gemm(a, w, bias, lora_buf=buf)
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_graph_capture_replays_the_eager_result():
    """One `ops.gemm` in fp8 mode is two launches on one stream — a linear chain — with no host synchronisation: it captures."""
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    c, buf, w = _routed_pair()
    w.compute = "fp8"
    a, bias = buf[:, :512], c["bias"].to(DEV)
    out = torch.zeros(200, 272, dtype=BF, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = ops.gemm(a, w, bias, out=out).clone()            # also sizes this stream's scratch before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.gemm(a, w, bias, out=out)
    a.copy_(a * 2)                                               # new input, same buffers
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = ops.gemm(a, w, bias)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and not torch.equal(out, eager)
