"""The run-time LoRA form of the FP8 GEMM on the GPU: `ops.gemm_fp8(lora_t=, lora_B=)`, the fp8-LoRA route of
`ops.gemm`, `WanTransformer3DModel.set_fp8_compute(True, lora=True)` and the engines' `fp8_lora`.

Exact probes (operands and references: tests/gemm_fp8_lora_probes.py; their conditions and what the comparison rejects:
tests/test_gemm_fp8_lora_host.py): whole sentinel-filled buffers compared with torch.equal.  Operands travel the way the product
passes them: t is a column view right behind the bf16 source of the codes (ldt > Rp), B' has ldb > Rp, the codes have a padded row
stride, out is a guarded column slice.  tanh GELU is judged by gemm_fp8_probes.gelu_judge on the exact pre-activation.

Found by these probes: no kernel or wrapper bug.  Measured on the MI355X (profiles/gemm_fp8_lora_measured.jsonl; `measured`
records them): the values stand beside the calls."""
import pytest
import torch

from tests import gemm_fp8_lora_probes as L
from tests import gemm_fp8_probes as P
from tests.conftest import measured
from tests.gemm_fp8_probes import BF, F8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U8 = torch.uint8


def _ops():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    return ops


def _codes_and_t(codes, t, extra=64):
    """(codes [M, K] with a padded row stride, t [M, Rp] as the columns K .. K + Rp of a wider bf16 buffer whose first K columns
    stand for the codes' bf16 source): lda > K, ldt = K + Rp + extra"""
    M, K = codes.shape
    Rp = t.shape[1]
    qbuf = torch.full((M, K + 128), P.SENTINEL_CODE, dtype=U8, device=DEV)
    qbuf[:, :K] = codes.to(DEV)
    abuf = torch.full((M, K + Rp + extra), P.SENTINEL, dtype=BF, device=DEV)
    abuf[:, K:K + Rp] = t.to(BF).to(DEV)
    return qbuf[:, :K], abuf[:, K:K + Rp]


def _padded_b(lb, extra=64):
    N, Rp = lb.shape
    bbuf = torch.full((N, Rp + extra), P.SENTINEL, dtype=BF, device=DEV)
    bbuf[:, :Rp] = lb.to(BF).to(DEV)
    return bbuf[:, :Rp]


def _check_exact(buf, want, what):
    torch.cuda.synchronize()
    msg = P.buffer_mismatches(buf.cpu(), want)
    assert not msg, f"{what}: {msg}"


def _check_gelu(buf, x, what):
    """the view under the project's GELU bars, everything around it still the sentinel"""
    torch.cuda.synchronize()
    host = buf.cpu()
    M, N = x.shape
    got = host[1:M + 1, P.GUARD:P.GUARD + N]
    full = torch.full_like(host, P.SENTINEL)
    full[1:M + 1, P.GUARD:P.GUARD + N] = got
    assert torch.equal(host, full), f"{what}: store outside the output view"
    assert not bool((got == P.SENTINEL).any()), f"{what}: elements left at the sentinel"
    worst, equal = P.gelu_judge(got, x)
    print(f"[{what}] worst {worst} bf16 ulp from the float64 definition, {100 * equal:.3f} % equal")
    assert worst <= P.GELU_MAX_ULP and equal > P.GELU_MIN_EQUAL, (what, worst, equal)


# ------------------------------------------------------------------------------------------------------------ fixed point
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_fixed_point_adapter_tail_is_exact(case):
    """scales in the accumulators, then the adapter tail, then the bias: bias / gate_res (separate and in place) exactly, per-row
    and single sw, bias present and None; gelu under the project's bars"""
    ops = _ops()
    M, N, K, Rp = case
    lo = L.fixed_point(*case)
    op = lo.op
    qa, t = _codes_and_t(P.codes_of(op.qa), lo.t)
    lb = _padded_b(lo.lb)
    assert t.stride(0) > Rp and lb.stride(0) > Rp and qa.stride(0) > K
    qw = P.codes_of(op.qw).view(F8).to(DEV)
    w = {True: ops.Fp8Weight(qw, op.sw.to(DEV)), False: ops.Fp8Weight(qw, op.sw_one.to(DEV))}
    sa, bias_d, gate, res = op.sa.to(DEV), op.bias.to(BF).to(DEV), op.gate.to(DEV), op.res.to(BF).to(DEV)
    for epilogue, per_row, bias in L.EXACT_VARIANTS + L.GELU_VARIANTS:
        for inplace in ((False, True) if epilogue == "gate_res" else (False,)):
            what = f"gemm_fp8 lora {L.case_id(case)} {epilogue} sw={'row' if per_row else 'one'} bias={bias} inplace={inplace}"
            buf, view = P.sentinel_buffer(M, N, DEV)
            kw = {}
            if epilogue == "gate_res":
                if inplace:
                    view.copy_(res)
                kw = dict(gate=gate, residual=view if inplace else res)
            out = ops.gemm_fp8(qa, sa, w[per_row], bias_d if bias else None, out=view, epilogue=epilogue, lora_t=t, lora_B=lb, **kw)
            assert out.data_ptr() == view.data_ptr()
            if epilogue == "gelu":
                assert L.span_log2(lo, "bias", per_row, bias) < L.SPAN_BITS
                _check_gelu(buf, L.pre_activation(lo, per_row, bias), what)
            else:
                _check_exact(buf, L.want(M, N, K, Rp, epilogue, per_row, bias), what)
    # the plain form on the same operands is still the plain result: the two forms do not share state
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(qa, sa, w[True], bias_d, out=view)
    _check_exact(buf, P.want(M, N, K), f"plain gemm_fp8 {M}x{N}x{K} after the LoRA launches")


def test_one_hot_rank_pins_the_bf16_lane_map_and_the_rank_tile_order():
    """all codes zero, one product per output: every one of the 64 positions of a rank tile, in both tiles of Rp = 128"""
    ops = _ops()
    oh = L.one_hot()
    M, N, K, Rp = L.ONE_HOT
    qa, t = _codes_and_t(torch.zeros(M, K, dtype=U8), oh.t)
    w = ops.Fp8Weight(torch.zeros(N, K, dtype=U8, device=DEV).view(F8), oh.sw.to(DEV))
    buf, view = P.sentinel_buffer(M, N, DEV)
    ops.gemm_fp8(qa, oh.sa.to(DEV), w, None, out=view, lora_t=t, lora_B=_padded_b(oh.lb))
    _check_exact(buf, P.expected(oh.ref()), "one-hot rank")


def test_c_entry_point_with_padded_weight_rows():
    """apexmi_gemm_fp8_lora called directly: ldw > K (ops.Fp8Weight always packs) and ldr != ldc"""
    _ops()
    from apex_studio_amd import lib
    case = L.CASES[0]
    M, N, K, Rp = case
    lo = L.fixed_point(*case)
    op = lo.op
    qa, t = _codes_and_t(P.codes_of(op.qa), lo.t)
    lb = _padded_b(lo.lb)
    qw = torch.full((N, K + 64), P.SENTINEL_CODE, dtype=U8, device=DEV)
    qw[:, :K] = P.codes_of(op.qw).to(DEV)
    sw, sa, bias, gate = op.sw.to(BF).to(DEV), op.sa.to(DEV), op.bias.to(BF).to(DEV), op.gate.to(DEV)
    rbuf = torch.full((M, N + 40), P.SENTINEL, dtype=BF, device=DEV)
    res = rbuf[:, 4:4 + N]
    res.copy_(op.res.to(BF).to(DEV))
    st = torch.cuda.current_stream().cuda_stream
    for epi, name in ((lib.EPI_BIAS, "bias"), (lib.EPI_BIAS_GATE_RES, "gate_res")):
        buf, view = P.sentinel_buffer(M, N, DEV)
        rc = lib.load().apexmi_gemm_fp8_lora(qa.data_ptr(), qa.stride(0), sa.data_ptr(), qw.data_ptr(), qw.stride(0), 0, sw.data_ptr(), N,
                                             bias.data_ptr(), view.data_ptr(), view.stride(0), M, N, K, epi, gate.data_ptr(),
                                             res.data_ptr(), res.stride(0), t.data_ptr(), t.stride(0), lb.data_ptr(), lb.stride(0),
                                             Rp, st)
        lib.check(rc, "gemm_fp8_lora")
        _check_exact(buf, L.want(M, N, K, Rp, name), f"C entry point {name}")


# -------------------------------------------------------------------------------------------------------- random operands
_CASES = {}


def quant_reference(a):
    """The formula of `apexmi_quant_rows_fp8`, restated with torch on the CPU (tests/test_gpu_gemm_fp8.py's)."""
    x = a.float()
    amax = x.abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    y = torch.minimum(torch.maximum(x / scale, torch.full_like(x, -448.0)), torch.full_like(x, 448.0))
    return y.to(F8).view(U8), scale.reshape(-1)


def _case(M, N, K, Rp, per_row):
    """tests/test_gpu_gemm_fp8.py's `_case` recipe, plus random bf16 t and B' sized so that the adapter term is as large as the
    base product: t rows on the scale of the activation rows (sa x 128 = their standard deviation), B' at 0.02 sqrt(K / Rp)"""
    key = (M, N, K, Rp, per_row)
    if key not in _CASES:
        g = torch.Generator().manual_seed(M + 3 * N + 7 * K + per_row)
        qa, sa = quant_reference((torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)).to(BF))
        w = torch.randn(N, K, generator=g) * 0.02
        sw = ((w.abs().amax(dim=1) if per_row else w.abs().max().reshape(1)) / 448.0).to(BF)
        qw = (w / sw.float().view(-1, 1)).clamp(-448, 448).to(F8)
        bias = torch.randn(N, generator=g).to(BF) * 0.5
        gate = torch.randn(N, generator=g)
        res = torch.randn(M, N, generator=g).to(BF)
        t = (torch.randn(M, Rp, generator=g) * sa.view(-1, 1) * 128.0).to(BF)
        lb = (torch.randn(N, Rp, generator=g) * 0.02 * (K / Rp) ** 0.5).to(BF)
        base = (qa.view(F8).float() @ qw.float().T) * sa.view(-1, 1) * sw.float().view(1, -1) + bias.float()
        y = (qa.view(F8).float() @ qw.float().T) * sa.view(-1, 1) * sw.float().view(1, -1) + t.float() @ lb.float().T + bias.float()
        matters = float((y - base).norm() / y.norm())
        assert matters > 0.3, f"the adapter term must matter: rel-L2 with against without {matters:.3f}"
        gelu = torch.nn.functional.gelu(y.double(), approximate="tanh").float()          # float64: see tests/test_gpu_gemm_fp8.py
        ref = {"bias": y, "gelu": gelu, "gate_res": res.float() + gate * y}
        _CASES[key] = dict(qa=qa, sa=sa, qw=qw.view(U8), sw=sw, bias=bias, gate=gate, res=res, t=t, lb=lb, ref=ref)
    return _CASES[key]


# The project's bar for this kernel family (tests/test_gpu_gemm_fp8.py's _BARS): the adapter term adds f32 accumulation only, no
# rounding point.  Measured on the MI355X over the two shapes and both scale kinds (profiles/gemm_fp8_lora_measured.jsonl):
# bias 1.657e-3 .. 1.685e-3, gelu 1.653e-3 .. 1.668e-3, gate_res 1.655e-3 .. 1.704e-3; within 1 bf16 ulp 99.14 % .. 99.97 %
_BAR = 3.3e-3


@pytest.mark.parametrize("epilogue", ["bias", "gelu", "gate_res"])
@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("shape", [(200, 272, 512, 64), (129, 5120, 256, 128)], ids=L.case_id)
def test_random_operands_under_every_epilogue(shape, per_row, epilogue):
    ops = _ops()
    M, N, K, Rp = shape
    c = _case(M, N, K, Rp, per_row)
    w = ops.Fp8Weight(c["qw"].view(F8).to(DEV), c["sw"].to(DEV))
    qa, t = _codes_and_t(c["qa"], c["t"])
    big = torch.full((M, N + 32), 7.0, dtype=BF, device=DEV)                  # out is a column slice
    kw = dict(gate=c["gate"].to(DEV), residual=c["res"].to(DEV)) if epilogue == "gate_res" else {}
    out = ops.gemm_fp8(qa, c["sa"].to(DEV), w, c["bias"].to(DEV), out=big[:, 16:16 + N], epilogue=epilogue, lora_t=t,
                       lora_B=_padded_b(c["lb"]), **kw)
    torch.cuda.synchronize()
    assert float((big[:, :16].float() - 7).abs().max()) == 0 and float((big[:, 16 + N:].float() - 7).abs().max()) == 0
    got, ref = out.cpu(), c["ref"][epilogue]
    rel = float((got.float() - ref).norm() / ref.norm())
    ulp = (P.G._ordered(got) - P.G._ordered(ref.to(BF))).abs()
    within = float((ulp <= 1).float().mean())
    print(f"[gemm_fp8 lora {L.case_id(shape)} {'row' if per_row else 'one'} {epilogue}] rel-L2 {rel:.3e}, within 1 bf16 ulp "
          f"{within:.5f}, max ulp {int(ulp.max())}")
    measured(f"gemm_fp8_lora.{epilogue}.{M}x{N}x{K}.r{Rp}.{'row' if per_row else 'one'}", rel, _BAR)
    assert within >= 0.99, within


# ------------------------------------------------------------------------------------------------------------------ route
def _routed(M=200, N=272, K=512, rank=4):
    ops = _ops()
    c = _case(M, N, K, 64, True)
    w = ops.Fp8Weight(c["qw"].view(F8).to(DEV), c["sw"].to(DEV))
    g = torch.Generator().manual_seed(6)
    w.parts = [("lin", 0, N)]
    Rp = w.set_lora([("lin", torch.randn(rank, K, generator=g) * 0.1, torch.randn(N, rank, generator=g) * 0.1, 1.0)])
    buf = torch.zeros(M, K + Rp, dtype=BF, device=DEV)
    buf[:, :K] = torch.randn(M, K, generator=g).to(BF).to(DEV)
    return c, buf, w, Rp


@pytest.mark.parametrize("epilogue", ["bias", "gelu", "gate_res"])
def test_ops_gemm_routes_to_the_hand_made_sequence_bit_for_bit(epilogue):
    ops = _ops()
    c, buf, w, Rp = _routed()
    M, K = buf.shape[0], 512
    a, bias = buf[:, :K], c["bias"].to(DEV)
    kw = dict(gate=c["gate"].to(DEV), residual=c["res"].to(DEV)) if epilogue == "gate_res" else {}
    today = ops.gemm(a, w, bias, lora_buf=buf, epilogue=epilogue, **kw).clone()           # compute = "bf16": _gemm_fp8_lora
    w.compute = "fp8"
    assert not ops.fp8_lora_route(a, w, None, epilogue, buf) and not ops.fp8_compute_route(a, w, None, epilogue)
    fallback = ops.gemm(a, w, bias, lora_buf=buf, epilogue=epilogue, **kw).clone()        # the flag cleared: today's path
    w.lora_compute = "fp8"
    assert ops.fp8_lora_route(a, w, None, epilogue, buf)
    buf[:, K:].zero_()
    routed = ops.gemm(a, w, bias, lora_buf=buf, epilogue=epilogue, **kw).clone()
    tbuf = torch.zeros(M, Rp + 8, dtype=BF, device=DEV)
    t = ops.gemm(a, w.lora_A, None, out=tbuf[:, :Rp])
    q, s = ops.quant_rows_fp8(a)
    manual = ops.gemm_fp8(q, s, w, bias, epilogue=epilogue, lora_t=t, lora_B=w.lora_B, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf[:, K:K + Rp], t), "the skinny GEMM writes t behind the activations"
    assert torch.equal(routed, manual)
    assert torch.equal(fallback, today), "with the flag cleared the launches are today's, bit for bit"
    assert not torch.equal(routed, today)
    rel = float((routed.float() - today.float()).norm() / today.float().norm())
    assert rel < 0.1, rel          # the same product in narrower arithmetic, not another result


# ---------------------------------------------------------------------------------------------- tiny resident-fp8 Wan model
DIM, FFN, LAYERS = 256, 512, 3
CFG = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=FFN, num_layers=LAYERS, cross_attn_norm=True, eps=1e-6)


def _fp8_scaled_file(tmp_path):
    """tests/test_gpu_wan_fp8_compute.py's recipe: an original-format Wan file whose block Linears are fp8-scaled"""
    from safetensors.torch import save_file
    from tests.golden.make_golden_specs import wan_original_spec
    from tests.golden.seeded import spec_tensors
    wan = {k: v.to(BF) for k, v in spec_tensors(wan_original_spec(dim=DIM, ffn=FFN, text_dim=64, freq=256, layers=LAYERS), 5200).items()}
    for k in [k for k in wan if k.startswith("blocks.") and k.endswith(".weight") and wan[k].dim() == 2]:
        w = wan[k].float()
        s = (w.abs().max() / 448.0).reshape(())
        wan[k] = (w / s).to(F8)
        wan[k[:-len("weight")] + "scale_weight"] = s
    wan["scaled_fp8"] = torch.zeros(2, dtype=F8)
    path = str(tmp_path / "wan_fp8.safetensors")
    save_file({k: v.contiguous() for k, v in wan.items()}, path)
    return path


def _model(tmp_path):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import weights
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**CFG, device="cuda", dtype=BF)
    assert weights.load_checkpoint_into(m, [_fp8_scaled_file(tmp_path)], keep_fp8=True) == ([], [])
    return m


def _fwd(m):
    from tests.golden.seeded import seeded
    x, txt, t = seeded((1, 16, 3, 16, 24), 41).to(BF).to("cuda"), seeded((1, 20, 64), 42).to(BF).to("cuda"), torch.tensor([537.0], device="cuda")
    out = m(hidden_states=x, timestep=t, encoder_hidden_states=txt, return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def _adapter():
    """the rank-4 adapter of test_run_time_lora_falls_back_to_the_bf16_path: every block Linear"""
    from tests.golden.seeded import spec_tensors
    r, spec = 4, {}
    for i in range(LAYERS):
        for at, n in (("self_attn", "q"), ("self_attn", "o"), ("cross_attn", "q"), ("cross_attn", "k"), ("cross_attn", "v"),
                      ("cross_attn", "o")):
            k = f"diffusion_model.blocks.{i}.{at}.{n}"
            spec.update({k + ".lora_down.weight": (r, DIM), k + ".lora_up.weight": (DIM, r), k + ".alpha": ()})
        spec.update({f"diffusion_model.blocks.{i}.ffn.0.lora_down.weight": (r, DIM), f"diffusion_model.blocks.{i}.ffn.0.lora_up.weight": (FFN, r),
                     f"diffusion_model.blocks.{i}.ffn.2.lora_down.weight": (r, FFN), f"diffusion_model.blocks.{i}.ffn.2.lora_up.weight": (DIM, r)})
    return {k: (v * 0.3 if v.dim() == 2 else v) for k, v in spec_tensors(spec, 3100).items()}


@pytest.fixture(scope="module")
def forwards(tmp_path_factory):
    """every forward of the model tests, computed once: plain and with the adapter, in the three modes"""
    m = _model(tmp_path_factory.mktemp("wan_fp8_lora"))
    f = {"bf16_plain": _fwd(m)}
    m.set_fp8_compute(True)
    f["fp8_plain"] = _fwd(m)
    m.set_fp8_compute(False)
    m.load_lora_adapter({k: v.clone() for k, v in _adapter().items()}, adapter_name="lx")
    assert all(rec.lora_A is not None for rec in m._fp8_records.values())
    f["bf16_lora"] = _fwd(m)
    m.set_fp8_compute(True)
    f["fallback_lora"] = _fwd(m)
    m.set_fp8_compute(True, lora=True)
    assert all(rec.lora_compute == "fp8" and rec.compute == "fp8" for rec in m._fp8_records.values())
    f["fp8_lora"] = _fwd(m)
    m.delete_adapters("lx")
    f["fp8_after_delete"] = _fwd(m)
    m.set_fp8_compute(False)
    assert all(rec.lora_compute == "bf16" and rec.compute == "bf16" for rec in m._fp8_records.values())
    f["bf16_after_off"] = _fwd(m)
    # adapters loaded AFTER the call take the flag as well: it lives on the records
    m.set_fp8_compute(True, lora=True)
    m.load_lora_adapter({k: v.clone() for k, v in _adapter().items()}, adapter_name="ly")
    f["fp8_lora_loaded_after"] = _fwd(m)
    return f


def test_wan_switch_identities(forwards):
    f = forwards
    assert not torch.equal(f["bf16_lora"], f["bf16_plain"])
    assert torch.equal(f["fallback_lora"], f["bf16_lora"]), "set_fp8_compute(True) alone: today's documented fallback"
    assert torch.isfinite(f["fp8_lora"]).all() and not torch.equal(f["fp8_lora"], f["bf16_lora"])
    assert not torch.equal(f["fp8_lora"], f["fp8_plain"])
    assert torch.equal(f["fp8_after_delete"], f["fp8_plain"]), "delete_adapters returns to the plain fp8 forward"
    assert torch.equal(f["bf16_after_off"], f["bf16_plain"]), "set_fp8_compute(False) returns to the plain bf16 forward"
    assert torch.equal(f["fp8_lora_loaded_after"], f["fp8_lora"]), "adapters loaded before or after the call"


def test_wan_fp8_lora_forward_is_bounded(forwards):
    """The references are the parent's bf16 forwards.  d compares the adapter's EFFECT in the two modes; a missing or mis-scaled
    adapter term gives d of about 1, hence the a-priori condition d < 0.5."""
    f = forwards

    def rel(x, ref):
        return float((x - ref).norm() / ref.norm())
    e_plain = rel(f["fp8_plain"], f["bf16_plain"])
    e_lora = rel(f["fp8_lora"], f["bf16_lora"])
    d = rel(f["fp8_lora"] - f["fp8_plain"], f["bf16_lora"] - f["bf16_plain"])
    print(f"[wan fp8 lora] {LAYERS} blocks of width {DIM}: e_plain {e_plain:.3e}, e_lora {e_lora:.3e}, adapter effect d {d:.3e} "
          f"(effect / output {rel(f['bf16_lora'], f['bf16_plain']):.3e})")
    assert d < 0.5, d
    # measured on the MI355X (profiles/gemm_fp8_lora_measured.jsonl): e_plain 2.700e-2, e_lora 2.648e-2, d 2.330e-1 (the adapter
    # changes the bf16 output by 1.600e-1 rel-L2); the bars are 2x those
    measured("wan.fp8_lora.tiny.e_plain", e_plain, 5.4e-2)
    measured("wan.fp8_lora.tiny.e_lora", e_lora, 5.3e-2)
    measured("wan.fp8_lora.tiny.d", d, 4.7e-1)


def test_engine_sets_the_flag_on_both_experts(tmp_path):
    from apex_studio_amd.engine_wan import WanT2VEngine
    hi, lo = _model(tmp_path), _model(tmp_path)
    eng = WanT2VEngine(hi, lo, fp8_compute=True, fp8_lora=True)
    assert eng.fp8_compute and eng.fp8_lora
    for m in (hi, lo):
        assert all(r.compute == "fp8" and r.lora_compute == "fp8" for r in m._fp8_records.values())
    with pytest.raises(ValueError, match="fp8_compute=True"):
        WanT2VEngine(hi, lo, fp8_lora=True)
    eng = WanT2VEngine(hi, lo, fp8_compute=True)
    assert all(r.compute == "fp8" and r.lora_compute == "bf16" for r in hi._fp8_records.values())
