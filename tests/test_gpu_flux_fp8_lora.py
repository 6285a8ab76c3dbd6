"""Flux run-time LoRA on resident fp8 weights on the GPU: `FluxTransformer2DModel.set_fp8_compute(True, lora=True)`
and `FluxT2IEngine(fp8_lora=True)`, on the tiny Flux of tests/test_gpu_flux_fp8_compute.py (2 heads of 128, width 256; its
`fp8_file` recipe restated here) with a rank-4 adapter on every block Linear of every block.  Every forward is computed once."""
import pytest
import torch

from tests.conftest import measured

pytestmark = pytest.mark.gpu
DEV, BF = "cuda:0", torch.bfloat16
DOUBLE, SINGLE = 2, 2
CFG = dict(patch_size=1, in_channels=64, num_layers=DOUBLE, num_single_layers=SINGLE, attention_head_dim=128, num_attention_heads=2,
           joint_attention_dim=256, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
H2 = W2 = 16
DIM, MLP = 256, 1024


def _flux():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.flux import FluxTransformer2DModel
    return FluxTransformer2DModel(**CFG, device=DEV, dtype=BF)


@pytest.fixture(scope="module")
def fp8_file(tmp_path_factory):
    """A diffusers-keyed Flux file whose block Linears are fp8-scaled: per-tensor absmax / 448, `scale_weight` beside each"""
    from safetensors.torch import save_file
    from tests.golden.seeded import synthetic_state_dict
    m = _flux()
    sd = {k: v.to(BF) for k, v in synthetic_state_dict(m, 5).items()}
    for k in [k for k in sd if m._fp8_resident_key(k) and sd[k].dim() == 2]:
        w = sd[k].float()
        s = (w.abs().max() / 448.0).reshape(())
        sd[k] = (w / s).to(torch.float8_e4m3fn)
        sd[k[:-len("weight")] + "scale_weight"] = s
    path = str(tmp_path_factory.mktemp("flux_fp8_lora") / "flux_fp8.safetensors")
    save_file({k: v.contiguous() for k, v in sd.items()}, path)
    return path


def _load(path, keep_fp8):
    from apex_studio_amd import weights
    m = _flux()
    assert weights.load_checkpoint_into(m, [path], keep_fp8=keep_fp8) == ([], [])
    return m


def _inputs(s_txt=72):
    from oracle import flux as OF
    from tests.golden.seeded import seeded
    return dict(hidden_states=seeded((1, H2 * W2, 64), 31).to(DEV).to(BF), encoder_hidden_states=seeded((1, s_txt, 256), 32).to(DEV).to(BF),
                pooled_projections=seeded((1, 64), 33).to(DEV).to(BF), timestep=torch.tensor([0.5], device=DEV),
                guidance=torch.tensor([4.0], device=DEV), img_ids=OF.latent_image_ids(H2, W2).to(DEV),
                txt_ids=torch.zeros(s_txt, 3, device=DEV))


def _fwd(m, s_txt=72):
    out = m(return_dict=False, **_inputs(s_txt))[0]
    torch.cuda.synchronize()
    return out.float().cpu()


ADAPTER_STD = 0.053       # sized so that the adapter changes the bf16 output by roughly a tenth in rel-L2 (printed by the test)


def _adapter(bias_on=None):
    """rank 4 on every block Linear of every block (PEFT keys)"""
    from tests.golden.seeded import seeded
    mods = []
    for i in range(DOUBLE):
        b = f"transformer_blocks.{i}."
        mods += [(b + f"attn.{n}", DIM, DIM) for n in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out")]
        mods += [(b + "ff.net.0.proj", DIM, MLP), (b + "ff.net.2", MLP, DIM), (b + "ff_context.net.0.proj", DIM, MLP),
                 (b + "ff_context.net.2", MLP, DIM)]
    for i in range(SINGLE):
        b = f"single_transformer_blocks.{i}."
        mods += [(b + f"attn.{n}", DIM, DIM) for n in ("to_q", "to_k", "to_v")]
        mods += [(b + "proj_mlp", DIM, MLP), (b + "proj_out", DIM + MLP, DIM)]
    sd = {}
    for j, (m, k, n) in enumerate(mods):
        sd[f"{m}.lora_A.weight"] = seeded((4, k), 700 + 2 * j) * ADAPTER_STD
        sd[f"{m}.lora_B.weight"] = seeded((n, 4), 701 + 2 * j) * ADAPTER_STD
    if bias_on is not None:
        sd[f"{bias_on}.lora_B.bias"] = torch.zeros(DIM)
    return sd


def _count(ops, names):
    calls = {n: 0 for n in names}
    orig = {n: getattr(ops, n) for n in names}

    def counted(n):
        def wrapper(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return wrapper
    for n in names:
        setattr(ops, n, counted(n))
    return calls, orig


@pytest.fixture(scope="module")
def forwards(fp8_file):
    from apex_studio_amd import ops
    f = {}
    a = _load(fp8_file, False)
    f["bf16_plain"] = _fwd(a)
    a.load_lora_adapter(_adapter(), adapter_name="lx")
    f["bf16_lora"] = _fwd(a)
    del a
    m = _load(fp8_file, True).set_fp8_compute(True)
    f["fp8_plain"], f["fp8_plain_77"] = _fwd(m), _fwd(m, 77)
    m.set_fp8_compute(True, lora=True)
    assert all(r.compute == "fp8" and r.lora_compute == "fp8" for r in m._fp8_records.values())
    m.load_lora_adapter(_adapter(), adapter_name="lx")
    assert all(r.lora_A is not None and r.lora_A.shape[0] == 64 for r in m._fp8_records.values())
    names = ("gemm_grouped", "dequant_fp8_scaled", "gemm_fp8_grouped_qkv", "gemm_fp8_grouped", "gemm_fp8")
    calls, orig = _count(ops, names)
    try:
        f["fp8_lora"] = _fwd(m)
    finally:
        for n in names:
            setattr(ops, n, orig[n])
    f["calls"] = calls
    f["fp8_lora_77"] = _fwd(m, 77)
    m.fuse_qkv = False
    f["two_pass"], f["two_pass_77"] = _fwd(m), _fwd(m, 77)
    m.fuse_qkv = True
    m.set_fp8_compute(True, fused_quant=True, lora=True)
    f["fused_quant"] = _fwd(m)
    m.set_fp8_compute(True, mx_ffn=True, lora=True)
    f["mx_ffn"] = _fwd(m)
    m.set_fp8_compute(True, lora=True)
    m.set_adapters(["lx"], [0.0])
    f["scale0"] = _fwd(m)
    m.set_adapters(["lx"], [1.0])
    f["scale1_again"] = _fwd(m)
    m.delete_adapters("lx")
    assert all(r.lora_A is None for r in m._fp8_records.values())
    f["after_delete"] = _fwd(m)
    m2 = _load(fp8_file, True)
    m2.set_fp8_compute(True, lora=True)
    m2.load_lora_adapter(_adapter(), adapter_name="ly", activate=False)
    m2.set_adapters(["ly"])
    f["loaded_deferred"] = _fwd(m2)
    return f


def test_switch_identities(forwards):
    f = forwards
    assert torch.isfinite(f["fp8_lora"]).all() and not torch.equal(f["fp8_lora"], f["fp8_plain"])
    assert torch.equal(f["after_delete"], f["fp8_plain"]), "delete_adapters returns to the plain fp8 forward"
    assert torch.equal(f["scale0"], f["fp8_plain"]), "scale 0 is the plain fp8 forward"
    assert torch.equal(f["scale1_again"], f["fp8_lora"])
    assert torch.equal(f["loaded_deferred"], f["fp8_lora"]), "adapters registered in another order / on another model"
    assert torch.equal(f["two_pass"], f["fp8_lora"]), "fuse_qkv on / off"
    assert torch.equal(f["fused_quant"], f["fp8_lora"]), "fused_quant on / off"
    assert torch.equal(f["mx_ffn"], f["fp8_lora"]), "mx_ffn with factors on the FF records keeps the per-row launches"


def test_text_length_77(forwards):
    f = forwards
    assert torch.isfinite(f["fp8_lora_77"]).all() and not torch.equal(f["fp8_lora_77"], f["fp8_plain_77"])
    assert torch.equal(f["two_pass_77"], f["fp8_lora_77"]), "the element-wise V^T store with an adapter"


def test_launch_counts(forwards):
    """every block launch stays on the fp8 GEMM: the only bf16 grouped launches are the skinny ones, nothing is dequantised"""
    c = forwards["calls"]
    skinny = 4 * DOUBLE + 2 * SINGLE          # QKV, out, FF-up, FF-down per double block; QKV + MLP-up, proj_out per single block
    assert c["gemm_grouped"] == skinny and c["dequant_fp8_scaled"] == 0, c
    assert c["gemm_fp8_grouped_qkv"] == DOUBLE + SINGLE and c["gemm_fp8_grouped"] == 3 * DOUBLE and c["gemm_fp8"] == SINGLE, c


def test_bounded(forwards):
    """d compares the adapter's EFFECT in the two modes; a missing or mis-scaled adapter term gives d of about 1, hence the
    a-priori condition d < 0.5.  The references are the shipped bf16 forwards (adapter merged at load)."""
    f = forwards

    def rel(x, ref):
        return float((x - ref).norm() / ref.norm())
    effect = rel(f["bf16_lora"], f["bf16_plain"])
    e_plain, e_lora = rel(f["fp8_plain"], f["bf16_plain"]), rel(f["fp8_lora"], f["bf16_lora"])
    d = rel(f["fp8_lora"] - f["fp8_plain"], f["bf16_lora"] - f["bf16_plain"])
    print(f"[flux fp8 lora] e_plain {e_plain:.3e}, e_lora {e_lora:.3e}, adapter effect d {d:.3e} (effect / output {effect:.3e})")
    assert d < 0.5, d
    # measured on the MI355X (profiles/flux_fp8_lora_measured.jsonl); the bars are 2x those
    measured("flux.fp8_lora.tiny.e_plain", e_plain, E_PLAIN_BAR)
    measured("flux.fp8_lora.tiny.e_lora", e_lora, E_LORA_BAR)
    measured("flux.fp8_lora.tiny.d", d, D_BAR)


# measured: e_plain 2.092e-2, e_lora 2.133e-2, d 2.682e-1
E_PLAIN_BAR, E_LORA_BAR, D_BAR = 4.18e-2, 4.27e-2, 5.4e-1


def test_refusals_leave_the_model_unchanged(fp8_file):
    from apex_studio_amd import lib
    m = _load(fp8_file, True)
    m.set_fp8_compute(True)
    before = _fwd(m)
    with pytest.raises(lib.ApexMIError, match=r"lora=True\)` first"):          # the flag is off
        m.load_lora_adapter(_adapter(), adapter_name="lx")
    assert "lx" not in m._lora_state() and torch.equal(_fwd(m), before)
    m.set_fp8_compute(True, lora=True)
    with pytest.raises(NotImplementedError, match="lora_B.bias"):
        m.load_lora_adapter(_adapter(bias_on="transformer_blocks.0.attn.to_out.0"), adapter_name="lb")
    assert "lb" not in m._lora_state() and torch.equal(_fwd(m), before)
    m.load_lora_adapter(_adapter(), adapter_name="lx")
    with_adapter = _fwd(m)
    for args, kw in (((False,), {}), ((True,), {}), ((True,), {"fused_quant": True})):
        with pytest.raises(lib.ApexMIError, match="delete or unload"):
            m.set_fp8_compute(*args, **kw)
    with pytest.raises(lib.ApexMIError, match="delete or unload"):
        m.set_residual_dtype(torch.float32)
    with pytest.raises(lib.ApexMIError, match="bf16 storage"):
        m.set_storage_dtype(torch.float32)
    assert torch.equal(_fwd(m), with_adapter)
    m.delete_adapters("lx")
    m.set_residual_dtype(torch.float32)
    with pytest.raises(lib.ApexMIError, match="bf16 residual stream"):
        m.load_lora_adapter(_adapter(), adapter_name="lx")
    assert "lx" not in m._lora_state()
    m.set_residual_dtype(torch.bfloat16)
    assert torch.equal(_fwd(m), before)


def test_engine(fp8_file):
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from tests.golden.seeded import seeded
    m = _load(fp8_file, True)
    with pytest.raises(ValueError, match="fp8_compute=True"):
        FluxT2IEngine(m, fp8_lora=True)
    eng = FluxT2IEngine(m, fp8_compute=True, fp8_lora=True)
    assert eng.fp8_lora and all(r.compute == "fp8" and r.lora_compute == "fp8" for r in m._fp8_records.values())

    def run():
        lat = eng.run(prompt_embeds=seeded((1, 72, 256), 32).to(DEV), pooled_prompt_embeds=seeded((1, 64), 33).to(DEV), height=256,
                      width=256, num_inference_steps=2, guidance_scale=3.5, latents=seeded((1, H2 * W2, 64), 41).to(DEV),
                      return_latents=True)
        torch.cuda.synchronize()
        return lat.float().cpu()
    plain = run()
    eng.apply_loras([(_adapter(), 1.0)])
    lat = run()
    assert torch.isfinite(lat).all() and float(lat.std()) > 0 and not torch.equal(lat, plain)
