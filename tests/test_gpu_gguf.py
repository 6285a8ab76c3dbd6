"""GGUF on the GPU: `apexmi_dequant_gguf` against the numpy reference dequantisers bit for bit, GGUF files loaded into the packed
Wan / Flux models, and block weights resident in HBM (`keep_quantized=True`) with run-time LoRA."""
import numpy as np
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import gguf_file as G
from tests.test_gguf_host import F16_FIELDS, random_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu(blocks, t, shape, ldo=None, fill=7.0):
    """ops.dequant_gguf into a [rows, ldo] buffer; returns (result view, the whole buffer) on the host"""
    from apex_studio_amd import ops
    rows, K = shape
    b = torch.from_numpy(np.ascontiguousarray(blocks)).to(DEV)
    if ldo is None:
        return ops.dequant_gguf(b, t, shape).cpu(), None
    buf = torch.full((rows, ldo), fill, dtype=torch.bfloat16, device=DEV)
    ops.dequant_gguf(b, t, shape, out=buf[:, :K])
    torch.cuda.synchronize()
    return buf[:, :K].cpu(), buf.cpu()


def _ref(blocks, t, shape):
    return G.dequantize_bf16(t, blocks).reshape(shape)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("t", sorted(G.TYPES), ids=lambda t: G.type_name(t))
def test_kernel_equals_reference_dequantiser(t):
    blk = max(G.TYPES[t][1], 32)
    for i, shape in enumerate([(1, blk), (3, 2 * blk), (40, 5120), (7, 13824)]):
        blocks = random_blocks(t, shape[0] * shape[1], 100 * t + i)
        want = _ref(blocks, t, shape)
        assert torch.isfinite(want.float()).all() or t in (G.F32,)          # F32 magnitudes may round to bf16 infinity: still bit-compared
        for ldo in (shape[1], shape[1] + 64):
            got, buf = _gpu(blocks, t, shape, ldo)
            assert _same_bits(got, want), (G.type_name(t), shape, ldo, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
            assert bool((buf[:, shape[1]:] == 7.0).all()), "columns behind K must stay untouched"
        got, _ = _gpu(blocks, t, shape)
        assert _same_bits(got, want)
        # a row range of the tensor (a byte range of the blocks) equals the same rows of the full call
        if shape[0] > 2:
            rb = blocks.size // shape[0]
            a, b = 1, shape[0] - 1
            part, _ = _gpu(blocks[a * rb:b * rb], t, (b - a, shape[1]))
            assert _same_bits(part, want[a:b]), (G.type_name(t), shape)


def _sweep(t):
    """Blocks in which every byte position of the payload and of the packed integer scales takes all 256 values."""
    _, blk, bs = G.TYPES[t]
    n = 256
    b = ((np.arange(n)[:, None] + 7 * np.arange(bs)[None, :]) & 255).astype(np.uint8)
    rng = np.random.default_rng(t)
    for o in F16_FIELDS[t]:
        b[:, o:o + 2] = np.array(rng.choice([1.0, -0.375, 3.0517578125e-05, 2.0e-7, 1001.0], n), dtype=np.float16).reshape(-1, 1).view(np.uint8)
    return b.reshape(-1), (n * blk // 1024, 1024)


@pytest.mark.parametrize("t", [G.Q8_0, G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1, G.Q4_K, G.Q5_K], ids=lambda t: G.type_name(t))
def test_exhaustive_integer_fields(t):
    blocks, shape = _sweep(t)
    payload = {G.Q8_0: (2, 34), G.Q4_0: (2, 18), G.Q4_1: (4, 20), G.Q5_0: (2, 22), G.Q5_1: (4, 24), G.Q4_K: (4, 144), G.Q5_K: (4, 176)}[t]
    by = blocks.reshape(256, -1)
    assert all(len(set(by[:, o])) == 256 for o in range(*payload)), "every payload byte takes every value"
    got, _ = _gpu(blocks, t, shape)
    assert _same_bits(got, _ref(blocks, t, shape))


def test_exhaustive_q6_k():
    """All 64 six-bit values in each of the four quarters x all 256 int8 scales."""
    b = np.zeros((256, 210), dtype=np.uint8)
    v = np.arange(32)[None, :] + 32 * np.arange(2)[:, None]                  # [half, l]: values 0..63
    nib = (v & 15).astype(np.uint8)
    b[:, 0:128] = np.stack([nib | (nib << 4)] * 2, axis=1).reshape(-1)       # ql[l], ql[l + 32] of both halves
    b[:, 128:192] = ((v >> 4) * 0b01010101).astype(np.uint8).reshape(-1)
    b[:, 192:208] = np.arange(256, dtype=np.uint8)[:, None]                  # every int8 scale
    b[:, 208:210] = np.array([0.5, -3.0, 6.1e-5, 1.2e-7] * 64, dtype=np.float16).reshape(-1, 1).view(np.uint8)
    ref = G.dequantize(G.Q6_K, b.reshape(-1)).reshape(256, 2, 4, 32)
    d, sc = b[:, 208:210].copy().view(np.float16).astype(np.float32), b[:, 192].view(np.int8).astype(np.float32)
    for q in range(4):      # the layout puts value v - 32 under scale sc in every quarter
        assert np.array_equal(ref[:, :, q, :], ((d[:, 0] * sc)[:, None, None] * (v - 32).astype(np.float32)[None]))
    got, _ = _gpu(b.reshape(-1), G.Q6_K, (16, 4096))
    assert _same_bits(got, _ref(b.reshape(-1), G.Q6_K, (16, 4096)))


def test_bad_arguments_raise():
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    b = torch.zeros(34 * 4, dtype=torch.uint8, device=DEV)
    for bad_type in (10, 11, 16, 39, 99):
        with pytest.raises(ApexMIError, match=f"type {bad_type}"):
            ops.dequant_gguf(b, bad_type, (1, 128))
    with pytest.raises(ApexMIError, match="multiple of the block length"):
        ops.dequant_gguf(b, G.Q8_0, (1, 100))
    with pytest.raises(ApexMIError, match="multiple of the block length"):
        ops.dequant_gguf(torch.zeros(144, dtype=torch.uint8, device=DEV), G.Q4_K, (2, 128))
    out = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ApexMIError, match="ldo=16"):
        import ctypes  # noqa: F401
        from apex_studio_amd import lib
        lib.check(lib.load().apexmi_dequant_gguf(b.data_ptr(), G.Q8_0, 4, 32, out.data_ptr(), 16, None), "dequant_gguf")
    with pytest.raises(ApexMIError, match="misaligned"):
        ops.dequant_gguf(b, G.Q8_0, (4, 32), out=torch.zeros(4, 36, dtype=torch.bfloat16, device=DEV)[:, :32])
    with pytest.raises(ApexMIError):
        ops.dequant_gguf(b.cpu(), G.Q8_0, (4, 32))
    with pytest.raises(ApexMIError, match="bytes do not hold"):
        ops.dequant_gguf(b, G.Q8_0, (8, 32))


# ---------------------------------------------------------------- model level
WAN_CFG = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
               freq_dim=256, ffn_dim=512, num_layers=2, cross_attn_norm=True, eps=1e-6)
FLUX_CFG = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2,
                joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))


def _write_pair(tmp_path, name, sd, block_prefixes):
    """`sd` (original-format keys) as a GGUF file — 2-D block weights quantised: `….q.weight` Q8_0, `….k.weight` Q4_0, `….v.weight` Q4_K
    (so the q | k | v the Wan model fuses mixes three types), every other one Q8_0 / Q4_0 / Q4_K by turns; the rest
    F16 (>= 2-D; > 4-D flattened with its original shape in the metadata) / F32 — and as a safetensors file of the
    reference-dequantised bf16 tensors."""
    from safetensors.torch import save_file
    w = G.GGUFWriter(str(tmp_path / f"{name}.gguf"))
    w.add_meta("general.architecture", name, G.STRING)
    ref, n_q, kinds = {}, 0, (G.Q8_0, G.Q4_0, G.Q4_K)
    for k, v in sd.items():
        v = v.float().numpy()
        if v.ndim == 2 and k.endswith(".weight") and k.startswith(block_prefixes) and v.shape[1] % 256 == 0:
            t = {"q": G.Q8_0, "k": G.Q4_0, "v": G.Q4_K}.get(k.split(".")[-2], kinds[n_q % 3])
            n_q += 1
            blocks = G.quantize(t, v)
            ref[k] = G.dequantize_bf16(t, blocks).reshape(v.shape).clone()
            w.add_tensor(k, v.shape, t, blocks)
        elif v.ndim >= 2:
            h = v.astype(np.float16)
            ref[k] = torch.from_numpy(h).to(torch.bfloat16)
            if v.ndim > 4:
                w.add_tensor(k, (v.shape[0], int(np.prod(v.shape[1:]))), G.F16, h, orig_shape=v.shape)
            else:
                w.add_tensor(k, v.shape, G.F16, h)
        else:
            ref[k] = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16)
            w.add_tensor(k, v.shape, G.F32, v.astype(np.float32))
    assert n_q >= 12
    pst = str(tmp_path / f"{name}_ref.safetensors")
    save_file({k: v.contiguous() for k, v in ref.items()}, pst)
    return w.write(), pst


def _wan_files(tmp_path):
    from tests.golden.make_golden_specs import wan_original_spec
    from tests.golden.seeded import spec_tensors
    sd = spec_tensors(wan_original_spec(dim=256, ffn=512, text_dim=64, freq=256), 5000)
    assert "blocks.0.self_attn.q.weight" in sd                               # original-format keys
    return _write_pair(tmp_path, "wan", sd, ("blocks.",))


def _wan_inputs():
    from tests.golden.seeded import seeded
    return (seeded((1, 16, 3, 16, 24), 41).to(torch.bfloat16), seeded((1, 20, 64), 42).to(torch.bfloat16), torch.tensor([537.0]))


def _wan_fwd(m, x, txt, t):
    out = m(hidden_states=x.to(DEV), timestep=t.to(DEV), encoder_hidden_states=txt.to(DEV), return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def test_gguf_files_load_into_the_packed_models(tmp_path):
    """Original-key GGUF files of a tiny Wan and a tiny Flux: nothing missing or unexpected, every parameter and the forward
    bit-identical to a model loaded from the reference-dequantised bf16 tensors through the safetensors path."""
    from apex_studio_amd import weights
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.wan import WanTransformer3DModel
    from tests.golden.make_golden_specs import flux_original_spec
    from tests.golden.seeded import seeded, spec_tensors
    pg, ps = _wan_files(tmp_path)
    a = WanTransformer3DModel(**WAN_CFG, device=DEV, dtype=torch.bfloat16)
    b = WanTransformer3DModel(**WAN_CFG, device=DEV, dtype=torch.bfloat16)
    assert weights.load_checkpoint_into(a, [pg]) == ([], [])
    assert weights.load_checkpoint_into(b, [ps]) == ([], [])
    sa, sb = a.state_dict(), b.state_dict()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    oa, ob = _wan_fwd(a, *_wan_inputs()), _wan_fwd(b, *_wan_inputs())
    assert torch.isfinite(oa).all() and float(oa.std()) > 0 and torch.equal(oa, ob)

    sd = spec_tensors(flux_original_spec(dim=256, txt=128, pooled=64), 6000)
    assert "double_blocks.0.img_attn.qkv.weight" in sd
    pg, ps = _write_pair(tmp_path, "flux", sd, ("double_blocks.", "single_blocks."))
    fa = FluxTransformer2DModel(**FLUX_CFG, device=DEV, dtype=torch.bfloat16)
    fb = FluxTransformer2DModel(**FLUX_CFG, device=DEV, dtype=torch.bfloat16)
    fa.pack()                                           # targets are row views of the fused matrices
    assert weights.load_checkpoint_into(fa, [pg]) == ([], [])
    assert weights.load_checkpoint_into(fb, [ps]) == ([], [])
    sa, sb = fa.state_dict(), fb.state_dict()
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    S, T = 64, 16
    args = dict(hidden_states=seeded((1, S, 64), 1).to(DEV, torch.bfloat16), encoder_hidden_states=seeded((1, T, 128), 2).to(DEV, torch.bfloat16),
                pooled_projections=seeded((1, 64), 3).to(DEV, torch.bfloat16), timestep=torch.tensor([0.7], device=DEV),
                guidance=torch.tensor([3.5], device=DEV), img_ids=torch.zeros(S, 3, device=DEV), txt_ids=torch.zeros(T, 3, device=DEV),
                return_dict=False)
    args["img_ids"][:, 1] = torch.arange(S, device=DEV) // 8
    args["img_ids"][:, 2] = torch.arange(S, device=DEV) % 8
    oa, ob = fa(**args)[0].float().cpu(), fb(**args)[0].float().cpu()
    assert torch.isfinite(oa).all() and float(oa.std()) > 0 and torch.equal(oa, ob)

    # a quantised tensor aimed at a parameter it does not fill, or at a float parameter, raises with the key
    w = G.GGUFWriter(str(tmp_path / "bad.gguf"))
    w.add_tensor("blocks.0.ffn.2.weight", (256, 256), G.Q8_0, G.quantize(G.Q8_0, np.ones(256 * 256)))
    with pytest.raises(ValueError, match=r"blocks\.0\.ffn\.net\.2\.weight"):
        weights.load_checkpoint_into(a, [w.write()])
    lin = torch.nn.Linear(256, 4, bias=False, device=DEV)
    w = G.GGUFWriter(str(tmp_path / "f32.gguf"))
    w.add_tensor("weight", (4, 256), G.Q8_0, G.quantize(G.Q8_0, np.ones(4 * 256)))
    with pytest.raises(TypeError, match="weight"):
        weights.load_checkpoint_into(lin, [w.write()], converter=None)


def test_gguf_blocks_resident_in_hbm_with_runtime_lora(tmp_path):
    """`keep_quantized=True` on the tiny Wan model: the block Linears stay ggml blocks in HBM (fused q | k | v of three types =
    three row segments), the forward is bit-identical to the dequantise-at-load model, fewer weight bytes are held, state_dict()
    raises; and the run-time LoRA case of tests/test_weights.py::test_fp8_resident_expert_runs_a_lightx2v_keyed_lora_at_run_time
    on GGUF weights, with that test's bars."""
    from apex_studio_amd import lib, lora, ops, weights
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.wan import WanTransformer3DModel
    from oracle import layers as OL, lora as OLR, wan as OWan
    from tests.golden.seeded import spec_tensors
    cfg = WAN_CFG
    pg, _ = _wan_files(tmp_path)
    a = WanTransformer3DModel(**cfg, device=DEV, dtype=torch.bfloat16)
    assert weights.load_checkpoint_into(a, [pg]) == ([], [])
    b = WanTransformer3DModel(**cfg, device=DEV, dtype=torch.bfloat16)
    assert weights.load_checkpoint_into(b, [pg], keep_quantized=True) == ([], [])
    lin = [p for n, p in b.named_parameters() if n.startswith("blocks.") and n.endswith(".weight") and p.dim() <= 2
           and ".norm" not in n and "scale_shift" not in n]
    assert lin and all(p.numel() == 0 for p in lin), [tuple(p.shape) for p in lin if p.numel()][:4]
    rec = b.blocks[0]._wqkv
    assert isinstance(rec, ops.GgufWeight) and isinstance(rec, ops.ResidentWeight) and tuple(rec.shape) == (768, 256)
    assert [(t, n) for t, n, _ in rec.segments] == [(G.Q8_0, 256), (G.Q4_0, 256), (G.Q4_K, 256)]
    n_lin = sum(p.numel() for n, p in a.named_parameters() if b._fp8_resident_key(n) and p.dim() == 2)
    assert 0.5 * n_lin < b._fp8_bytes < 1.07 * n_lin                        # 0.5625 - 1.0625 bytes a weight
    bytes_a = sum(p.numel() * 2 for n, p in a.named_parameters() if n.startswith("blocks."))
    bytes_b = sum(p.numel() * 2 for n, p in b.named_parameters() if n.startswith("blocks.")) + b._fp8_bytes
    print(f"[gguf resident] block bytes: bf16 {bytes_a}, resident {bytes_b} ({bytes_b / bytes_a:.3f})")
    assert bytes_b < 0.56 * bytes_a
    x, txt, t = _wan_inputs()

    def fwd(m):
        return _wan_fwd(m, x, txt, t)
    plain = fwd(b)
    assert torch.isfinite(plain).all() and float(plain.std()) > 0
    assert torch.equal(plain, fwd(a)) and torch.equal(plain, fwd(b))
    base_sd = {k: v.float().cpu() for k, v in a.state_dict().items()}
    with pytest.raises(lib.ApexMIError, match="keep_quantized"):
        b.state_dict()
    with pytest.raises(NotImplementedError):
        weights.load_checkpoint_into(FluxTransformer2DModel(**FLUX_CFG, device=DEV), [pg], keep_quantized=True)

    r, spec, d, f = 4, {}, 256, 512
    for i in range(2):
        for at, n in (("self_attn", "q"), ("self_attn", "o"), ("cross_attn", "q"), ("cross_attn", "k"), ("cross_attn", "v")):
            m = f"diffusion_model.blocks.{i}.{at}.{n}"
            spec.update({m + ".lora_down.weight": (r, d), m + ".lora_up.weight": (d, r), m + ".alpha": ()})
        spec.update({f"diffusion_model.blocks.{i}.ffn.0.lora_down.weight": (r, d), f"diffusion_model.blocks.{i}.ffn.0.lora_up.weight": (f, r),
                     f"diffusion_model.blocks.{i}.ffn.2.lora_down.weight": (r, f), f"diffusion_model.blocks.{i}.ffn.2.lora_up.weight": (d, r),
                     f"diffusion_model.blocks.{i}.cross_attn.k.diff_b": (d,)})
    raw = {k: (v * 0.3 if v.dim() == 2 else v) for k, v in spec_tensors(spec, 3100).items()}
    a.load_lora_adapter({k: v.clone() for k, v in raw.items()}, adapter_name="lx")
    b.load_lora_adapter({k: v.clone() for k, v in raw.items()}, adapter_name="lx")
    assert b._lora_pad == 64 and b._fp8_bytes > 0
    rec = b.blocks[0]._wkv2                                   # fused k | v record: two adapters, block-diagonal up factors
    assert isinstance(rec, ops.GgufWeight) and rec.lora_A.shape == (64, d) and rec.lora_B.shape == (2 * d, 64)
    assert float(rec.lora_B[:d, r:].abs().max()) == 0 and float(rec.lora_B[d:, :r].abs().max()) == 0
    assert float(rec.lora_A[2 * r:].abs().max()) == 0 and b.blocks[0]._wqkv.lora_A is not None
    mods = lora.split_modules(lora.convert_lora_state_dict(raw, "wan.base", list(base_sd)))
    assert len(mods) == 14 and "blocks.1.ffn.net.2" in mods

    def oracle(scale):
        orc = OWan.WanTransformer3DModel(**cfg).eval()
        sd = dict(base_sd)
        for m, dd in mods.items():
            sd[m + ".weight"] = OLR.merged_weight(sd[m + ".weight"], [(dd["A"].float(), dd["B"].float(), scale)])
        orc.load_state_dict(sd, strict=True)
        with torch.no_grad():
            return orc(x.float(), t, txt.float(), policy=OL.BF16_STORAGE), orc(x.float(), t, txt.float())
    rel = lambda u, v: float((u - v).norm() / v.norm())          # noqa: E731
    for scale in (1.0, 0.5):
        if scale != 1.0:
            a.set_adapters("lx", scale)
            b.set_adapters("lx", scale)
        ref16, ref32 = oracle(scale)
        got_b, got_a = fwd(b), fwd(a)
        e_like, e_true, e_emul = rel(got_b, ref16), rel(got_b, ref32), rel(ref16, ref32)
        print(f"[gguf + run-time LoRA, scale {scale}] vs the bf16-storage oracle {e_like:.2e}, vs fp32 {e_true:.2e} (emulation "
              f"{e_emul:.2e}); vs the dequantise-at-load model with MERGED weights {rel(got_b, got_a):.2e}; LoRA changed the output "
              f"by {rel(got_b, plain):.2e}")
        assert rel(got_b, plain) > 2e-2, "the adapter must matter for this test to mean anything"
        assert e_like < 6e-3 and e_true < 2 * e_emul + 2e-3 and rel(got_b, got_a) < 6e-3
        assert torch.equal(fwd(b), got_b), "deterministic"
    b.disable_lora()
    assert b._lora_pad == 0 and b.blocks[0]._wkv2.lora_A is None
    assert torch.equal(fwd(b), plain), "without adapters the resident forward is the plain one again, bit for bit"
    b.enable_lora()
    b.delete_adapters("lx")
    assert torch.equal(fwd(b), plain) and b._lora_pad == 0
