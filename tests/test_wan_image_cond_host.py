"""Wan-2.1 I2V / FLF2V image conditioning, host side (no GPU): the image-conditioned transformer config and its diffusers
state-dict keys, the CLIP vision tower's keys, the CLIPImageProcessor-equivalent preprocessing, and the engine's FLF2V mask and
choice between the CLIP image-embeds branch and the Wan-2.2 A14B branch on stand-in modules."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd.wan import WanTransformer3DModel

BASE = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=36, out_channels=16,
            text_dim=64, freq_dim=256, ffn_dim=512, num_layers=2, cross_attn_norm=True, eps=1e-6)


def _image_keys(n_layers, pos_embed):
    ie = "condition_embedder.image_embedder."
    keys = {ie + f"{m}.{p}" for m in ("norm1", "ff.net.0.proj", "ff.net.2", "norm2") for p in ("weight", "bias")}
    if pos_embed:
        keys.add(ie + "pos_embed")
    for i in range(n_layers):
        a = f"blocks.{i}.attn2."
        keys |= {a + f"{m}.{p}" for m in ("add_k_proj", "add_v_proj") for p in ("weight", "bias")}
        keys.add(a + "norm_added_k.weight")
    return keys


@pytest.mark.parametrize("pos_len", [None, 514])
def test_image_config_builds_on_meta_with_diffusers_keys(pos_len):
    plain = WanTransformer3DModel(**BASE, device="meta")
    m = WanTransformer3DModel(**BASE, image_dim=128, added_kv_proj_dim=256, pos_embed_seq_len=pos_len, device="meta")
    sd, sd0 = m.state_dict(), plain.state_dict()
    assert set(sd) - set(sd0) == _image_keys(2, pos_len is not None)
    assert set(sd0) <= set(sd)
    ie = "condition_embedder.image_embedder."
    assert tuple(sd[ie + "ff.net.0.proj.weight"].shape) == (128, 128)
    assert tuple(sd[ie + "ff.net.2.weight"].shape) == (256, 128)
    assert tuple(sd[ie + "norm1.weight"].shape) == (128,) and tuple(sd[ie + "norm2.bias"].shape) == (256,)
    assert tuple(sd["blocks.1.attn2.add_k_proj.weight"].shape) == (256, 256)
    assert tuple(sd["blocks.0.attn2.norm_added_k.weight"].shape) == (256,)
    if pos_len:
        assert tuple(sd[ie + "pos_embed"].shape) == (1, 514, 128)
    assert m.config.image_dim == 128 and m.config.added_kv_proj_dim == 256 and m.config.pos_embed_seq_len == pos_len


def test_image_config_guards():
    with pytest.raises(NotImplementedError):
        WanTransformer3DModel(**BASE, image_dim=128, added_kv_proj_dim=256, ip_adapter=True, device="meta")
    with pytest.raises(NotImplementedError):
        WanTransformer3DModel(**BASE, use_enhance=True, device="meta")
    with pytest.raises(NotImplementedError):
        WanTransformer3DModel(**BASE, image_dim=128, device="meta")                   # image tokens nothing reads
    with pytest.raises(ValueError):
        WanTransformer3DModel(**BASE, added_kv_proj_dim=256, device="meta")          # no image embedder to feed it
    with pytest.raises(ValueError):
        WanTransformer3DModel(**BASE, image_dim=128, added_kv_proj_dim=128, device="meta")
    with pytest.raises(ValueError):
        WanTransformer3DModel(**BASE, image_dim=96, added_kv_proj_dim=256, device="meta")           # GEMM K: multiples of 64


def test_image_kv_weights_stay_bf16_under_keep_fp8():
    key = WanTransformer3DModel._fp8_resident_key
    assert key("blocks.3.attn2.to_k.weight") and key("blocks.3.ffn.net.0.proj.weight")
    assert not key("blocks.3.attn2.add_k_proj.weight") and not key("blocks.3.attn2.add_v_proj.weight")
    assert not key("blocks.3.attn2.norm_added_k.weight")


def test_clip_vision_keys_match_transformers():
    transformers = pytest.importorskip("transformers")
    from apex_studio_amd.clip_vision import CLIPVisionModel
    cfg = transformers.CLIPVisionConfig(hidden_size=320, intermediate_size=640, num_hidden_layers=2, num_attention_heads=4,
                                        image_size=224, patch_size=14, hidden_act="gelu")
    m = CLIPVisionModel._from_config(cfg, device="meta")
    ref = transformers.CLIPVisionModel(cfg).state_dict()
    ours = m.state_dict()
    want = {k if k.startswith("vision_model.") else "vision_model." + k: v for k, v in ref.items()
            if not k.endswith("position_ids")}
    assert set(ours) == set(want)
    for k, v in want.items():
        assert tuple(ours[k].shape) == tuple(v.shape), k
    assert tuple(ours["vision_model.embeddings.position_embedding.weight"].shape) == (257, 320)


def test_clip_preprocess_equals_transformers_processor():
    transformers = pytest.importorskip("transformers")
    from PIL import Image
    from apex_studio_amd.clip_vision import clip_preprocess
    proc_cls = getattr(transformers, "CLIPImageProcessorPil", None) or transformers.CLIPImageProcessor
    proc = proc_cls()
    rng = np.random.default_rng(3)
    sizes = [(300, 500), (480, 832), (231, 224), (1000, 257), (97, 400), (720, 1280)]
    imgs = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
    for im in imgs:
        ref = proc(images=im, return_tensors="pt")["pixel_values"]
        assert torch.equal(clip_preprocess(im), ref)
    assert torch.equal(clip_preprocess(imgs[:2]), proc(images=imgs[:2], return_tensors="pt")["pixel_values"])


# ---- engine on stand-in modules --------------------------------------------------------------------------------------------

class _StubTransformer:
    def __init__(self, image_dim=None):
        self.config = SimpleNamespace(in_channels=36, out_channels=16, image_dim=image_dim)
        self.device, self.dtype = torch.device("cpu"), torch.float32
        self.calls = []

    def __call__(self, hidden_states, timestep, encoder_hidden_states, return_dict=False, **kw):
        self.calls.append(dict(kw, text=encoder_hidden_states))
        return (torch.zeros(hidden_states.shape[0], 16, *hidden_states.shape[2:]),)


class _StubVae:
    dtype, device = torch.float32, torch.device("cpu")

    def __init__(self):
        self.videos = []

    def enable_tiling(self, *a, **k):
        pass

    def encode(self, video, return_dict=False):
        self.videos.append(video.clone())
        B, _, F, H, W = video.shape
        return (SimpleNamespace(mode=lambda: torch.ones(B, 16, (F - 1) // 4 + 1, H // 8, W // 8)),)

    def normalize_latents(self, lat):
        return lat


class _StubClip:
    device = torch.device("cpu")

    def __init__(self):
        self.seen = []

    def __call__(self, pixel_values, output_hidden_states=False):
        self.seen.append(pixel_values.clone())
        n = pixel_values.shape[0]
        hs = tuple(torch.full((n, 257, 8), float(i)) + torch.arange(n).view(n, 1, 1) * 10 for i in range(3))
        return SimpleNamespace(hidden_states=hs)


def _engine(image_dim, image_encoder=None, boundary_ratio=None):
    from apex_studio_amd.engine_wan import WanI2VEngine
    tr = _StubTransformer(image_dim)
    return WanI2VEngine(tr, vae=_StubVae(), boundary_ratio=boundary_ratio, image_encoder=image_encoder), tr


def _run(eng, **kw):
    pe, ne = torch.randn(1, 12, 64), torch.randn(1, 12, 64)
    img = torch.rand(1, 3, 32, 48) * 2 - 1
    return eng.run(image=img, prompt_embeds=pe, negative_prompt_embeds=ne, height=32, width=48, duration=9,
                   num_inference_steps=2, guidance_scale=5.0, seed=0, return_latents=True, **kw)


def test_flf2v_mask_first_and_last_pixel_frames():
    eng, _ = _engine(None)
    F_, f = 9, eng.vae_scale_factor_temporal
    m = eng.first_frame_mask(1, F_, 2, 3, last_frame=True)
    assert tuple(m.shape) == (1, f, (F_ - 1) // f + 1, 2, 3)
    # pixel frames: 0 repeated x4 (latent frame 0), then 1..8 -> latent frames 1, 2; frame 8 (the last) is 1
    assert torch.all(m[:, :, 0] == 1) and torch.all(m[:, :, 1] == 0)
    assert torch.equal(m[0, :, 2, 0, 0], torch.tensor([0.0, 0.0, 0.0, 1.0]))
    m1 = eng.first_frame_mask(1, F_, 2, 3)
    assert torch.all(m1[:, :, 0] == 1) and torch.all(m1[:, :, 1:] == 0)


def test_a14b_branch_passes_no_image_tokens():
    eng, tr = _engine(None, boundary_ratio=0.875)
    _run(eng)
    assert len(tr.calls) == 4 and all("encoder_hidden_states_image" not in c for c in tr.calls)


def test_image_embeds_branch_conditions_every_call():
    clip = _StubClip()
    eng, tr = _engine(8, clip)
    lat = _run(eng)
    assert tuple(lat.shape) == (1, 16, 3, 4, 6)
    assert len(clip.seen) == 1 and tuple(clip.seen[0].shape) == (1, 3, 224, 224)       # once per run
    assert len(tr.calls) == 4                                                            # 2 steps x (cond, uncond)
    for c in tr.calls:
        img = c["encoder_hidden_states_image"]
        assert tuple(img.shape) == (1, 257, 8) and torch.all(img == 1.0)                 # hidden_states[-2]


def test_flf2v_encodes_both_images_and_conditions_the_last_frame():
    clip = _StubClip()
    eng, tr = _engine(8, clip)
    _run(eng, last_image=torch.rand(1, 3, 32, 48) * 2 - 1)
    assert tuple(clip.seen[0].shape) == (2, 3, 224, 224)
    img = tr.calls[0]["encoder_hidden_states_image"]
    assert tuple(img.shape) == (1, 514, 8)
    assert torch.all(img[:, :257] == 1.0) and torch.all(img[:, 257:] == 11.0)            # [image, last_image] order
    video = eng.vae.videos[0]
    assert tuple(video.shape) == (1, 3, 9, 32, 48)
    assert video[:, :, 1:-1].abs().max() == 0 and video[:, :, -1].abs().max() > 0
    with pytest.raises(ValueError):
        _run(eng, last_image=torch.rand(1, 3, 48, 48) * 2 - 1)                           # pixels of another size


def test_precomputed_image_embeds_and_missing_encoder():
    eng, tr = _engine(8)
    with pytest.raises(ValueError, match="image_encoder"):
        _run(eng)
    emb = torch.randn(1, 257, 8)
    _run(eng, image_embeds=emb)
    assert all(torch.equal(c["encoder_hidden_states_image"], emb) for c in tr.calls)
