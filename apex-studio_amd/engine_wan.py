"""Wan text-to-video (2.2 A14B) and image-to-video (2.2 A14B; 2.1 14B I2V / FLF2V with CLIP image conditioning) engine surfaces
on the HIP transformer + HIP VAE (+ the HIP CLIP vision tower for Wan-2.1).

Mirrors reference engine/wan/t2v.py:12-247 (`run`) and engine/wan/shared/__init__.py:478-608
(`moe_denoise`), :464-476 (`_select_dual_noise_guidance_scale`), :309-462 (expert selection by
`t >= boundary_timestep`): same argument names, the `(progress, message)` callback protocol and the
`render_on_step_callback(frames)` preview hook.  Both 14B experts stay resident (57 GB of 288 GB), so
the reference's load/offload choreography between experts has no counterpart.  Text encoding (UMT5) is
outside the hot path: prompt embeddings are inputs.  The sampler loop stays in Python.
"""
from __future__ import annotations

from typing import List, Optional, Union

import torch

from .lora import EngineLoraMixin

from .engine_flux import _emit, compute_dtype, initial_noise
from .schedulers import UniPCMultistepScheduler


class WanT2VEngine(EngineLoraMixin):
    def __init__(self, high_noise_transformer, low_noise_transformer=None, vae=None,
                 scheduler: Optional[UniPCMultistepScheduler] = None, boundary_ratio: Optional[float] = 0.875,
                 vae_scale_factor_temporal: int = 4, vae_scale_factor_spatial: int = 8, text_encoder=None,
                 residual_dtype: Optional[torch.dtype] = None, attention_window=None, fp8_compute: bool = False,
                 attention_band: Optional[int] = None, fp8_lora: bool = False, fp8_fused_quant: bool = False,
                 fp8_mx_ffn: bool = False, fp4_compute: bool = False, fp4_linears=None,
                 fp6_compute: bool = False, fp6_linears=None, fp4_fused_quant: bool = False, fp4_mx_ffn: bool = False):
        from .prompt import TextEncoder
        self.text_encoder = text_encoder if text_encoder is None or isinstance(text_encoder, TextEncoder) \
            else TextEncoder(text_encoder)                      # UMT5-XXL (manifest wan-2.2-a14b-text-to-video yml)
        self.high_noise_transformer = high_noise_transformer
        self.low_noise_transformer = low_noise_transformer or high_noise_transformer
        # float32: both experts keep their residual stream in float (`set_residual_dtype`); None = bf16
        self.residual_dtype = residual_dtype
        if residual_dtype is not None:
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                tr.set_residual_dtype(residual_dtype)
        # (frames, rows, cols) in token units: both experts' self-attention stays inside that window (`set_attention_window`,
        # an opt-in approximation); None = dense
        self.attention_window = None if attention_window is None else tuple(attention_window)
        if attention_window is not None:
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                tr.set_attention_window(self.attention_window)
        # frames: both experts' self-attention stays inside per-block key bands of that temporal radius (`set_attention_band`,
        # an opt-in approximation, exclusive with the window); None = dense
        self.attention_band = attention_band
        if attention_band is not None:
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                tr.set_attention_band(attention_band)
        # resident fp8 block weights multiply as fp8 (`set_fp8_compute`, DESIGN.md §3.6: an opt-in approximation; needs a
        # keep_fp8=True load of both experts); False = dequantise per call and multiply in bf16
        # fp8_lora: records carrying run-time LoRA factors stay on the fp8 GEMM too (its bf16 adapter tail) instead of falling
        # back to the bf16 path; needs fp8_compute
        # fp8_fused_quant: the norms in front of the q|k|v, cross-attention query and FFN-up Linears write the e4m3 codes
        # themselves (`set_fp8_compute(fused_quant=True)`: fewer launches and bytes, the same numbers); needs fp8_compute
        # fp8_mx_ffn: the FFN hidden state stays in MX fp8 between the two FFN Linears (`set_fp8_compute(mx_ffn=True)`: one
        # quantise launch and the bf16 round trip fewer per block; block scales, so the numbers change); needs fp8_compute
        self.fp8_compute, self.fp8_lora, self.fp8_fused_quant = bool(fp8_compute), bool(fp8_lora), bool(fp8_fused_quant)
        self.fp8_mx_ffn = bool(fp8_mx_ffn)
        if self.fp8_mx_ffn and not self.fp8_compute:
            raise ValueError("fp8_mx_ffn=True needs fp8_compute=True: the MX hidden state belongs to the FP8 GEMMs")
        if self.fp8_lora and not self.fp8_compute:
            raise ValueError("fp8_lora=True needs fp8_compute=True: it keeps adapter-carrying Linears on the FP8 compute path")
        if self.fp8_fused_quant and not self.fp8_compute:
            raise ValueError("fp8_fused_quant=True needs fp8_compute=True: the fused norm quantises for the FP8 GEMM")
        if self.fp8_compute:
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                if self.fp8_mx_ffn:
                    tr.set_fp8_compute(True, lora=self.fp8_lora, fused_quant=self.fp8_fused_quant, mx_ffn=True)
                elif self.fp8_fused_quant:
                    tr.set_fp8_compute(True, lora=self.fp8_lora, fused_quant=True)
                elif self.fp8_lora:
                    tr.set_fp8_compute(True, lora=True)
                else:
                    tr.set_fp8_compute(True)
        # the block Linears of bf16 experts multiply as MXFP4 (`set_fp4_compute`, DESIGN.md §3.6: an opt-in approximation on MXFP4
        # copies beside the bf16 weights; not for resident-fp8 experts, so never together with fp8_compute); fp4_linears: a subset
        # of the seven block Linears, None = all
        self.fp4_compute = bool(fp4_compute)
        self.fp4_linears = None if fp4_linears is None else tuple(fp4_linears)
        if self.fp4_linears is not None and not self.fp4_compute:
            raise ValueError("fp4_linears needs fp4_compute=True: it names the Linears of the MXFP4 compute mode")
        # fp4_fused_quant / fp4_mx_ffn: the norms in front of the fp4 q|k|v, cross-attention query and FFN-up Linears write the MXFP4
        # codes themselves / the FFN hidden state stays MXFP4 between the two FFN Linears (`set_fp4_compute(fused_quant=, mx_ffn=)`:
        # fewer launches and bytes, the same numbers); both need fp4_compute
        self.fp4_fused_quant, self.fp4_mx_ffn = bool(fp4_fused_quant), bool(fp4_mx_ffn)
        if self.fp4_fused_quant and not self.fp4_compute:
            raise ValueError("fp4_fused_quant=True needs fp4_compute=True: the fused norm quantises for the MXFP4 GEMM")
        if self.fp4_mx_ffn and not self.fp4_compute:
            raise ValueError("fp4_mx_ffn=True needs fp4_compute=True: the MXFP4 hidden state belongs to the MXFP4 GEMMs")
        if self.fp4_compute:
            more = {k: True for k, v in (("fused_quant", self.fp4_fused_quant), ("mx_ffn", self.fp4_mx_ffn)) if v}
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                tr.set_fp4_compute(True, linears=self.fp4_linears, **more)
        # the same with MXFP6 (`set_fp6_compute`: the error class of fp8 on the fp4 matrix rate); both may be on with disjoint
        # `*_linears`, e.g. fp6 for the attention projections and fp4 for the FFN pair — the model refuses a name selected by both
        self.fp6_compute = bool(fp6_compute)
        self.fp6_linears = None if fp6_linears is None else tuple(fp6_linears)
        if self.fp6_linears is not None and not self.fp6_compute:
            raise ValueError("fp6_linears needs fp6_compute=True: it names the Linears of the MXFP6 compute mode")
        if self.fp6_compute:
            for tr in {id(t): t for t in (self.high_noise_transformer, self.low_noise_transformer)}.values():
                tr.set_fp6_compute(True, linears=self.fp6_linears)
        self.vae = vae
        self.scheduler = scheduler or UniPCMultistepScheduler(shift=3.0)
        self.boundary_ratio = boundary_ratio
        self.vae_scale_factor_temporal = vae_scale_factor_temporal
        self.vae_scale_factor_spatial = vae_scale_factor_spatial
        # the latent the scheduler steps (the VAE's z_dim): `out_channels` — an image-to-video expert takes 36 input channels
        self.num_channels_latents = getattr(high_noise_transformer.config, "out_channels", None) or high_noise_transformer.config.in_channels

    @property
    def device(self):
        return self.high_noise_transformer.device

    @staticmethod
    def _select_dual_noise_guidance_scale(t, boundary_timestep, guidance_scale) -> float:
        high = boundary_timestep is not None and bool(t >= boundary_timestep)
        if isinstance(guidance_scale, (list, tuple)):
            return float(guidance_scale[0] if high else guidance_scale[1])
        return float(guidance_scale)

    def _select_dual_noise_transformer(self, t, boundary_timestep):
        if boundary_timestep is None or bool(t >= boundary_timestep):
            return self.high_noise_transformer
        return self.low_noise_transformer

    def vae_decode(self, latents: torch.Tensor) -> torch.Tensor:
        """reference engine/base_engine.py:2030-2059: denormalize -> enable tiling -> decode."""
        z = self.vae.denormalize_latents(latents.to(torch.float32)).to(compute_dtype(self.vae))
        self.vae.enable_tiling()
        return self.vae.decode(z, return_dict=False)[0]

    def moe_denoise(self, latents, timesteps, prompt_embeds, negative_prompt_embeds=None,
                    guidance_scale: Union[float, List[float]] = 5.0, boundary_timestep=None,
                    use_cfg_guidance: bool = True, transformer_dtype=None, render_on_step: bool = False,
                    render_on_step_callback=None, render_on_step_interval: int = 3,
                    denoise_progress_callback=None, easy_cache_thresh: float = 0.0, easy_cache_ret_steps: int = 10,
                    latent_condition: Optional[torch.Tensor] = None, image_embeds: Optional[torch.Tensor] = None):
        """`easy_cache_thresh` > 0: EasyCache step skipping (R/src/engine/wan/shared/__init__.py:372-381, :435-444, :502-504).  The
        reference enables it on the high-noise expert WITH a reset of its (module-global) state and on the low-noise expert WITHOUT
        one, so the call count, the rate K, the accumulated error and the caches run on across the expert switch: no second
        warm-up of `ret_steps` pairs, and the last pair of the clip (`cnt >= 2n - 2`) is always computed.  Both experts are
        resident here: the first expert of the loop gets a fresh state, every later one continues it
        (`share_easy_cache_state`), and the cache is switched off when the loop ends.  `image_embeds` (Wan-2.1 I2V / FLF2V: CLIP
        image tokens [B, 257 n, image_dim]) goes to every transformer call, conditional and unconditional, as
        `encoder_hidden_states_image`; without it the calls are exactly those of the text- / latent-conditioned path."""
        _emit(denoise_progress_callback, 0.0, "Starting denoise")
        try:
            return self._moe_loop(latents, timesteps, prompt_embeds, negative_prompt_embeds, guidance_scale, boundary_timestep,
                                  use_cfg_guidance, transformer_dtype, render_on_step, render_on_step_callback, render_on_step_interval,
                                  denoise_progress_callback, easy_cache_thresh, easy_cache_ret_steps, latent_condition,
                                  image_embeds)
        finally:
            if easy_cache_thresh > 0.0:
                for tr in {id(self.high_noise_transformer): self.high_noise_transformer,
                           id(self.low_noise_transformer): self.low_noise_transformer}.values():
                    if hasattr(tr, "disable_easy_cache"):
                        tr.disable_easy_cache()

    def _moe_loop(self, latents, timesteps, prompt_embeds, negative_prompt_embeds, guidance_scale, boundary_timestep, use_cfg_guidance,
                  transformer_dtype, render_on_step, render_on_step_callback, render_on_step_interval, denoise_progress_callback,
                  easy_cache_thresh, easy_cache_ret_steps, latent_condition=None, image_embeds=None):
        n = len(timesteps)
        img_kw = {} if image_embeds is None else {"encoder_hidden_states_image": image_embeds}
        current = None
        for i, t in enumerate(timesteps):
            timestep = t.expand(latents.shape[0])
            transformer = self._select_dual_noise_transformer(t, boundary_timestep)
            if easy_cache_thresh > 0.0 and transformer is not current and hasattr(transformer, "enable_easy_cache"):
                first = current is None
                if not first and hasattr(transformer, "share_easy_cache_state"):
                    transformer.share_easy_cache_state(current)
                transformer.enable_easy_cache(n, easy_cache_thresh, easy_cache_ret_steps, should_reset_global_cache=first)
            current = transformer
            dt_x = transformer_dtype or compute_dtype(transformer)
            # image-to-video: [noisy latents | first-frame mask | encoded condition video] along channels (moe_denoise,
            # R/src/engine/wan/shared/__init__.py:515-520); the scheduler steps the 16 latent channels only
            x = latents.to(dt_x) if latent_condition is None else torch.cat([latents, latent_condition.to(latents.dtype)], dim=1).to(dt_x)
            scale = self._select_dual_noise_guidance_scale(t, boundary_timestep, guidance_scale)
            noise_pred = transformer(hidden_states=x, timestep=timestep, encoder_hidden_states=prompt_embeds,
                                     return_dict=False, **img_kw)[0]
            if use_cfg_guidance and negative_prompt_embeds is not None:
                uncond = transformer(hidden_states=x, timestep=timestep,
                                     encoder_hidden_states=negative_prompt_embeds, return_dict=False, **img_kw)[0]
                noise_pred = uncond + scale * (noise_pred - uncond)
            latents = self.scheduler.step(noise_pred.to(torch.float32), t, latents, return_dict=False)[0]
            if (render_on_step and render_on_step_callback and self.vae is not None
                    and ((i + 1) % render_on_step_interval == 0 or i == 0) and i != n - 1):
                try:
                    render_on_step_callback(self.vae_decode(latents))
                except Exception:
                    pass
            _emit(denoise_progress_callback, float(i + 1) / n, f"Denoising step {i + 1}/{n}")
        return latents

    def encode_prompt(self, prompt=None, prompt_ids=None, num_videos: int = 1, text_encoder_kwargs=None):
        """`self.text_encoder.encode(prompt, num_videos_per_prompt=..., **text_encoder_kwargs)` of R/src/engine/wan/t2v.py:77-95
        with the manifest's `use_attention_mask: true`: 512 tokens, masked encoder, embeddings past the prompt's length zeroed."""
        from .prompt import split_ids
        if self.text_encoder is None:
            raise RuntimeError("WanT2VEngine: prompts need a text_encoder (UMT5); or pass prompt_embeds")
        kw = {"use_attention_mask": True, **(text_encoder_kwargs or {})}
        a = dict(text=prompt) if prompt_ids is None else dict(zip(("input_ids", "attention_mask"), split_ids(prompt_ids)))
        return self.text_encoder.encode(num_videos_per_prompt=num_videos, **a, **kw)

    @torch.no_grad()
    def run(self, prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
            height: int = 720, width: int = 1280, duration: int = 81, num_inference_steps: int = 30,
            guidance_scale: Union[float, List[float]] = (4.0, 3.0), seed: Optional[int] = None,
            generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None,
            return_latents: bool = False, progress_callback=None, render_on_step: bool = False,
            render_on_step_callback=None, render_on_step_interval: int = 3, output_type: Optional[str] = None,
            prompt=None, negative_prompt=None, prompt_ids=None, negative_prompt_ids=None, num_videos: int = 1,
            text_encoder_kwargs=None, easy_cache_thresh: float = 0.0, easy_cache_ret_steps: int = 10, **_ignored):
        """`engine.run(prompt=..., negative_prompt=..., ...)` (R/src/engine/wan/t2v.py:12-247): prompts as strings (text
        encoder with a tokenizer) or token ids `(input_ids, attention_mask)`, or pre-computed embeddings."""
        dev = self.device
        if prompt_embeds is None:
            _emit(progress_callback, 0.05, "Encoding prompt")
            prompt_embeds = self.encode_prompt(prompt, prompt_ids, num_videos, text_encoder_kwargs)
            if negative_prompt is not None or negative_prompt_ids is not None:
                negative_prompt_embeds = self.encode_prompt(negative_prompt, negative_prompt_ids, num_videos, text_encoder_kwargs)
        B = prompt_embeds.shape[0]
        num_latent_frames = (duration - 1) // self.vae_scale_factor_temporal + 1
        shape = (B, self.num_channels_latents, num_latent_frames, height // self.vae_scale_factor_spatial,
                 width // self.vae_scale_factor_spatial)
        if latents is None:
            latents = initial_noise(shape, dev, torch.float32, seed, generator)
        else:
            latents = latents.to(device=dev, dtype=torch.float32)
        _emit(progress_callback, 0.2, "Prepared latents")
        timesteps = self.scheduler.set_timesteps(num_inference_steps, device=dev)
        boundary = None
        if self.boundary_ratio is not None:
            boundary = self.boundary_ratio * self.scheduler.config["num_train_timesteps"]
        cfg = negative_prompt_embeds is not None
        dt = compute_dtype(self.high_noise_transformer)
        pe = prompt_embeds.to(dev, dt)
        ne = negative_prompt_embeds.to(dev, dt) if cfg else None

        def mapped(p, msg):
            _emit(progress_callback, 0.5 + 0.4 * p, msg)

        latents = self.moe_denoise(latents=latents, timesteps=timesteps, prompt_embeds=pe,
                                   negative_prompt_embeds=ne, guidance_scale=list(guidance_scale)
                                   if isinstance(guidance_scale, (list, tuple)) else guidance_scale,
                                   boundary_timestep=boundary, use_cfg_guidance=cfg,
                                   render_on_step=render_on_step, render_on_step_callback=render_on_step_callback,
                                   render_on_step_interval=render_on_step_interval,
                                   denoise_progress_callback=mapped, easy_cache_thresh=easy_cache_thresh,
                                   easy_cache_ret_steps=easy_cache_ret_steps)
        if return_latents or self.vae is None:
            _emit(progress_callback, 1.0, "Returning latents")
            return latents
        _emit(progress_callback, 0.92, "Decoding video")
        video = self.vae_decode(latents)
        _emit(progress_callback, 1.0, "Completed text-to-video pipeline")
        if output_type is not None:      # t2v.py: `self._tensor_to_frames(video)` — uint8 frames made on the GPU
            from .postprocess import tensor_to_frames
            return tensor_to_frames(video, output_type)
        return video


class WanI2VEngine(WanT2VEngine):
    """Wan image-to-video (R/src/engine/wan/i2v.py:13-314).  Two model families:

    * Wan-2.2 A14B (the `boundary_ratio` branch: two experts with `in_channels` = 36, no `image_dim`): the first frame conditions
      the clip through the latent path only (the reference's `moe_denoise` drops `encoder_hidden_states_image`,
      shared/__init__.py:494-495).
    * Wan-2.1 14B I2V / FLF2V (one transformer, `boundary_ratio=None`; its config has `image_dim`): the latent path as below AND
      CLIP image embeddings (diffusers WanImageToVideoPipeline.encode_image: `image_encoder(...).hidden_states[-2]` of the
      preprocessed ORIGINAL image, or of [image, last_image] for FLF2V), computed once per run (or passed as `image_embeds=`),
      repeated over the batch and given to every transformer call as `encoder_hidden_states_image`.  `image_encoder`: a
      `clip_vision.CLIPVisionModel` (or anything with its call surface); missing when the model needs one -> ValueError.

    The latent path:

        video_condition = [image | zeros x (num_frames - 1)]                           (i2v.py:186-198)
        latent_condition = normalize_latents(vae.encode(video_condition).mode())       (BaseEngine.vae_encode, base_engine.py:2062-2165)
        mask = 1 on the first frame's four sub-frames, 0 after -> [B, 4, T_lat, h, w]  (i2v.py:220-249)
        every step:  hidden_states = cat([latents, mask, latent_condition], dim=1)     (36 channels)

    FLF2V (`last_image`): video_condition = [image | zeros x (num_frames - 2) | last_image] and the mask is 1 on the first AND the
    last pixel frame; `last_image` is resized to the first image's size.

    `image`: a PIL image / HWC uint8 array (resized to the aspect-preserving size of area height x width on the reference's
    rule, `_aspect_ratio_resize`, base_engine.py:501-514, then x / 127.5 - 1) or pixels [B|1, 3, H, W] in [-1, 1] (used as they
    are: H, W multiples of 16).  The TI2V-5B form (`expand_timesteps`: per-token timesteps) is a different model and raises."""

    def __init__(self, high_noise_transformer, low_noise_transformer=None, vae=None,
                 scheduler: Optional[UniPCMultistepScheduler] = None, boundary_ratio: Optional[float] = 0.875,
                 vae_scale_factor_temporal: int = 4, vae_scale_factor_spatial: int = 8, text_encoder=None, image_encoder=None,
                 residual_dtype: Optional[torch.dtype] = None, attention_window=None, fp8_compute: bool = False,
                 attention_band: Optional[int] = None, fp8_lora: bool = False, fp8_fused_quant: bool = False,
                 fp8_mx_ffn: bool = False, fp4_compute: bool = False, fp4_linears=None,
                 fp6_compute: bool = False, fp6_linears=None, fp4_fused_quant: bool = False, fp4_mx_ffn: bool = False):
        super().__init__(high_noise_transformer, low_noise_transformer, vae, scheduler, boundary_ratio,
                         vae_scale_factor_temporal, vae_scale_factor_spatial, text_encoder, residual_dtype=residual_dtype,
                         attention_window=attention_window, fp8_compute=fp8_compute,
                         attention_band=attention_band, fp8_lora=fp8_lora, fp8_fused_quant=fp8_fused_quant,
                         fp8_mx_ffn=fp8_mx_ffn, fp4_compute=fp4_compute, fp4_linears=fp4_linears,
                         fp6_compute=fp6_compute, fp6_linears=fp6_linears, fp4_fused_quant=fp4_fused_quant, fp4_mx_ffn=fp4_mx_ffn)
        self.image_encoder = image_encoder

    @property
    def uses_image_embeds(self) -> bool:
        """True for a transformer whose config has `image_dim` (Wan-2.1 I2V / FLF2V): the CLIP branch."""
        return getattr(self.high_noise_transformer.config, "image_dim", None) is not None

    def encode_image(self, images, batch: int = 1) -> torch.Tensor:
        """CLIP image tokens of one image, or of [image, last_image] (FLF2V): `hidden_states[-2]` of the image encoder on the
        CLIPImageProcessor-preprocessed images -> [batch, 257 n, image_dim], repeated over the batch."""
        from .clip_vision import clip_preprocess
        if self.image_encoder is None:
            raise ValueError("wan i2v: this transformer conditions on CLIP image embeddings (its config has image_dim): pass "
                             "image_encoder= to the engine, or image_embeds= to run()")
        images = list(images) if isinstance(images, (list, tuple)) else [images]
        pil = [self._to_pil(im) for im in images]
        px = clip_preprocess(pil).to(self.image_encoder.device)
        h = self.image_encoder(pixel_values=px, output_hidden_states=True).hidden_states[-2]
        return h.reshape(1, -1, h.shape[-1]).repeat(batch, 1, 1)

    @staticmethod
    def _to_pil(image):
        """PIL image / HWC uint8 array / pixels [1|3, H, W] or [1, 3, H, W] in [-1, 1] -> RGB PIL image."""
        import numpy as np
        from PIL import Image
        if isinstance(image, Image.Image):
            return image.convert("RGB")
        if isinstance(image, torch.Tensor):
            x = image[0] if image.dim() == 4 else image
            x = ((x.detach().float().cpu().clamp(-1, 1) + 1.0) * 127.5).round().to(torch.uint8)
            return Image.fromarray(x.permute(1, 2, 0).numpy())
        return Image.fromarray(np.asarray(image)).convert("RGB")

    @staticmethod
    def aspect_ratio_size(h0: int, w0: int, max_area: int, mod_value: int = 16):
        """`_aspect_ratio_resize` (base_engine.py:501-514): the size of area <= max_area with the image's aspect ratio, floored to
        multiples of mod_value."""
        import numpy as np
        aspect = h0 / w0
        return (int(round(np.sqrt(max_area * aspect))) // mod_value * mod_value,
                int(round(np.sqrt(max_area / aspect))) // mod_value * mod_value)

    def preprocess_image(self, image, height: int, width: int, size=None):
        """-> (pixels [B, 3, H, W] float32 in [-1, 1] on the device, H, W).  `size` (H, W): resize to exactly that (FLF2V's
        last image takes the first image's size)."""
        if isinstance(image, torch.Tensor):
            x = image if image.dim() == 4 else image[None]
            if x.shape[1] != 3 or x.shape[-2] % 16 or x.shape[-1] % 16:
                raise ValueError(f"wan i2v: pixel tensors must be [B, 3, H, W] with H, W multiples of 16, got {tuple(image.shape)}")
            if size is not None and tuple(x.shape[-2:]) != tuple(size):
                raise ValueError(f"wan i2v: the last-frame pixels {tuple(x.shape[-2:])} must match the first image's {tuple(size)}")
            return x.to(self.device, torch.float32), int(x.shape[-2]), int(x.shape[-1])
        import numpy as np
        from PIL import Image
        img = image if isinstance(image, Image.Image) else Image.fromarray(np.asarray(image))
        img = img.convert("RGB")
        h, w = size if size is not None else self.aspect_ratio_size(img.height, img.width, height * width, 16)
        img = img.resize((w, h), Image.Resampling.LANCZOS)
        x = torch.from_numpy(np.asarray(img).astype(np.float32) / 255.0).permute(2, 0, 1)[None]      # VideoProcessor.preprocess:
        return (2.0 * x - 1.0).to(self.device), h, w                                                  # [0, 1] -> [-1, 1]

    def vae_encode(self, video: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
        """BaseEngine.vae_encode (base_engine.py:2139-2160): tiling on, `encode(...).mode()`, normalised in `dtype`."""
        self.vae.enable_tiling()
        lat = self.vae.encode(video.to(self.device, compute_dtype(self.vae)), return_dict=False)[0].mode()
        return self.vae.normalize_latents(lat.to(dtype))

    def first_frame_mask(self, batch: int, num_frames: int, latent_height: int, latent_width: int,
                         last_frame: bool = False) -> torch.Tensor:
        """i2v.py:220-249: ones on pixel frame 0 (and on the last pixel frame with `last_frame`, FLF2V), zeros between; frame 0
        repeated to the temporal factor so every latent frame owns `vae_scale_factor_temporal` mask channels -> [B, 4, T_lat, h, w]."""
        f = self.vae_scale_factor_temporal
        m = torch.ones(batch, 1, num_frames, latent_height, latent_width, device=self.device)
        m[:, :, 1:num_frames - 1 if last_frame else num_frames] = 0
        m = torch.cat([torch.repeat_interleave(m[:, :, 0:1], dim=2, repeats=f), m[:, :, 1:]], dim=2)
        return m.view(batch, -1, f, latent_height, latent_width).transpose(1, 2)

    def prepare_latent_condition(self, pixels: torch.Tensor, num_frames: int, batch: int,
                                 last_pixels: Optional[torch.Tensor] = None) -> torch.Tensor:
        B0, _, H, W = pixels.shape
        first = pixels[:, :, None]
        if last_pixels is None:
            video = torch.cat([first, first.new_zeros(B0, 3, num_frames - 1, H, W)], dim=2)
        else:       # FLF2V: [image | zeros x (F - 2) | last_image]
            last = last_pixels.expand(B0, -1, -1, -1)[:, :, None].to(first.dtype)
            video = torch.cat([first, first.new_zeros(B0, 3, num_frames - 2, H, W), last], dim=2)
        cond = self.vae_encode(video, dtype=torch.float32)
        if cond.shape[0] != batch:
            cond = cond.repeat(batch // cond.shape[0], 1, 1, 1, 1)
        mask = self.first_frame_mask(batch, num_frames, cond.shape[-2], cond.shape[-1],
                                     last_frame=last_pixels is not None).to(cond.dtype)
        return torch.cat([mask, cond], dim=1)

    @torch.no_grad()
    def run(self, image=None, prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
            height: int = 480, width: int = 832, duration: int = 81, num_inference_steps: int = 30,
            guidance_scale: Union[float, List[float], None] = None, high_noise_guidance_scale: Optional[float] = 1.0,
            low_noise_guidance_scale: Optional[float] = 1.0, seed: Optional[int] = None,
            generator: Optional[torch.Generator] = None, latents: Optional[torch.Tensor] = None, return_latents: bool = False,
            progress_callback=None, render_on_step: bool = False, render_on_step_callback=None, render_on_step_interval: int = 3,
            output_type: Optional[str] = None, prompt=None, negative_prompt=None, prompt_ids=None, negative_prompt_ids=None,
            num_videos: int = 1, text_encoder_kwargs=None, easy_cache_thresh: float = 0.0, easy_cache_ret_steps: int = 10,
            expand_timesteps: bool = False, ip_image=None, last_image=None, image_embeds: Optional[torch.Tensor] = None,
            **_ignored):
        if image is None:
            raise ValueError("wan i2v: `image` is required")
        if expand_timesteps or ip_image is not None:
            raise NotImplementedError("wan i2v: the TI2V-5B (`expand_timesteps`) and IP-image forms are other models; this engine "
                                      "serves the Wan-2.2 A14B and Wan-2.1 I2V / FLF2V image-to-video paths")
        if self.uses_image_embeds and image_embeds is None and self.image_encoder is None:
            raise ValueError("wan i2v: this transformer conditions on CLIP image embeddings (its config has image_dim): pass "
                             "image_encoder= to the engine, or image_embeds= to run()")
        if self.vae is None:
            raise RuntimeError("WanI2VEngine needs the VAE (the condition video is encoded with it)")
        if self.high_noise_transformer.config.in_channels != 36:
            raise ValueError(f"wan i2v: the experts must take 36 input channels (16 latent + 4 mask + 16 condition), got "
                             f"{self.high_noise_transformer.config.in_channels}")
        dev = self.device
        _emit(progress_callback, 0.0, "Starting image-to-video pipeline")
        if high_noise_guidance_scale is not None and low_noise_guidance_scale is not None and guidance_scale is None:
            guidance_scale = [high_noise_guidance_scale, low_noise_guidance_scale]        # i2v.py:46-53
        if prompt_embeds is None:
            _emit(progress_callback, 0.05, "Encoding prompt")
            prompt_embeds = self.encode_prompt(prompt, prompt_ids, num_videos, text_encoder_kwargs)
            if negative_prompt is not None or negative_prompt_ids is not None:
                negative_prompt_embeds = self.encode_prompt(negative_prompt, negative_prompt_ids, num_videos, text_encoder_kwargs)
        # i2v.py:56-64: CFG only with a negative prompt AND both scales above 1
        gs = list(guidance_scale) if isinstance(guidance_scale, (list, tuple)) else guidance_scale
        cfg = negative_prompt_embeds is not None and (all(g > 1.0 for g in gs) if isinstance(gs, list) else gs > 1.0)
        B = prompt_embeds.shape[0]
        if self.uses_image_embeds:
            if image_embeds is None:       # once per run, from the original image(s)
                _emit(progress_callback, 0.1, "Encoding image")
                image_embeds = self.encode_image(image if last_image is None else [image, last_image], B)
            elif image_embeds.shape[0] != B:
                image_embeds = image_embeds.repeat(B // image_embeds.shape[0], 1, 1)
            image_embeds = image_embeds.to(dev, compute_dtype(self.high_noise_transformer))
        else:
            image_embeds = None            # the A14B experts take no image tokens
        pixels, height, width = self.preprocess_image(image, height, width)
        last_pixels = None if last_image is None else self.preprocess_image(last_image, height, width, size=(height, width))[0]
        z_dim = 16
        num_latent_frames = (duration - 1) // self.vae_scale_factor_temporal + 1
        shape = (B, z_dim, num_latent_frames, height // self.vae_scale_factor_spatial, width // self.vae_scale_factor_spatial)
        if latents is None:
            latents = initial_noise(shape, dev, torch.float32, seed, generator)
        else:
            latents = latents.to(device=dev, dtype=torch.float32)
        _emit(progress_callback, 0.3, "Initialized latent noise")
        latent_condition = self.prepare_latent_condition(pixels, duration, B, last_pixels)
        if tuple(latent_condition.shape[2:]) != tuple(latents.shape[2:]):
            raise ValueError(f"wan i2v: condition latents {tuple(latent_condition.shape)} do not match the video latents {tuple(latents.shape)}")
        timesteps = self.scheduler.set_timesteps(num_inference_steps, device=dev)
        boundary = None if self.boundary_ratio is None else self.boundary_ratio * self.scheduler.config["num_train_timesteps"]
        dt = compute_dtype(self.high_noise_transformer)
        pe = prompt_embeds.to(dev, dt)
        ne = negative_prompt_embeds.to(dev, dt) if cfg else None
        _emit(progress_callback, 0.45, "Starting denoise phase")

        def mapped(p, msg):
            _emit(progress_callback, 0.5 + 0.4 * p, msg)

        latents = self.moe_denoise(latents=latents, timesteps=timesteps, prompt_embeds=pe, negative_prompt_embeds=ne,
                                   guidance_scale=gs, boundary_timestep=boundary, use_cfg_guidance=cfg,
                                   render_on_step=render_on_step, render_on_step_callback=render_on_step_callback,
                                   render_on_step_interval=render_on_step_interval, denoise_progress_callback=mapped,
                                   easy_cache_thresh=easy_cache_thresh, easy_cache_ret_steps=easy_cache_ret_steps,
                                   latent_condition=latent_condition, image_embeds=image_embeds)
        _emit(progress_callback, 0.92, "Denoising complete")
        if return_latents:
            _emit(progress_callback, 1.0, "Returning latents")
            return latents
        video = self.vae_decode(latents)
        _emit(progress_callback, 1.0, "Completed image-to-video pipeline")
        if output_type is not None:
            from .postprocess import tensor_to_frames
            return tensor_to_frames(video, output_type)
        return video
