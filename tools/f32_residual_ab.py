#!/usr/bin/env python
"""What the f32 residual stream costs (`set_residual_dtype(torch.float32)`): in ONE process on one board, the
two modes interleaved (the discipline of profiles/r06_step_ab.log),

  * the Flux-Dev 1024^2 denoise step (19 + 38 blocks, S 4096 + 512) and
  * the Wan-2.2-A14B 720p x 81 f step (40 blocks, S 75600 + 512 text),

each as ms/step per mode and round and the ratio of the medians; and the achieved bandwidth of the norm kernel that reads the
float rows (apexmi_ln_modulate2_f32in) at both models' shapes next to the bf16 norm and to torch's copy of the same bytes.  The
live shader clock over the GEMM K-loops (apexmi_clk_*) is reported with every timed run: the boards of a pool differ.

  MODELS=flux,wan  STEPS=8 WAN_STEPS=2 ROUNDS=3  OUT=profiles/f32_residual_ab.json
"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import lib, ops  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
MODELS = [m for m in os.environ.get("MODELS", "flux,wan").split(",") if m]
STEPS = int(os.environ.get("STEPS", "8"))
WAN_STEPS = int(os.environ.get("WAN_STEPS", "2"))
ROUNDS = int(os.environ.get("ROUNDS", "3"))
OUT = os.environ.get("OUT", "")
ARMS = (("bf16", BF), ("f32_residual", F32))


def timed(fn):
    torch.cuda.synchronize()
    lib.clk_enable(True)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ghz = lib.clk_read()["ghz"]
    lib.clk_enable(False)
    return dt, ghz, out


def ab(model, run, steps):
    res = {a: [] for a, _ in ARMS}
    clk = {a: [] for a, _ in ARMS}
    finals = {}
    for a, dt_ in ARMS:                       # warm every shape of both modes (workspaces, code objects)
        model.set_residual_dtype(dt_)
        run(1)
    for r in range(ROUNDS):
        for a, dt_ in ARMS:
            model.set_residual_dtype(dt_)
            run(1)                            # the mode switch drops the workspace: its allocation stays out of the timed window
            dt, ghz, lat = timed(lambda: run(steps))
            res[a].append(1e3 * dt / steps)
            clk[a].append(ghz)
            finals.setdefault(a, lat.float().cpu())
            print(json.dumps({"round": r, "arm": a, "ms_per_step": res[a][-1], "gemm_clock_ghz": ghz}), flush=True)
    model.set_residual_dtype(BF)
    med = {a: statistics.median(v) for a, v in res.items()}
    d = finals["f32_residual"] - finals["bf16"]
    return {"steps": steps, "rounds": ROUNDS, "ms_per_step": res, "median_ms": med, "min_ms": {a: min(v) for a, v in res.items()},
            "gemm_clock_ghz_median": {a: statistics.median(v) for a, v in clk.items()},
            "ratio_f32_residual_over_bf16": med["f32_residual"] / med["bf16"],
            "final_latents_rel_l2_between_modes": float(d.norm() / finals["bf16"].norm())}


def flux():
    from apex_studio_amd.engine_flux import calculate_shift, latent_image_ids
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.schedulers import FlowMatchEulerDiscreteScheduler
    cfg = dict(patch_size=1, in_channels=64, num_layers=19, num_single_layers=38, attention_head_dim=128, num_attention_heads=24,
               joint_attention_dim=4096, pooled_projection_dim=768, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
    model = FluxTransformer2DModel(**cfg, device=DEV, dtype=BF).init_synthetic(seed=1234)
    model.pack()
    g = torch.Generator(device=DEV).manual_seed(100)
    lat0 = torch.randn(1, 4096, 64, generator=g, device=DEV).to(BF)
    enc = torch.randn(1, 512, 4096, generator=g, device=DEV).to(BF)
    pooled = torch.randn(1, 768, generator=g, device=DEV).to(BF)
    img_ids, txt_ids = latent_image_ids(64, 64).to(DEV), torch.zeros(512, 3, device=DEV)
    guidance = torch.full([1], 3.5, device=DEV, dtype=F32)
    sched = FlowMatchEulerDiscreteScheduler.flux_dev()

    def run(n):
        ts = sched.set_timesteps(sigmas=torch.linspace(1.0, 1.0 / n, n).tolist(), mu=calculate_shift(4096), device=DEV)
        sched.set_begin_index(0)
        lat = lat0
        h = model.begin_schedule(torch.stack([t.expand(1).to(lat.dtype) / 1000 for t in ts]), guidance, pooled)
        for i, t in enumerate(ts):
            v = model(hidden_states=lat, timestep=t.expand(1).to(lat.dtype) / 1000, guidance=guidance, pooled_projections=pooled,
                      encoder_hidden_states=enc, txt_ids=txt_ids, img_ids=img_ids, joint_attention_kwargs={"modulation_step": i},
                      return_dict=False)[0]
            lat = sched.step(v, t, lat, return_dict=False)[0]
        torch.cuda.synchronize()
        model.end_schedule(h)
        return lat
    out = ab(model, run, STEPS)
    out["workload"] = "flux-dev 1024x1024 denoise step (19 + 38 blocks, S_img 4096 + S_txt 512, B=1) + FlowMatch-Euler step"
    return out


def wan():
    from apex_studio_amd.schedulers import UniPCMultistepScheduler
    from apex_studio_amd.wan import WanTransformer3DModel
    model = WanTransformer3DModel(device=DEV, dtype=BF).init_synthetic(seed=999)
    model.pack()
    lat0 = torch.randn(1, 16, 21, 90, 160, generator=torch.Generator(device=DEV).manual_seed(300), device=DEV)
    enc = torch.randn(1, 512, 4096, generator=torch.Generator(device=DEV).manual_seed(9), device=DEV).to(BF)
    sched = UniPCMultistepScheduler(shift=3.0)

    def run(n):
        ts = sched.set_timesteps(max(n, 2), device=DEV)
        lat = lat0
        for t in ts[:n]:
            v = model(hidden_states=lat.to(BF), timestep=t.expand(1), encoder_hidden_states=enc, return_dict=False)[0]
            lat = sched.step(v.float(), t, lat, return_dict=False)[0]
        return lat
    out = ab(model, run, WAN_STEPS)
    out["workload"] = "wan-2.2-a14b text-to-video 720p x 81 frames: one expert forward (40 blocks, S 75600 + 512 text, B=1, no CFG) + UniPC step"
    return out


def norm_bandwidth():
    """ln_modulate at the step's shapes, buffers rotating over 4 (MALL-warm, as behind the producing GEMM in the step)."""
    def timeit(fn, iters=200, warm=20):
        for i in range(warm):
            fn(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(iters):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters       # us

    res = {}
    g = torch.Generator(device=DEV).manual_seed(0)
    for tag, S, C, split, nb in (("flux 4608 x 3072", 4608, 3072, 512, 4), ("wan 75600 x 5120", 75600, 5120, 0, 2)):
        xf = [torch.randn(S, C, generator=g, device=DEV) for _ in range(nb)]
        xb = [x.to(BF) for x in xf]
        ob = [torch.empty(S, C, dtype=BF, device=DEV) for _ in range(nb)]
        sc, sh, sc2, sh2 = (torch.randn(C, generator=g, device=DEV) * 0.1 for _ in range(4))
        kw = dict(split=split, scale2=sc2, shift2=sh2) if split else {}
        us = {"f32in": [], "bf16": [], "torch copy f32 -> bf16": [], "torch copy bf16 -> bf16": []}
        for _ in range(3):
            us["f32in"].append(timeit(lambda i: ops.ln_modulate(xf[i % nb], sc, sh, out=ob[i % nb], **kw)))
            us["bf16"].append(timeit(lambda i: ops.ln_modulate(xb[i % nb], sc, sh, out=ob[i % nb], **kw)))
            us["torch copy f32 -> bf16"].append(timeit(lambda i: ob[i % nb].copy_(xf[i % nb])))
            us["torch copy bf16 -> bf16"].append(timeit(lambda i: ob[i % nb].copy_(xb[i % nb])))
        by = {"f32in": 6.0 * S * C, "bf16": 4.0 * S * C, "torch copy f32 -> bf16": 6.0 * S * C, "torch copy bf16 -> bf16": 4.0 * S * C}
        res[tag] = {"bytes": by, "us_best": {k: round(min(v), 2) for k, v in us.items()},
                    "GBps_best": {k: round(by[k] / min(v) / 1e3, 1) for k, v in us.items()}}
        print(json.dumps({tag: res[tag]}), flush=True)
    return res


def main():
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU path"
    out = {"device": torch.cuda.get_device_name(0), "norm_kernel": norm_bandwidth()}
    for name in MODELS:
        out[name] = {"flux": flux, "wan": wan}[name]()
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if OUT:
        with open(OUT, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
