"""Times the Wan-2.1 I2V / FLF2V image-conditioned cross-attention on the MI355X.

    python tools/wan_image_cond_bench.py [--rounds 5] [--depth 4] [--out profiles/wan_image_cond_bench.json] [--quick]

1. Kernel: the fused two-context launch (ops.attention_prepared_dual) against the unfused composition (two
   ops.attention_prepared launches + a bf16 ops.add), H = 40, Sk_t = 512, Sk_i in {257 (I2V), 514 (FLF2V)},
   Sq in {32 760 (480p x 81 f), 75 600 (720p x 81 f)}.  HIP events around a batch of calls; every cell is warmed up, then
   `--rounds` interleaved rounds (fused, unfused, fused, ...); reported: median and spread of the per-call time, the ratio
   fused / unfused, and TFLOP/s on the attention FLOPs 4 H Sq (Sk_t + Sk_i) 128.
2. Model: one 480p x 81 f forward step (S = 32 760) of a full-width Wan-2.1-I2V-shaped transformer (5120 = 40 x 128, ffn 13824,
   in_channels 36, text 4096 x 512, image_dim 1280, 257 image tokens), random weights, at `--depth` blocks, with and without
   the image tokens (the text-only run is the same model with encoder_hidden_states_image=None)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import ops  # noqa: E402

PEAK = 2.5e15


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters     # us per call


def kernel_cells(rounds, quick):
    dev, bf, H, sk_t = "cuda", torch.bfloat16, 40, 512
    rows = []
    g = torch.Generator(device=dev).manual_seed(0)
    for sq in ((32760,) if quick else (32760, 75600)):
        q = torch.randn(1, H, sq, 128, generator=g, device=dev).to(bf)
        kt = torch.randn(1, H, sk_t, 128, generator=g, device=dev).to(bf)
        vtt = torch.randn(1, H, 128, sk_t, generator=g, device=dev).to(bf)
        fused = torch.empty(1, sq, H, 128, dtype=bf, device=dev)
        o1, o2, o3 = (torch.empty(1, sq, H, 128, dtype=bf, device=dev) for _ in range(3))
        for sk_i in (257, 514):
            skp = (sk_i + 63) // 64 * 64
            ki = torch.randn(1, H, sk_i, 128, generator=g, device=dev).to(bf)
            vti = torch.zeros(1, H, 128, skp, dtype=bf, device=dev)
            vti[..., :sk_i] = torch.randn(1, H, 128, sk_i, generator=g, device=dev).to(bf)

            def run_fused():
                ops.attention_prepared_dual(q, kt, vtt, sk_t, ki, vti, sk_i, fused)

            def run_unfused():
                ops.attention_prepared(q, kt, vtt, o1, sk_t)
                ops.attention_prepared(q, ki, vti, o2, sk_i)
                ops.add(o1, o2, out=o3)
            cells = {"fused": run_fused, "unfused": run_unfused}
            for fn in cells.values():          # warm-up
                fn()
                timed(fn, 3)
            iters = 20
            times = {k: [] for k in cells}
            for _ in range(rounds):
                for k, fn in cells.items():
                    times[k].append(timed(fn, iters))
            same = float((fused == o3).float().mean())
            rel = float((fused.float() - o3.float()).norm() / o3.float().norm())
            flops = 4.0 * H * sq * (sk_t + sk_i) * 128
            row = dict(H=H, Sq=sq, Sk_t=sk_t, Sk_i=sk_i, rounds=rounds, iters=iters, bit_identical_fraction=round(same, 4),
                       rel_l2_fused_vs_unfused=rel)
            for k, ts in times.items():
                us = statistics.median(ts)
                row[k] = dict(us=round(us, 1), spread_us=round(max(ts) - min(ts), 1), tflops=round(flops / us * 1e-6, 1),
                              frac_of_peak=round(flops / us * 1e-6 / (PEAK * 1e-12), 3))
            row["ratio_fused_over_unfused"] = round(row["fused"]["us"] / row["unfused"]["us"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del q, kt, vtt, fused, o1, o2, o3
        torch.cuda.empty_cache()
    return rows


def model_step(depth, rounds):
    from apex_studio_amd.wan import WanTransformer3DModel
    dev, bf = "cuda", torch.bfloat16
    cfg = dict(patch_size=(1, 2, 2), num_attention_heads=40, attention_head_dim=128, in_channels=36, out_channels=16,
               text_dim=4096, freq_dim=256, ffn_dim=13824, num_layers=depth, cross_attn_norm=True, eps=1e-6,
               image_dim=1280, added_kv_proj_dim=5120)
    m = WanTransformer3DModel(**cfg, device=dev, dtype=bf).init_synthetic(0)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(1, 36, 21, 60, 104, generator=g, device=dev).to(bf)          # 480p x 81 f latent: S = 21 x 30 x 52 = 32 760
    t = torch.tensor([500.0], device=dev)
    txt = torch.randn(1, 512, 4096, generator=g, device=dev).to(bf)
    img = torch.randn(1, 257, 1280, generator=g, device=dev).to(bf)
    cells = {"image": lambda: m(hidden_states=x, timestep=t, encoder_hidden_states=txt, encoder_hidden_states_image=img,
                                return_dict=False),
             "text_only": lambda: m(hidden_states=x, timestep=t, encoder_hidden_states=txt, return_dict=False)}
    for fn in cells.values():
        fn()
        timed(fn, 1)
    times = {k: [] for k in cells}
    for _ in range(rounds):
        for k, fn in cells.items():
            times[k].append(timed(fn, 2))
    row = dict(model="wan2.1-i2v-shaped", depth=depth, full_depth=40, S=32760, rounds=rounds)
    for k, ts in times.items():
        ms = statistics.median(ts) / 1e3
        row[k] = dict(ms=round(ms, 2), spread_ms=round((max(ts) - min(ts)) / 1e3, 2), ms_per_block=round(ms / depth, 3))
    row["image_over_text_only"] = round(row["image"]["ms"] / row["text_only"]["ms"], 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--out", default="profiles/wan_image_cond_bench.json")
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wan_image_cond_bench: needs the GPU")
    kern = kernel_cells(args.rounds, args.quick)
    model = model_step(args.depth, max(2, args.rounds // 2))
    gates = [dict(gate="fused no slower than unfused", Sq=r["Sq"], Sk_i=r["Sk_i"], ratio=r["ratio_fused_over_unfused"],
                  ok=r["ratio_fused_over_unfused"] <= 1.0) for r in kern]
    for gte in gates:
        print(json.dumps(gte), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, kernel=kern, model=model, gates=gates), f,
                  indent=1)


if __name__ == "__main__":
    main()
