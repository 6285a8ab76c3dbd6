"""Times the "hip_mfma_sdpa" backend (ops.attention_masked) on the MI355X against `hip_mfma` without a mask (the w64
ceiling) and torch's own F.scaled_dot_product_attention on the GPU with the same arguments (what a manifest gets with "sdpa").

    python tools/sdpa_masked_bench.py [--rounds 3] [--out profiles/sdpa_masked_bench.json] [--quick]

HIP events around a batch of calls; every (shape, variant, backend) is warmed up first, then `--rounds` interleaved rounds
(every cell once per round); reported: median and spread (max - min) of the per-call time, TFLOP/s on the dense FLOPs
(4 B H Sq Sk D) and on the allowed-fraction FLOPs, and the fraction of 2.5 PF (the dense bf16 MFMA peak)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import attention_backend as ab  # noqa: E402
from apex_studio_amd import ops  # noqa: E402

PEAK = 2.5e15
SHAPES = [(1, 24, 4096, 128), (1, 40, 16384, 128), (2, 16, 4096, 64)]


def variants(B, H, S, dev):
    i = torch.arange(S, device=dev)
    keep = torch.ones(B, S, dtype=torch.bool, device=dev)
    keep[:, S - S // 4:] = False
    out = {
        "none": (None, False),
        "causal": (None, True),
        "all_true": (torch.ones(S, S, dtype=torch.bool, device=dev), False),
        "joint_pad25": (keep[:, None, :, None] & keep[:, None, None, :], False),
        "window1024": (((i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - 1024)), False),
    }
    hb = H if S <= 8192 else 1
    slopes = torch.linspace(-0.5, -0.01, hb, device=dev)[:, None, None]
    out["bias_f32"] = ((slopes * (i[None, :] - i[:, None]).abs().float())[None], False)   # [1,H,S,S] (ALiBi-like) | [1,1,S,S]
    return out


def allowed_fraction(mask, causal, B, H, S):
    if mask is None:
        return (S + 1) / (2 * S) if causal else 1.0
    if mask.dtype == torch.bool:
        return float(mask.float().mean())
    return float(torch.isfinite(mask).float().mean())


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/sdpa_masked_bench.json")
    ap.add_argument("--quick", action="store_true", help="first shape only")
    args = ap.parse_args()
    dev = "cuda:0"
    results = []
    for (B, H, S, D) in SHAPES[:1] if args.quick else SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        q, k, v = (torch.randn(B, H, S, D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))
        cells = []
        for vname, (mask, causal) in variants(B, H, S, dev).items():
            frac = allowed_fraction(mask, causal, B, H, S)
            cells.append((vname, "hip_mfma_sdpa", frac,
                          lambda m=mask, c=causal: ab.hip_mfma_sdpa(q, k, v, attn_mask=m, is_causal=c)))
            cells.append((vname, "torch_sdpa", frac,
                          lambda m=mask, c=causal: F.scaled_dot_product_attention(q, k, v, attn_mask=m, is_causal=c)))
        cells.append(("none", "hip_mfma", 1.0, lambda: ops.attention(q, k, v)))
        iters, times, errors = {}, {}, {}
        for vname, backend, frac, fn in cells:          # warm-up; iteration count for ~20 ms per round
            key = (vname, backend)
            try:
                fn()
                t1 = timed(fn, 1)
                iters[key] = max(1, min(50, int(20000 / max(t1, 1.0))))
                timed(fn, iters[key])
                times[key] = []
            except Exception as e:   # torch may refuse or run out of memory on a shape: reported, not timed
                errors[key] = f"{type(e).__name__}: {str(e)[:200]}"
                torch.cuda.synchronize()
        for _ in range(args.rounds):
            for vname, backend, frac, fn in cells:
                key = (vname, backend)
                if key in times:
                    times[key].append(timed(fn, iters[key]))
        flops = 4.0 * B * H * S * S * D
        for vname, backend, frac, fn in cells:
            key = (vname, backend)
            row = dict(shape=[B, H, S, D], variant=vname, backend=backend, allowed_fraction=round(frac, 4))
            if key in errors:
                row["error"] = errors[key]
            else:
                ts = times[key]
                us = statistics.median(ts)
                row.update(us=round(us, 1), spread_us=round(max(ts) - min(ts), 1), rounds=len(ts), iters=iters[key],
                           tflops_dense=round(flops / us * 1e-6, 1), tflops_allowed=round(flops * frac / us * 1e-6, 1),
                           frac_of_peak=round(flops * frac / us * 1e-6 / (PEAK * 1e-12), 3))
            results.append(row)
            print(json.dumps(row), flush=True)
        del q, k, v
        torch.cuda.empty_cache()

    def us(shape, variant, backend):
        for r in results:
            if r["shape"] == shape and r["variant"] == variant and r["backend"] == backend:
                return r.get("us")
        return None

    gates = []
    for (B, H, S, D) in SHAPES[:1] if args.quick else SHAPES:
        shp = [B, H, S, D]
        base = us(shp, "none", "hip_mfma_sdpa")
        for vname in ("causal", "all_true", "joint_pad25", "window1024", "bias_f32"):
            mine, theirs = us(shp, vname, "hip_mfma_sdpa"), us(shp, vname, "torch_sdpa")
            gates.append(dict(shape=shp, gate="faster than torch sdpa", variant=vname, ours_us=mine, torch_us=theirs,
                              ok=bool(mine and (theirs is None or mine < theirs))))
        for vname, lim in (("causal", 0.6), ("all_true", 1.05), ("joint_pad25", 1.3)):
            r = us(shp, vname, "hip_mfma_sdpa")
            gates.append(dict(shape=shp, gate=f"<= {lim} x no-mask", variant=vname, ratio=round(r / base, 3), ok=r / base <= lim))
        w64 = us(shp, "none", "hip_mfma")
        gates.append(dict(shape=shp, gate="no-mask vs hip_mfma (not gated)", ratio=round(base / w64, 3) if w64 else None))
    for gte in gates:
        print(json.dumps(gte), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results, gates=gates), f, indent=1)


if __name__ == "__main__":
    main()
