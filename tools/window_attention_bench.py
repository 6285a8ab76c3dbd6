"""Times coordinate-window attention on prepared operands (ops.attention_prepared_window) against dense prepared attention
(ops.attention_prepared) in the same process, at the Wan video shapes.

    python tools/window_attention_bench.py [--rounds 3] [--out profiles/window_attention_bench.json] [--quick]

HIP events around a batch of calls; every cell is warmed up first, then `--rounds` interleaved rounds (every cell once per
round), medians reported.  Per (shape, radius): us per launch of the window kernel, us of the dense kernel, the allowed-pair
fraction, the SKIP / DENSE / PARTIAL tile counts, the one-time plan build, and two yardsticks: DENSE (the dense kernel's time)
and IDEAL (that time x the fraction of non-SKIP tiles); `above_ideal` = window / ideal.  The live shader clock (apexmi_clk_*
over a GEMM K-loop beside the measurement) is recorded with every shape: the boards of a pool differ.  Nothing is asserted."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import lib, ops  # noqa: E402

BIG = 1 << 15
# (H, token grid): Wan 480p x 81 frames (21 x 30 x 52 = 32 760) and 720p x 81 frames (21 x 45 x 80 = 75 600)
SHAPES = [(40, (21, 30, 52)), (40, (21, 45, 80))]
RADII = [(2, BIG, BIG), (4, 11, BIG), (4, 11, 20)]


def raster(grid, dev):
    f, h, w = grid
    return torch.stack(torch.meshgrid(torch.arange(f, device=dev), torch.arange(h, device=dev), torch.arange(w, device=dev),
                                      indexing="ij"), dim=-1).reshape(-1, 3)


def allowed_fraction(grid, radius):
    """exact, per axis: the rule is a product of three 1-D bands"""
    frac = 1.0
    for n, r in zip(grid, radius):
        i = torch.arange(n)
        frac *= float(((i[:, None] - i[None, :]).abs() <= r).double().mean())
    return frac


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / iters   # us per call


def live_clock(dev):
    a = torch.randn(4096, 4096, device=dev).to(torch.bfloat16)
    lib.clk_enable(True)
    for _ in range(4):
        ops.gemm(a, a)
    torch.cuda.synchronize()
    ghz = lib.clk_read()["ghz"]
    lib.clk_enable(False)
    return ghz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="profiles/window_attention_bench.json")
    ap.add_argument("--quick", action="store_true", help="first shape only")
    args = ap.parse_args()
    dev = "cuda:0"
    results = []
    for H, grid in SHAPES[:1] if args.quick else SHAPES:
        S = grid[0] * grid[1] * grid[2]
        skp = (S + 63) // 64 * 64
        g = torch.Generator(device=dev).manual_seed(0)
        q, k = (torch.randn(1, H, S, 128, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(2))
        vt = torch.zeros(1, H, 128, skp, device=dev, dtype=torch.bfloat16)
        vt[..., :S] = torch.randn(1, H, 128, S, device=dev, generator=g, dtype=torch.bfloat16)
        out = torch.empty(1, S, H, 128, device=dev, dtype=torch.bfloat16)
        coords = raster(grid, dev)
        plans, build_us = {}, {}
        ops.window_plan(coords, radius=(0, 0, 0))        # first launch of the pre-pass outside the timing
        for r in RADII:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plans[r] = ops.window_plan(coords, radius=r)
            torch.cuda.synchronize()
            build_us[r] = (time.perf_counter() - t0) * 1e6
        cells = [("dense", lambda: ops.attention_prepared(q, k, vt, out, S))]
        cells += [(r, lambda p=plans[r]: ops.attention_prepared_window(q, k, vt, out, S, p)) for r in RADII]
        iters, times = {}, {}
        for name, fn in cells:                            # warm-up; iteration count for ~50 ms per round
            fn()
            t1 = timed(fn, 1)
            iters[name] = max(1, min(20, int(50000 / max(t1, 1.0))))
            timed(fn, iters[name])
            times[name] = []
        ghz = live_clock(dev)
        for _ in range(args.rounds):
            for name, fn in cells:
                times[name].append(timed(fn, iters[name]))
        dense_us = statistics.median(times["dense"])
        for r in RADII:
            skip, dense, part = plans[r].tile_counts()
            kept = (dense + part) / (skip + dense + part)
            us = statistics.median(times[r])
            row = dict(H=H, grid=list(grid), S=S, radius=[x if x < BIG else "inf" for x in r], window_us=round(us, 1),
                       spread_us=round(max(times[r]) - min(times[r]), 1), dense_us=round(dense_us, 1),
                       allowed_fraction=round(allowed_fraction(grid, r), 4), tiles=dict(skip=skip, dense=dense, partial=part),
                       kept_tile_fraction=round(kept, 4), ideal_us=round(dense_us * kept, 1),
                       above_ideal=round(us / (dense_us * kept), 3), vs_dense=round(us / dense_us, 3),
                       plan_build_us=round(build_us[r], 1), rounds=len(times[r]), iters=iters[r], gemm_clock_ghz=ghz)
            results.append(row)
            print(json.dumps(row), flush=True)
        del q, k, vt, out, plans
        torch.cuda.empty_cache()
    # the crossover: the kept-tile fraction below which a window beats dense, from the measured cost per kept tile
    rel = [r["above_ideal"] for r in results]
    summary = dict(above_ideal_min=min(rel), above_ideal_max=max(rel),
                   crossover_kept_fraction=round(1.0 / statistics.median(rel), 3),
                   note="a window is faster than dense attention below about this fraction of kept tiles (1 / median above_ideal)")
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
