"""Times per-block key bands on the large-attention kernel (ops.attention_prepared_band) against dense prepared attention
(ops.attention_prepared) and the coordinate window of the same temporal radius (ops.attention_prepared_window at (r, inf, inf)),
in one process, at the Wan video shapes.

    python tools/attn_band_bench.py [--rounds 5] [--out profiles/attn_band_bench.json] [--quick]

Prepared operands, H 40, D 128, token grids 21 x 30 x 52 and 21 x 45 x 80, radius 1, 2 and 4 frames.  HIP events around a batch of
calls; every cell is warmed up first, then `--rounds` interleaved rounds (every cell once per round), medians reported.  Per
(grid, radius): ms per launch of the band, of the window and of the dense kernel, the plan's kept fraction (host arithmetic),
"x dense" (band / dense) and "x ideal" (band / (dense x kept fraction)).  Per grid also the ALL-KEYS band (every block [0, S)) against the
dense launch — the same loop over the same keys, so the ratio shows what the band's shell costs — next to the dense launch's own
round-to-round spread, which is what that ratio is to be judged against.  The live shader clock (apexmi_clk_* over a GEMM K-loop
beside the measurement) is recorded with every grid: the boards of a pool differ.  Nothing is asserted."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import lib, ops  # noqa: E402

BIG = 1 << 15
H = 40
GRIDS = [(21, 30, 52), (21, 45, 80)]      # Wan 480p x 81 frames (32 760 tokens) and 720p x 81 frames (75 600)
RADII = [1, 2, 4]


def raster(grid, dev):
    f, h, w = grid
    return torch.stack(torch.meshgrid(torch.arange(f, device=dev), torch.arange(h, device=dev), torch.arange(w, device=dev),
                                      indexing="ij"), dim=-1).reshape(-1, 3)


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters   # ms per call


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/attn_band_bench.json")
    ap.add_argument("--quick", action="store_true", help="first grid only")
    args = ap.parse_args()
    dev = "cuda:0"
    results, full = [], []
    for grid in GRIDS[:1] if args.quick else GRIDS:
        S = grid[0] * grid[1] * grid[2]
        tpf = grid[1] * grid[2]
        skp = (S + 63) // 64 * 64
        nqb = (S + 255) // 256
        g = torch.Generator(device=dev).manual_seed(0)
        q, k = (torch.randn(1, H, S, 128, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(2))
        vt = torch.zeros(1, H, 128, skp, device=dev, dtype=torch.bfloat16)
        vt[..., :S] = torch.randn(1, H, 128, S, device=dev, generator=g, dtype=torch.bfloat16)
        out = torch.empty(1, S, H, 128, device=dev, dtype=torch.bfloat16)
        coords = raster(grid, dev)
        bands = {r: ops.frame_band_plan(grid[0], tpf, r, dev) for r in RADII}
        windows = {r: ops.window_plan(coords, radius=(r, BIG, BIG)) for r in RADII}
        all_keys = ops.band_plan([0] * nqb, [S] * nqb, S, S, dev)
        cells = [("dense", lambda: ops.attention_prepared(q, k, vt, out, S)),
                 ("band_all", lambda: ops.attention_prepared_band(q, k, vt, out, S, all_keys))]
        for r in RADII:
            cells.append((("window", r), lambda p=windows[r]: ops.attention_prepared_window(q, k, vt, out, S, p)))
            cells.append((("band", r), lambda p=bands[r]: ops.attention_prepared_band(q, k, vt, out, S, p)))
        iters, times = {}, {}
        for name, fn in cells:                            # warm-up; iteration count for ~50 ms per round
            fn()
            t1 = timed(fn, 1)
            iters[name] = max(1, min(20, int(50.0 / max(t1, 1e-3))))
            timed(fn, iters[name])
            times[name] = []
        lib.attn_w64_fallbacks()
        ghz = live_clock(dev)
        for _ in range(args.rounds):
            for name, fn in cells:
                times[name].append(timed(fn, iters[name]))
        fallbacks = lib.attn_w64_fallbacks()
        med = {name: statistics.median(t) for name, t in times.items()}
        dense_ms = med["dense"]
        dense_spread = (max(times["dense"]) - min(times["dense"])) / dense_ms
        row = dict(H=H, grid=list(grid), S=S, blocks=nqb * H, dense_ms=round(dense_ms, 3),
                   dense_rounds_ms=[round(t, 3) for t in times["dense"]], dense_spread=round(dense_spread, 4),
                   band_all_ms=round(med["band_all"], 3), band_all_rounds_ms=[round(t, 3) for t in times["band_all"]],
                   band_all_vs_dense=round(med["band_all"] / dense_ms, 4),
                   band_all_within_dense_spread=bool(abs(med["band_all"] / dense_ms - 1.0) <= dense_spread),
                   w64_fallbacks=fallbacks, rounds=args.rounds, gemm_clock_ghz=ghz)
        full.append(row)
        print(json.dumps(row), flush=True)
        for r in RADII:
            kept = bands[r].kept_fraction
            band_ms, win_ms = med[("band", r)], med[("window", r)]
            longest = max(e - a for a, e in zip(bands[r].lo[0], bands[r].hi[0]))
            row = dict(H=H, grid=list(grid), S=S, radius_frames=r, kept_fraction=round(kept, 4), longest_band_fraction=round(longest / S, 4),
                       band_ms=round(band_ms, 3), band_spread_ms=round(max(times[("band", r)]) - min(times[("band", r)]), 3),
                       window_ms=round(win_ms, 3), dense_ms=round(dense_ms, 3), ideal_ms=round(dense_ms * kept, 3),
                       x_dense=round(band_ms / dense_ms, 4), x_ideal=round(band_ms / (dense_ms * kept), 4),
                       window_x_dense=round(win_ms / dense_ms, 4), band_vs_window=round(band_ms / win_ms, 4),
                       rounds=args.rounds, iters=iters[("band", r)], gemm_clock_ghz=ghz)
            results.append(row)
            print(json.dumps(row), flush=True)
        del q, k, vt, out, bands, windows, all_keys, cells
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, all_keys=full, results=results), f, indent=1)


if __name__ == "__main__":
    main()
