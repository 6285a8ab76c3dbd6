"""Times the one-launch wide-head attention (ops.attention_wide) against the materialised path it is an
alternative to (ops.attention / ops.attention_framecausal: the baseline) on the MI355X, bf16, one head:

  * (T, 1, 1024, 1024, 384) for T = 1 and T = 4: the Wan VAE mid block of one tile, q / k / v the column slices of one fused buffer;
  * (1, 1, 4096, 4096, 512) and (1, 1, 16384, 16384, 512): the Flux VAE mid block at 512² and 1024²;
  * (1, 1, 4096, 4096, 512) frame-causal with 1024 tokens a frame (4 frames of a 32 x 32 latent tile).

    python tools/attn_wide_bench.py [--rounds 5] [--out profiles/attn_wide_bench.json]
    python tools/attn_wide_bench.py --splits [--out profiles/attn_wide_split_bench.json]

--splits adds, for every shape, the cells flash/splits=2, 4, 8 and flash/auto (ops.attention_wide's key_splits; the split count
"auto" picked stands in its row) beside the same two baselines, in the same rounds, and one row per shape for the partial-merge
launch alone at 8 partials (the library's own profiler class of that launch, event-timed around the one kernel, over the
splits=8 cell of every round).  The summary says, per shape, whether the count "auto" picks is slower than the unsplit launch by
more than the larger of the two cells' round-to-round spreads.

HIP events around a batch of calls; every cell is warmed up first, then `--rounds` interleaved rounds in one process (every cell
once per round), medians and spreads reported.  The live shader clock (apexmi_clk_* over a GEMM K-loop beside the measurement)
is sampled before the first round and after every round and stands in every row.  Whole VAE decodes are not timed: this tool builds
no model, and timing the decodes in both modes was not attempted.  Nothing is asserted."""
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

# (name, T, S, D, frame_tokens)
SHAPES = (("wan_tile_T1", 1, 1024, 384, 0), ("wan_tile_T4", 4, 1024, 384, 0), ("flux_512", 1, 4096, 512, 0),
          ("flux_1024", 1, 16384, 512, 0), ("framecausal_4x1024", 1, 4096, 512, 1024))


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


def merge_us(p):
    """us per launch of the library profiler's merge class (apexmi_attn_merge and the wide kernel's partial merge share it)"""
    r = p[lib.PROF_CLASSES[5]]
    return 1000.0 * r["ms"] / max(1, r["launches"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--splits", action="store_true", help="add the key-split cells and the partial-merge launch")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or ("profiles/attn_wide_split_bench.json" if args.splits else "profiles/attn_wide_bench.json")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    cells, meta = {}, {}
    for name, T, S, D, ft in SHAPES:
        qkv = torch.randn(T, 1, S, 3 * D, device=dev, generator=g, dtype=torch.bfloat16)
        q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
        if ft:
            cells[name + "/materialised"] = lambda q=q, k=k, v=v, ft=ft: ops.attention_framecausal(q, k, v, ft)
        else:
            cells[name + "/materialised"] = lambda q=q, k=k, v=v: ops.attention(q, k, v)
        cells[name + "/flash"] = lambda q=q, k=k, v=v, ft=ft: ops.attention_wide(q, k, v, frame_tokens=ft)
        nf = S // ft if ft else 0
        pairs = ft * ft * nf * (nf + 1) / 2 if ft else S * S
        modes = ["materialised", "flash"]
        if args.splits:
            n_auto = int(lib.load().apexmi_attn_wide_auto_splits(T * ((S + 127) // 128), (S + 63) // 64, cus))
            for ks in (2, 4, 8, "auto"):
                mode = "flash/auto" if ks == "auto" else f"flash/splits={ks}"
                cells[f"{name}/{mode}"] = lambda q=q, k=k, v=v, ft=ft, ks=ks: ops.attention_wide(q, k, v, frame_tokens=ft, key_splits=ks)
                modes.append(mode)
        for mode in modes:
            meta[f"{name}/{mode}"] = dict(shape=[T, 1, S, S, D], frame_tokens=ft, flops=4.0 * T * pairs * D)
        for mode in modes[2:]:
            n = n_auto if mode == "flash/auto" else int(mode.rsplit("=", 1)[1])
            meta[f"{name}/{mode}"].update(key_splits=n, workspace_bytes=int(lib.load().apexmi_attn_wide_split_workspace_bytes(T, 1, S, S, D, n)))
        meta[name + "/flash"]["workspace_bytes"] = int(lib.load().apexmi_attn_wide_workspace_bytes(T, 1, S, D))
        meta[name + "/materialised"]["workspace_bytes"] = int(lib.load().apexmi_attn_framecausal_workspace_bytes(S, D) if ft else
                                                              lib.load().apexmi_attn_workspace_bytes(T, 1, S, S, D, lib.BF16))

    iters, times = {}, {}
    for name, fn in cells.items():                        # warm-up; iteration count for ~50 ms per round
        fn()
        t1 = timed(fn, 1)
        iters[name] = max(1, min(200, int(50000 / max(t1, 1.0))))
        timed(fn, iters[name])
        times[name] = []
    ghz = [live_clock(dev)]                               # sampled before the first round and after every round
    merge = {name: [] for name, *_ in SHAPES} if args.splits else {}
    for _ in range(args.rounds):
        for name, fn in cells.items():
            times[name].append(timed(fn, iters[name]))
        for name in merge:                                # the merge launch alone: its profiler class over the splits=8 cell
            lib.prof_reset()
            lib.prof_enable(True)
            for _i in range(20):
                cells[name + "/flash/splits=8"]()
            torch.cuda.synchronize()
            p = lib.prof_read()
            lib.prof_enable(False)
            merge[name].append(merge_us(p))
        ghz.append(live_clock(dev))
    clock = dict(gemm_clock_ghz=statistics.median(ghz), gemm_clock_ghz_min=min(ghz), gemm_clock_ghz_max=max(ghz))

    results = []
    for name in cells:
        ts = times[name]
        us = statistics.median(ts)
        m = meta[name]
        row = dict(cell=name, shape=m["shape"], frame_tokens=m["frame_tokens"], dtype="bf16", us=round(us, 2),
                   spread_us=round(max(ts) - min(ts), 2), rounds=len(ts), iters=iters[name], workspace_bytes=m["workspace_bytes"],
                   tflops_allowed=round(m["flops"] / us * 1e-6, 1), **clock)
        if "key_splits" in m:
            row["key_splits"] = m["key_splits"]
        results.append(row)
        print(json.dumps(row), flush=True)
    for name, ts in merge.items():
        m = meta[name + "/flash/splits=8"]
        row = dict(cell=name + "/merge_alone/partials=8", shape=m["shape"], frame_tokens=m["frame_tokens"], dtype="bf16",
                   us=round(statistics.median(ts), 2), spread_us=round(max(ts) - min(ts), 2), rounds=len(ts), iters=20, **clock)
        results.append(row)
        print(json.dumps(row), flush=True)
    med = {r["cell"]: r["us"] for r in results}
    spread = {r["cell"]: r["spread_us"] for r in results}
    summary = {name + "_materialised_over_flash": round(med[name + "/materialised"] / med[name + "/flash"], 3) for name, *_ in SHAPES}
    if args.splits:
        for name, *_ in SHAPES:
            a, f = name + "/flash/auto", name + "/flash"
            summary[name + "_auto_splits"] = meta[a]["key_splits"]
            summary[name + "_flash_over_auto"] = round(med[f] / med[a], 3)
            summary[name + "_materialised_over_auto"] = round(med[name + "/materialised"] / med[a], 3)
            summary[name + "_auto_slower_than_unsplit_beyond_spread"] = bool(med[a] - med[f] > max(spread[a], spread[f]))
    summary.update(clock)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
