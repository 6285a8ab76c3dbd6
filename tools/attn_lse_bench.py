"""Times the log-sum-exp output and the merge over key chunks on the MI355X at B 1, H 24, S 4096, D 128, bf16:

  * ops.attention_masked with and without return_lse (the cost of the lse instantiation and its store);
  * ops.attention_chunked over 2 and 4 equal key chunks against the single call (the cost of not concatenating);
  * ops.attention_merge alone over 2, 4 and 8 partials, in GB/s of the bytes it has to move (n + 1 outs and n + 1 lse arrays).

    python tools/attn_lse_bench.py [--rounds 5] [--out profiles/attn_lse_bench.json]

HIP events around a batch of calls; every cell is warmed up first, then `--rounds` interleaved rounds in one process (every cell
once per round), medians and spreads reported.  The live shader clock (apexmi_clk_* over a GEMM K-loop beside the measurement)
is sampled before the first round and after every round and stands in every row: the boards of a pool differ.  Nothing is asserted."""
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

B, H, S, D = 1, 24, 4096, 128


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/attn_lse_bench.json")
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(B, H, S, D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))

    def chunks(t, n):
        return [t[:, :, i * (S // n):(i + 1) * (S // n)] for i in range(n)]

    cells = {"masked": lambda: ops.attention_masked(q, k, v),
             "masked_lse": lambda: ops.attention_masked(q, k, v, return_lse=True)}
    for n in (2, 4):
        cells[f"chunked_{n}"] = lambda ks=chunks(k, n), vs=chunks(v, n): ops.attention_chunked(q, ks, vs)
    partial = [ops.attention_masked(q, kc, vc, return_lse=True) for kc, vc in zip(chunks(k, 8), chunks(v, 8))]
    merged = torch.empty_like(partial[0][0].permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
    for n in (2, 4, 8):
        cells[f"merge_{n}"] = lambda o=[p[0] for p in partial[:n]], l=[p[1] for p in partial[:n]]: ops.attention_merge(o, l, out=merged)

    iters, times = {}, {}
    for name, fn in cells.items():                        # warm-up; iteration count for ~50 ms per round
        fn()
        t1 = timed(fn, 1)
        iters[name] = max(1, min(200, int(50000 / max(t1, 1.0))))
        timed(fn, iters[name])
        times[name] = []
    ghz = [live_clock(dev)]                               # sampled before the first round and after every round
    for _ in range(args.rounds):
        for name, fn in cells.items():
            times[name].append(timed(fn, iters[name]))
        ghz.append(live_clock(dev))
    clock = dict(gemm_clock_ghz=statistics.median(ghz), gemm_clock_ghz_min=min(ghz), gemm_clock_ghz_max=max(ghz))

    flops = 4.0 * B * H * S * S * D
    results = []
    for name in cells:
        ts = times[name]
        us = statistics.median(ts)
        row = dict(cell=name, shape=[B, H, S, D], dtype="bf16", us=round(us, 2), spread_us=round(max(ts) - min(ts), 2), rounds=len(ts),
                   iters=iters[name], **clock)
        if name.startswith("merge_"):
            n = int(name.split("_")[1])
            nbytes = (n + 1) * (B * S * H * D * 2 + B * H * S * 4)
            row.update(partials=n, bytes=nbytes, gb_per_s=round(nbytes / us * 1e-3, 1))
        else:
            row.update(tflops_dense=round(flops / us * 1e-6, 1))
        results.append(row)
        print(json.dumps(row), flush=True)
    med = {r["cell"]: r["us"] for r in results}
    summary = dict(lse_over_plain=round(med["masked_lse"] / med["masked"], 4),
                   chunked_2_over_single=round(med["chunked_2"] / med["masked_lse"], 4),
                   chunked_4_over_single=round(med["chunked_4"] / med["masked_lse"], 4),
                   **clock)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
