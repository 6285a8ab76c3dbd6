"""Times attention over a packed variable-length batch (ops.attention_varlen) on the MI355X at H 24, D 128,
bf16, against the two ways the same job is done without it:

  * varlen  one ops.attention_varlen launch on the packed [T, H, D] operands and cu_seqlens;
  * loop    one ops.attention_masked call per sequence, on views of the packed operands (what a per-sample loop costs once the
            lengths are on the host; the host synchronisation that puts them there is NOT in the time);
  * padded  one ops.attention_masked call on the padded [n, H, max, D] batch with a key-padding bool mask [n, 1, 1, max]
            (the padding copy is NOT in the time; the padded query rows are computed and thrown away);

for 8 equal sequences of 512, 8 ragged sequences of 64 .. 1024 and 160 sequences of 64 tokens (10 240 tokens: the Qwen2.5-VL
vision tower's windows).

    python tools/attn_varlen_bench.py [--rounds 5] [--out profiles/attn_varlen_bench.json]

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

H, D = 24, 128
SHAPES = {"equal 8 x 512": (512,) * 8,
          "ragged 8 x 64..1024": (64, 128, 192, 320, 448, 640, 832, 1024),
          "vision 160 x 64": (64,) * 160}


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


def cells_of(lens, dev, g):
    n, T, mx = len(lens), sum(lens), max(lens)
    q, k, v = (torch.randn(T, H, D, device=dev, generator=g, dtype=torch.bfloat16) for _ in range(3))
    cu_host = [0]
    for l in lens:
        cu_host.append(cu_host[-1] + l)
    cu = torch.tensor(cu_host, dtype=torch.int32, device=dev)
    views = [tuple(t[a:b].permute(1, 0, 2)[None] for t in (q, k, v)) for a, b in zip(cu_host[:-1], cu_host[1:])]
    qp, kp, vp = (torch.zeros(n, mx, H, D, device=dev, dtype=torch.bfloat16) for _ in range(3))
    keep = torch.zeros(n, 1, 1, mx, dtype=torch.bool, device=dev)
    for i, (a, b) in enumerate(zip(cu_host[:-1], cu_host[1:])):
        qp[i, :b - a], kp[i, :b - a], vp[i, :b - a] = q[a:b], k[a:b], v[a:b]
        keep[i, ..., :b - a] = True
    qp, kp, vp = (t.permute(0, 2, 1, 3) for t in (qp, kp, vp))

    def loop():
        for qi, ki, vi in views:
            ops.attention_masked(qi, ki, vi)

    return {"varlen": lambda: ops.attention_varlen(q, k, v, cu, cu, mx, mx),
            "loop": loop,
            "padded": lambda: ops.attention_masked(qp, kp, vp, keep)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/attn_varlen_bench.json")
    args = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(0)
    cells = {(shape, name): fn for shape, lens in SHAPES.items() for name, fn in cells_of(lens, dev, g).items()}

    iters, times = {}, {}
    for key, fn in cells.items():                         # warm-up; iteration count for ~50 ms per round
        fn()
        t1 = timed(fn, 1)
        iters[key] = max(1, min(200, int(50000 / max(t1, 1.0))))
        timed(fn, iters[key])
        times[key] = []
    ghz = [live_clock(dev)]                               # sampled before the first round and after every round
    for _ in range(args.rounds):
        for key, fn in cells.items():
            times[key].append(timed(fn, iters[key]))
        ghz.append(live_clock(dev))
    clock = dict(gemm_clock_ghz=statistics.median(ghz), gemm_clock_ghz_min=min(ghz), gemm_clock_ghz_max=max(ghz))

    results = []
    for (shape, name), ts in times.items():
        lens = SHAPES[shape]
        us = statistics.median(ts)
        flops = 4.0 * H * D * sum(l * l for l in lens)    # the pairs the rule allows
        row = dict(shape=shape, cell=name, sequences=len(lens), tokens=sum(lens), heads=H, head_dim=D, dtype="bf16", us=round(us, 2),
                   spread_us=round(max(ts) - min(ts), 2), rounds=len(ts), iters=iters[(shape, name)],
                   tflops_useful=round(flops / us * 1e-6, 1), **clock)
        results.append(row)
        print(json.dumps(row), flush=True)
    med = {(r["shape"], r["cell"]): r["us"] for r in results}
    summary = {shape: dict(varlen_over_loop=round(med[(shape, "varlen")] / med[(shape, "loop")], 4),
                           varlen_over_padded=round(med[(shape, "varlen")] / med[(shape, "padded")], 4)) for shape in SHAPES}
    summary.update(clock)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results, summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
