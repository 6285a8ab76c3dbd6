#!/usr/bin/env python3
"""Streaming rate of the GGUF dequantisation kernels (apexmi_dequant_gguf) on weight shapes of the Wan-14B blocks.

Per block type at [5120 x 5120] and [13824 x 5120]: microseconds per launch, bytes moved (blocks read + bf16 written), TB/s and
the ratio to torch's device copy of the same OUTPUT bytes; the fp8-scaled kernel (apexmi_dequant_fp8_scaled) at the same shape
is the comparison point.  All candidates of one shape run INTERLEAVED in one process: `--rounds` rounds, each timing `--iters`
back-to-back launches of every candidate between two device events; the median over rounds is reported with the min / max.
Buffers rotate over `--sets` copies so that a 50 MB weight is not served from the 256 MB MALL on every launch.

    python tools/gguf_dequant_bench.py --out profiles/gguf_dequant_bench.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gguf_dequant_bench.json")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--shapes", default="5120x5120,13824x5120")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gguf_dequant_bench: no GPU (a CPU run cannot give a time)")
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import gguf_file as G, ops
    dev = "cuda"
    rng = np.random.default_rng(0)
    results = []
    for shape in [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]:
        N, K = shape
        outs = [torch.empty((N, K), dtype=torch.bfloat16, device=dev) for _ in range(args.sets)]
        srcs = [torch.randn((N, K), device=dev).to(torch.bfloat16) for _ in range(args.sets)]
        cands = {}

        def copy(i, outs=outs, srcs=srcs):
            outs[i].copy_(srcs[i])
        cands["torch_copy_bf16"] = (copy, 2 * N * K, 2 * N * K)
        q8 = [torch.randn((N, K), device=dev).to(torch.float8_e4m3fn) for _ in range(args.sets)]
        sc = torch.rand(N, device=dev) + 0.5
        cands["fp8_scaled"] = ((lambda i, q8=q8, outs=outs, sc=sc: ops.dequant_fp8_scaled(q8[i], sc, out=outs[i])), N * K + 2 * N, 2 * N * K)
        for t in sorted(G.TYPES):
            name, blk, bs = G.TYPES[t]
            nb = N * K // blk * bs
            raw = rng.integers(0, 256, nb, dtype=np.uint8)
            if blk > 1:                                     # finite block scales (the rate does not depend on the values)
                r2 = raw.reshape(-1, bs)
                for o in {G.Q6_K: [208]}.get(t, [0, 2] if t in (G.Q4_1, G.Q5_1, G.Q4_K, G.Q5_K) else [0]):
                    r2[:, o + 1] &= 0x3F
            bl = [torch.from_numpy(np.roll(raw, 64 * i)).to(dev) for i in range(args.sets)]
            cands[name] = ((lambda i, bl=bl, t=t, outs=outs: ops.dequant_gguf(bl[i], t, (N, K), out=outs[i])), nb, 2 * N * K)
        times = {k: [] for k in cands}
        for k, (fn, _, _) in cands.items():                 # warm every candidate
            for i in range(args.sets):
                fn(i)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, (fn, _, _) in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for j in range(args.iters):
                    fn(j % args.sets)
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        base = statistics.median(times["torch_copy_bf16"])
        for k, (_, rd, wr) in cands.items():
            us = statistics.median(times[k])
            results.append({"shape": [N, K], "kernel": k, "us_per_launch": round(us, 2), "us_min": round(min(times[k]), 2),
                            "us_max": round(max(times[k]), 2), "bytes_read": rd, "bytes_written": wr,
                            "TBps": round((rd + wr) / us * 1e-6, 3), "time_over_copy": round(us / base, 3)})
            print(json.dumps(results[-1]), flush=True)
        del outs, srcs, q8, cands
        torch.cuda.empty_cache()
    doc = {"tool": "tools/gguf_dequant_bench.py", "device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": args.rounds,
           "buffer_sets": args.sets, "timing": "device events around `iters` back-to-back launches, median over rounds, candidates interleaved",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
