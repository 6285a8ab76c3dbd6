#!/usr/bin/env python
"""Run-time LoRA on a resident e4m3 weight: the FP8 GEMM with the adapter tail against the bf16 path it replaces,
at the Wan-2.2 A14B block shapes, in one process.

For every (M, K -> N) of the block Linears at 720p x 81 f (M = 75 600) and 480p x 81 f (M = 32 760) and padded rank 64 and 128:
  (i)   parent : `_gemm_fp8_lora` — skinny GEMM, dequantise W into the [N, K + Rp] scratch, copy B' behind it, ONE bf16 GEMM over
                 K + Rp                                                       (`Fp8Weight.lora_compute = "bf16"`, any `compute`)
  (ii)  fp8    : skinny GEMM + apexmi_quant_rows_fp8 + apexmi_gemm_fp8_lora   (`compute = "fp8"`, `lora_compute = "fp8"`)
  (iii) plain  : apexmi_quant_rows_fp8 + apexmi_gemm_fp8, no adapters: (ii) - (iii) prices the skinny GEMM and the tail
timed like tools/gemm_fp8_bench.py: HIP events around `--iters` back-to-back calls, `--rounds` interleaved rounds, medians; random
operands; the live GEMM clock (`apexmi_clk_enable`) of the two fp8 kernels read in a separate, untimed pass.  TFLOP/s count
2 M N K for all three.  A whole Wan step with adapters is NOT measured here.  Writes one JSON document (`--out`)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import lib, ops  # noqa: E402

DEV = torch.device("cuda", 0)
SHAPES = [(5120, 15360), (5120, 5120), (5120, 13824), (13824, 5120)]          # K -> N: q|k|v, attention out / cross q, FFN up, FFN down
MS = [75600, 32760]
RANKS = [64, 128]


def fp8_weight(N, K, g):
    w = torch.randn(N, K, generator=g, device=DEV) * 0.02
    s = w.abs().amax(dim=1) / 448.0
    rec = ops.Fp8Weight((w / s.view(-1, 1)).to(torch.float8_e4m3fn), s)
    rec.parts = [("lin", 0, N)]
    return rec


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


def clock_of(fn):
    lib.clk_enable(True)
    fn()
    torch.cuda.synchronize()
    ghz = lib.clk_read()["ghz"]
    lib.clk_enable(False)
    return None if ghz is None else round(ghz, 3)


def bench_shape(M, K, N, Rp, g, rounds, iters):
    buf = torch.zeros(M, K + Rp, dtype=torch.bfloat16, device=DEV)
    buf[:, :K] = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    a = buf[:, :K]
    w, plain = fp8_weight(N, K, g), fp8_weight(N, K, g)
    w.set_lora([("lin", torch.randn(Rp, K, generator=g, device=DEV) * 0.02, torch.randn(N, Rp, generator=g, device=DEV) * 0.02, 1.0)])
    assert w.lora_A.shape[0] == Rp
    plain.compute = "fp8"
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    q, s = ops.quant_rows_fp8(a)
    t = buf[:, K:K + Rp]

    def lora(compute, lora_compute):
        def run():
            w.compute, w.lora_compute = compute, lora_compute
            ops.gemm(a, w, None, out=out, lora_buf=buf)
        return run
    arms = {"parent": lora("bf16", "bf16"), "fp8_lora": lora("fp8", "fp8"), "fp8_plain": lambda: ops.gemm(a, plain, None, out=out),
            "skinny": lambda: ops.gemm(a, w.lora_A, None, out=t),
            "gemm_fp8_lora": lambda: ops.gemm_fp8(q, s, w, None, out=out, lora_t=t, lora_B=w.lora_B),
            "gemm_fp8": lambda: ops.gemm_fp8(q, s, plain, None, out=out)}
    w.compute = w.lora_compute = "fp8"
    assert ops.fp8_lora_route(a, w, out, "bias", buf) and ops.fp8_compute_route(a, plain, out)
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            ts[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in ts.items()}
    fl = 2.0 * M * N * K
    return {"M": M, "K": K, "N": N, "Rp": Rp, "ms": {k: round(v * 1e3, 4) for k, v in med.items()},
            "tflops": {k: round(fl / med[k] / 1e12, 1) for k in ("parent", "fp8_lora", "fp8_plain")},
            "fp8_lora_over_parent": round(med["parent"] / med["fp8_lora"], 4),
            "tail_and_skinny_ms": round((med["fp8_lora"] - med["fp8_plain"]) * 1e3, 4),
            "clock_ghz": {"gemm_fp8_lora": clock_of(arms["gemm_fp8_lora"]), "gemm_fp8": clock_of(arms["gemm_fp8"])}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "paths": {"parent": "skinny gemm_bf16 + dequant_fp8_scaled + copy of B' + gemm_bf16 over K + Rp",
                     "fp8_lora": "skinny gemm_bf16 + quant_rows_fp8 + gemm_fp8_lora",
                     "fp8_plain": "quant_rows_fp8 + gemm_fp8 (no adapters)"},
           "not_measured": "a whole Wan step with adapters", "shapes": []}
    for M in MS:
        for K, N in SHAPES:
            for Rp in RANKS:
                row = bench_shape(M, K, N, Rp, g, args.rounds, args.iters)
                print(json.dumps(row), flush=True)
                doc["shapes"].append(row)
                if args.out:                      # after every row: a run cut short keeps what it measured
                    with open(args.out, "w") as f:
                        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
