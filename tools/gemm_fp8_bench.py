#!/usr/bin/env python
"""The opt-in FP8 GEMM against the path it replaces, at the Wan-2.2 A14B block shapes, in one process.

For every (M, K -> N) of the block Linears at 720p x 81 f (M = 75 600) and 480p x 81 f (M = 32 760), with a resident e4m3 weight:
  (a) parent path : apexmi_dequant_fp8_scaled into the stream scratch + apexmi_gemm_bf16      (`Fp8Weight.compute = "bf16"`)
  (b) fp8 path    : apexmi_quant_rows_fp8 of the activations + apexmi_gemm_fp8                 (`Fp8Weight.compute = "fp8"`)
timed with HIP events around `--iters` back-to-back calls, `--rounds` interleaved rounds, medians.  Operands are random (N(0,1)
activations, N(0, 0.02^2) weights): zero-filled operands read high.  TFLOP/s count 2 M N K for both, so the ratio b/a is the
speed-up of the whole Linear.  The parts of both paths are timed on their own as well, and the live GEMM clock
(`apexmi_clk_enable`) of each path's GEMM kernel is read in a separate, untimed pass.  `--step` adds one Wan 720p x 81 f expert
forward on `--layers` blocks with the mode off and on.  Writes one JSON document (`--out`)."""
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


def fp8_weight(N, K, g):
    w = torch.randn(N, K, generator=g, device=DEV) * 0.02
    s = w.abs().amax(dim=1) / 448.0
    return ops.Fp8Weight((w / s.view(-1, 1)).to(torch.float8_e4m3fn), s)


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


def bench_shape(M, K, N, g, rounds, iters):
    a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = fp8_weight(N, K, g)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    wb = torch.empty(N, K, dtype=torch.bfloat16, device=DEV)
    q, s = ops.quant_rows_fp8(a)

    def path(mode):
        def run():
            w.compute = mode
            ops.gemm(a, w, None, out=out)
        return run
    arms = {"parent": path("bf16"), "fp8": path("fp8"), "dequant": lambda: w.dequant(out=wb), "gemm_bf16": lambda: ops.gemm(a, wb, None, out=out),
            "quant": lambda: ops.quant_rows_fp8(a, out=q, scale_out=s), "gemm_fp8": lambda: ops.gemm_fp8(q, s, w, None, out=out)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    fl = 2.0 * M * N * K
    row = {"M": M, "K": K, "N": N, "ms": {k: round(v * 1e3, 4) for k, v in med.items()},
           "tflops": {k: round(fl / med[k] / 1e12, 1) for k in ("parent", "fp8", "gemm_bf16", "gemm_fp8")},
           "fp8_over_parent": round(med["parent"] / med["fp8"], 4),
           "clock_ghz": {"gemm_bf16": clock_of(arms["gemm_bf16"]), "gemm_fp8": clock_of(arms["gemm_fp8"])}}
    w.compute = "bf16"
    return row


def bench_step(layers, rounds):
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(num_layers=layers, device=DEV, dtype=torch.bfloat16).init_synthetic(2)
    m.pack()
    for name, p in m.named_parameters():           # the stand-in for a keep_fp8 load: every block Linear becomes an e4m3 record
        if m._fp8_resident_key(name) and p.dim() == 2:
            w = p.data.float()
            s = (w.abs().max() / 448.0).reshape(1)
            p._fp8 = ops.Fp8Weight((w / s).to(torch.float8_e4m3fn), s)
    m._fp8_adopt()
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 16, 21, 90, 160, generator=g, device=DEV)
    enc = torch.randn(1, 512, 4096, generator=g, device=DEV).to(torch.bfloat16)
    ts = torch.tensor([500.0], device=DEV)
    t = {"off": [], "on": []}
    outs = {}
    for k in ("off", "on"):                        # warm both
        m.set_fp8_compute(k == "on")
        outs[k] = m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)[0].float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k in t:
            m.set_fp8_compute(k == "on")
            t[k].append(timed(lambda: m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False), 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"workload": f"wan2.2-a14b 720p x 81f, one expert forward on {layers} blocks, resident fp8 weights",
            "s_per_forward": {k: round(v, 4) for k, v in med.items()}, "on_over_off_speedup": round(med["off"] / med["on"], 4),
            "rel_l2_on_vs_off": float((outs["on"] - outs["off"]).norm() / outs["off"].norm())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "paths": {"parent": "dequant_fp8_scaled + gemm_bf16", "fp8": "quant_rows_fp8 + gemm_fp8"}, "shapes": []}
    for M in MS:
        for K, N in SHAPES:
            row = bench_shape(M, K, N, g, args.rounds, args.iters)
            print(json.dumps(row), flush=True)
            doc["shapes"].append(row)
    if args.step:
        doc["wan_step"] = bench_step(args.layers, args.rounds)
        print(json.dumps(doc["wan_step"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
