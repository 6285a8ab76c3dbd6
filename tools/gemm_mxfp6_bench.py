#!/usr/bin/env python
"""The opt-in MXFP6 GEMM against the bf16 path it replaces and the two other block-format modes, at the Wan-2.2 A14B
block shapes, in one process.

For every (M, K -> N) of the block Linears at 720p x 81 f (M = 75 600) and 480p x 81 f (M = 32 760), with a bf16 weight:
  (a) bf16      : the shipped `ops.gemm` on the bf16 weight — what a bf16 model runs, the baseline
  (b) fp6_pair  : `ops.quant_blocks_mxfp6` of the activations + `ops.gemm_mxfp6` — what the mode costs per Linear
  (c) gemm_fp6  : `ops.gemm_mxfp6` alone, also in PFLOP/s
  (d) fp4_pair  : `ops.quant_blocks_mxfp4` + `ops.gemm_mxfp4`
  (e) fp8_pair  : `ops.quant_rows_fp8` + `ops.gemm_fp8` on an e4m3 copy of the weight
timed with HIP events around `--iters` back-to-back calls, `--rounds` interleaved rounds, medians.  Operands are random (N(0,1)
activations, N(0, 0.02^2) weights): zero-filled operands read high.  FLOP counts are 2 M N K for every arm.  Each row also carries the
rel-L2 error of the fp6, fp4 and fp8 outputs against the bf16 kernel's output on the first 512 rows.  The live GEMM clock
(`apexmi_clk_enable`) of each GEMM kernel is read in ONE separate, untimed call after the timed rounds: it is not the clock of the timed
iterations, and a table that quotes it says so.  `--step` adds one Wan 720p x 81 f expert forward on `--layers` blocks with the modes
off, fp6 on all seven Linears, fp4 on all seven, and the mix "fp6 attention projections + fp4 FFN pair", with time and rel-L2 against
the mode-off forward.  Writes one JSON document (`--out`)."""
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
ATTENTION, FFN_PAIR = ("qkv", "attn_out", "cross_q", "cross_kv", "cross_out"), ("ffn_up", "ffn_down")


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
    w32 = torch.randn(N, K, generator=g, device=DEV) * 0.02
    w = w32.to(torch.bfloat16)
    s8 = w32.abs().amax(dim=1) / 448.0
    w8 = ops.Fp8Weight((w32 / s8.view(-1, 1)).to(torch.float8_e4m3fn), s8)
    w8.compute = "fp8"
    del w32
    w6, w4 = ops.Mxfp6Weight.from_bf16(w), ops.Mxfp4Weight.from_bf16(w)
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    q6, s6 = ops.quant_blocks_mxfp6(a)
    q4, s4 = ops.quant_blocks_mxfp4(a)
    q8, sc8 = ops.quant_rows_fp8(a)

    def fp6_pair():
        ops.quant_blocks_mxfp6(a, out=q6, scale_out=s6)
        ops.gemm_mxfp6(q6, s6, w6, None, out=out)

    def fp4_pair():
        ops.quant_blocks_mxfp4(a, out=q4, scale_out=s4)
        ops.gemm_mxfp4(q4, s4, w4, None, out=out)

    def fp8_pair():
        ops.quant_rows_fp8(a, out=q8, scale_out=sc8)
        ops.gemm_fp8(q8, sc8, w8, None, out=out)

    arms = {"bf16": lambda: ops.gemm(a, w, None, out=out), "fp6_pair": fp6_pair,
            "gemm_fp6": lambda: ops.gemm_mxfp6(q6, s6, w6, None, out=out), "fp4_pair": fp4_pair, "fp8_pair": fp8_pair,
            "quant_fp6": lambda: ops.quant_blocks_mxfp6(a, out=q6, scale_out=s6),
            "gemm_fp4": lambda: ops.gemm_mxfp4(q4, s4, w4, None, out=out), "gemm_fp8": lambda: ops.gemm_fp8(q8, sc8, w8, None, out=out)}
    # the approximation itself, on the first rows: each mode's output against the bf16 kernel's
    R = min(M, 512)
    ref = ops.gemm(a[:R], w).float()
    rel = lambda y: float((y.float() - ref).norm() / ref.norm())          # noqa: E731
    err = {"fp6": rel(ops.gemm_mxfp6(q6[:R], s6[:R], w6)), "fp4": rel(ops.gemm_mxfp4(q4[:R], s4[:R], w4)), "fp8": rel(ops.gemm_fp8(q8[:R], sc8[:R], w8))}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    fl = 2.0 * M * N * K
    return {"M": M, "K": K, "N": N, "ms": {k: round(v * 1e3, 4) for k, v in med.items()},
            "pflops": {k: round(fl / med[k] / 1e15, 3) for k in ("bf16", "fp6_pair", "gemm_fp6", "fp4_pair", "gemm_fp4", "fp8_pair", "gemm_fp8")},
            "fp6_pair_over_bf16": round(med["bf16"] / med["fp6_pair"], 4), "fp6_pair_over_fp8_pair": round(med["fp8_pair"] / med["fp6_pair"], 4),
            "fp6_pair_over_fp4_pair": round(med["fp4_pair"] / med["fp6_pair"], 4), "rel_l2_vs_bf16_kernel": {k: round(v, 5) for k, v in err.items()},
            "clock_ghz": {k: clock_of(arms[k]) for k in ("bf16", "gemm_fp6", "gemm_fp4", "gemm_fp8")}}


def bench_step(layers, rounds):
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(num_layers=layers, device=DEV, dtype=torch.bfloat16).init_synthetic(2)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 16, 21, 90, 160, generator=g, device=DEV)
    enc = torch.randn(1, 512, 4096, generator=g, device=DEV).to(torch.bfloat16)
    ts = torch.tensor([500.0], device=DEV)

    def switch(fp6, fp4):
        m.set_fp6_compute(False)
        m.set_fp4_compute(False)
        if fp6 is not None:
            m.set_fp6_compute(True, linears=fp6 or None)
        if fp4 is not None:
            m.set_fp4_compute(True, linears=fp4 or None)

    modes = {"off": lambda: switch(None, None), "fp6": lambda: switch((), None), "fp4": lambda: switch(None, ()),
             "fp6_attention_fp4_ffn": lambda: switch(ATTENTION, FFN_PAIR)}
    t, outs = {k: [] for k in modes}, {}
    for k, sw in modes.items():                # warm every mode
        sw()
        outs[k] = m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)[0].float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, sw in modes.items():
            sw()
            torch.cuda.synchronize()
            t[k].append(timed(lambda: m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False), 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    on = [k for k in modes if k != "off"]
    return {"workload": f"wan2.2-a14b 720p x 81f, one expert forward on {layers} blocks, synthetic bf16 weights",
            "s_per_forward": {k: round(v, 4) for k, v in med.items()},
            "speedup_over_off": {k: round(med["off"] / med[k], 4) for k in on},
            "rel_l2_vs_off": {k: float((outs[k] - outs["off"]).norm() / outs["off"].norm()) for k in on}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "arms": {"bf16": "ops.gemm on the bf16 weight", "fp6_pair": "quant_blocks_mxfp6 + gemm_mxfp6", "gemm_fp6": "gemm_mxfp6 alone",
                    "fp4_pair": "quant_blocks_mxfp4 + gemm_mxfp4", "fp8_pair": "quant_rows_fp8 + gemm_fp8 on an e4m3 copy of the weight"},
           "shapes": []}
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
