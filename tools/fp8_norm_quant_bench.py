#!/usr/bin/env python
"""The norm that quantises its own output (`ops.ln_modulate_quant_fp8`) against the two launches it replaces, at
the Wan-2.2 A14B width (C = 5120) and the 720p x 81 f / 480p x 81 f row counts (M = 75 600 / 32 760), in one process.

  (a) pair        : apexmi_ln_modulate2 (bf16 row out) + apexmi_quant_rows_fp8          7 bytes per element
  (b) fused       : apexmi_ln_modulate_quant_fp8 without `out`                          3 bytes per element
  (c) fused + row : apexmi_ln_modulate_quant_fp8 with `out` (run-time LoRA reads it)    5 bytes per element
timed with HIP events around `--iters` back-to-back calls, `--rounds` interleaved rounds, medians; the pair's own round-to-round
spread is reported next to every ratio.  Bytes are the algorithmic ones (computed from the shape; + 4 bytes of scale per row,
modulation vectors left out), TB/s = bytes / median time.  Inputs are random: zero-filled operands read high.  The outputs of (b)
and (c) are compared with (a)'s, bit for bit, at the timed size.  The live clock is the GEMM probe's (`apexmi_clk_enable`) over an
fp8 GEMM on the codes, read in a separate, untimed pass.  `--step` adds one Wan 720p x 81 f expert forward on `--layers` blocks in
fp8 mode without and with `fused_quant`.  Writes one JSON document (`--out`)."""
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
C = 5120
MS = [75600, 32760]
BF = torch.bfloat16


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


def bytes_moved(M, x_bytes, row):
    """algorithmic bytes of one call: x in, codes out, the bf16 row (written, and for the pair read again), 4 bytes of scale"""
    return {"pair": M * C * (x_bytes + 2 + 2 + 1) + 4 * M, "fused": M * C * (x_bytes + 1) + 4 * M,
            "fused_row": M * C * (x_bytes + 2 + 1) + 4 * M}[row]


def bench_norm(M, g, rounds, iters, x_dtype=BF):
    x = (torch.randn(M, C, generator=g, device=DEV) * 2.0).to(x_dtype)
    scale, shift = torch.randn(C, generator=g, device=DEV) * 0.3, torch.randn(C, generator=g, device=DEV) * 0.2
    xn, xn2 = torch.empty(M, C, dtype=BF, device=DEV), torch.empty(M, C, dtype=BF, device=DEV)
    q = {k: torch.empty(M, C, dtype=torch.uint8, device=DEV) for k in ("pair", "fused", "fused_row")}
    s = {k: torch.empty(M, dtype=torch.float32, device=DEV) for k in q}
    kw = dict(scale=scale, shift=shift, eps=1e-6)

    def pair():
        ops.ln_modulate(x, out=xn, **kw)
        ops.quant_rows_fp8(xn, out=q["pair"], scale_out=s["pair"])
    arms = {"pair": pair, "norm": lambda: ops.ln_modulate(x, out=xn, **kw),
            "quant": lambda: ops.quant_rows_fp8(xn, out=q["pair"], scale_out=s["pair"]),
            "fused": lambda: ops.ln_modulate_quant_fp8(x, codes=q["fused"], scale_out=s["fused"], **kw),
            "fused_row": lambda: ops.ln_modulate_quant_fp8(x, codes=q["fused_row"], scale_out=s["fused_row"], out=xn2, **kw)}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(q[k], q["pair"]) and torch.equal(s[k], s["pair"]) for k in ("fused", "fused_row")) and torch.equal(xn2, xn)
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["pair"]) - min(t["pair"])) / med["pair"]
    xb = x.element_size()
    by = {k: bytes_moved(M, xb, k) for k in ("pair", "fused", "fused_row")}
    by["norm"], by["quant"] = M * C * (xb + 2), M * C * 3 + 4 * M
    w = ops.Fp8Weight(torch.zeros(256, C, device=DEV).to(torch.float8_e4m3fn), torch.ones(1, device=DEV))
    row = {"M": M, "C": C, "x": str(x_dtype).replace("torch.", ""), "bit_identical_to_pair": bool(same),
           "ms": {k: round(v * 1e3, 4) for k, v in med.items()}, "bytes": by,
           "tb_per_s": {k: round(by[k] / med[k] / 1e12, 3) for k in med},
           "pair_round_spread": round(spread, 4),
           "fused_over_pair_speedup": round(med["pair"] / med["fused"], 4),
           "fused_row_over_pair_speedup": round(med["pair"] / med["fused_row"], 4),
           "byte_ratio": {"fused": round(by["fused"] / by["pair"], 4), "fused_row": round(by["fused_row"] / by["pair"], 4)},
           # "faster" = ahead of the pair by more than 10 % over the pair's own round-to-round spread
           "fused_is_faster": bool(med["pair"] / med["fused"] > 1.0 + 1.1 * spread),
           "fused_row_is_faster": bool(med["pair"] / med["fused_row"] > 1.0 + 1.1 * spread),
           "clock_ghz": clock_of(lambda: ops.gemm_fp8(q["fused"], s["fused"], w))}
    return row


def bench_step(layers, rounds):
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(num_layers=layers, device=DEV, dtype=BF).init_synthetic(2)
    m.pack()
    for name, p in m.named_parameters():           # the stand-in for a keep_fp8 load: every block Linear becomes an e4m3 record
        if m._fp8_resident_key(name) and p.dim() == 2:
            w = p.data.float()
            sc = (w.abs().max() / 448.0).reshape(1)
            p._fp8 = ops.Fp8Weight((w / sc).to(torch.float8_e4m3fn), sc)
    m._fp8_adopt()
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 16, 21, 90, 160, generator=g, device=DEV)
    enc = torch.randn(1, 512, 4096, generator=g, device=DEV).to(BF)
    ts = torch.tensor([500.0], device=DEV)
    modes = {"bf16": dict(on=False), "fp8": dict(on=True), "fp8_fused_quant": dict(on=True, fused_quant=True)}
    t = {k: [] for k in modes}
    outs = {}
    for k, kw in modes.items():                    # warm all three
        m.set_fp8_compute(**kw)
        outs[k] = m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)[0].float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, kw in modes.items():
            m.set_fp8_compute(**kw)
            t[k].append(timed(lambda: m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False), 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = (max(t["fp8"]) - min(t["fp8"])) / med["fp8"]
    return {"workload": f"wan2.2-a14b 720p x 81f, one expert forward on {layers} blocks, resident fp8 weights",
            "s_per_forward": {k: round(v, 4) for k, v in med.items()}, "fp8_round_spread": round(spread, 4),
            "fp8_over_bf16_speedup": round(med["bf16"] / med["fp8"], 4),
            "fused_quant_over_fp8_speedup": round(med["fp8"] / med["fp8_fused_quant"], 4),
            "fused_quant_over_bf16_speedup": round(med["bf16"] / med["fp8_fused_quant"], 4),
            "fused_quant_bit_identical_to_fp8": bool(torch.equal(outs["fp8_fused_quant"], outs["fp8"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--f32", action="store_true", help="also time the float-x form (the f32 residual stream)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "arms": {"pair": "ln_modulate + quant_rows_fp8", "fused": "ln_modulate_quant_fp8, no bf16 row",
                    "fused_row": "ln_modulate_quant_fp8 with the bf16 row"}, "shapes": []}
    for M in MS:
        for dt in (BF, torch.float32) if args.f32 else (BF,):
            row = bench_norm(M, g, args.rounds, args.iters, dt)
            print(json.dumps(row), flush=True)
            doc["shapes"].append(row)
    if args.step:
        doc["wan_step"] = bench_step(args.layers, args.rounds)
        print(json.dumps(doc["wan_step"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
