#!/usr/bin/env python
"""Per-step cost of GGUF block weights RESIDENT in HBM (weights.load_checkpoint_into(keep_quantized=True)) on the Wan-2.2 A14B
720p x 81f expert forward, against the same model with bf16 weights (the dequantise-at-load form), interleaved in one process.

The resident model is the synthetic stand-in for a keep_quantized load: every block Linear becomes an ops.GgufWeight of random
blocks of `--type` with finite scales (the time does not depend on the values), then `_fp8_adopt()` fuses the projections' records
and releases the bf16 storage.  Prints one JSON line: seconds per forward of both (median, min, max), the ratio, and the HBM bytes
one expert's block weights hold in each mode."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import gguf_file as G, ops  # noqa: E402

DEV = torch.device("cuda", 0)


def quantise_blocks(model, t):
    _, blk, bs = G.TYPES[t]
    offs = {G.Q6_K: [208]}.get(t, [0, 2] if t in (G.Q4_1, G.Q5_1, G.Q4_K, G.Q5_K) else [0])
    g = torch.Generator(device=DEV).manual_seed(3)
    for name, p in model.named_parameters():
        if model._fp8_resident_key(name) and p.dim() == 2:
            N, K = p.shape
            b = torch.randint(0, 256, (N * K // blk, bs), generator=g, device=DEV, dtype=torch.uint8)
            for o in offs:                      # f16 scale fields: small finite magnitudes
                b[:, o + 1] = (b[:, o + 1] & 0x83) | 0x10
            p._fp8 = ops.GgufWeight([(t, N, b.reshape(-1))], K)
    return model._fp8_adopt()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--type", default="Q4_K")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    t = {n: i for i, (n, _, _) in G.TYPES.items()}[args.type]
    from apex_studio_amd.wan import WanTransformer3DModel
    a = WanTransformer3DModel(device=DEV, dtype=torch.bfloat16).init_synthetic(2)
    a.pack()
    b = WanTransformer3DModel(device=DEV, dtype=torch.bfloat16).init_synthetic(2)
    b.pack()
    bf16_bytes = sum(p.numel() * 2 for n, p in a.named_parameters() if a._fp8_resident_key(n) and p.dim() == 2)
    quantise_blocks(b, t)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 16, 21, 90, 160, generator=g, device=DEV)
    enc = torch.randn(1, 512, 4096, generator=g, device=DEV).to(torch.bfloat16)
    ts = torch.tensor([500.0], device=DEV)
    times = {"bf16": [], "resident": []}
    models = {"bf16": a, "resident": b}
    for m in models.values():                   # warm both
        m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, m in models.items():
            t0 = time.perf_counter()
            m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    med = {k: statistics.median(v) for k, v in times.items()}
    doc = {"workload": "wan2.2-a14b 720p x 81f, one expert forward", "ggml_type": args.type, "rounds": args.rounds,
           "s_per_step": {k: {"median": round(med[k], 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()},
           "resident_over_bf16": round(med["resident"] / med["bf16"], 4),
           "block_weight_bytes": {"bf16": bf16_bytes, "resident": int(b._fp8_bytes)}, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
