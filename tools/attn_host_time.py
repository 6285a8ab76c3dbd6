#!/usr/bin/env python
"""Per-call host time of the attention wrappers at launch-bound shapes, where the Python and C front end dominates the call.

One process is one run of one checkout: `python tools/attn_host_time.py [--root CHECKOUT]` imports the package of CHECKOUT
(default: this repository) and prints one JSON line {case: us per call}.  A run is the wall time per call over --calls calls after
--warmup calls, with one synchronise at the end.  Compare checkouts by alternating runs of this tool (profiles/attn_host_refactor.md)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--calls", type=int, default=2000)
ap.add_argument("--warmup", type=int, default=200)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402

import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import ops  # noqa: E402

DEV, BF = "cuda", torch.bfloat16
g = torch.Generator().manual_seed(5)
R = lambda *shape: torch.randn(shape, generator=g).to(device=DEV, dtype=BF)     # noqa: E731

q, k, v = R(1, 2, 64, 64), R(1, 2, 64, 64), R(1, 2, 64, 64)
pq, pk, pv = R(128, 2, 64), R(128, 2, 64), R(128, 2, 64)
cu = torch.tensor([0, 64, 128], dtype=torch.int32, device=DEV)
wq, wk, wv = R(1, 1, 64, 256), R(1, 1, 64, 256), R(1, 1, 64, 256)
rq, rk, rvt = R(1, 2, 256, 128), R(1, 2, 256, 128), R(1, 2, 128, 256)
rout = torch.empty(1, 256, 2, 128, dtype=BF, device=DEV)
CASES = {
    "masked 1x2x64x64": lambda: ops.attention_masked(q, k, v),
    "masked 1x2x64x64 lse": lambda: ops.attention_masked(q, k, v, return_lse=True),
    "varlen 2x64 D64": lambda: ops.attention_varlen(pq, pk, pv, cu, cu, 64, 64),
    "wide 1x1x64x256": lambda: ops.attention_wide(wq, wk, wv),
    "prepared 1x2x256x128": lambda: ops.attention_prepared(rq, rk, rvt, rout, 256),
}

out = {"ops": ops.__file__}
for name, fn in CASES.items():
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.calls):
        fn()
    torch.cuda.synchronize()
    out[name] = round((time.perf_counter() - t0) / args.calls * 1e6, 3)
print(json.dumps(out), flush=True)
