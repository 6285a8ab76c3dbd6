#!/usr/bin/env python
"""Opt-in MXFP4 compute on Flux against the shipped bf16 launches, at the Flux-Dev 1024^2 shapes (S = 4096 image +
512 text rows, dim 3072, 24 heads, MLP 12288), in one process.

Per launch class of a block — the QKV pair with the fused q/k/v epilogue, the to_out pair, the FF-up pair, the FF-down pair (double
block: image and text stream in one grouped launch), the single block's fused QKV + MLP-up launch and its proj_out — three arms:
  bf16       the shipped launch on bf16 weights (`gemm_grouped`; the QKV classes `gemm_grouped_qkv`; proj_out `gemm`)
  fp4        `quant_blocks_mxfp4` of the joint activation buffer + the fp4 launch (`gemm_mxfp4_grouped`, `gemm_mxfp4_grouped_qkv`,
             `gemm_mxfp4`): what the model runs
  fp4_gemm   the fp4 launch alone, on codes quantised beforehand
timed with HIP events around `--iters` back-to-back calls, arms interleaved over `--rounds` rounds, medians.  Operands are random
(N(0,1) activations, N(0, 0.02^2) weights): zero-filled operands read high.  The live GEMM clock (`apexmi_clk_enable`) of each arm's
GEMM kernel is read in a separate, untimed pass.  `--forward` adds a whole Flux-Dev-depth forward (19 + 38 blocks, synthetic
weights) with the mode off, on, and on for ("ffn_up", "ffn_down") only, with the rel-L2 of each against the off forward.  Writes one
JSON document (`--out`, default profiles/flux_fp4_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import lib, ops  # noqa: E402

DEV = torch.device("cuda", 0)
BF = torch.bfloat16
S_IMG, S_TXT, H = 4096, 512, 24
DIM, MLP = H * 128, 4 * H * 128
S = S_IMG + S_TXT


def pair_of(N, K, g):
    """(bf16 weight, its MXFP4 record)"""
    w = (torch.randn(N, K, generator=g, device=DEV) * 0.02).to(BF)
    return w, ops.Mxfp4Weight.from_bf16(w)


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


def launch_classes(g):
    """{class: (flops, {arm: fn}, {arm: fn of the GEMM launch alone, for the clock})}"""
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)          # noqa: E731
    XN, FFH, CAT = r(S, DIM).to(BF), r(S, MLP).to(BF), r(S, DIM + MLP).to(BF)
    X, Y = r(S, DIM).to(BF), torch.empty(S, DIM, device=DEV, dtype=BF)
    UP = torch.empty(S, MLP, device=DEV, dtype=BF)
    att = CAT[:, :DIM]
    Q, K_ = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    VT = torch.zeros(H, 128, S, device=DEV, dtype=BF)
    ang = torch.rand(S, 64, generator=g, device=DEV) * 6.283
    rope = torch.stack([ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)]).contiguous().float()
    ops.rope_pairs(rope, trusted=True)                               # the compact copy the bf16 fused epilogue reads
    nw = [r(128).to(BF) * 0.2 + 1 for _ in range(4)]
    gate = [r(DIM) * 1e-2 for _ in range(2)]
    img, txt = slice(S_TXT, None), slice(0, S_TXT)
    bias = lambda n: r(n).to(BF) * 0.1                               # noqa: E731
    out = {}

    def quant(src):
        qa, sa = ops._act_scratch_mx(ops._MXFP4, src.device, src.shape[0], src.shape[1])
        return ops.quant_blocks_mxfp4(src, out=qa, scale_out=sa)

    def three(flops, bf16, fp4_gemm, src):
        held = ops.quant_blocks_mxfp4(src)
        return (flops, {"bf16": bf16, "fp4": lambda: fp4_gemm(*quant(src)), "fp4_gemm": lambda: fp4_gemm(*held)},
                {"bf16": bf16, "fp4": lambda: fp4_gemm(*held)})

    def pair_class(name, src, N, Kk, outs, epi, gated):
        (wa, ra), (wb, rb) = pair_of(N, Kk, g), pair_of(N, Kk, g)
        bs = [bias(N), bias(N)]
        kw = dict(gate_list=gate, residual_list=[X[img], X[txt]]) if gated else {}

        def bf16():
            ops.gemm_grouped([src[img], src[txt]], [wa, wb], bs, outs, epilogue=epi, **kw)

        def fp4_gemm(qa, sa):
            ops.gemm_mxfp4_grouped([qa[img], qa[txt]], [sa[img], sa[txt]], [ra, rb], bs, outs, epilogue=epi, **kw)
        out[name] = three(2.0 * S * N * Kk, bf16, fp4_gemm, src)

    # the QKV pair of a double block, fused q/k/v epilogue on both sides
    (wa, ra), (wb, rb) = pair_of(3 * DIM, DIM, g), pair_of(3 * DIM, DIM, g)
    bq = [bias(3 * DIM), bias(3 * DIM)]
    qkv_args = ([None, None], "bias", [1, 1], [nw[0], nw[2]], [nw[1], nw[3]], [S_TXT, 0], H, 1e-6, rope, Q, K_, VT)
    out["qkv_pair_fused"] = three(
        2.0 * S * 3 * DIM * DIM, lambda: ops.gemm_grouped_qkv([XN[img], XN[txt]], [wa, wb], bq, *qkv_args),
        lambda qa, sa: ops.gemm_mxfp4_grouped_qkv([qa[img], qa[txt]], [sa[img], sa[txt]], [ra, rb], bq, *qkv_args), XN)
    pair_class("to_out_pair", att, DIM, DIM, [Y[img], Y[txt]], "gate_res", True)
    pair_class("ff_up_pair", XN, MLP, DIM, [UP[img], UP[txt]], "gelu", False)
    pair_class("ff_down_pair", FFH, DIM, MLP, [Y[img], Y[txt]], "gate_res", True)

    # the single block's fused QKV + MLP-up launch
    (wq, rq), (wm, rm) = pair_of(3 * DIM, DIM, g), pair_of(MLP, DIM, g)
    bsm = [bias(3 * DIM), bias(MLP)]
    s_args = ([None, CAT[:, DIM:]], ["bias", "gelu"], [1, 0], [nw[0], None], [nw[1], None], [0, 0], H, 1e-6, rope, Q, K_, VT)
    out["single_qkv_mlp_fused"] = three(
        2.0 * S * (3 * DIM + MLP) * DIM, lambda: ops.gemm_grouped_qkv([XN, XN], [wq, wm], bsm, *s_args),
        lambda qa, sa: ops.gemm_mxfp4_grouped_qkv([qa, qa], [sa, sa], [rq, rm], bsm, *s_args), XN)

    # the single block's proj_out: one problem, K = 15360
    wo, ro = pair_of(DIM, DIM + MLP, g)
    bo = bias(DIM)
    out["single_proj_out"] = three(
        2.0 * S * DIM * (DIM + MLP), lambda: ops.gemm(CAT, wo, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X),
        lambda qa, sa: ops.gemm_mxfp4(qa, sa, ro, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X), CAT)
    return out


def bench_classes(g, rounds, iters):
    rows = []
    for name, (flops, arms, gemms) in launch_classes(g).items():
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                t[k].append(timed(fn, iters))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"class": name, "ms": {k: round(v * 1e3, 4) for k, v in med.items()},
               "tflops": {k: round(flops / v / 1e12, 1) for k, v in med.items()},
               "fp4_over_bf16": round(med["bf16"] / med["fp4"], 4), "fp4_gemm_over_bf16": round(med["bf16"] / med["fp4_gemm"], 4),
               "clock_ghz": {k: clock_of(fn) for k, fn in gemms.items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_forward(double, single, rounds):
    from apex_studio_amd.engine_flux import latent_image_ids
    from apex_studio_amd.flux import FluxTransformer2DModel
    m = FluxTransformer2DModel(num_layers=double, num_single_layers=single, guidance_embeds=True, device=DEV, dtype=BF).init_synthetic(2)
    m.pack()
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)          # noqa: E731
    inp = dict(hidden_states=r(1, S_IMG, 64), encoder_hidden_states=r(1, S_TXT, 4096), pooled_projections=r(1, 768),
               timestep=torch.tensor([0.5], device=DEV), guidance=torch.tensor([3.5], device=DEV), img_ids=latent_image_ids(64, 64, device=DEV),
               txt_ids=torch.zeros(S_TXT, 3, device=DEV))
    fwd = lambda: m(return_dict=False, **inp)[0]                           # noqa: E731
    arms = [("off", lambda: m.set_fp4_compute(False)), ("on", lambda: m.set_fp4_compute(True)),
            ("ffn_only", lambda: m.set_fp4_compute(True, linears=("ffn_up", "ffn_down")))]
    t, outs, extra = {k: [] for k, _ in arms}, {}, {}
    for k, setup in arms:                                # warm every arm; the switch (quantising the weights) is outside the timing
        setup()
        outs[k] = fwd().float()
        extra[k] = m._fp4_bytes
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, setup in arms:
            setup()
            torch.cuda.synchronize()
            t[k].append(timed(fwd, 1))
    m.set_fp4_compute(False)
    med = {k: statistics.median(v) for k, v in t.items()}
    rel = lambda a: float((outs[a] - outs["off"]).norm() / outs["off"].norm())  # noqa: E731
    return {"workload": f"flux-dev 1024^2 (S {S_IMG} + {S_TXT}), one forward on {double} + {single} blocks, synthetic weights",
            "ms_per_forward": {k: round(v * 1e3, 3) for k, v in med.items()},
            "speedup_over_off": {k: round(med["off"] / v, 4) for k, v in med.items()},
            "rel_l2_vs_off": {"on": rel("on"), "ffn_only": rel("ffn_only")},
            "finite": {k: bool(torch.isfinite(v).all()) for k, v in outs.items()},
            "fp4_record_bytes": extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--double", type=int, default=19)
    ap.add_argument("--single", type=int, default=38)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_fp4_bench.json"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "shape": {"s_img": S_IMG, "s_txt": S_TXT, "dim": DIM, "heads": H, "mlp": MLP},
           "arms": {"bf16": "gemm_grouped / gemm_grouped_qkv (fused q/k/v) / gemm on bf16 weights",
                    "fp4": "quant_blocks_mxfp4 + gemm_mxfp4_grouped / gemm_mxfp4_grouped_qkv (fused q/k/v) / gemm_mxfp4",
                    "fp4_gemm": "the fp4 launch alone, on codes quantised beforehand"},
           "classes": bench_classes(g, args.rounds, args.iters)}
    if args.forward:
        doc["forward"] = bench_forward(args.double, args.single, args.rounds)
        print(json.dumps(doc["forward"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
