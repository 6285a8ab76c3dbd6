#!/usr/bin/env python
"""Opt-in FP8 compute on Flux against the shipped bf16 launches, at the Flux-Dev 1024^2 shapes (S = 4096 image +
512 text rows, dim 3072, 24 heads, MLP 12288), in one process.

Per launch class of a block — the QKV pair, the to_out pair, the FF-up pair, the FF-down pair (double block: image and text
stream in one grouped launch), the single block's QKV + MLP-up launch and its proj_out — three arms, each with every launch it
needs counted in:
  bf16       the shipped launch on bf16 weights (`gemm_grouped`; the QKV classes with the fused q/k/v epilogue, `gemm_grouped_qkv`)
  fp8        `quant_rows_fp8` of the joint activation buffer + `gemm_fp8_grouped` (+ `qkv_prepare` for the QKV classes: two-pass)
  fp8_fused  `quant_rows_fp8` + `gemm_fp8_grouped_qkv` (QKV classes only)
timed with HIP events around `--iters` back-to-back calls, arms interleaved over `--rounds` rounds, medians.  Operands are random
(N(0,1) activations, N(0, 0.02^2) weights quantised per tensor): zero-filled operands read high.  The live GEMM clock
(`apexmi_clk_enable`) of each arm's GEMM kernel is read in a separate, untimed pass.  `--forward` adds a whole Flux-Dev-depth
forward (19 + 38 blocks, synthetic weights) in the shipped bf16 mode, with resident fp8 weights and bf16 compute, and in fp8
compute without and with `fused_quant`.  Writes one JSON document (`--out`, default profiles/flux_fp8_bench.json)."""
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
    """(bf16 weight, its per-tensor e4m3 record with compute = "fp8")"""
    w = torch.randn(N, K, generator=g, device=DEV) * 0.02
    s = (w.abs().max() / 448.0).reshape(1)
    rec = ops.Fp8Weight((w / s).to(torch.float8_e4m3fn), s)
    rec.compute = "fp8"
    return rec.dequant(), rec


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
    QKV, UP = torch.empty(S, 3 * DIM, device=DEV, dtype=BF), torch.empty(S, MLP, device=DEV, dtype=BF)
    att = CAT[:, :DIM]
    Q, K_ = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    VT = torch.zeros(H, 128, S, device=DEV, dtype=BF)
    ang = torch.rand(S, 64, generator=g, device=DEV) * 6.283
    rope = torch.stack([ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)]).contiguous().float()
    nw = [r(128).to(BF) * 0.2 + 1 for _ in range(4)]
    gate = [r(DIM) * 1e-2 for _ in range(2)]
    img, txt = slice(S_TXT, None), slice(0, S_TXT)
    bias = lambda n: r(n).to(BF) * 0.1                               # noqa: E731
    out = {}

    def quant(src):
        qa, sa = ops._act_scratch(src.device, src.shape[0], src.shape[1])
        return ops.quant_rows_fp8(src, out=qa, scale_out=sa)

    def prepare(split):
        ops.qkv_prepare(QKV[:, :DIM], QKV[:, DIM:2 * DIM], QKV[:, 2 * DIM:], H, Q, K_, VT, wq=nw[0], wk=nw[1],
                        wq2=nw[2] if split else None, wk2=nw[3] if split else None, split=split, eps=1e-6, rope=rope,
                        rope_mode=lib.ROPE_INTERLEAVED)

    def pair_class(name, src, N, Kk, outs, epi, gated):
        (wa, ra), (wb, rb) = pair_of(N, Kk, g), pair_of(N, Kk, g)
        bs = [bias(N), bias(N)]
        kw = dict(gate_list=gate, residual_list=[X[img], X[txt]]) if gated else {}

        def bf16():
            ops.gemm_grouped([src[img], src[txt]], [wa, wb], bs, outs, epilogue=epi, **kw)

        def fp8_gemm(qa, sa):
            ops.gemm_fp8_grouped([qa[img], qa[txt]], [sa[img], sa[txt]], [ra, rb], bs, outs, epilogue=epi, **kw)

        def fp8():
            fp8_gemm(*quant(src))
        held = ops.quant_rows_fp8(src)
        out[name] = (2.0 * S * N * Kk, {"bf16": bf16, "fp8": fp8}, {"bf16": bf16, "fp8": lambda: fp8_gemm(*held)})

    # the QKV pair of a double block
    (wa, ra), (wb, rb) = pair_of(3 * DIM, DIM, g), pair_of(3 * DIM, DIM, g)
    bq = [bias(3 * DIM), bias(3 * DIM)]
    qkv_args = ([None, None], "bias", [1, 1], [nw[0], nw[2]], [nw[1], nw[3]], [S_TXT, 0], H, 1e-6, rope, Q, K_, VT)

    def d_bf16():
        ops.gemm_grouped_qkv([XN[img], XN[txt]], [wa, wb], bq, *qkv_args)

    def d_fp8_gemm(qa, sa):
        ops.gemm_fp8_grouped([qa[img], qa[txt]], [sa[img], sa[txt]], [ra, rb], bq, [QKV[img], QKV[txt]])

    def d_fp8():
        d_fp8_gemm(*quant(XN))
        prepare(S_TXT)

    def d_fused_gemm(qa, sa):
        ops.gemm_fp8_grouped_qkv([qa[img], qa[txt]], [sa[img], sa[txt]], [ra, rb], bq, *qkv_args)
    held = ops.quant_rows_fp8(XN)
    out["qkv_pair"] = (2.0 * S * 3 * DIM * DIM, {"bf16": d_bf16, "fp8": d_fp8, "fp8_fused": lambda: d_fused_gemm(*quant(XN))},
                       {"bf16": d_bf16, "fp8": lambda: d_fp8_gemm(*held), "fp8_fused": lambda: d_fused_gemm(*held)})
    pair_class("to_out_pair", att, DIM, DIM, [Y[img], Y[txt]], "gate_res", True)
    pair_class("ff_up_pair", XN, MLP, DIM, [UP[img], UP[txt]], "gelu", False)
    pair_class("ff_down_pair", FFH, DIM, MLP, [Y[img], Y[txt]], "gate_res", True)

    # the single block's QKV + MLP-up launch
    (wq, rq), (wm, rm) = pair_of(3 * DIM, DIM, g), pair_of(MLP, DIM, g)
    bsm = [bias(3 * DIM), bias(MLP)]
    s_args = ([None, CAT[:, DIM:]], ["bias", "gelu"], [1, 0], [nw[0], None], [nw[1], None], [0, 0], H, 1e-6, rope, Q, K_, VT)

    def s_bf16():
        ops.gemm_grouped_qkv([XN, XN], [wq, wm], bsm, *s_args)

    def s_fp8_gemm(qa, sa):
        ops.gemm_fp8_grouped([qa, qa], [sa, sa], [rq, rm], bsm, [QKV, CAT[:, DIM:]], epilogue=["bias", "gelu"])

    def s_fp8():
        s_fp8_gemm(*quant(XN))
        prepare(0)

    def s_fused_gemm(qa, sa):
        ops.gemm_fp8_grouped_qkv([qa, qa], [sa, sa], [rq, rm], bsm, *s_args)
    out["single_qkv_mlp"] = (2.0 * S * (3 * DIM + MLP) * DIM, {"bf16": s_bf16, "fp8": s_fp8, "fp8_fused": lambda: s_fused_gemm(*quant(XN))},
                             {"bf16": s_bf16, "fp8": lambda: s_fp8_gemm(*held), "fp8_fused": lambda: s_fused_gemm(*held)})

    # the single block's proj_out: one problem, K = 15360
    wo, ro = pair_of(DIM, DIM + MLP, g)
    bo = bias(DIM)
    heldc = ops.quant_rows_fp8(CAT)
    out["single_proj_out"] = (
        2.0 * S * DIM * (DIM + MLP),
        {"bf16": lambda: ops.gemm(CAT, wo, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X),
         "fp8": lambda: ops.gemm(CAT, ro, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X)},
        {"bf16": lambda: ops.gemm(CAT, wo, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X),
         "fp8": lambda: ops.gemm_fp8(heldc[0], heldc[1], ro, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X)})
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
               "fp8_over_bf16": round(med["bf16"] / med["fp8"], 4), "clock_ghz": {k: clock_of(fn) for k, fn in gemms.items()}}
        if "fp8_fused" in med:
            row["fp8_fused_over_bf16"] = round(med["bf16"] / med["fp8_fused"], 4)
            row["fp8_fused_over_fp8_two_pass"] = round(med["fp8"] / med["fp8_fused"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_forward(double, single, rounds):
    from apex_studio_amd.flux import FluxTransformer2DModel
    m = FluxTransformer2DModel(num_layers=double, num_single_layers=single, guidance_embeds=True, device=DEV, dtype=BF).init_synthetic(2)
    m.pack()
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)          # noqa: E731
    from apex_studio_amd.engine_flux import latent_image_ids
    inp = dict(hidden_states=r(1, S_IMG, 64), encoder_hidden_states=r(1, S_TXT, 4096), pooled_projections=r(1, 768),
               timestep=torch.tensor([0.5], device=DEV), guidance=torch.tensor([3.5], device=DEV), img_ids=latent_image_ids(64, 64, device=DEV),
               txt_ids=torch.zeros(S_TXT, 3, device=DEV))
    fwd = lambda: m(return_dict=False, **inp)[0]                           # noqa: E731
    t, outs = {}, {}

    def measure(names_and_setups):
        for k, setup in names_and_setups:                # warm every arm
            setup()
            outs[k] = fwd().float()
            t[k] = []
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, setup in names_and_setups:
                setup()
                t[k].append(timed(fwd, 1))
    measure([("bf16_shipped", lambda: None)])
    for name, p in m.named_parameters():               # the stand-in for a keep_fp8 load: every block Linear becomes an e4m3 record
        if m._fp8_resident_key(name) and p.dim() == 2:
            w = p.data.float()
            s = (w.abs().max() / 448.0).reshape(1)
            p._fp8 = ops.Fp8Weight((w / s).to(torch.float8_e4m3fn), s)
    m._fp8_adopt()
    measure([("resident_bf16_compute", lambda: m.set_fp8_compute(False)), ("fp8_compute", lambda: m.set_fp8_compute(True)),
             ("fp8_compute_fused_quant", lambda: m.set_fp8_compute(True, fused_quant=True))])
    med = {k: statistics.median(v) for k, v in t.items()}
    rel = lambda a, b: float((outs[a] - outs[b]).norm() / outs[b].norm())  # noqa: E731
    return {"workload": f"flux-dev 1024^2 (S {S_IMG} + {S_TXT}), one forward on {double} + {single} blocks, synthetic weights",
            "ms_per_forward": {k: round(v * 1e3, 3) for k, v in med.items()},
            "speedup_over_bf16_shipped": {k: round(med["bf16_shipped"] / v, 4) for k, v in med.items()},
            "rel_l2_fp8_vs_resident_bf16": rel("fp8_compute", "resident_bf16_compute"),
            "fused_quant_equals_fp8": bool(torch.equal(outs["fp8_compute_fused_quant"], outs["fp8_compute"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--double", type=int, default=19)
    ap.add_argument("--single", type=int, default=38)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_fp8_bench.json"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "shape": {"s_img": S_IMG, "s_txt": S_TXT, "dim": DIM, "heads": H, "mlp": MLP},
           "arms": {"bf16": "gemm_grouped / gemm_grouped_qkv (fused q/k/v) / gemm on bf16 weights",
                    "fp8": "quant_rows_fp8 + gemm_fp8_grouped (+ qkv_prepare on the QKV classes)",
                    "fp8_fused": "quant_rows_fp8 + gemm_fp8_grouped_qkv"},
           "classes": bench_classes(g, args.rounds, args.iters)}
    if args.forward:
        doc["forward"] = bench_forward(args.double, args.single, args.rounds)
        print(json.dumps(doc["forward"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
