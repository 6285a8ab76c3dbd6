#!/usr/bin/env python
"""The MX block-scaled FFN hidden state (`set_fp8_compute(mx_ffn=True)`) against the per-row fp8 launches it
replaces, in one process.  For up K -> F (GELU) then down F -> K (gate x y + residual, in place) with resident e4m3 weights, at
Wan-2.2 A14B 5120 -> 13824 -> 5120 for M = 75 600 (720p x 81 f) and 32 760 (480p x 81 f) and at the Flux 1024^2 FF pair
3072 -> 12288 -> 3072 for M = 4096 (image stream):
  (a) per_row   : gemm_fp8 up with bf16 output + quant_rows_fp8 of the hidden state + gemm_fp8 down      (the launches of today)
  (b) mx_chain  : gemm_fp8(out_mx=) + gemm_fp8(block_scales=)
  (c) up_bf16 / up_mx      : the up GEMM alone, bf16 output against MX output
  (d) down_row / down_blk  : the down GEMM alone, per-row scales against block scales
  (e) `--step`: one Wan 720p x 81 f expert forward on `--layers` blocks and one Flux 1024^2 forward on `--double` + `--single`
      blocks, fp8 compute with mx_ffn off and on
The Flux FF pair is also timed as the model issues it: the grouped launches over the image (4096 rows) and text (512 rows) streams,
(a) gemm_fp8_grouped + quant_rows_fp8 + gemm_fp8_grouped against (b) gemm_fp8_grouped(out_mx_list=) + (block_scales_list=);
timed with HIP events around `--iters` back-to-back calls, `--rounds` interleaved rounds, medians; the baseline of every ratio is
the per-row arm of the same run.  The live clock of each GEMM (`apexmi_clk_enable`) is read in a separate, untimed pass.  Operands
are random.  Writes one JSON document (`--out`)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import ops  # noqa: E402
from gemm_fp8_bench import DEV, clock_of, fp8_weight, timed  # noqa: E402

CASES = [("wan 720p", 75600, 5120, 13824), ("wan 480p", 32760, 5120, 13824), ("flux 1024^2 img", 4096, 3072, 12288)]
U8 = torch.uint8


def bench_pair(name, M, K, F, g, rounds, iters):
    a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w_up, w_dn = fp8_weight(F, K, g), fp8_weight(K, F, g)
    b_up, b_dn = torch.randn(F, generator=g, device=DEV).to(torch.bfloat16), torch.randn(K, generator=g, device=DEV).to(torch.bfloat16)
    gate = torch.randn(K, generator=g, device=DEV)
    x = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    qa, sa = ops.quant_rows_fp8(a)
    h = torch.empty(M, F, dtype=torch.bfloat16, device=DEV)
    hq, hs = torch.empty(M, F, dtype=U8, device=DEV), torch.empty(M, dtype=torch.float32, device=DEV)
    mq, ms = torch.empty(M, F, dtype=U8, device=DEV), torch.empty(M, F // 32, dtype=U8, device=DEV)

    def up_bf16():
        ops.gemm_fp8(qa, sa, w_up, b_up, out=h, epilogue="gelu")

    def up_mx():
        ops.gemm_fp8(qa, sa, w_up, b_up, epilogue="gelu", out_mx=(mq, ms))

    def quant():
        ops.quant_rows_fp8(h, out=hq, scale_out=hs)

    def down_row():
        ops.gemm_fp8(hq, hs, w_dn, b_dn, out=x, epilogue="gate_res", gate=gate, residual=x)

    def down_blk():
        ops.gemm_fp8(mq, None, w_dn, b_dn, out=x, epilogue="gate_res", gate=gate, residual=x, block_scales=ms)

    def per_row():
        up_bf16(), quant(), down_row()

    def mx_chain():
        up_mx(), down_blk()
    arms = {"per_row": per_row, "mx_chain": mx_chain, "up_bf16": up_bf16, "up_mx": up_mx, "quant_rows": quant, "down_row": down_row,
            "down_blk": down_blk}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    spread = {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()}
    return {"case": name, "M": M, "K": K, "F": F, "ms": {k: round(v * 1e3, 4) for k, v in med.items()}, "spread": spread,
            "mx_chain_over_per_row": round(med["per_row"] / med["mx_chain"], 4), "up_mx_over_up_bf16": round(med["up_bf16"] / med["up_mx"], 4),
            "down_blk_over_down_row": round(med["down_row"] / med["down_blk"], 4),
            "clock_ghz": {k: clock_of(arms[k]) for k in ("up_bf16", "up_mx", "down_row", "down_blk")}}


def bench_flux_pair(g, rounds, iters, s_img=4096, s_txt=512, K=3072, F=12288):
    S = s_img + s_txt
    rows = [slice(s_txt, None), slice(0, s_txt)]
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)  # noqa: E731
    xn, x = r(S, K).to(torch.bfloat16), r(S, K).to(torch.bfloat16)
    w_up, w_dn = [fp8_weight(F, K, g) for _ in rows], [fp8_weight(K, F, g) for _ in rows]
    b_up, b_dn = [r(F).to(torch.bfloat16) for _ in rows], [r(K).to(torch.bfloat16) for _ in rows]
    gate = [r(K) for _ in rows]
    qa, sa = ops.quant_rows_fp8(xn)
    h = torch.empty(S, F, dtype=torch.bfloat16, device=DEV)
    hq, hs = torch.empty(S, F, dtype=U8, device=DEV), torch.empty(S, dtype=torch.float32, device=DEV)
    raw = torch.empty(S, 2 * F, dtype=U8, device=DEV)            # as the model: codes and scale bytes in the rows of the bf16 buffer
    mq, ms = raw[:, :F], raw[:, F:F + F // 32]
    sl = lambda t: [t[i] for i in rows]  # noqa: E731

    def up_bf16():
        ops.gemm_fp8_grouped(sl(qa), sl(sa), w_up, b_up, sl(h), epilogue="gelu")

    def up_mx():
        ops.gemm_fp8_grouped(sl(qa), sl(sa), w_up, b_up, [None, None], epilogue="gelu", out_mx_list=list(zip(sl(mq), sl(ms))))

    def quant():
        ops.quant_rows_fp8(h, out=hq, scale_out=hs)

    def down_row():
        ops.gemm_fp8_grouped(sl(hq), sl(hs), w_dn, b_dn, sl(x), epilogue="gate_res", gate_list=gate, residual_list=sl(x))

    def down_blk():
        ops.gemm_fp8_grouped(sl(mq), [None, None], w_dn, b_dn, sl(x), epilogue="gate_res", gate_list=gate, residual_list=sl(x),
                             block_scales_list=sl(ms))

    def per_row():
        up_bf16(), quant(), down_row()

    def mx_chain():
        up_mx(), down_blk()
    arms = {"per_row": per_row, "mx_chain": mx_chain, "up_bf16": up_bf16, "up_mx": up_mx, "quant_rows": quant, "down_row": down_row,
            "down_blk": down_blk}
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"case": "flux 1024^2 FF pair, grouped img + txt", "M": [s_img, s_txt], "K": K, "F": F,
            "ms": {k: round(v * 1e3, 4) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()},
            "mx_chain_over_per_row": round(med["per_row"] / med["mx_chain"], 4), "up_mx_over_up_bf16": round(med["up_bf16"] / med["up_mx"], 4),
            "down_blk_over_down_row": round(med["down_row"] / med["down_blk"], 4),
            "clock_ghz": {k: clock_of(arms[k]) for k in ("up_bf16", "up_mx", "down_row", "down_blk")}}


def bench_flux_step(double, single, rounds, s_img=4096, s_txt=512):
    from apex_studio_amd.engine_flux import latent_image_ids
    from apex_studio_amd.flux import FluxTransformer2DModel
    m = FluxTransformer2DModel(num_layers=double, num_single_layers=single, guidance_embeds=True, device=DEV,
                               dtype=torch.bfloat16).init_synthetic(2)
    m.pack()
    for name, p in m.named_parameters():           # the stand-in for a keep_fp8 load: every block Linear becomes an e4m3 record
        if m._fp8_resident_key(name) and p.dim() == 2:
            w = p.data.float()
            s = (w.abs().max() / 448.0).reshape(1)
            p._fp8 = ops.Fp8Weight((w / s).to(torch.float8_e4m3fn), s)
    m._fp8_adopt()
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(torch.bfloat16)  # noqa: E731
    inp = dict(hidden_states=r(1, s_img, 64), encoder_hidden_states=r(1, s_txt, 4096), pooled_projections=r(1, 768),
               timestep=torch.tensor([0.5], device=DEV), guidance=torch.tensor([3.5], device=DEV),
               img_ids=latent_image_ids(64, 64, device=DEV), txt_ids=torch.zeros(s_txt, 3, device=DEV))
    fwd = lambda: m(return_dict=False, **inp)[0]  # noqa: E731
    modes = {"per_row": {}, "mx_ffn": {"mx_ffn": True}, "fused_quant": {"fused_quant": True}, "fused_quant+mx_ffn": {"fused_quant": True, "mx_ffn": True}}
    t, outs = {k: [] for k in modes}, {}
    for k, kw in modes.items():                    # warm all
        m.set_fp8_compute(True, **kw)
        outs[k] = fwd().float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, kw in modes.items():
            m.set_fp8_compute(True, **kw)
            t[k].append(timed(fwd, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"workload": f"flux-dev 1024^2 (S {s_img} + {s_txt}), one forward on {double} + {single} blocks, resident fp8 weights, fp8 compute on",
            "ms_per_forward": {k: round(v * 1e3, 3) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()},
            "mx_ffn_over_per_row": round(med["per_row"] / med["mx_ffn"], 4),
            "fused_quant_mx_ffn_over_fused_quant": round(med["fused_quant"] / med["fused_quant+mx_ffn"], 4),
            "rel_l2_mx_ffn_vs_per_row": float((outs["mx_ffn"] - outs["per_row"]).norm() / outs["per_row"].norm())}


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
    modes = {"per_row": {}, "mx_ffn": {"mx_ffn": True}, "fused_quant": {"fused_quant": True}, "fused_quant+mx_ffn": {"fused_quant": True, "mx_ffn": True}}
    t, outs = {k: [] for k in modes}, {}
    for k, kw in modes.items():                    # warm all
        m.set_fp8_compute(True, **kw)
        outs[k] = m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False)[0].float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, kw in modes.items():
            m.set_fp8_compute(True, **kw)
            t[k].append(timed(lambda: m(hidden_states=x, timestep=ts, encoder_hidden_states=enc, return_dict=False), 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"workload": f"wan2.2-a14b 720p x 81f, one expert forward on {layers} blocks, resident fp8 weights, fp8 compute on",
            "s_per_forward": {k: round(v, 4) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in t.items()},
            "mx_ffn_over_per_row": round(med["per_row"] / med["mx_ffn"], 4),
            "fused_quant_mx_ffn_over_fused_quant": round(med["fused_quant"] / med["fused_quant+mx_ffn"], 4),
            "rel_l2_mx_ffn_vs_per_row": float((outs["mx_ffn"] - outs["per_row"]).norm() / outs["per_row"].norm())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--double", type=int, default=19)
    ap.add_argument("--single", type=int, default=38)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "arms": {"per_row": "gemm_fp8 (bf16 out) + quant_rows_fp8 + gemm_fp8", "mx_chain": "gemm_fp8(out_mx) + gemm_fp8(block_scales)"},
           "pairs": []}
    for name, M, K, F in CASES:
        row = bench_pair(name, M, K, F, g, args.rounds, args.iters)
        print(json.dumps(row), flush=True)
        doc["pairs"].append(row)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(doc, f, indent=1)
    doc["flux_pair"] = bench_flux_pair(g, args.rounds, args.iters)
    print(json.dumps(doc["flux_pair"]), flush=True)
    if args.step:
        doc["wan_step"] = bench_step(args.layers, args.rounds)
        print(json.dumps(doc["wan_step"]), flush=True)
        torch.cuda.empty_cache()
        doc["flux_step"] = bench_flux_step(args.double, args.single, args.rounds)
        print(json.dumps(doc["flux_step"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
