#!/usr/bin/env python
"""Flux run-time LoRA on resident fp8 weights at the Flux-Dev 1024^2 shapes (S = 4096 image + 512 text rows, dim
3072, 24 heads, MLP 12288), padded rank 64 and 128 on every block Linear, in one process.

Per launch class of a block (tools/flux_fp8_bench.py's classes) three arms, each with every launch it needs counted in:
  a  fp8 compute WITHOUT adapters: `quant_rows_fp8` + `gemm_fp8_grouped` (the QKV classes: `gemm_fp8_grouped_qkv`; proj_out: `gemm_fp8`)
  b  fp8 compute WITH run-time adapters: the grouped skinny GEMM (`gemm_grouped` over the problems' lora_A) + `quant_rows_fp8` + the
     same launch with `lora_t_list=` / `lora_B_list=` (proj_out: `gemm_fp8(lora_t=, lora_B=)`), per rank
  c  the shipped bf16 launch on bf16 weights — what an adapter merged at load costs at run time
timed with HIP events around `--iters` back-to-back calls, arms interleaved over `--rounds` rounds, medians; b / a and b / c are
time ratios (above 1 = b is slower).  The live GEMM clock (`apexmi_clk_enable`) of each arm's GEMM is read in a separate, untimed
pass.  `--forward` adds the 19 + 38-block forward (synthetic weights) in the same arms: a bf16 model and a resident fp8 model of
the same weights side by side, the adapters given to every resident record directly (`set_lora`; the fused q|k|v records take
three adapters of a third of the rank each, so that their padded rank is the class's too).  Writes one JSON document (`--out`,
default profiles/flux_fp8_lora_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import apex_studio_amd  # noqa: E402,F401
from apex_studio_amd import ops  # noqa: E402
from flux_fp8_bench import BF, DEV, DIM, H, MLP, S, S_IMG, S_TXT, clock_of, pair_of, timed  # noqa: E402

RANKS = (64, 128)


def factors(rec, Rp, g):
    """random bf16 (lora_A [Rp, K], B' [N, Rp]) for a record, sized like tests/test_gpu_gemm_fp8_lora.py's random operands"""
    N, K = rec.shape
    return ((torch.randn(Rp, K, generator=g, device=DEV) * K ** -0.5).to(BF), (torch.randn(N, Rp, generator=g, device=DEV) * 0.02).to(BF))


def launch_classes(g):
    """{class: (flops, {arm: fn}, {arm: fn of the GEMM launch alone, for the clock})}; arms a, c, b64, b128"""
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)          # noqa: E731
    XN, FFH, CAT = r(S, DIM).to(BF), r(S, MLP).to(BF), r(S, DIM + MLP).to(BF)
    X, Y = r(S, DIM).to(BF), torch.empty(S, DIM, device=DEV, dtype=BF)
    UP = torch.empty(S, MLP, device=DEV, dtype=BF)
    att = CAT[:, :DIM]
    Q, K_ = (torch.empty(H, S, 128, device=DEV, dtype=BF) for _ in range(2))
    VT = torch.zeros(H, 128, S, device=DEV, dtype=BF)
    ang = torch.rand(S, 64, generator=g, device=DEV) * 6.283
    rope = torch.stack([ang.cos().repeat_interleave(2, dim=1), ang.sin().repeat_interleave(2, dim=1)]).contiguous().float()
    nw = [r(128).to(BF) * 0.2 + 1 for _ in range(4)]
    gate = [r(DIM) * 1e-2 for _ in range(2)]
    img, txt = slice(S_TXT, None), slice(0, S_TXT)
    bias = lambda n: r(n).to(BF) * 0.1                               # noqa: E731
    tbuf = torch.empty(2 * S * max(RANKS), device=DEV, dtype=BF)     # the t workspace of a launch (two problems at most)
    out = {}

    def quant(src):
        qa, sa = ops._act_scratch(src.device, src.shape[0], src.shape[1])
        return ops.quant_rows_fp8(src, out=qa, scale_out=sa)

    def skinny(a_list, fs):
        ts, off = [], 0
        for a, (A, _) in zip(a_list, fs):
            n = a.shape[0] * A.shape[0]
            ts.append(tbuf[off:off + n].view(a.shape[0], A.shape[0]))
            off += n
        ops.gemm_grouped(a_list, [A for A, _ in fs], None, ts)
        return ts

    def add_class(name, flops, a_list, rows, recs, bf16_fn, fp8_fn, src):
        """fp8_fn(qa_list, sa_list, **lora lists): the fp8 launch of the class; a_list = the bf16 rows its skinny GEMM reads"""
        fs = {Rp: [factors(rec, Rp, g) for rec in recs] for Rp in RANKS}
        held = ops.quant_rows_fp8(src)
        cut = lambda q: ([q[0][r_] for r_ in rows], [q[1][r_] for r_ in rows])     # noqa: E731
        arms, gemms = {"a": lambda: fp8_fn(*cut(quant(src))), "c": bf16_fn}, {"a": lambda: fp8_fn(*cut(held)), "c": bf16_fn}
        for Rp in RANKS:
            def b(Rp=Rp, q=None):
                ts = skinny(a_list, fs[Rp])
                fp8_fn(*cut(quant(src) if q is None else q), lora_t_list=ts, lora_B_list=[B for _, B in fs[Rp]])
            arms[f"b{Rp}"] = b
            ts0 = skinny(a_list, fs[Rp])
            ts0 = [t.clone() for t in ts0]
            gemms[f"b{Rp}"] = lambda Rp=Rp, ts0=ts0: fp8_fn(*cut(held), lora_t_list=ts0, lora_B_list=[B for _, B in fs[Rp]])
        out[name] = (flops, arms, gemms)

    def pair_class(name, src, N, Kk, outs, epi, gated):
        (wa, ra), (wb, rb) = pair_of(N, Kk, g), pair_of(N, Kk, g)
        bs = [bias(N), bias(N)]
        kw = dict(gate_list=gate, residual_list=[X[img], X[txt]]) if gated else {}
        add_class(name, 2.0 * S * N * Kk, [src[img], src[txt]], [img, txt], [ra, rb],
                  lambda: ops.gemm_grouped([src[img], src[txt]], [wa, wb], bs, outs, epilogue=epi, **kw),
                  lambda qa, sa, **lo: ops.gemm_fp8_grouped(qa, sa, [ra, rb], bs, outs, epilogue=epi, **kw, **lo), src)

    (wa, ra), (wb, rb) = pair_of(3 * DIM, DIM, g), pair_of(3 * DIM, DIM, g)
    bq = [bias(3 * DIM), bias(3 * DIM)]
    qkv_args = ([None, None], "bias", [1, 1], [nw[0], nw[2]], [nw[1], nw[3]], [S_TXT, 0], H, 1e-6, rope, Q, K_, VT)
    add_class("qkv_pair", 2.0 * S * 3 * DIM * DIM, [XN[img], XN[txt]], [img, txt], [ra, rb],
              lambda: ops.gemm_grouped_qkv([XN[img], XN[txt]], [wa, wb], bq, *qkv_args),
              lambda qa, sa, **lo: ops.gemm_fp8_grouped_qkv(qa, sa, [ra, rb], bq, *qkv_args, **lo), XN)
    pair_class("to_out_pair", att, DIM, DIM, [Y[img], Y[txt]], "gate_res", True)
    pair_class("ff_up_pair", XN, MLP, DIM, [UP[img], UP[txt]], "gelu", False)
    pair_class("ff_down_pair", FFH, DIM, MLP, [Y[img], Y[txt]], "gate_res", True)

    (wq, rq), (wm, rm) = pair_of(3 * DIM, DIM, g), pair_of(MLP, DIM, g)
    bsm = [bias(3 * DIM), bias(MLP)]
    s_args = ([None, CAT[:, DIM:]], ["bias", "gelu"], [1, 0], [nw[0], None], [nw[1], None], [0, 0], H, 1e-6, rope, Q, K_, VT)
    al = slice(None)
    add_class("single_qkv_mlp", 2.0 * S * (3 * DIM + MLP) * DIM, [XN, XN], [al, al], [rq, rm],
              lambda: ops.gemm_grouped_qkv([XN, XN], [wq, wm], bsm, *s_args),
              lambda qa, sa, **lo: ops.gemm_fp8_grouped_qkv(qa, sa, [rq, rm], bsm, *s_args, **lo), XN)

    wo, ro = pair_of(DIM, DIM + MLP, g)
    bo = bias(DIM)

    def proj_out(qa, sa, lora_t_list=None, lora_B_list=None):
        lo = {} if lora_t_list is None else dict(lora_t=lora_t_list[0], lora_B=lora_B_list[0])
        ops.gemm_fp8(qa[0], sa[0], ro, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X, **lo)
    add_class("single_proj_out", 2.0 * S * DIM * (DIM + MLP), [CAT], [al], [ro],
              lambda: ops.gemm(CAT, wo, bo, out=Y, epilogue="gate_res", gate=gate[0], residual=X), proj_out, CAT)
    return out


def ratios(med):
    """b / a and b / c as TIME ratios (above 1 = the adapter arm is slower), and the NOT-faster mark against the shipped bf16 launch"""
    out = {}
    for Rp in RANKS:
        b = med[f"b{Rp}"]
        out[f"r{Rp}"] = {"b_over_a": round(b / med["a"], 4), "b_over_c": round(b / med["c"], 4), "faster_than_c": bool(b < med["c"])}
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
               "spread": {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in t.items()},
               **ratios(med), "clock_ghz": {k: clock_of(fn) for k, fn in gemms.items()}}
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_forward(double, single, rounds):
    from apex_studio_amd.engine_flux import latent_image_ids
    from apex_studio_amd.flux import FluxTransformer2DModel

    def model():
        m = FluxTransformer2DModel(num_layers=double, num_single_layers=single, guidance_embeds=True, device=DEV, dtype=BF).init_synthetic(2)
        m.pack()
        return m
    shipped, m = model(), model()
    for name, p in m.named_parameters():               # the stand-in for a keep_fp8 load: every block Linear becomes an e4m3 record
        if m._fp8_resident_key(name) and p.dim() == 2:
            w = p.data.float()
            s = (w.abs().max() / 448.0).reshape(1)
            p._fp8 = ops.Fp8Weight((w / s).to(torch.float8_e4m3fn), s)
    m._fp8_adopt()
    recs = list({id(r): r for r in m._fp8_records.values()}.values())
    g = torch.Generator(device=DEV).manual_seed(3)
    fs = {}
    for Rp in RANKS:                                   # built once through set_lora, then swapped in per arm
        for rec in recs:
            r_ = Rp // len(rec.parts) if len(rec.parts) > 1 else Rp
            K = rec.shape[1]
            rec.set_lora([(mod, torch.randn(r_, K, generator=g, device=DEV) * K ** -0.5, torch.randn(n, r_, generator=g, device=DEV) * 0.02, 1.0)
                          for mod, _, n in rec.parts])
            assert rec.lora_A.shape[0] == Rp, (rec.parts, rec.lora_A.shape)
            fs[(id(rec), Rp)] = (rec.lora_A, rec.lora_B)
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)          # noqa: E731
    inp = dict(hidden_states=r(1, S_IMG, 64), encoder_hidden_states=r(1, S_TXT, 4096), pooled_projections=r(1, 768),
               timestep=torch.tensor([0.5], device=DEV), guidance=torch.tensor([3.5], device=DEV), img_ids=latent_image_ids(64, 64, device=DEV),
               txt_ids=torch.zeros(S_TXT, 3, device=DEV))

    def plain():
        for rec in recs:
            rec.lora_A = rec.lora_B = None
        m.set_fp8_compute(True)
        return m

    def with_rank(Rp):
        def setup():
            for rec in recs:
                rec.lora_A = rec.lora_B = None
            m.set_fp8_compute(True, lora=True)
            for rec in recs:
                rec.lora_A, rec.lora_B = fs[(id(rec), Rp)]
            return m
        return setup
    arms = [("c", lambda: shipped), ("a", plain)] + [(f"b{Rp}", with_rank(Rp)) for Rp in RANKS]
    t, outs = {k: [] for k, _ in arms}, {}
    for k, setup in arms:                              # warm every arm
        outs[k] = setup()(return_dict=False, **inp)[0].float()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, setup in arms:
            mm = setup()
            t[k].append(timed(lambda: mm(return_dict=False, **inp)[0], 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    rel = lambda a, b: float((outs[a] - outs[b]).norm() / outs[b].norm())  # noqa: E731
    return {"workload": f"flux-dev 1024^2 (S {S_IMG} + {S_TXT}), one forward on {double} + {single} blocks, synthetic weights, adapters on "
                        "every block Linear", "ms_per_forward": {k: round(v * 1e3, 3) for k, v in med.items()},
            "spread": {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in t.items()}, **ratios(med),
            "rel_l2_a_vs_c": rel("a", "c"), "rel_l2_b64_vs_a": rel("b64", "a"), "finite": bool(all(torch.isfinite(o).all() for o in outs.values()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--forward", action="store_true")
    ap.add_argument("--double", type=int, default=19)
    ap.add_argument("--single", type=int, default=38)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_fp8_lora_bench.json"))
    args = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(1)
    doc = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters,
           "shape": {"s_img": S_IMG, "s_txt": S_TXT, "dim": DIM, "heads": H, "mlp": MLP, "padded_ranks": list(RANKS)},
           "arms": {"a": "fp8 compute without adapters: quant_rows_fp8 + gemm_fp8_grouped / gemm_fp8_grouped_qkv / gemm_fp8",
                    "b": "fp8 compute with run-time adapters: grouped skinny GEMM + quant_rows_fp8 + the same launch with lora_t / lora_B",
                    "c": "the shipped bf16 launches (gemm_grouped / gemm_grouped_qkv / gemm): what a load-time merge costs at run time"},
           "ratios": "b_over_a and b_over_c are time ratios: above 1 = the adapter arm is slower",
           "classes": bench_classes(g, args.rounds, args.iters)}
    if args.forward:
        doc["forward"] = bench_forward(args.double, args.single, args.rounds)
        print(json.dumps(doc["forward"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
