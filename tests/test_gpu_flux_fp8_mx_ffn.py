"""`FluxTransformer2DModel.set_fp8_compute(True, mx_ffn=True)` on the tiny resident-fp8 Flux of
tests/test_gpu_flux_fp8_compute.py (width 256, FF 1024, 2 double + 2 single blocks): the double block's FF hidden state stays in MX
fp8 between the grouped FF-up pair and the grouped FF-down pair.  Off (the default) every launch is the one of
`set_fp8_compute(True)`, to the bit; on, one `ops.quant_rows_fp8` launch per double block disappears (counted), the bf16 hidden
buffer is never written (sentinel bytes), and the forward stays within the measured distance of the bf16-compute forward.  Each
property is shown with a text stream of 72 rows and one of 77 (no multiple of 8: the image rows of the joint buffers start at an odd
row)."""
import pytest
import torch

from tests.conftest import measured
from tests.test_gpu_flux_fp8_compute import DEV, DOUBLE, H2, SINGLE, W2, _fwd, _load, fp8_file  # noqa: F401  (fp8_file: a fixture)
from tests.test_gpu_wan_fp8_fused_quant import _count_quant_rows

pytestmark = pytest.mark.gpu
SENTINEL_BYTE = 0xA5
FF = 1024
# ops.quant_rows_fp8 launches of one forward: QKV, to_out, FF-up and FF-down pairs per double block, QKV | MLP-up and proj_out per
# single block; the quantising norms take the QKV and FF-up ones; mx_ffn takes the FF-down one
PLAIN, PLAIN_FUSED = 4 * DOUBLE + 2 * SINGLE, 2 * DOUBLE + SINGLE
MX, MX_FUSED = PLAIN - DOUBLE, PLAIN_FUSED - DOUBLE
S_TXT = [72, 77]
# rel-L2 against the bf16-compute forward, s_txt: (per-row fp8 bar, mx_ffn bar); each bar is 2x the value measured on the MI355X:
#   72 text rows: per-row 2.092e-2 (as tests/test_gpu_flux_fp8_compute.py), mx_ffn 2.096e-2, ratio 1.002
#   77 text rows: per-row 2.081e-2, mx_ffn 2.111e-2, ratio 1.015            (MX is not more accurate than per-row here)
BARS = {72: (4.18e-2, 4.19e-2), 77: (4.16e-2, 4.22e-2)}


def _workspace(m):
    (ws,) = m._ws.values()
    return ws


@pytest.mark.parametrize("s_txt", S_TXT)
def test_default_and_explicit_off_are_the_fp8_forward_bit_for_bit(fp8_file, s_txt):  # noqa: F811
    m = _load(fp8_file, True)
    first = _fwd(m, s_txt)
    m.set_fp8_compute(True)
    assert m._fp8_mx_ffn is False
    with _count_quant_rows() as calls:
        plain = _fwd(m, s_txt)
    assert len(calls) == PLAIN
    m.set_fp8_compute(True, mx_ffn=False)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m, s_txt), plain), "mx_ffn=False: the forward of set_fp8_compute(True)"
    assert len(calls) == PLAIN
    m.set_fp8_compute(True, fused_quant=True, mx_ffn=False)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m, s_txt), plain)
    assert len(calls) == PLAIN_FUSED
    with pytest.raises(ValueError, match="mx_ffn=True.*needs on=True"):
        m.set_fp8_compute(False, mx_ffn=True)
    m.set_fp8_compute(False)
    assert torch.equal(_fwd(m, s_txt), first)


@pytest.mark.parametrize("s_txt", S_TXT)
def test_one_quantise_launch_per_double_block_disappears_and_on_off_on_restores(fp8_file, s_txt):  # noqa: F811
    from apex_studio_amd import ops
    m = _load(fp8_file, True)
    m.set_fp8_compute(True)
    plain = _fwd(m, s_txt)
    ws = _workspace(m)
    raw = ws.FFH.view(torch.uint8)
    assert tuple(raw.shape) == (s_txt + H2 * W2, 2 * FF)
    used = FF + FF // 32                                      # codes, then one scale byte per 32 columns
    # the per-row path writes the bf16 hidden state over a planted pattern
    raw.fill_(SENTINEL_BYTE)
    assert torch.equal(_fwd(m, s_txt), plain)
    assert not bool((raw[:, used:] == SENTINEL_BYTE).all()), "set_fp8_compute(True) stores bf16 rows in FFH"
    real, grouped = ops.gemm_fp8_grouped, []

    def counted(*a, **k):
        grouped.append((k.get("out_mx_list") is not None, k.get("block_scales_list") is not None))
        return real(*a, **k)
    for fused, want in ((False, MX), (True, MX_FUSED)):
        m.set_fp8_compute(True, fused_quant=fused, mx_ffn=True)
        raw.fill_(SENTINEL_BYTE)
        del grouped[:]
        ops.gemm_fp8_grouped = counted
        try:
            with _count_quant_rows() as calls:
                mx = _fwd(m, s_txt)
        finally:
            ops.gemm_fp8_grouped = real
        assert _workspace(m) is ws
        assert len(calls) == want, f"mx_ffn (fused_quant={fused}): {len(calls)} quantise launches, expected {want}"
        # to_out, FF-up (MX output) and FF-down (block scales) pairs of each double block, in that order
        assert grouped == [(False, False), (True, False), (False, True)] * DOUBLE, grouped
        assert torch.isfinite(mx).all() and not torch.equal(mx, plain), "block scales change the numbers"
        host = raw.cpu()
        assert bool((host[:, used:] == SENTINEL_BYTE).all()), "bytes behind the codes and scale bytes: no bf16 row was stored"
        codes, scales = host[:, :FF], host[:, FF:used]
        assert not bool(((codes & 0x7F) == 0x7F).any()) and int(scales.max()) < 255 and int(scales.min()) >= 1
        for rows in (slice(0, s_txt), slice(s_txt, None)):       # both streams wrote their row slice
            assert codes[rows].unique().numel() > 64 and scales[rows].unique().numel() > 2, "the MX hidden state of the last block"
        if fused:
            assert torch.equal(mx, unfused), "fused_quant composes: a launch change only"
        unfused = mx
    # off again: the earlier forward, to the bit
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m, s_txt), plain), "mx_ffn off again restores the per-row forward bit for bit"
    assert len(calls) == PLAIN
    m.set_fp8_compute(True, mx_ffn=True)
    assert torch.equal(_fwd(m, s_txt), unfused), "and on again is the same MX forward"


@pytest.mark.parametrize("s_txt", S_TXT)
def test_accuracy_against_the_bf16_compute_forward(fp8_file, s_txt):  # noqa: F811
    m = _load(fp8_file, True)
    ref = _fwd(m, s_txt)
    m.set_fp8_compute(True)
    row = _fwd(m, s_txt)
    m.set_fp8_compute(True, mx_ffn=True)
    mx = _fwd(m, s_txt)
    rel_row = float((row - ref).norm() / ref.norm())
    rel_mx = float((mx - ref).norm() / ref.norm())
    print(f"[flux mx_ffn] {DOUBLE} + {SINGLE} blocks of width 256, {s_txt} text rows: rel-L2 against the bf16-compute forward: "
          f"per-row fp8 {rel_row:.3e}, mx_ffn {rel_mx:.3e}, ratio mx / per-row {rel_mx / rel_row:.3f}")
    # the measured values stand beside BARS; the ratio is reported above, not asserted
    bar_row, bar_mx = BARS[s_txt]
    measured(f"flux.fp8_mx_ffn.tiny.s{s_txt}.per_row.rel_l2", rel_row, bar_row)
    measured(f"flux.fp8_mx_ffn.tiny.s{s_txt}.mx.rel_l2", rel_mx, bar_mx)


def test_the_f32_residual_stream_keeps_its_launches(fp8_file):  # noqa: F811
    m = _load(fp8_file, True)
    m.set_residual_dtype(torch.float32)
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        plain = _fwd(m)
    n_plain = len(calls)
    m.set_fp8_compute(True, mx_ffn=True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain), "a float residual stream: fp8_mx_route is False, today's launches"
    assert len(calls) == n_plain > 0


def test_engine_switch(fp8_file):  # noqa: F811
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from tests.golden.seeded import seeded
    m = _load(fp8_file, True)
    with pytest.raises(ValueError, match="fp8_mx_ffn=True needs fp8_compute=True"):
        FluxT2IEngine(m, fp8_mx_ffn=True)
    eng = FluxT2IEngine(m, fp8_compute=True)
    assert eng.fp8_mx_ffn is False and m._fp8_mx_ffn is False
    eng = FluxT2IEngine(m, fp8_compute=True, fp8_mx_ffn=True)
    assert eng.fp8_mx_ffn is True and m._fp8_mx_ffn is True and m._fp8_fused_quant is False
    with _count_quant_rows() as calls:
        lat = eng.run(prompt_embeds=seeded((1, 72, 256), 32).to(DEV), pooled_prompt_embeds=seeded((1, 64), 33).to(DEV), height=256,
                      width=256, num_inference_steps=2, guidance_scale=3.5, latents=seeded((1, H2 * W2, 64), 41).to(DEV),
                      return_latents=True)
        torch.cuda.synchronize()
    assert len(calls) == 2 * MX, "two steps of a guidance-distilled model: two forwards"
    assert lat.shape == (1, H2 * W2, 64) and torch.isfinite(lat.float()).all() and float(lat.float().std()) > 0
