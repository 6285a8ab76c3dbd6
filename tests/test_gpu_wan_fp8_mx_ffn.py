"""`WanTransformer3DModel.set_fp8_compute(True, mx_ffn=True)` on the tiny resident-fp8 Wan model of
tests/test_gpu_wan_fp8_compute.py (width 256, FFN 512, 3 layers): the FFN hidden state stays in MX fp8 between the two FFN
Linears.  Off (the default) every launch is the one of `set_fp8_compute(True)`, to the bit; on, one `ops.quant_rows_fp8` launch
per block disappears (counted), the bf16 hidden buffer is never written (sentinel bytes), and the forward stays within the
measured distance of the bf16-compute forward."""
import pytest
import torch

from tests.conftest import measured
from tests.test_gpu_wan_fp8_compute import DEV, DIM, FFN, LAYERS, _fwd, _model
from tests.test_gpu_wan_fp8_fused_quant import _count_quant_rows, _lora_state

pytestmark = pytest.mark.gpu
SENTINEL_BYTE = 0xA5


def _workspace(m):
    (ws,) = m._ws.values()
    return ws


def test_default_and_explicit_off_are_the_fp8_forward_bit_for_bit(tmp_path):
    m = _model(tmp_path)
    first = _fwd(m)
    m.set_fp8_compute(True)
    assert m._fp8_mx_ffn is False
    with _count_quant_rows() as calls:
        plain = _fwd(m)
    assert len(calls) == 7 * LAYERS
    m.set_fp8_compute(True, mx_ffn=False)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain), "mx_ffn=False: the forward of set_fp8_compute(True)"
    assert len(calls) == 7 * LAYERS
    m.set_fp8_compute(True, fused_quant=True, mx_ffn=False)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain)
    assert len(calls) == 4 * LAYERS
    with pytest.raises(ValueError, match="mx_ffn=True.*needs on=True"):
        m.set_fp8_compute(False, mx_ffn=True)
    m.set_fp8_compute(False)
    assert torch.equal(_fwd(m), first)


def test_one_quantise_launch_per_block_disappears_and_the_bf16_hidden_state_is_never_written(tmp_path):
    m = _model(tmp_path)
    m.set_fp8_compute(True)
    plain = _fwd(m)
    ws = _workspace(m)
    raw = ws.FFHf.view(torch.uint8)
    assert raw.shape[1] == 2 * FFN, "no adapter pad: the rows of the hidden buffer are 2 FFN bytes"
    used = FFN + FFN // 32                                    # codes, then one scale byte per 32 columns
    # the per-row path writes the bf16 hidden state over a planted pattern
    raw.fill_(SENTINEL_BYTE)
    assert torch.equal(_fwd(m), plain)
    assert not bool((raw[:, used:] == SENTINEL_BYTE).all()), "set_fp8_compute(True) stores bf16 rows in FFH"
    for fused, want in ((False, 6), (True, 3)):
        m.set_fp8_compute(True, fused_quant=fused, mx_ffn=True)
        raw.fill_(SENTINEL_BYTE)
        with _count_quant_rows() as calls:
            mx = _fwd(m)
        assert _workspace(m) is ws
        assert len(calls) == want * LAYERS, f"mx_ffn (fused_quant={fused}): {len(calls)} quantise launches, expected {want} per block"
        assert torch.isfinite(mx).all() and not torch.equal(mx, plain), "block scales change the numbers"
        host = raw.cpu()
        assert bool((host[:, used:] == SENTINEL_BYTE).all()), "bytes behind the codes and scale bytes: no bf16 row was stored"
        codes, scales = host[:, :FFN], host[:, FFN:used]
        assert not bool(((codes & 0x7F) == 0x7F).any()) and int(scales.max()) < 255 and int(scales.min()) >= 1
        assert codes.unique().numel() > 64 and scales.unique().numel() > 2, "the MX hidden state of the last block"
        if fused:
            assert torch.equal(mx, unfused), "fused_quant composes: a launch change only"
        unfused = mx
    # off again: the earlier forward, to the bit
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain), "mx_ffn off again restores the per-row forward bit for bit"
    assert len(calls) == 7 * LAYERS
    m.set_fp8_compute(True, mx_ffn=True)
    assert torch.equal(_fwd(m), unfused), "and on again is the same MX forward"


def test_accuracy_against_the_bf16_compute_forward(tmp_path):
    m = _model(tmp_path)
    ref = _fwd(m)
    m.set_fp8_compute(True)
    row = _fwd(m)
    m.set_fp8_compute(True, mx_ffn=True)
    mx = _fwd(m)
    rel_row = float((row - ref).norm() / ref.norm())
    rel_mx = float((mx - ref).norm() / ref.norm())
    print(f"[wan mx_ffn] {LAYERS} blocks of width {DIM}: rel-L2 against the bf16-compute forward: per-row fp8 {rel_row:.3e}, "
          f"mx_ffn {rel_mx:.3e}, ratio mx / per-row {rel_mx / rel_row:.3f}")
    # measured 2.700e-2 on the MI355X (tests/test_gpu_wan_fp8_compute.py); the bar is 2x that
    measured("wan.fp8_mx_ffn.tiny.per_row.rel_l2", rel_row, 5.4e-2)
    # measured 2.740e-2 on the MI355X (ratio to per-row 1.015: MX is not more accurate here); the bar is 2x that.  The ratio is
    # reported above, not asserted
    measured("wan.fp8_mx_ffn.tiny.mx.rel_l2", rel_mx, 5.48e-2)


def test_the_f32_residual_stream_keeps_its_launches(tmp_path):
    m = _model(tmp_path)
    m.set_residual_dtype(torch.float32)
    m.set_fp8_compute(True)
    with _count_quant_rows() as calls:
        plain = _fwd(m)
    n_plain = len(calls)
    m.set_fp8_compute(True, mx_ffn=True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), plain), "a float residual stream: fp8_mx_route is False, today's launches"
    assert len(calls) == n_plain > 0


def test_run_time_lora_keeps_the_adapter_tail_launches(tmp_path):
    m = _model(tmp_path)
    m.load_lora_adapter({k: v.clone() for k, v in _lora_state().items()}, adapter_name="lx")
    m.set_fp8_compute(True, lora=True)
    tail = _fwd(m)
    m.set_fp8_compute(True, lora=True, mx_ffn=True)
    with _count_quant_rows() as calls:
        assert torch.equal(_fwd(m), tail), "run-time LoRA on the FFN Linears: the adapter-tail launches are kept"
    assert len(calls) == 7 * LAYERS


def test_engine_switch(tmp_path):
    from apex_studio_amd.engine_wan import WanT2VEngine
    from apex_studio_amd.vae_wan import AutoencoderKLWan
    from tests.golden.seeded import seeded, vae_synthetic_state_dict
    from tests.test_gpu_wan_fp8_compute import BF
    m = _model(tmp_path)
    vae = AutoencoderKLWan(base_dim=32, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=1, temperal_downsample=[False, True, True],
                           device=DEV, dtype=BF)
    vae.load_state_dict({k: v.to(BF) for k, v in vae_synthetic_state_dict(vae, 23).items()}, strict=True)
    with pytest.raises(ValueError, match="fp8_mx_ffn=True needs fp8_compute=True"):
        WanT2VEngine(m, m, vae=vae, fp8_mx_ffn=True)
    eng = WanT2VEngine(m, m, vae=vae, fp8_compute=True)
    assert eng.fp8_mx_ffn is False and m._fp8_mx_ffn is False
    eng = WanT2VEngine(m, m, vae=vae, fp8_compute=True, fp8_mx_ffn=True)
    assert eng.fp8_mx_ffn is True and m._fp8_mx_ffn is True
    with _count_quant_rows() as calls:
        frames = eng.run(prompt_embeds=seeded((1, 20, 64), 42).to(DEV), negative_prompt_embeds=seeded((1, 20, 64), 43).to(DEV),
                         height=64, width=64, duration=5, num_inference_steps=2, guidance_scale=(4.0, 3.0),
                         latents=seeded((1, 16, 2, 8, 8), 41).to(DEV))
        torch.cuda.synchronize()
    assert len(calls) == 2 * 2 * 6 * LAYERS, f"{len(calls)}: two steps x (conditional, unconditional) forwards of 6 per block"
    assert frames.shape[-2:] == (64, 64) and torch.isfinite(frames.float()).all() and float(frames.float().std()) > 0
