"""Host side of the f32 residual stream: the C-ABI entries are declared and bound, `set_residual_dtype`
checks its argument on models built without a GPU, and the engines hand the option to their transformer(s)."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF = torch.float32, torch.bfloat16
NEW = ("apexmi_ln_modulate_f32in", "apexmi_ln_modulate2_f32in")

FLUX = dict(patch_size=1, in_channels=64, num_layers=1, num_single_layers=1, attention_head_dim=128, num_attention_heads=2,
            joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
WAN = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=512, num_layers=1, cross_attn_norm=True, eps=1e-6)


def test_f32in_entries_are_declared_and_bound():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    src = open(os.path.join(ROOT, "include", "apexmi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*const float\*\s*x", code), f"{name}: float x in the header"
        assert name in lib.SIGNATURES
    assert lib.SIGNATURES["apexmi_ln_modulate_f32in"] == lib.SIGNATURES["apexmi_ln_modulate"]
    assert lib.SIGNATURES["apexmi_ln_modulate2_f32in"] == lib.SIGNATURES["apexmi_ln_modulate2"]
    # the header says what the float epilogue flag means with a plain bf16 A
    doc = src[src.index("OR-ed into any epilogue above"):src.index("#define APEXMI_EPI_F32_IO")]
    assert "plain bf16" in doc and "R may alias C" in doc and "APEXMI_EPI_BIAS_GATE_RES | APEXMI_EPI_F32_IO" in doc


def test_f32in_entries_validate_their_arguments_on_the_host():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000
    assert L.apexmi_ln_modulate_f32in(P, 3072, P, 3072, 4, 3076, None, None, None, None, 1e-6, 0, None) != 0
    assert "C=3076" in L.apexmi_last_error().decode()
    assert L.apexmi_ln_modulate2_f32in(P, 3072, P, 3072, 4, 3072, None, None, None, None, 1e-6, 0, 9, None, None, None) != 0
    assert "split=9" in L.apexmi_last_error().decode()
    # ldx counts floats (4 per 16 bytes), ldo bf16 elements (8 per 16 bytes)
    assert L.apexmi_ln_modulate_f32in(P, 3076, P, 3076, 4, 3072, None, None, None, None, 1e-6, 0, None) != 0
    assert "16-byte aligned" in L.apexmi_last_error().decode()


@pytest.mark.parametrize("kind", ["flux", "wan"])
@pytest.mark.parametrize("device", ["meta", "cpu"])
def test_set_residual_dtype_checks_its_argument(kind, device):
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.flux import FluxTransformer2DModel
    from apex_studio_amd.wan import WanTransformer3DModel
    m = (FluxTransformer2DModel(**FLUX, device=device, dtype=BF) if kind == "flux"
         else WanTransformer3DModel(**WAN, device=device, dtype=BF))
    assert m.residual_dtype == BF and m.storage_dtype == BF
    m._ws = {"stale": object()}
    assert m.set_residual_dtype(F32) is m and m.residual_dtype == F32 and m._ws == {}, "the workspace is dropped"
    for bad in (torch.float16, torch.float64, None, "float32"):
        with pytest.raises(ValueError, match="residual stream"):
            m.set_residual_dtype(bad)
    assert m.residual_dtype == F32
    with pytest.raises(ValueError, match="residual"):            # all-float storage on top of a float residual
        m.set_storage_dtype(F32)
    assert m.storage_dtype == BF
    m.set_residual_dtype(BF).set_storage_dtype(F32)
    with pytest.raises(ValueError, match="storage_dtype=float32"):
        m.set_residual_dtype(F32)
    assert m.residual_dtype == BF
    m.set_residual_dtype(BF)                                       # bf16 is always allowed


class _Tr:
    def __init__(self):
        self.config = SimpleNamespace(in_channels=64, out_channels=16, guidance_embeds=True)
        self.device, self.dtype = torch.device("cpu"), BF
        self.seen = []

    def set_residual_dtype(self, dtype):
        self.seen.append(dtype)
        return self


def test_engines_forward_the_option():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd.engine_flux import FluxT2IEngine
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    t = _Tr()
    assert FluxT2IEngine(t).residual_dtype is None and t.seen == [], "default: the transformer is left alone (bf16)"
    assert FluxT2IEngine(t, residual_dtype=F32).residual_dtype == F32 and t.seen == [F32]
    for cls in (WanT2VEngine, WanI2VEngine):
        hi, lo = _Tr(), _Tr()
        cls(hi, lo)
        assert hi.seen == [] and lo.seen == []
        cls(hi, lo, residual_dtype=F32)
        assert hi.seen == [F32] and lo.seen == [F32], "both experts"
        one = _Tr()
        cls(one, residual_dtype=BF)
        assert one.seen == [BF], "one model serving as both experts is set once"
