"""Coordinate-window attention, host side (no GPU): plan validation and refusals, the "hip_mfma_window" registration, the Wan
switch and the engines forwarding it."""
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import attention_backend as ab
from apex_studio_amd import ops
from apex_studio_amd.lib import ApexMIError


def _raster(f, h, w):
    return torch.stack(torch.meshgrid(torch.arange(f), torch.arange(h), torch.arange(w), indexing="ij"), dim=-1).reshape(-1, 3)


def test_plan_refuses_bad_radii():
    c = _raster(2, 3, 4)
    for radius in ((-1, 0, 0), (0, 0, -3), (1, 2), (1, 2, 3, 4), 5):
        with pytest.raises(ApexMIError, match="radius"):
            ops.window_plan(c, radius=radius)


def test_plan_refuses_bad_coordinates():
    c = _raster(2, 3, 4)
    with pytest.raises(ApexMIError, match=r"\[S, 3\]"):
        ops.window_plan(c.reshape(2, 12, 3), radius=(1, 1, 1))          # wrong rank
    with pytest.raises(ApexMIError, match=r"\[S, 3\]"):
        ops.window_plan(c[:, :2], radius=(1, 1, 1))                     # two coordinates
    with pytest.raises(ApexMIError, match=r"\[S, 3\]"):
        ops.window_plan(c, c.flatten(), radius=(1, 1, 1))               # wrong rank on the keys
    with pytest.raises(ApexMIError, match="integer tensor"):
        ops.window_plan(c.float(), radius=(1, 1, 1))
    with pytest.raises(ApexMIError, match="integer tensor"):
        ops.window_plan(c.tolist(), radius=(1, 1, 1))
    hi = c.clone()
    hi[3, 1] = 32768
    with pytest.raises(ApexMIError, match="int16"):
        ops.window_plan(hi, radius=(1, 1, 1))
    lo = c.clone()
    lo[0, 2] = -32769
    with pytest.raises(ApexMIError, match="int16"):
        ops.window_plan(c, lo, radius=(1, 1, 1))


def test_plan_refuses_the_cpu():
    c = _raster(2, 3, 4)
    with pytest.raises(ApexMIError, match="ROCm device"):
        ops.window_plan(c, radius=(1, 1, 1), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(ApexMIError, match="ROCm device"):
            ops.window_plan(c, radius=(1, 1, 1))


def test_plan_checks_shape_and_device_of_a_launch():
    qc, kc = torch.zeros(10, 4, dtype=torch.int16), torch.zeros(7, 4, dtype=torch.int16)
    plan = ops.WindowPlan(qc, kc, (1, 2, 3), torch.zeros(1, 1, dtype=torch.uint8))
    assert (plan.Sq, plan.Sk, plan.radius) == (10, 7, (1, 2, 3)) and plan.device == torch.device("cpu")
    plan.check(10, 7, torch.device("cpu"), "t")
    with pytest.raises(ApexMIError, match=r"\(10, 7\)"):
        plan.check(7, 10, torch.device("cpu"), "t")
    with pytest.raises(ApexMIError, match="the operands on cuda:0"):
        plan.check(10, 7, torch.device("cuda:0"), "t")


def test_window_ops_refuse_cpu_tensors_and_foreign_plans():
    q = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    plan = ops.WindowPlan(torch.zeros(8, 4, dtype=torch.int16), torch.zeros(8, 4, dtype=torch.int16), (0, 0, 0),
                          torch.zeros(1, 1, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match="no CPU fallback"):
        ops.attention_window(q, q, q, plan)
    with pytest.raises(ApexMIError, match="no CPU fallback"):
        ops.attention_prepared_window(q, q, q, q, 8, plan)


def test_backend_refusals_come_before_any_launch():
    q = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    plan = object()
    with pytest.raises(ApexMIError, match="window_plan"):
        ab.hip_mfma_window(q, q, q)
    with pytest.raises(ApexMIError, match="attn_mask"):
        ab.hip_mfma_window(q, q, q, attn_mask=torch.ones(8, 8, dtype=torch.bool), window_plan=plan)
    with pytest.raises(ApexMIError, match="causal"):
        ab.hip_mfma_window(q, q, q, is_causal=True, window_plan=plan)
    with pytest.raises(ApexMIError, match="dropout"):
        ab.hip_mfma_window(q, q, q, dropout_p=0.1, window_plan=plan)


def test_registration_adds_the_key_and_disturbs_nothing():
    from apex_studio_amd.register import FunctionRegister
    reg = FunctionRegister()
    ab.register(reg, set_default=True)
    assert ab.KEY_WINDOW == "hip_mfma_window" and reg.get(ab.KEY_WINDOW) is ab.hip_mfma_window
    assert (ab.KEY, ab.KEY_SDPA) == ("hip_mfma", "hip_mfma_sdpa")
    assert reg.get(ab.KEY) is ab.hip_mfma and reg.get(ab.KEY_SDPA) is ab.hip_mfma_sdpa
    assert reg.get_default() == ab.KEY
    assert reg.is_available(ab.KEY_WINDOW) == reg.is_available(ab.KEY) == reg.is_available(ab.KEY_SDPA)
    assert sorted(reg) == sorted((ab.KEY, ab.KEY_SDPA, ab.KEY_WINDOW))
    reg2 = FunctionRegister()
    ab.register(reg2)                       # no default unless asked for
    assert not hasattr(reg2, "_default") and ab.KEY_WINDOW in reg2


WAN = dict(patch_size=(1, 2, 2), num_attention_heads=2, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=64,
           freq_dim=256, ffn_dim=512, num_layers=1, cross_attn_norm=True, eps=1e-6)


def test_wan_switch_validates_caches_and_clears(monkeypatch):
    from apex_studio_amd.wan import WanTransformer3DModel
    m = WanTransformer3DModel(**WAN, device="meta")
    assert m._attention_window is None and m._window_plans == {}
    for bad in ((1, 2), (1, -2, 3), 4):
        with pytest.raises(ValueError, match="radius"):
            m.set_attention_window(bad)
    built = []

    def fake_plan(coords, k_coords=None, radius=None, **kw):
        built.append((tuple(coords.shape), k_coords, radius))
        return ("plan", len(built))

    monkeypatch.setattr(ops, "window_plan", fake_plan)
    assert m.set_attention_window([2, 3, 4]) is m and m._attention_window == (2, 3, 4)
    p = m._window_plan((3, 4, 5))
    assert m._window_plan((3, 4, 5)) is p and len(built) == 1                 # cached per (grid, radius)
    assert built[0] == ((60, 3), None, (2, 3, 4))                              # self-attention over the grid's ids
    assert m._window_plan((3, 4, 6)) is not p and len(built) == 2             # another grid: another plan
    m.set_attention_window((2, 3, 5))
    assert m._window_plans == {}                                               # another radius drops the plans
    m._window_plan((3, 4, 6))
    assert built[-1][2] == (2, 3, 5) and len(built) == 3
    m.set_attention_window(None)
    assert m._attention_window is None and m._window_plans == {}
    # the ids the window measures are the ids RoPE rotates by: raster order over (frame, row, column)
    assert torch.equal(_raster(3, 4, 5), WanTransformer3DModel._grid_ids(_OnCpu(), (3, 4, 5)))
    m._window_plans = {"k": 1}
    m._invalidate("moved")                                                     # plans live on the device the model left
    assert m._window_plans == {}


class _OnCpu:
    device = torch.device("cpu")


class _Tr:
    def __init__(self):
        self.config = type("C", (), {"out_channels": 16, "in_channels": 16})()
        self.window = "unset"

    def set_attention_window(self, radius):
        self.window = radius

    def set_residual_dtype(self, dtype):
        self.residual = dtype


@pytest.mark.parametrize("engine", ["t2v", "i2v"])
def test_engines_forward_the_window_to_both_experts(engine):
    from apex_studio_amd.engine_wan import WanI2VEngine, WanT2VEngine
    cls = WanT2VEngine if engine == "t2v" else WanI2VEngine
    hi, lo = _Tr(), _Tr()
    e = cls(hi, lo, attention_window=[2, 11, 20])
    assert e.attention_window == (2, 11, 20) and hi.window == (2, 11, 20) and lo.window == (2, 11, 20)
    hi, lo = _Tr(), _Tr()
    e = cls(hi, lo)
    assert e.attention_window is None and hi.window == "unset" and lo.window == "unset"     # off: the experts are not touched
    one = _Tr()
    e = cls(one, attention_window=(1, 2, 3))
    assert one.window == (1, 2, 3) and e.low_noise_transformer is one


def test_c_entries_validate_on_the_host():
    """The window entry points refuse bad arguments before touching the device (dummy, never dereferenced pointers)."""
    from apex_studio_amd import lib
    L = lib.load()
    P = 0x100000
    i3 = lib.i64x3((128, 128, 128))

    def bad(rc, needle):
        msg = L.apexmi_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    assert L.apexmi_attn_window_map_bytes(585, 585) == 5 * 10 and L.apexmi_attn_window_map_bytes(0, 5) == 0
    bad(L.apexmi_attn_window_map(P, P, 0, 8, 1, 1, 1, P, 64, None), "empty problem")
    bad(L.apexmi_attn_window_map(P, P, 300, 300, 1, 1, 1, P, 14, None), "map buffer too small")
    bad(L.apexmi_attn_window_map(P, P, 300, 300, 1, -1, 1, P, 15, None), "negative radius")
    bad(L.apexmi_attn_window_map(None, P, 300, 300, 1, 1, 1, P, 15, None), "null window operand")
    bad(L.apexmi_attn_fwd_window(P, P, P, P, 1, 2, 2, 8, 8, 80, i3, i3, i3, i3, P, P, 1, 1, 1, P, 1.0, lib.BF16, P, 1 << 30, None),
        "head dim 80")
    bad(L.apexmi_attn_fwd_window(P, P, P, P, 1, 2, 2, 8, 8, 64, i3, i3, i3, i3, P, P, 1, 1, 1, None, 1.0, lib.BF16, P, 1 << 30, None),
        "null window operand")
    bad(L.apexmi_attn_fwd_window(P, P, P, P, 1, 3, 2, 8, 8, 64, i3, i3, i3, i3, P, P, 1, 1, 1, P, 1.0, lib.F16, P, 1 << 30, None),
        "head ratio")
    bad(L.apexmi_attn_fwd_prepared_window(P, P, P, P, 1, 2, 100, 100, 100, i3, P, P, 1, 1, 1, P, 1.0, None), "Skp=100")
    bad(L.apexmi_attn_fwd_prepared_window(P, P, P, P, 1, 2, 100, 100, 128, i3, P, P, 1, 1, -2, P, 1.0, None), "negative radius")
