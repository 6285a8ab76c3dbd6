"""GGUF on the host (no GPU): the container reader / writer, the numpy reference dequantisers the kernels are held to, the
test quantisers, and `weights.iter_checkpoint` on `.gguf` files."""
import struct

import numpy as np
import pytest
import torch

import apex_studio_amd  # noqa: F401
from apex_studio_amd import gguf_file as G, weights
from apex_studio_amd.lib import ApexMIError


def _f16(v):
    return np.array([v], dtype=np.float16).view(np.uint8)


def _rand_f16_bits(rng, n):
    """finite f16 bit patterns, half of them subnormal"""
    e = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 31, n)).astype(np.uint16)
    return ((rng.integers(0, 2, n).astype(np.uint16) << 15) | (e << 10) | rng.integers(0, 1024, n).astype(np.uint16)).astype(np.uint16)


F16_FIELDS = {G.Q4_0: [0], G.Q4_1: [0, 2], G.Q5_0: [0], G.Q5_1: [0, 2], G.Q8_0: [0], G.Q4_K: [0, 2], G.Q5_K: [0, 2], G.Q6_K: [208]}


def random_blocks(ggml_type, numel, seed):
    """Random bytes for `numel` elements of `ggml_type`, every value finite."""
    rng = np.random.default_rng(seed)
    _, blk, bs = G.TYPES[ggml_type]
    if ggml_type == G.F32:
        return (rng.standard_normal(numel) * 10.0 ** rng.integers(-30, 30, numel)).astype(np.float32).view(np.uint8)
    if ggml_type == G.F16:
        return _rand_f16_bits(rng, numel).view(np.uint8)
    if ggml_type == G.BF16:
        bits = rng.integers(0, 1 << 16, numel).astype(np.uint16)
        bits[(bits & 0x7F80) == 0x7F80] &= 0xBFFF
        return bits.view(np.uint8)
    b = rng.integers(0, 256, (numel // blk, bs)).astype(np.uint8)
    for o in F16_FIELDS[ggml_type]:
        b[:, o:o + 2] = _rand_f16_bits(rng, b.shape[0]).reshape(-1, 1).view(np.uint8)
    return b.reshape(-1)


ALL_META = [("t.u8", 200, G.U8), ("t.i8", -100, G.I8), ("t.u16", 60000, G.U16), ("t.i16", -30000, G.I16), ("t.u32", 4000000000, G.U32),
            ("t.i32", -2000000000, G.I32), ("t.f32", 0.5, G.F32V), ("t.bool", True, G.BOOL), ("t.str", "héllo wörld", G.STRING),
            ("t.arr_i32", [1, -2, 3], (G.ARRAY, G.I32)), ("t.arr_str", ["a", "", "ccc"], (G.ARRAY, G.STRING)),
            ("t.arr_f32", [0.25, -1.5], (G.ARRAY, G.F32V)), ("t.u64", 1 << 40, G.U64), ("t.i64", -(1 << 40), G.I64),
            ("t.f64", 1e-300, G.F64), ("general.architecture", "flux", G.STRING)]


@pytest.mark.parametrize("version,alignment", [(3, 32), (2, 32), (3, 64), (3, 4096)])
def test_writer_reader_round_trip(tmp_path, version, alignment):
    w = G.GGUFWriter(str(tmp_path / "a.gguf"), version=version, alignment=alignment)
    for k, v, t in ALL_META:
        w.add_meta(k, v, t)
    tensors = {"a.weight": ((6, 64), G.Q8_0), "b.weight": ((2, 3, 256), G.Q6_K), "c.bias": ((7,), G.F32), "d": ((5, 3), G.F16),
               "e": ((3, 8), G.BF16), "f.weight": ((4, 256), G.Q4_K), "g": ((2, 32), G.Q5_1)}
    data = {k: random_blocks(t, int(np.prod(s)), i) for i, (k, (s, t)) in enumerate(tensors.items())}
    for k, (s, t) in tensors.items():
        w.add_tensor(k, s, t, data[k])
    w.add_tensor("conv.weight", (8, 4 * 1 * 2 * 2), G.F16, random_blocks(G.F16, 128, 99), orig_shape=(8, 4, 1, 2, 2))
    r = G.GGUFReader(w.write())
    assert r.version == version and r.alignment == alignment
    for k, v, t in ALL_META:
        assert r.metadata[k] == (pytest.approx(v) if t in (G.F32V, (G.ARRAY, G.F32V)) else v), k
        assert r.metadata_types[k] == t, k
    assert list(r.keys()) == list(tensors) + ["conv.weight"]
    for k, (s, t) in tensors.items():
        x = r[k]
        assert x.shape == s and x.ggml_type == t and x.offset % alignment == 0 and x.quantized == (t in G.QUANTIZED)
        assert np.array_equal(np.asarray(x.data), data[k]), k
        rb = data[k].size // s[0]
        assert np.array_equal(np.asarray(x.rows(1, s[0])), data[k][rb:]), k        # a row range is a contiguous byte range
    assert r["conv.weight"].shape == (8, 4, 1, 2, 2) and r["conv.weight"].file_shape == (8, 16)
    # the stored ne[] is the torch shape reversed: the first tensor info says ne = [64, 6]
    raw = open(w.path, "rb").read()
    i = raw.index(b"a.weight") + len(b"a.weight")
    assert struct.unpack("<IQQ", raw[i:i + 20]) == (2, 64, 6)
    # loaders: float types as torch tensors, quantised ones as Quantized records
    assert torch.equal(r["c.bias"].read(), torch.from_numpy(data["c.bias"].view(np.float32)))
    assert r["e"].read().dtype == torch.bfloat16 and r["d"].read(1, 3).shape == (2, 3)
    q = r["a.weight"].read(2, 5)
    assert isinstance(q, G.Quantized) and q.shape == (3, 64) and np.array_equal(q.dequantize(), r["a.weight"].read().dequantize()[2:5])


def test_malformed_files_raise_clear_errors(tmp_path):
    p = str(tmp_path / "ok.gguf")
    w = G.GGUFWriter(p)
    w.add_tensor("a", (4, 32), G.Q4_0, random_blocks(G.Q4_0, 128, 1))
    raw = open(w.write(), "rb").read()

    def load(b, name):
        q = str(tmp_path / name)
        open(q, "wb").write(b)
        return G.GGUFReader(q)
    with pytest.raises(ApexMIError, match="bad magic"):
        load(b"GGML" + raw[4:], "magic.gguf")
    with pytest.raises(ApexMIError, match="version 4"):
        load(raw[:4] + struct.pack("<I", 4) + raw[8:], "ver.gguf")
    with pytest.raises(ApexMIError, match="version 1"):
        load(raw[:4] + struct.pack("<I", 1) + raw[8:], "ver1.gguf")
    with pytest.raises(ApexMIError, match="big-endian"):
        load(raw[:4] + struct.pack(">I", 3) + raw[8:], "be.gguf")
    with pytest.raises(ApexMIError, match="past the end"):
        load(raw[:-40], "short.gguf")         # 72 data bytes + 24 of padding: cut into the data
    with pytest.raises(ApexMIError, match="truncated"):
        load(raw[:30], "hdr.gguf")
    # an unsupported type opens (other tensors stay usable) and raises on access, naming the tensor and the type id
    i = raw.index(b"\x02\x00\x00\x00" + struct.pack("<Q", 0), raw.index(b"a") + 1)
    r = load(raw[:i] + struct.pack("<I", 10) + raw[i + 4:], "q2k.gguf")
    with pytest.raises(ApexMIError, match=r"'a'.*type id 10 \(Q2_K\)"):
        r["a"].read()
    with pytest.raises(ApexMIError, match="type id 10"):
        list(weights.iter_checkpoint([r.path]))[0][1]()
    with pytest.raises(ApexMIError, match="block length"):
        w2 = G.GGUFWriter(str(tmp_path / "k.gguf"))
        w2._tensors.append(("b", (2, 48), G.Q8_0, bytes(102)))
        G.GGUFReader(w2.write())


def _block(ggml_type, **fields):
    b = np.zeros(G.TYPES[ggml_type][2], dtype=np.uint8)
    for off, val in fields.values():
        val = np.atleast_1d(val)
        b[off:off + val.size] = val
    return b


def test_reference_dequantisers_on_hand_computed_blocks():
    """One block per type, every field zero but the scale(s) and one payload field; expected values worked out by hand from the
    format definitions."""
    def expect(n, base, **at):
        y = np.full(n, base, dtype=np.float32)
        for k, v in at.items():
            y[int(k[1:])] = v
        return y
    cases = [
        (G.Q4_0, _block(G.Q4_0, d=(0, _f16(2.0)), q=(2 + 3, 0x5A)), expect(32, -16.0, _3=4.0, _19=-6.0)),
        (G.Q4_1, _block(G.Q4_1, d=(0, _f16(0.5)), m=(2, _f16(1.0)), q=(4, 0xF1)), expect(32, 1.0, _0=1.5, _16=8.5)),
        (G.Q5_0, _block(G.Q5_0, d=(0, _f16(1.0)), qh=(2, np.array([(1 << 5) | (1 << 20)], dtype="<u4").view(np.uint8))),
         expect(32, -16.0, _5=0.0, _20=0.0)),
        (G.Q5_1, _block(G.Q5_1, d=(0, _f16(1.0)), m=(2, _f16(-2.0)), qh=(4, np.array([1 << 31], dtype="<u4").view(np.uint8)),
                        q=(8 + 15, 0x30)), expect(32, -2.0, _31=17.0)),
        (G.Q8_0, _block(G.Q8_0, d=(0, _f16(0.25)), q=(2 + 7, 0x80)), expect(32, 0.0, _7=-32.0)),
        # sub-block 5 (group 2, high nibbles): sc = 33 -> scales[9] low nibble 1, scales[1] top bits 2; mn = 17 -> scales[9] high
        # nibble 1, scales[5] top bits 1;  y = 33 * q - 17
        (G.Q4_K, _block(G.Q4_K, d=(0, _f16(1.0)), dm=(2, _f16(1.0)), s1=(4 + 1, 0x80), s5=(4 + 5, 0x40), s9=(4 + 9, 0x11),
                        q=(16 + 64 + 3, 0x70)),
         np.concatenate([np.zeros(160), expect(32, -17.0, _3=214.0), np.zeros(64)]).astype(np.float32)),
        # sub-block 0: sc = 3; element 4 has low nibble 5 and its fifth bit (qh[4] bit 0): y = (2 * 3) * 21
        (G.Q5_K, _block(G.Q5_K, d=(0, _f16(2.0)), s0=(4, 3), qh=(16 + 4, 1), q=(48 + 4, 0x05)), expect(256, 0.0, _4=126.0)),
        # second half, third quarter, l = 20: scale index 8 + 1 + 4 = 13 (= -3), ql[64 + 20] high nibble 11, qh[32 + 20] bits 4-5 = 2:
        # q = (11 | 32) - 32 = 11, y = (0.5 * -3) * 11; its 15 neighbours under the same scale have q = -32
        (G.Q6_K, _block(G.Q6_K, ql=(64 + 20, 0xB0), qh=(128 + 32 + 20, 0x20), sc=(192 + 13, np.array([-3], np.int8).view(np.uint8)),
                        d=(208, _f16(0.5))),
         np.concatenate([np.zeros(128 + 64 + 16), expect(16, 48.0, _4=-16.5), np.zeros(32)]).astype(np.float32)),
        (G.F32, np.array([1.5, -3e-40], np.float32).view(np.uint8), np.array([1.5, -3e-40], np.float32)),
        (G.F16, np.array([1.5, 6e-8], np.float16).view(np.uint8), np.array([1.5, 5.9604645e-08], np.float32)),
        (G.BF16, np.array([0x3FC0, 0xC000], np.uint16).view(np.uint8), np.array([1.5, -2.0], np.float32)),
    ]
    assert {c[0] for c in cases} == set(G.TYPES)
    for t, blk, want in cases:
        got = G.dequantize(t, blk)
        assert got.dtype == np.float32 and got.shape == want.shape, G.type_name(t)
        assert np.array_equal(got, want), (G.type_name(t), np.nonzero(got != want)[0][:8], got[got != want][:8])
    # bf16 rounding is to nearest even: 1 + 2^-8 is a tie and goes to 1, 1 + 3 * 2^-8 is a tie and goes up
    assert list(G.bf16_bits(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0], np.float32))) == [0x3F80, 0x3F82, 0xBF80]


@pytest.mark.parametrize("ggml_type", [G.Q8_0, G.Q4_0, G.Q4_K])
def test_quantise_then_dequantise_is_within_half_a_step(ggml_type):
    """A structural check of the layouts: every value comes back within half a quantisation step of its block
    (d for Q8_0 / Q4_0; d * sc of its sub-block for Q4_K)."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(64 * 256) * np.repeat(10.0 ** rng.uniform(-3, 1, 64 * 8), 32)).astype(np.float32)
    x[:256] = 0.0                                          # an all-zero block
    x[256:512] = np.abs(x[256:512])                        # no negative value: min offset 0
    blocks = G.quantize(ggml_type, x)
    y = G.dequantize(ggml_type, blocks).astype(np.float64)
    _, blk, bs = G.TYPES[ggml_type]
    b = blocks.reshape(-1, bs)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float64)
    if ggml_type == G.Q4_K:
        sc, _ = G._scale_min_k4(b[:, 4:16])
        step = np.repeat((d * sc).reshape(-1), 32)
    else:
        step = np.repeat(d.reshape(-1), blk)
    err = np.abs(y - x.astype(np.float64))
    print(f"[{G.type_name(ggml_type)}] max error / step = {float((err / np.where(step > 0, step, 1)).max()):.4f}")
    assert (err <= 0.5 * step).all(), float((err - 0.5 * step).max())
    assert float(err.max()) > 0 and np.array_equal(y[:256], np.zeros(256))


def _flux_gguf(tmp_path):
    """A BFL-keyed Flux file as GGUF: 2-D block weights quantised, the rest F16 / F32."""
    from tests.golden.make_golden_specs import flux_original_spec
    from tests.golden.seeded import spec_tensors
    sd = spec_tensors(flux_original_spec(dim=256, txt=128, pooled=64), 6000)
    kinds = (G.Q8_0, G.Q4_0, G.Q4_K)
    w = G.GGUFWriter(str(tmp_path / "flux.gguf"))
    w.add_meta("general.architecture", "flux", G.STRING)
    ref = {}
    for i, (k, v) in enumerate(sd.items()):
        v = v.float().numpy()
        if v.ndim == 2 and k.endswith(".weight") and ("double_blocks." in k or "single_blocks." in k) and v.shape[1] % 256 == 0:
            t = kinds[i % 3]
            blocks = G.quantize(t, v)
            ref[k] = G.dequantize_bf16(t, blocks).reshape(v.shape)
        elif v.ndim >= 2:
            t, blocks = G.F16, v.astype(np.float16)
            ref[k] = torch.from_numpy(blocks).to(torch.bfloat16)
        else:
            t, blocks = G.F32, v.astype(np.float32)
            ref[k] = torch.from_numpy(blocks).to(torch.bfloat16)
        w.add_tensor(k, v.shape, t, blocks)
    return w.write(), ref


def test_iter_checkpoint_reads_gguf(tmp_path):
    """Without a converter every tensor name of the file comes back with a loader (the parent commit hands the path to torch.load);
    with the Flux converter ("auto" resolves to it for the Flux model) original-format keys become diffusers keys and q / k / v are
    the right row ranges of the fused quantised tensor."""
    from apex_studio_amd import converters as CV
    from oracle import flux as OF
    path, ref = _flux_gguf(tmp_path)
    plain = dict(weights.iter_checkpoint([path]))
    assert list(plain) == list(ref)
    n_q = 0
    for k, ld in plain.items():
        t = ld()
        n_q += isinstance(t, G.Quantized)
        got = torch.from_numpy(G.bf16_bits(t.dequantize()).view(np.int16)).view(torch.bfloat16) if isinstance(t, G.Quantized) \
            else t.to(torch.bfloat16)
        assert tuple(got.shape) == tuple(ref[k].shape) and torch.equal(got, ref[k]), k
    assert n_q >= 8
    cfg = dict(patch_size=1, in_channels=64, num_layers=2, num_single_layers=2, attention_head_dim=128, num_attention_heads=2,
               joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=True, axes_dims_rope=(16, 56, 56))
    mk = list(OF.FluxTransformer2DModel(**cfg).state_dict().keys())
    conv = CV.get_transformer_converter("flux.base")
    assert isinstance(conv, CV.FluxKeyConverter)
    got = dict(weights.iter_checkpoint([path], conv, None, mk))
    want = CV.FluxKeyConverter().convert(dict(ref), list(mk))          # the same conversion on the dequantised tensors
    assert sorted(got) == sorted(want) == sorted(mk)
    fused = ref["double_blocks.1.img_attn.qkv.weight"]
    for j, n in enumerate(("to_q", "to_k", "to_v")):
        t = got[f"transformer_blocks.1.attn.{n}.weight"]()
        assert isinstance(t, G.Quantized) and t.shape == (256, 256)
        assert torch.equal(torch.from_numpy(G.bf16_bits(t.dequantize()).view(np.int16)).view(torch.bfloat16), fused[256 * j:256 * (j + 1)])
    for k, ld in got.items():
        t = ld()
        v = torch.from_numpy(G.bf16_bits(t.dequantize()).view(np.int16)).view(torch.bfloat16) if isinstance(t, G.Quantized) \
            else t.to(torch.bfloat16)
        assert torch.equal(v, want[k].to(torch.bfloat16)), k


def test_entry_point_validates_its_arguments_on_the_host():
    """apexmi_dequant_gguf checks its arguments before touching the device and leaves the reason in apexmi_last_error():
    exercised without a GPU, with dummy (never dereferenced) pointers."""
    from apex_studio_amd import lib
    L, P = lib.load(), 0x100000
    for args, needle in [((P, 10, 1, 256, P, 256, None), "ggml type 10 is not supported"), ((P, 39, 1, 256, P, 256, None), "type 39"),
                         ((P, G.Q8_0, 1, 100, P, 100, None), "K=100"), ((P, G.Q4_K, 2, 128, P, 128, None), "block length 256"),
                         ((P, G.Q8_0, 4, 32, P, 16, None), "ldo=16"), ((P, G.Q8_0, 4, 32, P, 36, None), "misaligned output"),
                         ((P, G.Q8_0, 4, 32, P + 2, 32, None), "misaligned output"), ((None, G.Q8_0, 4, 32, P, 32, None), "bad arguments")]:
        rc = L.apexmi_dequant_gguf(*args)
        assert rc != 0 and needle in L.apexmi_last_error().decode(), (args, L.apexmi_last_error().decode())
    with pytest.raises(ApexMIError):
        from apex_studio_amd import ops
        ops.dequant_gguf(torch.zeros(34, dtype=torch.uint8), G.Q8_0, (1, 32))          # CPU tensors are refused
