"""The format table behind the MXFP4 / MXFP6 host-side front end (ops._MX_FORMATS): for each row, the code-row bytes and their
inverse, the padded default buffer of the quantiser, the refusals of the record constructor (the same wording apart from the
format's own words), `dequant` of a hand-written record against the format's test reference, and that a format without an
MX-output entry point refuses `out_mx` before the library is asked.  No GPU: CPU and meta tensors."""
import re

import pytest
import torch

from tests import mxfp4_ref, mxfp6_ref

KS = (32, 64, 96, 128, 256)
# per format row: the mode word -> (public record class, test reference, bytes of a row of K codes written down here, K multiple of
# the route, N multiple of an MX output, the words of the messages)
WANT = {
    "fp4": dict(record="Mxfp4Weight", ref=mxfp4_ref, row_bytes=lambda K: K // 2, k_mult=256, mx_n_mult=128, slot="_fp4", bits=4,
                cols="K / 2", name="MXFP4"),
    "fp6": dict(record="Mxfp6Weight", ref=mxfp6_ref, row_bytes=lambda K: 3 * K // 4, k_mult=128, mx_n_mult=None, slot="_fp6", bits=6,
                cols="3 K / 4", name="MXFP6"),
}


def _formats():
    import apex_studio_amd  # noqa: F401
    from apex_studio_amd import ops
    assert [f.mode for f in ops._MX_FORMATS] == ["fp4", "fp6"], "the order `gemm` asks the formats in"
    return [(f, WANT[f.mode]) for f in ops._MX_FORMATS]


def test_the_rows_of_the_table():
    from apex_studio_amd import ops
    for fmt, want in _formats():
        cls = getattr(ops, want["record"])
        assert cls.fmt is fmt and fmt.record == want["record"] and issubclass(cls, ops._MxWeight)
        assert (fmt.slot, fmt.bits, fmt.k_mult, fmt.mx_n_mult, fmt.cols, fmt.name) == tuple(
            want[k] for k in ("slot", "bits", "k_mult", "mx_n_mult", "cols", "name"))
        assert fmt.values == tuple(want["ref"].MAGS) and len(fmt.values) == 1 << (fmt.bits - 1)
        assert callable(getattr(ops, fmt.quant)) and callable(getattr(ops, fmt.gemm))
        with pytest.raises(Exception):
            fmt.bits = 8                                   # frozen
    assert ops.E2M1_VALUES is ops._MXFP4.values and ops.E2M3_VALUES is ops._MXFP6.values


def test_code_row_bytes_and_their_inverse():
    for fmt, want in _formats():
        for K in KS:
            kb = want["row_bytes"](K)
            assert fmt.row_bytes(K) == kb and fmt.k_of(kb) == K, (fmt.mode, K)
            assert kb * 8 == K * fmt.bits


def test_the_default_codes_buffer_has_16_byte_rows():
    from apex_studio_amd import ops
    for fmt, want in _formats():
        for K in KS:
            for M in (1, 5):
                q = ops._empty_mx_codes(fmt, M, K, "meta")
                kb = want["row_bytes"](K)
                assert q.dtype == torch.uint8 and tuple(q.shape) == (M, kb) and q.stride(1) == 1, (fmt.mode, K)
                assert q.stride(0) % 16 == 0 and kb <= q.stride(0) < kb + 16, (fmt.mode, K, q.stride())
                assert q.storage_offset() == 0


def _pair(fmt, N, K):
    return torch.zeros(N, fmt.row_bytes(K), dtype=torch.uint8), torch.full((N, K // 32), 127, dtype=torch.uint8)


def test_the_record_constructor_refuses_malformed_pairs_in_the_formats_own_words():
    from apex_studio_amd import ops
    from apex_studio_amd.lib import ApexMIError
    N, K = 6, 128
    for fmt, want in _formats():
        cls, rec, kb = getattr(ops, want["record"]), want["record"], want["row_bytes"](K)
        q, s = _pair(fmt, N, K)
        r = cls(q, s)
        assert r.shape == (N, K) and r.compute == fmt.mode and r.q is q and r.s is s and r.nbytes() == N * (kb + K // 32)
        assert r.device == q.device and ops._mx_of(fmt, r) is r
        meta = cls(q.to("meta"), s.to("meta"))             # a record that is not on the GPU can still be asked for its route
        assert meta.shape == (N, K)

        def refused(q_, s_, text):
            with pytest.raises(ApexMIError, match="^" + re.escape(text) + "$"):
                cls(q_, s_)
        refused(q.to(torch.int8), s, f"{rec}: the codes must be a torch.uint8 tensor, got torch.int8")
        refused(q, s.float(), f"{rec}: the scales must be a torch.uint8 tensor, got torch.float32")
        refused(q, None, f"{rec}: the scales must be a torch.uint8 tensor, got NoneType")
        refused(q, s[:, :-1], f"{rec}: the scales must be [{N}, {K // 32}] with contiguous rows (K = {K}), got ({N}, {K // 32 - 1})")
        refused(q, s[:-1], f"{rec}: the scales must be [{N}, {K // 32}] with contiguous rows (K = {K}), got ({N - 1}, {K // 32})")
        wide = torch.zeros(N, 2 * kb, dtype=torch.uint8)[:, ::2]
        assert tuple(wide.shape) == (N, kb) and wide.stride(1) == 2
        refused(wide, s, f"{rec}: the codes must be [{N}, {kb}] with contiguous rows (K = {K}), got ({N}, {kb})")
        tall = torch.full((K // 32, N), 127, dtype=torch.uint8).t()
        refused(q, tall, f"{rec}: the scales must be [{N}, {K // 32}] with contiguous rows (K = {K}), got ({N}, {K // 32})")
        padded = torch.zeros(N, kb + 16, dtype=torch.uint8)[:, :kb]                  # a row stride wider than the row is fine
        assert cls(padded, s).shape == (N, K)
    # fp6 alone: a byte count that is not whole 24-byte blocks has no K
    for cols in (23, 25, 36, 100):
        with pytest.raises(ApexMIError, match=r"^Mxfp6Weight: the codes must be a uint8 \[N, 3 K / 4\] tensor of whole 24-byte blocks, "
                                              rf"got \({N}, {cols}\)$"):
            ops.Mxfp6Weight(torch.zeros(N, cols, dtype=torch.uint8), torch.zeros(N, 1, dtype=torch.uint8))
    with pytest.raises(ApexMIError, match=r"^Mxfp6Weight: the codes must be a uint8 \[N, 3 K / 4\] tensor of whole 24-byte blocks, got \(\)$"):
        ops.Mxfp6Weight(None, None)


def test_dequant_of_a_hand_written_record_equals_the_reference():
    from apex_studio_amd import ops
    N, K = 5, 128
    for fmt, want in _formats():
        ref, ncodes = want["ref"], 1 << fmt.bits
        # every code (the negative zero included) at positions that move with the row, and scale bytes on both sides of 2^0 that
        # differ per block and row
        codes = ((torch.arange(N * K).view(N, K) * 7 + torch.arange(N).view(N, 1)) % ncodes).to(torch.uint8)
        assert len(set(codes.flatten().tolist())) == ncodes
        s = (torch.arange(N * (K // 32)).view(N, K // 32) * 5 % 40 + 107).to(torch.uint8)
        q = ref.pack(codes)
        assert tuple(q.shape) == (N, fmt.row_bytes(K))
        assert torch.equal(ops._unpack_codes(fmt, q), codes.long())
        rec = getattr(ops, want["record"])(q, s)
        got, exact = rec.dequant(), ref.dequant(q, s)
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (N, K)
        assert torch.equal(got.double(), exact), fmt.mode                              # every value is exact in bf16
        assert torch.equal(torch.signbit(got), torch.signbit(exact.float())), "the sign of a zero code is kept"
        # the same record behind a row stride wider than the row
        wide = torch.full((N, q.shape[1] + 16), 0xAA, dtype=torch.uint8)
        wide[:, :q.shape[1]] = q
        assert torch.equal(getattr(ops, want["record"])(wide[:, :q.shape[1]], s).dequant(), got)


def test_out_mx_on_a_format_without_that_entry_point_raises_before_any_library_call(monkeypatch):
    from apex_studio_amd import lib, ops
    from apex_studio_amd.lib import ApexMIError

    def no_library():
        raise AssertionError("the library was asked")
    monkeypatch.setattr(lib, "load", no_library)
    M, N, K = 4, 128, 256
    bf = torch.empty(M, N, dtype=torch.bfloat16, device="meta")
    for fmt, want in _formats():
        q, s = _pair(fmt, N, K)
        w = getattr(ops, want["record"])(q.to("meta"), s.to("meta"))
        codes, scales = (t.to("meta") for t in _pair(fmt, M, K))
        out_mx = tuple(t.to("meta") for t in _pair(fmt, M, N))
        if fmt.mx_n_mult is None:
            with pytest.raises(ApexMIError, match=rf"^{fmt.gemm}: out_mx: the {fmt.name} GEMM has no epilogue that quantises its own output"):
                ops._gemm_mx(fmt, codes, scales, w, None, bf, "bias", None, None, out_mx=out_mx)
            assert "out_mx" not in getattr(ops, fmt.gemm).__code__.co_varnames, "the public wrapper keeps its signature"
        else:
            # a format that has the entry point gets as far as the device check of its operands: no refusal of `out_mx` itself
            with pytest.raises(ApexMIError) as err:
                ops._gemm_mx(fmt, codes, scales, w, None, bf, "bias", None, None, out_mx=out_mx)
            assert "out_mx: the" not in str(err.value) and str(err.value).startswith(fmt.gemm), str(err.value)
