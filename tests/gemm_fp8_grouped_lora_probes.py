"""Cases of the grouped run-time LoRA form of the FP8 GEMM (gemm_fp8.hip: apexmi_gemm_fp8_grouped_lora and
apexmi_gemm_fp8_grouped_qkv_lora; ops.gemm_fp8_grouped(lora_t_list=, lora_B_list=)), on top of tests/gemm_fp8_probes.py and
tests/gemm_fp8_lora_probes.py: which fixed-point problems share a launch, with which epilogue and scale kind, and the single wrong
decisions of a GROUPED kernel that the comparisons must reject.  Pure torch on the CPU.

The contract (include/apexmi.h): every problem of a launch leaves the bits of its own single launch — the arithmetic of
gemm_fp8_lora_probes (scales in the accumulators, adapter tail, bias) when it carries an adapter, the arithmetic of
gemm_fp8_probes when it does not.  tests/test_gpu_gemm_fp8_grouped_lora.py feeds the operands to the kernel;
tests/test_fp8_grouped_lora_host.py evaluates the conditions for every case it runs."""
import functools

import torch

from tests import gemm_fp8_lora_probes as L
from tests import gemm_fp8_probes as P
from tests.gemm_fp8_probes import BF, F8, SPAN_BITS  # noqa: F401

# (M, N, Rp) per problem and the K they share.  MIXED: edge rows and columns behind a full tile, the smallest legal problem
# WITHOUT an adapter, a 3 x 3 tile grid with two rank tiles.  TWIN: nk = 1 straight into two rank tiles, the same shape twice
# with different t / B' (a kernel that reads another problem's adapter entry stores another number).
MIXED = (((130, 144, 64), (1, 16, 0), (257, 272, 128)), 256)
TWIN = (((130, 144, 128), (130, 144, 128)), 128)
GROUPS = {"mixed": MIXED, "twin": TWIN}
# (epilogue, per-row sw, bias present) per problem, one tuple per launch: bias, gelu and gate_res each visit every problem of MIXED,
# with per-row and single sw
MIXED_LAUNCHES = (
    (("gate_res", True, True), ("bias", False, True), ("gelu", True, False)),
    (("bias", False, False), ("gelu", True, True), ("gate_res", False, True)),
    (("gelu", True, True), ("gate_res", True, False), ("bias", True, True)),
)
TWIN_LAUNCHES = (
    (("bias", True, True), ("gate_res", False, True)),
    (("gelu", False, True), ("bias", True, False)),
)
LAUNCHES = {"mixed": MIXED_LAUNCHES, "twin": TWIN_LAUNCHES}

# one-hot rank family on two problems with different Rp: each reads its own t / B' and its own rank count
ONE_HOT_GROUP = ((130, 144, 128), (77, 16, 64))
ONE_HOT_K = 128

# random operands
RANDOM = (((200, 272, 64), (77, 272, 64)), 512)


class Problem:
    """one problem of a group: the Fixed operands `op` and, with Rp > 0, the adapter operands `lo`"""

    def __init__(self, M, N, K, Rp, salt_shift=0):
        self.M, self.N, self.K, self.Rp = M, N, K, Rp
        if Rp:
            lo = L.fixed_point(M, N, K, Rp)
            self.lo = lo if salt_shift == 0 else L.Lora(lo.op, Rp, lo.salt + salt_shift)
            self.op = self.lo.op
        else:
            self.lo, self.op = None, P.fixed_point(M, N, K)

    def pre_activation(self, per_row=True, bias=True):
        return L.pre_activation(self.lo, per_row, bias) if self.lo is not None else P.pre_activation(self.op, per_row, bias)

    def ref(self, epilogue="bias", per_row=True, bias=True):
        """exact float64 result (bias / gate_res)"""
        return L.gemm_ref(self.lo, epilogue, per_row, bias) if self.lo is not None else P.gemm_ref(self.op, epilogue, per_row, bias)

    def span_log2(self, epilogue="bias", per_row=True, bias=True):
        e = "bias" if epilogue == "gelu" else epilogue          # gelu is judged on the exact pre-activation
        return L.span_log2(self.lo, e, per_row, bias) if self.lo is not None else P.span_log2(self.op, e, per_row, bias)

    def want(self, epilogue="bias", per_row=True, bias=True):
        assert self.span_log2(epilogue, per_row, bias) < SPAN_BITS
        return P.expected(self.ref(epilogue, per_row, bias))


@functools.lru_cache(maxsize=None)
def group(name):
    """the problems of one group, built once and shared (callers do not modify them); the second TWIN problem takes the next draw
    of t / B' on the same codes"""
    shapes, K = GROUPS[name]
    seen, out = {}, []
    for M, N, Rp in shapes:
        n = seen.get((M, N, Rp), 0)
        seen[(M, N, Rp)] = n + 1
        out.append(Problem(M, N, K, Rp, salt_shift=n))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def one_hot_group():
    return tuple(L.OneHot(M, N, ONE_HOT_K, Rp) for M, N, Rp in ONE_HOT_GROUP)


# ------------------------------------------------------------------------------- single wrong decisions of a grouped kernel
def grouped_mutants():
    """{name: (problem, wrong float64 pre-epilogue result y, per_row, bias)} — what a grouped kernel that takes ONE wrong decision
    leaves for one problem; the correct one is problem.pre_activation(per_row, bias)"""
    mixed, twin = group("mixed"), group("twin")
    out = {}
    p = mixed[0]
    out["the adapter term dropped for one problem"] = (p, L.mutants(p.lo)["adapter term omitted"], True, True)
    a, b = twin
    op = a.op
    scale = op.sa.double().view(-1, 1) * op.sw.double().view(1, -1)
    out["the problems' t swapped"] = (a, op.acc * scale + b.lo.t.double() @ a.lo.lb.double().T + op.bias.double(), True, True)
    out["the problems' B' swapped"] = (a, op.acc * scale + a.lo.t.double() @ b.lo.lb.double().T + op.bias.double(), True, True)
    p = mixed[2]
    t, lb = p.lo.t.double(), p.lo.lb.double()
    sc = p.op.sa.double().view(-1, 1) * p.op.sw.double().view(1, -1)
    out["the rank tiles swapped"] = (p, p.op.acc * sc + t[:, 64:] @ lb[:, :64].T + t[:, :64] @ lb[:, 64:].T + p.op.bias.double(), True, True)
    out["the rank count of another problem"] = (p, p.op.acc * sc + t[:, :64] @ lb[:, :64].T + p.op.bias.double(), True, True)
    return out


def changed(problem, y, per_row=True, bias=True):
    """number of elements of the expected bf16 buffer (bias epilogue) that the wrong result y changes"""
    return int((y.float().to(BF) != problem.pre_activation(per_row, bias).float().to(BF)).sum())


# --------------------------------------------------------------------------------------------------------- random operands
def quant_reference(a):
    """The formula of `apexmi_quant_rows_fp8`, restated with torch on the CPU (tests/test_gpu_gemm_fp8.py's)."""
    x = a.float()
    amax = x.abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    y = torch.minimum(torch.maximum(x / scale, torch.full_like(x, -448.0)), torch.full_like(x, 448.0))
    return y.to(F8).view(torch.uint8), scale.reshape(-1)


@functools.lru_cache(maxsize=None)
def random_case(M, N, K, Rp):
    """tests/test_gpu_gemm_fp8_lora.py's recipe (per-row sw): random codes and scales, random bf16 t and B' sized so that the
    adapter term is as large as the base product; `ref` = the float64 evaluation of the contract on the same codes"""
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + 11 * Rp)
    qa, sa = quant_reference((torch.randn(M, K, generator=g) * 10.0 ** (torch.rand(M, 1, generator=g) * 2 - 1)).to(BF))
    w = torch.randn(N, K, generator=g) * 0.02
    sw = (w.abs().amax(dim=1) / 448.0).to(BF)
    qw = (w / sw.float().view(-1, 1)).clamp(-448, 448).to(F8)
    bias = torch.randn(N, generator=g).to(BF) * 0.5
    t = (torch.randn(M, Rp, generator=g) * sa.view(-1, 1) * 128.0).to(BF)
    lb = (torch.randn(N, Rp, generator=g) * 0.02 * (K / Rp) ** 0.5).to(BF)
    acc = qa.view(F8).double() @ qw.double().T
    base = acc * sa.double().view(-1, 1) * sw.double().view(1, -1)
    ref = base + t.double() @ lb.double().T + bias.double()
    return dict(qa=qa, sa=sa, qw=qw.view(torch.uint8), sw=sw, bias=bias, t=t, lb=lb, acc=acc, ref=ref, ref_plain=base + bias.double())


def scaling_orders(c):
    """The two orders in which a kernel may apply the scales of a problem WITHOUT an adapter, on the random codes of `c`, as bf16:
    the SCALED epilogue's single expression (acc sa) sw + bias with the last multiply and the add fused, and the in-place order
    of the adapter form, acc = (acc sa) sw rounded to float32, then + bias.  (float64 holds (acc sa) sw + bias of float32 factors
    to well under half a float32 ulp, so rounding it once models the fused form.)"""
    a = (c["acc"].float() * c["sa"].view(-1, 1))
    sw, b = c["sw"].float().view(1, -1), c["bias"].float()
    fused = (a.double() * sw.double() + b.double()).float().to(BF)
    in_place = ((a * sw) + b).to(BF)
    return fused, in_place
