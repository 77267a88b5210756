"""CPU: the GEMM checker of tests/_gemm_check.py is proven before it judges a kernel.

The "kernel" here is an emulation with the product kernel's number formats: torch fp32 matmul of the bf16-rounded operands, bias
added in fp32, one bf16 rounding (GATE_RES: rounded to bf16, then res + gate * c in fp32, rounded again).  The checker must
  * ACCEPT the emulation for every epilogue at small, tail-heavy shapes and at K up to 12288 (suite input scales), and
  * REJECT each of five injected faults of the kind a wrong epilogue or a wrong k-loop produces,
and at the suite's (4160, 1024, 512) shape the test records which of those faults the old whole-tensor bar rel_l2 <= 4e-3 lets
through (OLD_BAR_PASSES below: measured here, asserted so that the record stays true).
"""
import pytest
import torch

import _gemm_check as G
from _util import bf16_round, rel_l2

BF16 = torch.bfloat16
SHAPES = [(257, 264, 64), (300, 264, 192), (257, 264, 3072), (130, 264, 12288)]
BIG = (4160, 1024, 512)
RPI = 100                       # rows per item: item boundaries inside a 256-row tile and inside a 4-row epilogue batch
FAULTS = ["vector8_zeroed", "bias_shift4", "gate_next_item", "k_tail_dropped", "ulp4"]
# rel_l2 of each fault at BIG (GATE_RES) against the fp64 reference, measured with this file; the unfaulted emulation has 1.7e-3:
#   vector8_zeroed 2.0e-3, ulp4 1.7e-3                                   -> the old bar passes them;
#   bias_shift4 5.5e-2, gate_next_item 1.7e-2, k_tail_dropped 2.2e-2      -> the old bar fails them.
# (The expectation that the old bar would also pass a bias shift inside one tile and one row with its neighbour's gate did not
# hold at this shape: one wrong row of 4160 already moves rel_l2 by 1 / sqrt(4160) = 1.6e-2 of a value-sized error.)
OLD_BAR_PASSES = {"vector8_zeroed": True, "bias_shift4": False, "gate_next_item": False, "k_tail_dropped": False, "ulp4": True}


def rnd(shape, seed, scale=1.0):
    return bf16_round(torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale)


class Problem:
    """Suite input scales (tests/test_gpu_ops.py): A ~ N(0, 1), W ~ 0.05 N (0.03 from K = 3072 up), bias ~ 0.5 N, res and gate ~ N."""

    def __init__(self, M, N, K):
        self.M, self.N, self.K = M, N, K
        self.a, self.w, self.b = rnd((M, K), 1), rnd((N, K), 2, 0.05 if K < 3072 else 0.03), rnd((N,), 3, 0.5)
        self.items = -(-M // RPI) + 1                      # one spare item: "the next item" exists for the last row too
        self.res, self.gate = rnd((M, N), 4), rnd((self.items, N), 5)
        self.item = torch.arange(M) // RPI

    def emulate(self, epi, *, bias=None, gate_item=None, drop=None):
        """fp32 emulation; `bias`, `gate_item`, `drop` = (row0, rows, k_from) inject the faults that live before the rounding."""
        c = self.a @ self.w.t()
        if drop is not None:
            r0, nr, k0 = drop
            c[r0:r0 + nr] = self.a[r0:r0 + nr, :k0] @ self.w[:, :k0].t()
        bias_rows = self.b.expand(self.M, self.N) if bias is None else bias
        c = c + bias_rows
        if epi == G.EPI_GELU:
            c = torch.nn.functional.gelu(c, approximate="tanh")
        if epi == G.EPI_GATE_RES:
            item = self.item if gate_item is None else gate_item
            c = self.res + self.gate[item] * bf16_round(c)
        return c.to(BF16)

    def ref(self, epi):
        return G.reference(self.a, self.w, self.b, epi, res=self.res, gate=self.gate, rows_per_item=RPI)

    def faulted(self, fault, epi):
        """The emulated output of epilogue `epi` with one fault injected, each at the spot where it is hardest to see: the last
        row / column tail, one tile, one row, one 32-row block."""
        M, N, K = self.M, self.N, self.K
        if fault == "vector8_zeroed":                      # one 16-byte store that never happened (or wrote zeros)
            y = self.emulate(epi)
            y[M - 1, N - 8:] = 0
            return y
        if fault == "bias_shift4":                         # rows 0..255 x columns 0..255: the bias of column n + 4 (wrapping in the tile)
            tile = min(N, 256)
            bias = self.b.expand(M, N).clone()
            bias[:256, :tile] = torch.roll(self.b[:tile], -4)
            return self.emulate(epi, bias=bias)
        if fault == "gate_next_item":                      # the last row of item 0 takes the gate of item 1
            item = self.item.clone()
            item[RPI - 1] += 1
            return self.emulate(epi, gate_item=item)
        if fault == "k_tail_dropped":                      # one 32-row block stops 64 k early
            return self.emulate(epi, drop=(32, 32, K - 64))
        if fault == "ulp4":                                # one element 4 bf16 steps off, where the bar can see it (see below)
            y = self.emulate(epi)
            r = self.ref(epi)
            bound = G.U * (r.ref.abs() + r.ref.pow(2).mean().sqrt()) + r.extra
            idx = int((r.ref.abs() / bound).argmax())      # the element whose bar is tightest relative to its value
            flat = y.view(-1).view(torch.int16)
            flat[idx] += 4                                 # same sign and binade or the next one up: 4 steps further from zero
            return y
        raise ValueError(fault)


@pytest.fixture(scope="module")
def problems():
    return {s: Problem(*s) for s in SHAPES + [BIG]}


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=str)
def test_checker_accepts_the_fp32_emulation_for_every_epilogue(problems, shape):
    p = problems[shape]
    for epi, name in ((G.EPI_BIAS, "bias"), (G.EPI_GELU, "gelu"), (G.EPI_GATE_RES, "gate_res")):
        r = p.ref(epi)
        G.assert_elementwise(p.emulate(epi), r.ref, r.extra, f"{shape} {name}")
    # the double rounding of GATE_RES stays inside the bar even WITHOUT the extra term at these shapes (worst 5.2e-3 here);
    # the extra term is there for the element whose intermediate sits on a rounding boundary
    r = p.ref(G.EPI_GATE_RES)
    assert G.scaled_error(p.emulate(G.EPI_GATE_RES), r.ref) <= 2 ** -7


def test_reference_honours_the_documented_gate_res_rounding_point():
    """c = 259, gate = 3, res = 0: bf16(259) = 260, so the contract gives 780; without the intermediate rounding 777 -> 776."""
    a, w, b = torch.ones(1, 64), torch.full((8, 64), 4.0), torch.full((8,), 3.0)
    r = G.reference(a, w, b, G.EPI_GATE_RES, res=torch.zeros(1, 8), gate=torch.full((1, 8), 3.0), rows_per_item=1)
    assert torch.equal(r.c64, torch.full((1, 8), 259.0, dtype=torch.float64))
    assert torch.equal(r.ref, torch.full((1, 8), 780.0, dtype=torch.float64))
    assert float(torch.tensor(777.0).to(BF16)) == 776.0


def test_reference_handles_maps_items_and_scales():
    a, w, b = rnd((40, 64), 1), rnd((16, 64), 2, 0.05), rnd((16,), 3, 0.5)
    amap = torch.tensor([5, 3, 39, 0, 7], dtype=torch.int32)
    omap = torch.tensor([2, 0, 6, 1, 4], dtype=torch.int32)
    item = torch.tensor([1, 0, 1, 2, 0], dtype=torch.int32)
    res, gate = rnd((7, 16), 4), rnd((3, 16), 5)
    r = G.reference(a, w, b, G.EPI_GATE_RES, a_row_map=amap, out_row_map=omap, res=res, gate=gate, row_item_map=item)
    for i in range(5):
        c = a[amap[i]].double() @ w.double().t() + b.double()
        assert torch.equal(r.c64[i], c)
        assert torch.equal(r.ref[i], res[omap[i]].double() + gate[item[i]].double() * c.to(BF16).double())
    sa, sw = torch.rand(40) + 0.5, torch.rand(16) + 0.5
    r8 = G.reference(a, w, b, G.EPI_BIAS, a_row_map=amap, a_scale=sa, w_scale=sw)
    want = (a[amap.long()].double() @ w.double().t()) * sa[amap.long()].double()[:, None] * sw.double()[None, :] + b.double()
    assert torch.equal(r8.ref, want)
    x = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    assert torch.allclose(G.gelu_tanh64(x), torch.nn.functional.gelu(x, approximate="tanh"), rtol=0, atol=1e-15)


def _epilogues_of(fault):
    return [G.EPI_GATE_RES] if fault == "gate_next_item" else [G.EPI_BIAS, G.EPI_GELU, G.EPI_GATE_RES]


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_checker_rejects_every_injected_fault(problems, shape, fault):
    """ulp4 is injected at the element where it is MOST visible: the one with the largest |ref| / bound, bound = the bar of that
    element including the GATE_RES extra term (not necessarily the largest |ref|).  4 bf16 steps are 2^-6 .. 2^-5 of the value, the
    bar is 2^-7 * (|ref| + rms) + extra, so this shows that a 4-step error is caught where |ref| is at or above about the rms (and
    the gate term is small) — NOT that it is caught everywhere: a smaller element may legitimately be off by that much in
    absolute terms (cancellation), and the bar lets it."""
    p = problems[shape]
    for epi in _epilogues_of(fault):
        r = p.ref(epi)
        with pytest.raises(AssertionError):
            G.assert_elementwise(p.faulted(fault, epi), r.ref, r.extra, f"{shape} {fault} epilogue {epi}")


@pytest.mark.parametrize("fault", FAULTS)
def test_faults_at_the_suite_shape_and_what_the_old_bar_makes_of_them(problems, fault):
    """(4160, 1024, 512), GATE_RES (the epilogue every fault applies to): the per-element bar fails each fault; the whole-tensor
    rel_l2 <= 4e-3 of the existing GEMM tests passes exactly those recorded in OLD_BAR_PASSES."""
    p = problems[BIG]
    r = p.ref(G.EPI_GATE_RES)
    y = p.faulted(fault, G.EPI_GATE_RES)
    old = rel_l2(y, r.ref.float())
    print(f"{fault}: rel_l2 {old:.3e} (old bar 4e-3), scaled error {G.scaled_error(y, r.ref, r.extra):.3e} (bar {G.U:.3e})")
    with pytest.raises(AssertionError):
        G.assert_elementwise(y, r.ref, r.extra, fault)
    assert (old <= 4e-3) == OLD_BAR_PASSES[fault], f"{fault}: rel_l2 {old:.3e}"


def test_checker_rejects_nan_and_wrong_shape():
    ref = torch.ones(4, 8, dtype=torch.float64)
    got = torch.ones(4, 8, dtype=BF16)
    G.assert_elementwise(got, ref)
    got[2, 3] = float("nan")
    with pytest.raises(AssertionError):
        G.assert_elementwise(got, ref)
    with pytest.raises(AssertionError):
        G.assert_elementwise(torch.ones(4, 7, dtype=BF16), ref)


def test_guard_bands_catch_one_changed_element_in_every_outside_region():
    rows, cols, ld, lead = 6, 16, 24, 64
    written = torch.zeros(rows, dtype=torch.bool)
    written[:4] = True                                     # the call writes rows 0..3; rows 4, 5 are not its to touch

    def fresh():
        view, check = G.guarded(rows, cols, ld, lead=lead, tail=64)
        assert view.shape == (rows, cols) and view.stride() == (ld, 1) and view.dtype == BF16
        assert (view.view(torch.int16) == G.GUARD_BITS).all()
        view[:4] = 1.0
        check(written)
        return view, check

    fresh()
    base = fresh()[0]
    storage_off = base.storage_offset()
    assert storage_off == lead
    for what, off in (("leading band", -1), ("leading band start", -lead), ("trailing band", rows * ld), ("trailing band end", rows * ld + 63),
                      ("slack column", 1 * ld + cols), ("last row's slack", 5 * ld + ld - 1), ("unwritten row", 4 * ld + 3)):
        view, check = fresh()
        raw = torch.as_strided(view, (lead + rows * ld + 64,), (1,), 0)          # the whole allocation
        raw[lead + off] = 2.0
        with pytest.raises(AssertionError):
            check(written, what)
    # an element mask: one element of a written row that the call must leave alone
    view, check = fresh()
    mask = written[:, None].expand(rows, cols).clone()
    mask[2, 5] = False
    with pytest.raises(AssertionError):
        check(mask)
    view.view(torch.int16)[2, 5] = G.GUARD_BITS
    check(mask)
    # without `written` the whole view is the call's
    view[4:] = 3.0
    check()


def test_bf16_ulp_distance():
    a = torch.tensor([1.0, -1.0, 0.0, 256.0]).to(BF16)
    b = torch.tensor([1.0078125, -1.0078125, -0.0, 258.0]).to(BF16)
    assert G.bf16_ulp_distance(a, b).tolist() == [1, 1, 0, 1]
