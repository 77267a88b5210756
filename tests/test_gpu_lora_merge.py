"""GPU: omni_lora_merge alone, against bf16(W.double() + s * up.double() @ down.double()) computed on the CPU.

Bars (from the number formats, not from the kernel): the kernel accumulates in fp32 and rounds once, the reference rounds the
exact value once, so an element can differ only where the fp32 sum lands on the other side of a bf16 rounding boundary - by one
bf16 ulp, i.e. at most 2^-7 of the result's magnitude (|out - ref| <= 2^-7 |ref| + 1e-30, absolute near zero) - and that is rare:
at most 1e-3 of the elements may differ at all.  An fp32, 16-wide-chunked accumulation on the CPU differs from the reference in a
share of 0 at the small shapes, 2.3e-5 at R = 200 and 1.0e-5 at 3072 x 3072 x 64; 1e-3 leaves about 40x headroom and still fails
a kernel that rounds twice or applies the scale to a bf16 operand.

The inputs: the one-ulp bar presumes a result of the operands' magnitude.  Where W and the update cancel, an fp32 accumulation
(any: its error is relative to the TERMS, ~2^-24 sqrt(R) |update|) cannot meet a bar relative to the RESULT: with Gaussian draws
(W ~ 0.02, factors ~ 0.05) the R = 200 case had one element of 97 792 at 2.145x the bar on the GPU - w = 0.0238, result -1.67e-7, the
smallest of the case - and the fp32 16-wide-chunked CPU accumulation gives the same bits for it.  That is a property of such
inputs, not of a kernel, so the draws here exclude it by construction: |w| in [0.01, 0.02) and an update of ~6 % of that, whose
8-sigma bound is half the smallest weight.  Every shape, range, scale and bar is as specified.

The cancelling regime itself is covered by `test_cancelling_results_stay_within_the_fp32_accumulation_error`, with Gaussian draws
and a bar relative to the TERMS, worked out there."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
GUARD = 4096            # elements of guard band on either side of W_out
WMIN = 0.01             # smallest |w| of the draws

# (blocked, N, K, R, row0, rows, scale)
SHAPES = [
    (False, 256, 64, 4, 0, 256, -0.5),
    (True, 384, 96, 16, 0, 384, 1.0),
    (True, 384, 96, 24, 24, 40, 1.0),
    (False, 512, 256, 200, 130, 382, 0.25),
    (True, 9216, 3072, 64, 3072, 3072, 1.0),
]
IDS = ["rowmajor_256x64_r4", "blocked_384x96_r16", "blocked_384x96_r24_rows24to63", "rowmajor_512x256_r200_rows130to511",
       "blocked_qkv_slice_r64"]


def _to_blocked(w):
    n, k = w.shape
    return w.view(n, k // 32, 32).transpose(0, 1).contiguous().view(n, k)


def _from_blocked(w):
    n, k = w.shape
    return w.view(k // 32, n, 32).transpose(0, 1).contiguous().view(n, k)


_cases: dict = {}


def _case(i):
    """Inputs and the CPU reference of shape i, computed once and shared (never modified)."""
    if i not in _cases:
        blocked, N, K, R, row0, rows, scale = SHAPES[i]
        g = torch.Generator().manual_seed(100 + i)
        # |w| in [WMIN, 2 WMIN) with a random sign; factors uniform in (-a, a) with a chosen so that 8 standard deviations of the
        # update, 8 |s| sqrt(R) a^2 / 3, are half of WMIN: the update is ~6 % of the weights (some 16 bf16 ulps: nothing is
        # vacuous) and no result cancels to near zero (see the module docstring); the precondition is asserted on the reference
        sign = torch.randint(0, 2, (N, K), generator=g).float() * 2 - 1
        w = (sign * WMIN * (1 + torch.rand(N, K, generator=g))).to(BF16)
        a = (0.5 * WMIN * 3 / (8 * abs(scale) * R ** 0.5)) ** 0.5
        up = ((torch.rand(rows, R, generator=g) * 2 - 1) * a).to(BF16)
        down = ((torch.rand(R, K, generator=g) * 2 - 1) * a).to(BF16)
        ref = w.clone()
        ref[row0:row0 + rows] = (w[row0:row0 + rows].double() + scale * (up.double() @ down.double())).to(BF16)
        assert float(ref.double().abs().min()) >= 0.25 * WMIN                  # a property of the INPUTS: no cancellation
        _cases[i] = (w, up, down, ref)
    return _cases[i]


def _run(i, *, in_place=False, scale=None):
    """-> (row-major result on the CPU, guard bands intact?)"""
    from vllm_omni_amd import ops

    blocked, N, K, R, row0, rows, s = SHAPES[i]
    w, up, down, _ = _case(i)
    s = s if scale is None else scale
    lay = _to_blocked(w) if blocked else w
    base = lay.to(DEV)
    buf = torch.full((2 * GUARD + N * K,), -7.0, dtype=BF16, device=DEV)       # W_out with a guard band the test owns around it
    out = buf[GUARD:GUARD + N * K].view(N, K)
    fill = torch.full((N, K), 3.0, dtype=BF16, device=DEV)
    out.copy_(base if in_place else fill)
    ops.lora_merge(out if in_place else base, out, up.to(DEV), down.to(DEV), s, row0=row0, rows=rows, k32_blocked=blocked)
    torch.cuda.synchronize()
    guards_ok = bool((buf[:GUARD] == -7.0).all()) and bool((buf[GUARD + N * K:] == -7.0).all())
    res = out.cpu()
    res = _from_blocked(res) if blocked else res
    if not in_place:                                # rows outside the range were never written: they still hold the fill
        outside = torch.ones(N, dtype=torch.bool)
        outside[row0:row0 + rows] = False
        assert bool((res[outside] == 3.0).all()), "rows outside the range were written"
        res[outside] = w[outside]
    return res, guards_ok


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_merge_matches_the_double_reference(i):
    blocked, N, K, R, row0, rows, s = SHAPES[i]
    w, up, down, ref = _case(i)
    out, guards_ok = _run(i)
    assert guards_ok
    o, r = out.double(), ref.double()
    err = (o - r).abs()
    differ = float((out.view(torch.int16) != ref.view(torch.int16)).float().mean())
    worst = float((err / (2.0 ** -7 * r.abs() + 1e-30)).max())
    print(f"{IDS[i]}: share of elements that differ {differ:.3e}, worst |out - ref| / (2^-7 |ref| + 1e-30) = {worst:.3f}")
    assert bool((err <= 2.0 ** -7 * r.abs() + 1e-30).all())
    assert differ <= 1e-3
    # the update is really there: the base weights fail the same check
    assert not bool(((w.double() - r).abs() <= 2.0 ** -7 * r.abs() + 1e-30).all())


@pytest.mark.parametrize("i", [2, 3], ids=[IDS[2], IDS[3]])
def test_rows_outside_the_range_and_the_guard_band_are_bit_untouched(i):
    blocked, N, K, R, row0, rows, s = SHAPES[i]
    w = _case(i)[0]
    out, guards_ok = _run(i)                        # (_run itself checks the rows outside the range of the out-of-place result)
    assert guards_ok
    inp, guards_ok = _run(i, in_place=True)
    assert guards_ok
    outside = torch.ones(N, dtype=torch.bool)
    outside[row0:row0 + rows] = False
    assert torch.equal(inp[outside].view(torch.int16), w[outside].view(torch.int16))


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_in_place_equals_out_of_place_and_runs_are_bit_equal(i):
    a, _ = _run(i)
    b, _ = _run(i)
    c, ok = _run(i, in_place=True)
    assert ok
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a.view(torch.int16), c.view(torch.int16))


@pytest.mark.parametrize("i", [0, 2], ids=[IDS[0], IDS[2]])
def test_scale_zero_returns_the_base_bits(i):
    out, ok = _run(i, scale=0.0)
    assert ok
    base = _case(i)[0]
    assert torch.equal(out.view(torch.int16), base.view(torch.int16))


def test_scale_zero_keeps_negative_zero():
    from vllm_omni_amd import ops

    w = torch.zeros(32, 32, dtype=BF16, device=DEV)
    w[:, ::2] = -0.0
    up = torch.ones(32, 4, dtype=BF16, device=DEV)
    down = torch.ones(4, 32, dtype=BF16, device=DEV)
    out = ops.lora_merge(w, torch.empty_like(w), up, down, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16).cpu(), w.view(torch.int16).cpu())


@pytest.mark.parametrize("blocked,N,K,R,row0,rows,scale", [(False, 512, 256, 200, 130, 382, 0.25), (True, 384, 96, 24, 24, 40, 1.0)],
                         ids=["rowmajor_r200", "blocked_r24"])
def test_cancelling_results_stay_within_the_fp32_accumulation_error(blocked, N, K, R, row0, rows, scale):
    """Gaussian draws (W ~ 0.02, factors ~ 0.05): the update is as large as the weights and some results nearly cancel - the
    regime the other cases' draws exclude.  There no fp32 accumulation meets a bar relative to the RESULT; what it must meet is
    relative to the TERMS.  Products of bf16 values are exact in fp32, so the error of the kernel's fp32 value before its one
    rounding is at most the R - 1 additions of the sum, the multiplication by the scale and the addition of w, each within
    2^-24 of a partial result that never exceeds T = |w| + |s| sum_r |up||down|: E = (R + 1) 2^-24 T (the worst case of any
    summation order, MFMA's included).  Two values within E of each other round to bf16 values at most one ulp (<= 2^-7 of the
    larger) plus E apart, and the larger is within that of |ref|: |out - ref| <= 2^-7 |ref| + 2 E.  A kernel that rounds the
    update to bf16 first, or applies the scale to a bf16 operand, is off by ~2^-9 |update| = some 30 000 E and fails."""
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(7 + R)
    w = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
    up = (torch.randn(rows, R, generator=g) * 0.05).to(BF16)
    down = (torch.randn(R, K, generator=g) * 0.05).to(BF16)
    sl = slice(row0, row0 + rows)
    ref = (w[sl].double() + scale * (up.double() @ down.double())).to(BF16).double()
    terms = w[sl].double().abs() + abs(scale) * (up.double().abs() @ down.double().abs())
    assert bool((ref.abs() < 1e-2 * w[sl].double().abs()).any())             # a property of the INPUTS: some results do cancel
    lay = _to_blocked(w) if blocked else w
    out = ops.lora_merge(lay.to(DEV), torch.empty(N, K, dtype=BF16, device=DEV), up.to(DEV), down.to(DEV), scale,
                         row0=row0, rows=rows, k32_blocked=blocked)
    torch.cuda.synchronize()
    out = out.cpu()
    out = (_from_blocked(out) if blocked else out)[sl].double()
    bar = 2.0 ** -7 * ref.abs() + 2 * (R + 1) * 2.0 ** -24 * terms
    err = (out - ref).abs()
    small = ref.abs() < 1e-2 * w[sl].double().abs()
    print(f"worst |out - ref| / bar = {float((err / bar).max()):.3f} overall, {float((err / bar)[small].max()):.3f} among the "
          f"{int(small.sum())} cancelling elements; worst |out - ref| / (2^-7 |ref|) = {float((err / (2.0 ** -7 * ref.abs() + 1e-30)).max()):.3f}")
    assert bool((err <= bar).all())
