"""GPU: the GEMM checked per element, with exact operands, inside guard bands, on every dispatch path of csrc/gemm.hip launch().

(a) EXACT operands — A in {-1, 0, 1} with at most 96 non-zeros per row, W integers in [-2, 2], bias integers in [-32, 32]: every
    A . W^T + bias is an integer of magnitude <= 224, representable in bf16 and in fp32 whatever the summation order, so every
    path must return the integer result BIT FOR BIT (BIAS, SPLIT3; GATE_RES with integer res and gate in {-1, 0, 1, 2}: the exact
    fp32 value rounded once).  GELU gets an exact input and must be within 1 bf16 step of bf16(gelu64(c)).
(b) ROUNDING-POINT probe — c = 259, gate = 3, res = 0 must give 780 = 3 * bf16(259) on every path (776 without the documented
    intermediate rounding: the direct epilogue of the ring kernel before this test existed).
(c) RANDOM operands at the suite's scales against the fp64 reference with the per-element bar of tests/_gemm_check.py, every
    epilogue on every path, K in {96, 3072, 12288}; the paths that promise the same bits as the default are held to it.
(d) GUARD BANDS on their own: scattered rows, K32-blocked outputs with more rows than the call writes, GATE_RES in place.
Every output of every test lives inside guard bands (leading / trailing band, slack columns of a wider row, rows the call must not
write) and every element is compared.  Paths (how launch() is steered to them):
  auto            ping-pong kernel; K % 64 == 32 -> ring kernel, coalesced epilogue, SADDR DMA
  ring            kernel_hint = GEMM_KERNEL_RING
  ring_vaddr      a row-major a_row_map (fails ring_saddr_ok): ring kernel, coalesced epilogue, VADDR DMA
  direct_*        ring kernel, direct epilogue, one cause each: out only 8-byte aligned, ldo = N + 4, bias only 8-byte aligned,
                  ldres = N + 4
  blocked         K32-blocked A (gathered) and W, K32-blocked out for BIAS / GELU where N % 32 == 0 (gemm_epilogue_direct_k32)
  splitk          workspace given: gemm_bf16_pp_kernel<EPI, 1> + gemm_splitk_finish_kernel, factors 2 / 3 / 4 / 6 / 8
  inlaunch        GEMM_KERNEL_SPLITK_IN_LAUNCH: gemm_bf16_pp_kernel<EPI, 3>
  tail            CU count + 16 tiles: gemm_bf16_pp_kernel<EPI, 2> + gemm_tail_finish_kernel
  fp8, fp8_gather e4m3 bytes written by hand (a table of bytes, all three mantissa bits in use) in the K64-blocked order, fp32 row /
                  channel scales; gemm_bf16_pp_kernel<EPI, 0, 1> with every epilogue, two groups, and a gathered A
Out-of-bounds READS are not tested, timing is not asserted.
"""
import pytest
import torch

import _gemm_check as G

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
CNT = 512                                      # csrc/gemm.hip SPLITK_CNT_INTS
EPI_NAMES = {G.EPI_BIAS: "bias", G.EPI_GELU: "gelu", G.EPI_GATE_RES: "gate_res", G.EPI_SPLIT3: "split3"}
RPI = 100                                      # rows per item of group 0: boundaries inside a tile and inside a 4-row epilogue batch
MT = 75                                        # rows of the second group

PATHS = {
    "auto": {},
    "ring": dict(ring=True),
    "ring_vaddr": dict(gather="rows"),
    "direct_out4": dict(out_lead=4100),
    "direct_ldo4": dict(ld_pad=4),
    "direct_bias4": dict(bias_off=4),
    "direct_ldres4": dict(ldres_pad=4),
    "blocked": dict(gather="blocked"),
    "blocked_ring": dict(gather="blocked", ring=True),
}
PATHS_FP8 = {"fp8": dict(fp8=True), "fp8_gather": dict(fp8=True, gather="blocked")}
# paths whose results are the default kernel's, bit for bit, for ANY operands (csrc/gemm.hip header comment; omni_cdna4.h kernel_hint)
SAME_BITS_AS_AUTO = ["ring", "ring_vaddr", "direct_out4", "direct_ldo4", "direct_bias4", "direct_ldres4", "blocked", "blocked_ring"]


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# OCP e4m3 (1 sign, 4 exponent bits with bias 7, 3 mantissa bits), written out by hand: value -> byte.  1.125 / 1.25 / 1.75 set
# mantissa bits 0 / 1 / 1+2, 0.5 and 3 leave the exponent of 1; negative values set bit 7.
E4M3 = {0.0: 0x00, 0.5: 0x30, 1.0: 0x38, 1.125: 0x39, 1.25: 0x3A, 1.5: 0x3C, 1.75: 0x3E, 2.0: 0x40, 3.0: 0x44}
E4M3.update({-v: b | 0x80 for v, b in list(E4M3.items()) if v})
E4M3_VALUES = sorted(E4M3)


def fp8_bytes(x):
    """[R, K] tensor whose values are all keys of E4M3 -> uint8 [R, K] holding their bytes in the K64-blocked order [K/64][R][64]."""
    vals = torch.tensor(E4M3_VALUES, dtype=torch.float32, device=DEV)
    idx = torch.searchsorted(vals, x.float().contiguous())
    assert bool((vals[idx.clamp(max=len(E4M3_VALUES) - 1)] == x.float()).all()), "a value outside the hand-written e4m3 table"
    b = torch.tensor([E4M3[v] for v in E4M3_VALUES], dtype=torch.uint8, device=DEV)[idx]
    R, K = b.shape
    return b.view(R, K // 64, 64).transpose(0, 1).contiguous().view(R, K)


class Group:
    """Logical operands of one group, on the device: a [M, K], w [N, K], bias [N], res [M, N] (logical rows), gate [items, N]."""

    def __init__(self, M, N, K, seed, kind, items_by_map=False, fp8=False):
        """fp8: a and w hold only values of the E4M3 table (the exact and the probe operands do anyway), and the group carries
        fp32 scales sa [M], sw [N]: c = (a . w^T) * sa[row] * sw[col] + bias.  Ones, except for the random operands."""
        g = _gen(seed)
        self.M, self.N, self.K = M, N, K
        self.sa = torch.ones(M, device=DEV) if fp8 else None
        self.sw = torch.ones(N, device=DEV) if fp8 else None
        self.items = -(-M // RPI) if not items_by_map else 3
        if kind == "exact":
            a = torch.randint(-1, 2, (M, K), generator=g, device=DEV)
            if K > 96:                                             # keep the 96 entries of lowest random rank per row
                rank = torch.rand(M, K, generator=g, device=DEV).argsort(1).argsort(1)
                a = a * (rank < 96)
            self.a = a.to(BF16)
            self.w = torch.randint(-2, 3, (N, K), generator=g, device=DEV).to(BF16)
            self.bias = torch.randint(-32, 33, (N,), generator=g, device=DEV).to(BF16)
            self.res = torch.randint(-64, 65, (M, N), generator=g, device=DEV).to(BF16)
            self.gate = torch.randint(-1, 3, (self.items, N), generator=g, device=DEV).to(BF16)
        elif kind == "probe":                                      # c = 256 + 3 = 259 in every element, gate 3, res 0
            kp = 1 << (K.bit_length() - 1)                         # ones in the first 2^j <= K columns: 256 / 2^j is exact in bf16
            self.a = torch.zeros(M, K, device=DEV, dtype=BF16)
            self.a[:, :kp] = 1.0
            self.w = torch.full((N, K), 256.0 / kp, device=DEV, dtype=BF16)
            self.bias = torch.full((N,), 3.0, device=DEV, dtype=BF16)
            self.res = torch.zeros(M, N, device=DEV, dtype=BF16)
            self.gate = torch.full((self.items, N), 3.0, device=DEV, dtype=BF16)
        else:                                                      # the suite's distributions (tests/test_gpu_ops.py)
            def rnd(shape, scale=1.0):
                return (torch.randn(shape, generator=g, device=DEV) * scale).to(BF16)
            self.a, self.w = rnd((M, K)), rnd((N, K), 0.05 if K < 3072 else 0.03)
            if fp8:                                                # table values (rms 1.5) times scales around 0.15: c of order 1
                vals = torch.tensor(E4M3_VALUES, device=DEV).to(BF16)
                self.a = vals[torch.randint(0, len(vals), (M, K), generator=g, device=DEV)]
                self.w = vals[torch.randint(0, len(vals), (N, K), generator=g, device=DEV)]
                self.sa = torch.rand(M, generator=g, device=DEV) * 0.2 + 0.05
                self.sw = torch.rand(N, generator=g, device=DEV) * 0.2 + 0.05
            self.bias, self.res, self.gate = rnd((N,), 0.5), rnd((M, N)), rnd((self.items, N))
        # group 0: uniform rows_per_item; group 1: a row_item_map with non-monotone items
        self.item = ((torch.arange(M, device=DEV) * 7 + 1) % 3).to(torch.int32) if items_by_map else None

    def reference(self, epi):
        return G.reference(self.a, self.w, self.bias, epi, res=self.res, gate=self.gate, row_item_map=self.item,
                           rows_per_item=0 if self.item is not None else RPI, a_scale=self.sa, w_scale=self.sw)


def make_groups(M, N, K, kind, seed=0, second=True, fp8=False):
    gs = [Group(M, N, K, 1000 + seed, kind, fp8=fp8)]
    if second:
        gs.append(Group(MT, N, K, 2000 + seed, kind, items_by_map=True, fp8=fp8))
    return gs


def run(groups, epi, *, ring=False, gather=None, out_lead=4096, ld_pad=0, bias_off=0, ldres_pad=0, scatter=False, inplace=False,
        out_blocked=None, extra_rows=3, ws=None, hint=None, fp8=False, expect_splitk=None, what=""):
    """One omni_gemm_bf16 call with every output inside guard bands; returns the outputs in LOGICAL row order (SPLIT3: q | k | v
    side by side) after checking the guards.  `ws`: a float32 tensor handed over as split-K workspace; `expect_splitk`: the
    split-K factor omni_gemm_splitk_factor must report for exactly this call; `fp8`: the operands go as e4m3 bytes (K64-blocked,
    which implies the blocked layouts) with the groups' scales; `out_blocked` with `scatter`: a K32-blocked output through an
    out_row_map."""
    from vllm_omni_amd import ops

    N, K = groups[0].N, groups[0].K
    split = epi == G.EPI_SPLIT3
    split_n = N // 3 if split else 0
    blocked = gather == "blocked" or fp8
    if out_blocked is None:
        out_blocked = blocked and epi in (G.EPI_BIAS, G.EPI_GELU) and N % 32 == 0 and not scatter
    args, post = [], []
    for gi, grp in enumerate(groups):
        M = grp.M
        gen = _gen(77 + gi)
        # ---- A: as it is, or gathered from a larger buffer whose other rows hold a value no result survives
        a, amap = grp.a, None
        if gather:
            Ra = M + 37
            amap = torch.randperm(Ra, generator=gen, device=DEV)[:M].to(torch.int32)
            a = torch.full((Ra, K), 7.0, device=DEV, dtype=BF16)
            a[amap.long()] = grp.a
        w = grp.w
        kw = {}
        if fp8:
            sa = grp.sa
            if gather:                                             # a_scale is indexed by the STORED row
                sa = torch.full((Ra,), 1e6, device=DEV)
                sa[amap.long()] = grp.sa
                a = torch.where(a == 7.0, torch.full_like(a, 3.0), a)      # the filler of the unused rows, as a table value
            a, w = fp8_bytes(a), fp8_bytes(w)
            kw.update(a_scale=sa, w_scale=grp.sw)
        elif blocked:
            a, w = ops.w_to_k32_blocked(a), ops.w_to_k32_blocked(w)
        bias = grp.bias
        if bias_off:
            bbuf = torch.zeros(N + 64, device=DEV, dtype=BF16)
            bias = bbuf[bias_off:bias_off + N]
            bias.copy_(grp.bias)
        # ---- outputs
        R = M + (19 if scatter else extra_rows)
        omap = torch.randperm(R, generator=gen, device=DEV)[:M].to(torch.int32) if scatter else None
        orow = omap.long() if scatter else torch.arange(M, device=DEV)
        ncols = split_n if split else N
        outs = [G.guarded(R, ncols, ncols + ld_pad, lead=out_lead if j == 0 else 4096, device=DEV) for j in range(3 if split else 1)]
        if split:
            kw.update(out1=outs[1][0], out2=outs[2][0])
        if epi == G.EPI_GATE_RES:
            if inplace:
                outs[0][0][orow] = grp.res
                res = outs[0][0]
            else:
                res = torch.zeros(R, N + ldres_pad, device=DEV, dtype=BF16)[:, :N]
                res[orow] = grp.res
            kw.update(res=res, gate=grp.gate, gate_item_stride=N, row_item_map=grp.item,
                      rows_per_item=0 if grp.item is not None else RPI)
        args.append(ops.GemmGroupArgs(a, w, bias, outs[0][0], a_row_map=amap, out_row_map=omap, a_k32_blocked=blocked,
                                      out_k32_blocked=out_blocked, **kw))
        post.append((M, R, orow, outs))
    if hint is None:
        hint = ops.GEMM_KERNEL_RING if ring else ops.GEMM_KERNEL_AUTO
    call = dict(split_n=split_n, w_k32_blocked=blocked, splitk_ws=ws, kernel_hint=hint, fp8=fp8)
    if expect_splitk is not None:
        assert ops.gemm_splitk_factor(args, epi, **call) == expect_splitk, f"{what}: not the split-K factor the test is about"
    ops.gemm(args, epi, **call)
    torch.cuda.synchronize()
    results = []
    for gi, (M, R, orow, outs) in enumerate(post):
        got = []
        for j, (view, check) in enumerate(outs):
            if out_blocked:                                        # [N/32][R][32] seen as the [R, N]-shaped buffer it is passed as
                mask = torch.zeros(N // 32, R, 32, dtype=torch.bool, device=DEV)
                mask[:, orow] = True
                check(mask.view(R, N), f"{what} group {gi} K32-blocked out")
                got.append(ops.k32_blocked_to_rows(view.contiguous())[orow])
            else:
                named = torch.zeros(R, dtype=torch.bool, device=DEV)
                named[orow] = True
                check(named, f"{what} group {gi} out{j}")
                got.append(view[orow])
        results.append(torch.cat(got, 1))
    return results


def applicable(path, epi):
    return epi == G.EPI_GATE_RES if path == "direct_ldres4" else True


def shape_n(N, epi):
    """SPLIT3 needs N = 3 * split_n with split_n % 32 == 0: the thirds are 32 (all in one tile), 96 (a third straddles the tile
    boundary) and 256 (one tile per third) columns wide in place of N = 8 / 264 / 520."""
    return {8: 96, 264: 288, 520: 768}[N] if epi == G.EPI_SPLIT3 else N


def check_exact(groups, epi, got, what):
    for gi, (grp, y) in enumerate(zip(groups, got)):
        r = grp.reference(epi)
        assert float(r.c64.abs().max()) <= 256 and torch.equal(r.c64, r.c64.round()), "the operands are not exact"
        if epi == G.EPI_GELU:
            d = G.bf16_ulp_distance(y, r.ref.float().to(BF16))
            assert int(d.max()) <= 1, f"{what} group {gi}: GELU of an exact input is {int(d.max())} bf16 steps from bf16(gelu64(c))"
        else:
            want = r.ref.float().to(BF16)              # an integer below 2^24: exact in fp32, rounded to bf16 once
            bad = (y.view(torch.int16) != want.view(torch.int16)).nonzero()
            assert bad.numel() == 0, (f"{what} group {gi}: {bad.shape[0]} elements differ from the exact result, first at "
                                      f"{bad[0].tolist()}: got {float(y[tuple(bad[0])])}, exact {float(want[tuple(bad[0])])}")


# ------------------------------------------------------------------------------------------------ (a) exact operands
@pytest.mark.parametrize("K", [32, 64, 96, 160, 192, 3072])
@pytest.mark.parametrize("path", list(PATHS))
def test_exact_operands_are_bit_exact_on_every_kernel_and_epilogue_path(path, K):
    shapes = [(M, N) for M in (1, 31, 255, 257, 513) for N in (8, 264, 520)]
    if path.startswith("blocked"):
        shapes += [(257, 288), (31, 32)]               # N % 32 == 0: the K32-blocked output
    if K == 3072:
        shapes = [(1, 8), (31, 264), (257, 520), (513, 264)] + shapes[15:]
    for M, N in shapes:
        for epi in EPI_NAMES:
            if not applicable(path, epi) or (epi == G.EPI_SPLIT3 and N not in (8, 264, 520)):
                continue
            n = shape_n(N, epi)
            groups = make_groups(M, n, K, "exact", seed=M + n, second=M >= 255)
            what = f"exact|{path}|{EPI_NAMES[epi]}|M{M}N{n}K{K}"
            check_exact(groups, epi, run(groups, epi, what=what, **PATHS[path]), what)


def _ws(floats, slack=8192):
    """A NaN-poisoned workspace of exactly `floats` floats inside a larger NaN-poisoned allocation."""
    full = torch.full((floats + slack,), float("nan"), dtype=torch.float32, device=DEV)
    return full, full[:floats]


# 6 tiles (257 + 75 rows x 264 or 288 columns): K -> the factor csrc/gemm.hip splitk_factor() picks (>= 4 K-tiles of 64 per piece)
SPLITK_FACTORS = {512: 2, 768: 3, 1024: 4, 1536: 6, 2048: 8, 3072: 8, 12288: 8}


def run_splitk(groups, epi, in_launch, what):
    """Whole-launch split-K with the workspace sized exactly.  Checks the factor of the call, that every partial was written,
    nothing behind the workspace was, and — in-launch reduce — that the counters behind the partials are zero again."""
    from vllm_omni_amd import ops

    N = groups[0].N
    mtot = sum(g.M for g in groups)
    s = SPLITK_FACTORS[groups[0].K]
    partials = s * mtot * N
    full, ws = _ws(partials + (CNT if in_launch else 0))
    hint = ops.GEMM_KERNEL_SPLITK_IN_LAUNCH if in_launch else ops.GEMM_KERNEL_AUTO
    got = run(groups, epi, ws=ws, hint=hint, expect_splitk=s, what=what)
    assert not bool(torch.isnan(full[:partials]).any()), f"{what}: a partial was not written — the split path did not run"
    assert bool(torch.isnan(full[ws.numel():]).all()), f"{what}: something was written behind the workspace"
    if in_launch:
        assert int(full[partials:partials + CNT].view(torch.int32).abs().sum()) == 0, f"{what}: counters not left zero"
    return got


@pytest.mark.parametrize("K", [512, 768, 1024, 1536, 2048])
@pytest.mark.parametrize("in_launch", [False, True], ids=["splitk", "inlaunch"])
def test_exact_operands_are_bit_exact_through_split_k(in_launch, K):
    for epi in EPI_NAMES:
        n = shape_n(264, epi)
        groups = make_groups(257, n, K, "exact", seed=K)
        if epi == G.EPI_SPLIT3 and K != 1024:
            continue                                   # N = 288 keeps 6 tiles; one K is enough for the scatter of the finish kernels
        what = f"exact|{'inlaunch' if in_launch else 'splitk'}|{EPI_NAMES[epi]}|M257N{n}K{K}"
        check_exact(groups, epi, run_splitk(groups, epi, in_launch, what), what)


def tail_shape():
    """(M, N, tail tiles): CU count + 16 tiles of 256 x 256 with a ragged last row tile and a ragged last column tile."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = cus + 16
    tn = next(t for t in (16, 8, 4, 2, 1) if tiles % t == 0)
    return (tiles // tn) * 256 - 225, tn * 256 - 248, 16


def run_tail(groups, epi, what):
    from vllm_omni_amd import ops

    full, ws = _ws(16 * 4 * 256 * 256, slack=65536)                # 16 tail tiles x 4 splits (K = 2048: 32 K-tiles, 8 per piece)
    got = run(groups, epi, ws=ws, what=what)
    assert not bool(torch.isnan(full[:ws.numel()]).all()), f"{what}: no partial was written — the tail split did not run"
    assert bool(torch.isnan(full[ws.numel():]).all()), f"{what}: something was written behind the workspace"
    plain = run(groups, epi, ws=ws, hint=ops.GEMM_KERNEL_NO_TAIL_SPLIT, what=what + " (no tail split)")
    return got, plain


@pytest.mark.parametrize("epi", list(EPI_NAMES), ids=list(EPI_NAMES.values()))
def test_exact_operands_are_bit_exact_through_the_tail_split(epi):
    M, N, _ = tail_shape()
    if epi == G.EPI_SPLIT3:
        N = (N + 248) // 3 // 32 * 32 * 3                          # a multiple of 96 with the same tile count: ragged last tile too
        assert -(-N // 256) == -(-tail_shape()[1] // 256) and N % 256
    groups = make_groups(M, N, 2048, "exact", seed=5, second=False)
    what = f"exact|tail|{EPI_NAMES[epi]}|M{M}N{N}K2048"
    got, plain = run_tail(groups, epi, what)
    check_exact(groups, epi, got, what)
    check_exact(groups, epi, plain, what + " (no tail split)")


@pytest.mark.parametrize("K", [128, 384])
def test_exact_operands_are_bit_exact_in_fp8(K):
    """Scales of 1: the e4m3 products and their sum are the integers of (a), through every epilogue, on two groups (uniform
    rows_per_item and a non-monotone row_item_map), without and with a gathered A (a_scale then follows the stored row)."""
    for M, N in ((1, 8), (31, 264), (257, 520), (513, 288)):
        for epi in EPI_NAMES:
            if epi == G.EPI_SPLIT3 and N == 288:
                continue
            n = shape_n(N, epi)
            groups = make_groups(M, n, K, "exact", seed=M + n, second=M >= 255, fp8=True)
            for path in PATHS_FP8:
                what = f"exact|{path}|{EPI_NAMES[epi]}|M{M}N{n}K{K}"
                check_exact(groups, epi, run(groups, epi, what=what, **PATHS_FP8[path]), what)


# ------------------------------------------------------------------------------------------------ (b) the rounding point
PROBE = [(p, 64) for p in PATHS] + [("auto", 32), ("ring_vaddr", 96), ("direct_ldres4", 160), ("splitk", 512), ("splitk", 1536),
                                    ("inlaunch", 1024), ("tail", 2048), ("fp8", 128), ("fp8_gather", 384)]


@pytest.mark.parametrize("path,K", PROBE)
def test_gate_res_rounds_the_linear_output_to_bf16_first(path, K):
    """c = 259 everywhere (K ones times 256 / K, + 3), gate 3, res 0: bf16(259) = 260, 3 * 260 = 780 — on every path."""
    what = f"probe|{path}|gate_res|K{K}"
    if path == "tail":
        M, N, _ = tail_shape()
        groups = make_groups(M, N, K, "probe", second=False)
        got = run_tail(groups, G.EPI_GATE_RES, what)[0]
    else:
        groups = make_groups(257, 264, K, "probe", fp8=path in PATHS_FP8)
        if path in ("splitk", "inlaunch"):
            got = run_splitk(groups, G.EPI_GATE_RES, path == "inlaunch", what)
        elif path in PATHS_FP8:                        # (256 / 128 = 2 and 256 / 256 = 1 are e4m3 values)
            got = run(groups, G.EPI_GATE_RES, what=what, **PATHS_FP8[path])
        else:
            got = run(groups, G.EPI_GATE_RES, what=what, **PATHS[path])
    for y in got:
        vals = torch.unique(y.float()).tolist()
        assert vals == [780.0], f"{what}: res + gate * (acc + bias) gave {vals}, the documented rounding point gives 780"


# ------------------------------------------------------------------------------------------------ (c) random operands
def check_random(groups, epi, got, what):
    for gi, (grp, y) in enumerate(zip(groups, got)):
        r = grp.reference(epi)
        G.assert_elementwise(y, r.ref, r.extra, f"{what}|g{gi}")


@pytest.mark.parametrize("K", [96, 3072, 12288])
@pytest.mark.parametrize("epi", list(EPI_NAMES), ids=list(EPI_NAMES.values()))
def test_random_operands_meet_the_elementwise_bar_on_every_path(epi, K):
    shapes = [(1, 8), (31, 264), (255, 520), (257, 264), (513, 520), (257, 288)] if K < 12288 else [(257, 264), (31, 288)]
    for M, N in shapes:
        if epi == G.EPI_SPLIT3 and N == 288:
            continue
        n = shape_n(N, epi)
        groups = make_groups(M, n, K, "random", seed=M + n + K, second=M >= 255)
        base = None
        for path in PATHS:
            if not applicable(path, epi):
                continue
            what = f"random|{path}|{EPI_NAMES[epi]}|M{M}N{n}K{K}"
            got = run(groups, epi, what=what, **PATHS[path])
            check_random(groups, epi, got, what)
            if path == "auto":
                base = got
            elif path in SAME_BITS_AS_AUTO:
                for gi, (x, y) in enumerate(zip(base, got)):
                    assert torch.equal(x, y), f"{what} group {gi}: not the bits of the default path"


@pytest.mark.parametrize("K", [1024, 1536, 3072, 12288])
@pytest.mark.parametrize("in_launch", [False, True], ids=["splitk", "inlaunch"])
def test_random_operands_meet_the_elementwise_bar_through_split_k(in_launch, K):
    """K = 3072 and 12288 split 8-way at 6 tiles (48 / 192 K-tiles); the finish kernel and the in-launch reduce share the summation
    code and must agree bit for bit (tests/test_gpu_splitk_inlaunch.py) — here both are held to the fp64 reference."""
    for epi in EPI_NAMES:
        n = shape_n(264, epi)
        groups = make_groups(257, n, K, "random", seed=K)
        what = f"random|{'inlaunch' if in_launch else 'splitk'}|{EPI_NAMES[epi]}|M257N{n}K{K}"
        check_random(groups, epi, run_splitk(groups, epi, in_launch, what), what)


@pytest.mark.parametrize("epi", list(EPI_NAMES), ids=list(EPI_NAMES.values()))
def test_random_operands_meet_the_elementwise_bar_through_the_tail_split(epi):
    """The unsplit tiles must be the bits of a launch without the tail split; the 16 tail tiles agree to summation order."""
    M, N, tt = tail_shape()
    if epi == G.EPI_SPLIT3:
        N = (N + 248) // 3 // 32 * 32 * 3
    groups = make_groups(M, N, 2048, "random", seed=9, second=False)
    what = f"random|tail|{EPI_NAMES[epi]}|M{M}N{N}K2048"
    got, plain = run_tail(groups, epi, what)
    check_random(groups, epi, got, what)
    check_random(groups, epi, plain, what.replace("tail", "auto_big"))
    d = got[0].view(torch.int16) != plain[0].view(torch.int16)     # (SPLIT3: q | k | v side by side = the GEMM's column order)
    touched = sum(bool(d[r0:r0 + 256, c0:c0 + 256].any()) for r0 in range(0, M, 256) for c0 in range(0, N, 256))
    assert 0 < touched <= tt, f"{what}: {touched} tiles differ from the launch without the tail split, {tt} are tail tiles"


@pytest.mark.parametrize("K", [128, 384])
def test_random_operands_meet_the_elementwise_bar_in_fp8(K):
    """Operands drawn from the hand-written e4m3 table (non-zero mantissas included) with random fp32 row / channel scales: the
    reference is the fp64 product of the dequantised operands, so only the kernel's decode of the bytes, its fp32 epilogue
    arithmetic (acc * a_scale * w_scale + bias, rounded to bf16 BEFORE the gated residual) and the bf16 rounding are in the
    error.  Every epilogue, two groups; the gathered launch must return the bits of the plain one."""
    for M, N in ((31, 264), (257, 520), (513, 288)):
        for epi in EPI_NAMES:
            if epi == G.EPI_SPLIT3 and N == 288:
                continue
            n = shape_n(N, epi)
            groups = make_groups(M, n, K, "random", seed=M + n + K, second=M >= 255, fp8=True)
            base = None
            for path in PATHS_FP8:
                what = f"random|{path}|{EPI_NAMES[epi]}|M{M}N{n}K{K}"
                got = run(groups, epi, what=what, **PATHS_FP8[path])
                check_random(groups, epi, got, what)
                if base is None:
                    base = got
                for gi, (x, y) in enumerate(zip(base, got)):
                    assert torch.equal(x, y), f"{what} group {gi}: not the bits of the launch without a row map"


def test_split3_fused_qk_norm_rope_is_bit_identical_to_the_two_kernel_path_inside_guard_bands():
    """OMNI_EPI_BIAS_SPLIT3_QKNORM_ROPE == SPLIT3 followed by omni_qk_norm_rope on q and k (v untouched), at 1 and 257 image rows
    plus 20 text rows, scattered into joint q / k / v buffers with five rows nobody names."""
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.rope import rope_table

    H, D, K, T, grid = 2, 256, 128, 20, (1, 18, 16)
    cos, sin = rope_table(grid, T)
    cosb, sinb = cos.to(DEV, BF16), sin.to(DEV, BF16)
    g = _gen(3)
    nw = [(torch.randn(128, generator=g, device=DEV) * 0.2 + 1).to(BF16) for _ in range(4)]      # q_img, k_img, q_txt, k_txt
    for Mi in (1, 257):
        img, txt = Group(Mi, 3 * D, K, 50 + Mi, "random"), Group(T, 3 * D, K, 60 + Mi, "random")
        rows = Mi + T
        R = rows + 5
        order = torch.randperm(R, generator=g, device=DEV)[:rows].to(torch.int32)       # joint rows of text (first T) and image
        mt, mi = order[:T].contiguous(), order[T:].contiguous()
        pos = torch.zeros(R, dtype=torch.int32, device=DEV)                              # RoPE table row of every joint row
        pos[mt.long()] = torch.arange(T, dtype=torch.int32, device=DEV)
        pos[mi.long()] = T + torch.arange(Mi, dtype=torch.int32, device=DEV)
        named = torch.zeros(R, dtype=torch.bool, device=DEV)
        named[order.long()] = True
        results = []
        for fused in (False, True):
            bufs = [G.guarded(R, D, device=DEV) for _ in range(3)]
            (q, _), (k, _), (v, _) = bufs
            kw_i = dict(qk_norm_q_w=nw[0], qk_norm_k_w=nw[1], qk_rope_cos=cosb, qk_rope_sin=sinb, qk_row_pos=pos[mi.long()]) if fused else {}
            kw_t = dict(qk_norm_q_w=nw[2], qk_norm_k_w=nw[3], qk_rope_cos=cosb, qk_rope_sin=sinb, qk_row_pos=pos[mt.long()]) if fused else {}
            ops.gemm([ops.GemmGroupArgs(img.a, img.w, img.bias, q, out1=k, out2=v, out_row_map=mi, **kw_i),
                      ops.GemmGroupArgs(txt.a, txt.w, txt.bias, q, out1=k, out2=v, out_row_map=mt, **kw_t)],
                     ops.EPI_BIAS_SPLIT3_QKNORM_ROPE if fused else ops.EPI_BIAS_SPLIT3, split_n=D)
            torch.cuda.synchronize()
            for j, (_, check) in enumerate(bufs):
                check(named, f"{'fused' if fused else 'split3'} Mi={Mi} out{j}")
            if not fused:
                for j, (x, wi, wt) in enumerate(((q, nw[0], nw[2]), (k, nw[1], nw[3]))):
                    dense = x[order.long()].contiguous()                 # the second kernel works on a dense copy of the named rows
                    ops.qk_norm_rope_(dense, H, wi, wt, cosb, sinb, pos[order.long()].contiguous(), T)
                    x[order.long()] = dense
                torch.cuda.synchronize()
            results.append([b[0][order.long()] for b in bufs])
        for j, (x, y) in enumerate(zip(*results)):
            assert torch.isfinite(y.float()).all() and torch.equal(x, y), f"Mi={Mi}: fused output {j} differs from the two-kernel path"
        r = img.reference(G.EPI_SPLIT3)
        G.assert_elementwise(results[0][2][T:], r.ref[:, 2 * D:], 0.0, f"random|auto|split3_v|M{Mi}N{3 * D}K{K}")


# ------------------------------------------------------------------------------------------------ (d) guard bands on their own
@pytest.mark.parametrize("path", ["auto", "ring", "direct_ldo4", "splitk", "inlaunch"])
@pytest.mark.parametrize("epi", list(EPI_NAMES), ids=list(EPI_NAMES.values()))
def test_scattered_rows_leave_the_unnamed_rows_untouched(epi, path):
    """out_row_map scatters M rows into M + 19: every kernel's store goes through the map, the 19 rows nobody names keep their bits
    (GATE_RES reads its residual through the same map)."""
    n = shape_n(264, epi)
    K = 1024 if path in ("splitk", "inlaunch") else 192
    groups = make_groups(257, n, K, "exact", seed=17)
    what = f"scatter|{path}|{EPI_NAMES[epi]}"
    if path in ("splitk", "inlaunch"):
        full, ws = _ws(4 * (257 + MT) * n + CNT)
        from vllm_omni_amd import ops
        got = run(groups, epi, scatter=True, ws=ws, what=what,
                  hint=ops.GEMM_KERNEL_SPLITK_IN_LAUNCH if path == "inlaunch" else ops.GEMM_KERNEL_AUTO)
        assert not bool(torch.isnan(full[:4 * (257 + MT) * n]).any())
    else:
        got = run(groups, epi, scatter=True, what=what, **PATHS[path])
    check_exact(groups, epi, got, what)


@pytest.mark.parametrize("ring", [False, True], ids=["pingpong", "ring"])
@pytest.mark.parametrize("epi", [G.EPI_BIAS, G.EPI_GELU], ids=["bias", "gelu"])
def test_k32_blocked_output_with_more_rows_than_the_call_writes(epi, ring):
    """[N/32][R][32] with R = M + 40: in every 32-column slab the rows M .. R keep their bits (gemm_epilogue_direct_k32 in the
    ping-pong kernel, the coalesced epilogue's blocked store in the ring kernel and — with a row map — in both)."""
    for M, N, K in ((257, 288, 192), (31, 32, 64), (513, 544, 3072)):
        groups = make_groups(M, N, K, "exact", seed=23)
        for scatter in (False, True):
            what = f"k32out|{'ring' if ring else 'auto'}|{EPI_NAMES[epi]}|M{M}N{N}K{K}{'|scatter' if scatter else ''}"
            got = run(groups, epi, gather="blocked", ring=ring, extra_rows=40, scatter=scatter, out_blocked=True, what=what)
            check_exact(groups, epi, got, what)


@pytest.mark.parametrize("path", ["auto", "ring", "ring_vaddr", "direct_out4", "direct_ldo4", "blocked", "splitk", "inlaunch"])
def test_gate_res_in_place(path):
    """res aliases out (the in-place residual of the DiT blocks): every row is read before it is written, by the same thread,
    also where rows are scattered — exact operands, so the result is the exact one bit for bit."""
    K = 1024 if path in ("splitk", "inlaunch") else 192
    for scatter in (False, True):
        groups = make_groups(257, 264, K, "exact", seed=29)
        what = f"inplace|{path}{'|scatter' if scatter else ''}"
        if path in ("splitk", "inlaunch"):
            from vllm_omni_amd import ops
            full, ws = _ws(4 * (257 + MT) * 264 + CNT)
            got = run(groups, G.EPI_GATE_RES, inplace=True, scatter=scatter, ws=ws, what=what,
                      hint=ops.GEMM_KERNEL_SPLITK_IN_LAUNCH if path == "inlaunch" else ops.GEMM_KERNEL_AUTO)
            assert not bool(torch.isnan(full[:4 * (257 + MT) * 264]).any())
        else:
            got = run(groups, G.EPI_GATE_RES, inplace=True, scatter=scatter, what=what, **PATHS[path])
        check_exact(groups, G.EPI_GATE_RES, got, what)
