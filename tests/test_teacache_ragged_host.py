"""CPU: TeaCache in mixed step batches — the host side (no GPU needed).

  1. `TeaCacheDeviceState` on a batch whose items differ in image rows: every item's views cover exactly its own row range
     [img_off[i], img_off[i + 1]) in both layouts (K32-blocked [D/32][rows][32] and row-major), `import_item` / `export_item`
     return a sample's history bit for bit, and the history moves between states of different compositions;
  2. `batch_key` with `mixed_step_batch_teacache`, and the flag's validation;
  3. a ragged state against a library without OMNI_FEATURE_TEACACHE_RAGGED is refused by name, an equal-row state is not."""
import pytest
import torch

from test_mixed_batch_host import _pipeline, _sample
from vllm_omni_amd import _native as N
from vllm_omni_amd.diffusion.batch import build_ragged_batch
from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
from vllm_omni_amd.diffusion.cache.teacache.native import TeaCacheDeviceState

BF16 = torch.bfloat16
GRIDS = [(1, 16, 16), (1, 8, 24), (1, 24, 24)]
OFF = [0, 256, 448, 1024]


@pytest.fixture
def ragged_lib(monkeypatch):
    """The feature query answered without loading a library: the state's own logic is under test here."""
    monkeypatch.setattr(N, "features", lambda: N.FEATURE_ATTN_F16 | N.FEATURE_TEACACHE_RAGGED)


def _saved(rows, D, seed):
    g = torch.Generator().manual_seed(seed)
    mod = torch.randn(rows, D, generator=g).to(BF16)
    res = torch.randn(rows, D, generator=g).to(BF16)
    return mod, res


def _as_saved(mod_rows, res, D, seed):
    """A sample's history in the form `export_item` hands out (prev_mod in the layout of the state)."""
    mod = mod_rows.view(-1, D // 32, 32).permute(1, 0, 2).contiguous() if D % 32 == 0 else mod_rows.clone()
    return dict(mod=mod, res=res.clone(), acc=torch.tensor([0.25 * seed]), cnt=torch.tensor([seed], dtype=torch.int32),
                skip_total=torch.tensor([seed + 1], dtype=torch.int32))


@pytest.mark.parametrize("D", [256, 40], ids=["k32_blocked", "row_major"])
def test_ragged_state_round_trip_and_layout(ragged_lib, D):
    rb = build_ragged_batch([5, 7, 6], GRIDS)
    assert rb.s_imgs == [256, 192, 576] and rb.img_offsets == OFF
    st = TeaCacheDeviceState(TeaCacheConfig(), rb, D, "cpu")
    assert st.img_off == OFF
    hist = []
    for i in range(3):
        mod, res = _saved(rb.s_imgs[i], D, seed=10 + i)
        hist.append((mod, res))
        st.import_item(i, _as_saved(mod, res, D, seed=i + 1))
    # the buffers against a hand-built index: element (row r, column d) of item i sits at image row OFF[i] + r
    all_mod, all_res = torch.cat([h[0] for h in hist]), torch.cat([h[1] for h in hist])
    assert torch.equal(st.prev_res.view(1024, D), all_res)
    if D % 32 == 0:
        want = torch.empty(D // 32 * 1024 * 32, dtype=BF16)
        r, d = torch.meshgrid(torch.arange(1024), torch.arange(D), indexing="ij")
        want[(d // 32) * (1024 * 32) + r * 32 + d % 32] = all_mod
        assert torch.equal(st.prev_mod, want)
    else:
        assert torch.equal(st.prev_mod.view(1024, D), all_mod)
    # every item comes back bit for bit, shaped by its own rows; the items' views do not overlap
    for i in range(3):
        out = st.export_item(i)
        want = _as_saved(*hist[i], D, seed=i + 1)
        assert out["res"].shape == (rb.s_imgs[i], D)
        assert out["mod"].shape == ((D // 32, rb.s_imgs[i], 32) if D % 32 == 0 else (rb.s_imgs[i], D))
        for k in ("mod", "res", "acc", "cnt", "skip_total"):
            assert torch.equal(out[k], want[k]), (i, k)
    # ... shown by painting: item i's views filled with i + 1 leave every element of both buffers painted by its row's owner
    for i in range(3):
        for v in st._item_views(i):
            v.fill_(i + 1)
    owner = torch.repeat_interleave(torch.arange(1, 4), torch.tensor(rb.s_imgs)).to(BF16)         # [1024]: image row -> item + 1
    assert torch.equal(st.prev_res.view(1024, D), owner[:, None].expand(1024, D))
    if D % 32 == 0:
        assert torch.equal(st.prev_mod.view(D // 32, 1024, 32), owner[None, :, None].expand(D // 32, 1024, 32))
    else:
        assert torch.equal(st.prev_mod.view(1024, D), owner[:, None].expand(1024, D))


def test_history_moves_between_compositions(ragged_lib):
    D = 256
    rb = build_ragged_batch([5, 7, 6], GRIDS)
    st = TeaCacheDeviceState(TeaCacheConfig(), rb, D, "cpu")
    hist = [_saved(s, D, seed=20 + i) for i, s in enumerate(rb.s_imgs)]
    for i in range(3):
        st.import_item(i, _as_saved(*hist[i], D, seed=i + 1))
    solo = TeaCacheDeviceState(TeaCacheConfig(), build_ragged_batch([7], GRIDS[1]), D, "cpu")
    solo.import_item(0, st.export_item(1))                             # the 192-row sample leaves the mixed batch ...
    assert torch.equal(solo.prev_res.view(192, D), hist[1][1])
    assert torch.equal(solo.prev_mod.view(D // 32, 192, 32).permute(1, 0, 2).reshape(192, D), hist[1][0])
    assert solo.cnt.tolist() == [2] and solo.skip_total.tolist() == [3] and solo.acc.tolist() == [0.5]
    # ... and joins another composition, in another slot, next to items of other sizes
    rb2 = build_ragged_batch([6, 7], [GRIDS[2], GRIDS[1]])
    st2 = TeaCacheDeviceState(TeaCacheConfig(), rb2, D, "cpu")
    st2.import_item(0, st.export_item(2))
    st2.import_item(1, solo.export_item(0))
    for slot, i in ((0, 2), (1, 1)):
        a, b = st2.export_item(slot), st.export_item(i)
        assert all(torch.equal(a[k], b[k]) for k in a), (slot, i)
    with pytest.raises(ValueError, match="different batch"):
        st2.struct_for(rb)
    with pytest.raises(ValueError, match="different batch"):           # same totals, another split of the rows
        st2.struct_for(build_ragged_batch([6, 7], [(1, 16, 24), (1, 16, 24)]))
    assert st2.struct_for(rb2) is not None


def test_batch_key_with_mixed_step_batch_teacache():
    from test_mixed_batch_host import G16, G58, G83, GODD

    a, b = _sample(G83, 4.0), _sample(G58, 2.5)
    off = _pipeline()
    tea = _pipeline(mixed_step_batch=True, cache_backend="tea_cache")
    both = _pipeline(mixed_step_batch=True, mixed_step_batch_teacache=True, cache_backend="tea_cache")
    assert both.transformer.teacache is not None
    assert both.batch_key(a) == both.batch_key(b) == ("mixed", True, True, None)
    # what a forward still cannot mix keeps its place in the key; a sample with condition rows keeps its grid
    assert both.batch_key(a) != both.batch_key(_sample(G83, 4.0, do_cfg=False))
    ca, cb = _sample((G16, GODD), 4.0, cond=torch.zeros(45, 64)), _sample((G16, (1, 4, 6)), 4.0, cond=torch.zeros(24, 64))
    assert both.batch_key(ca) != both.batch_key(cb) and both.batch_key(ca) == off.batch_key(ca)
    # the new flag off: exactly the keys there were
    assert tea.batch_key(a) != tea.batch_key(b)
    assert tea.batch_key(a) == off.batch_key(a) == (G83, True, 4.0, True, None)
    assert tea.batch_key(b) == off.batch_key(b) == (G58, True, 2.5, True, None)
    # without TeaCache the new flag changes nothing either
    plain, plain_both = _pipeline(mixed_step_batch=True), _pipeline(mixed_step_batch=True, mixed_step_batch_teacache=True)
    for s in (a, b, ca):
        assert plain.batch_key(s) == plain_both.batch_key(s)


def test_flag_alone_is_refused():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    with pytest.raises(ValueError, match="mixed_step_batch"):
        OmniDiffusionConfig(mixed_step_batch_teacache=True)
    cfg = OmniDiffusionConfig()
    assert cfg.mixed_step_batch_teacache is False
    assert OmniDiffusionConfig(mixed_step_batch=True, mixed_step_batch_teacache=True).mixed_step_batch_teacache is True


def test_ragged_state_needs_the_feature_bit(monkeypatch):
    assert N.FEATURE_TEACACHE_RAGGED == 2
    monkeypatch.setattr(N, "features", lambda: N.FEATURE_ATTN_F16)
    with pytest.raises(N.OmniNativeError, match="OMNI_FEATURE_TEACACHE_RAGGED"):
        TeaCacheDeviceState(TeaCacheConfig(), build_ragged_batch([5, 7, 6], GRIDS), 256, "cpu")
    st = TeaCacheDeviceState(TeaCacheConfig(), build_ragged_batch([5, 7, 6], GRIDS[0]), 256, "cpu")   # equal rows: as before
    assert st.img_off == [0, 256, 512, 768]


def test_built_library_reports_the_feature_bit():
    assert N.features() & N.FEATURE_TEACACHE_RAGGED and N.features() & N.FEATURE_ATTN_F16
    assert N.lib().omni_abi_version() == N.ABI_VERSION == 14
