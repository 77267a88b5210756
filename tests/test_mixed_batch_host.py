"""CPU: requests of different resolutions and true-CFG scales in one forward — the host side (no GPU needed).

  1. `build_ragged_batch` with a per-item list of grids: the maps equal the concatenation of the per-item solo batches;
     one grid given per item reproduces the single-grid batch exactly;
  2. the segmented RoPE table: the rows `joint_pos` selects are bit-equal to the rows a solo batch selects from
     `rope_table(grid_i, n_txt)`; text rows below `txt_pos_end`, image rows at or above it;
  3. `batch_key` with `mixed_step_batch`, and `ContinuousStepBatcher.next_group` with `max_step_tokens`;
  4. the compact attention grid: its slot bound covers every q-block, is never below the legacy grid for equal lengths (so
     uniform launches keep the legacy launch), and the slot lookup visits every (item, q-block) exactly once."""
import types

import numpy as np
import pytest
import torch

from vllm_omni_amd.diffusion.batch import build_ragged_batch
from vllm_omni_amd.diffusion.models.qwen_image.rope import rope_table, rope_table_multi

MAPS = ("cu_seqlens", "img_item", "txt_item", "img_joint_row", "txt_joint_row", "joint_pos")
G83, G58, G16, GODD = (1, 83, 83), (1, 58, 104), (1, 16, 16), (1, 5, 9)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_per_item_grids_equal_the_concatenated_solo_batches():
    txt_lens = [7, 3, 11, 5, 2]
    grids = [G16, GODD, G16, (1, 4, 6), GODD]
    temb = [0, 1, 2, 0, 1]
    rb = build_ragged_batch(txt_lens, grids, temb_rows=temb)
    assert rb.mixed and rb.s_imgs == [256, 45, 256, 24, 45] and rb.grids == tuple(grids)
    assert rb.n_img_rows == sum(rb.s_imgs) and rb.n_txt_rows == sum(txt_lens)
    assert rb.max_seqlen == 11 + 256 and rb.n_items == 5 and rb.n_temb == 3
    cu, img_item, txt_item, img_joint, txt_joint = [0], [], [], [], []
    for t, g, e in zip(txt_lens, grids, temb):
        solo = build_ragged_batch([t], g)
        j0 = cu[-1]
        cu.append(j0 + int(solo.cu_seqlens[1]))
        img_item.append(np.full(solo.n_img_rows, e, np.int32))
        txt_item.append(np.full(t, e, np.int32))
        img_joint.append(solo.img_joint_row + j0)
        txt_joint.append(solo.txt_joint_row + j0)
    assert np.array_equal(rb.cu_seqlens, np.asarray(cu, np.int32))
    assert np.array_equal(rb.img_item, np.concatenate(img_item)) and np.array_equal(rb.txt_item, np.concatenate(txt_item))
    assert np.array_equal(rb.img_joint_row, np.concatenate(img_joint)) and np.array_equal(rb.txt_joint_row, np.concatenate(txt_joint))
    for n in MAPS:
        assert getattr(rb, n).dtype == np.int32, n
    assert rb.img_offsets == [0, 256, 301, 557, 581, 626]
    # a mixed batch has no common grid / s_img: asking for one raises instead of answering with item 0's
    with pytest.raises(ValueError, match="different grids"):
        rb.s_img
    with pytest.raises(ValueError, match="different grids"):
        rb.grid
    with pytest.raises(ValueError):
        build_ragged_batch([3, 4], [G16])                               # one grid per item, or one for all
    with pytest.raises(ValueError):
        build_ragged_batch([3, 4], [G16, GODD], img_rows=(0, 8))        # a sequence-parallel chunk needs one grid


@pytest.mark.parametrize("grid", [G16, GODD, ((1, 4, 4), (1, 2, 6))])
def test_one_grid_per_item_reproduces_the_single_grid_batch(grid):
    txt_lens, temb = [5, 9, 2], [0, 1, 0]
    old = build_ragged_batch(txt_lens, grid, temb_rows=temb, txt_pos_end=12)
    new = build_ragged_batch(txt_lens, [grid] * 3, temb_rows=temb, txt_pos_end=12)
    for n in MAPS:
        assert np.array_equal(getattr(old, n), getattr(new, n)), n
    for n in ("txt_lens", "s_imgs", "temb_rows", "n_temb", "grids", "txt_pos_end", "img_start", "s_img", "grid", "n_img_rows",
              "n_txt_rows", "n_joint_rows", "max_seqlen", "mixed"):
        assert getattr(old, n) == getattr(new, n), n
    assert not old.mixed and old.txt_pos_end == 12 and old.s_img == old.s_imgs[0]
    # ... and the single-grid batch is what it always was: text rows 0.., image rows txt_pos_end + 0..
    s = old.s_img
    assert old.grid == tuple(grid) and np.array_equal(old.joint_pos[:5], np.arange(5))
    assert np.array_equal(old.joint_pos[5:5 + s], 12 + np.arange(s))


# ---------------------------------------------------------------------------------------------------------------- 2
def test_segmented_rope_table_is_bit_equal_to_the_solo_tables():
    grids = [G83, G58, G16, GODD, G58, G83]
    txt_lens = [40, 290, 7, 64, 13, 290]
    rb = build_ragged_batch(txt_lens, grids)
    n_txt = 290
    assert rb.distinct_grids == (G83, G58, G16, GODD) and rb.n_txt_pos == n_txt and rb.txt_pos_end == 4 * n_txt
    cos, sin = rope_table_multi(rb.distinct_grids, rb.n_txt_pos)
    assert cos.shape == (4 * n_txt + 83 * 83 + 58 * 104 + 256 + 45, 64) and sin.shape == cos.shape
    for i, (t, g) in enumerate(zip(txt_lens, grids)):
        solo = build_ragged_batch([t], g, txt_pos_end=n_txt)
        c1, s1 = rope_table(g, n_txt)
        rows = rb.joint_pos[rb.cu_seqlens[i]: rb.cu_seqlens[i + 1]]
        assert torch.equal(cos[rows], c1[solo.joint_pos]) and torch.equal(sin[rows], s1[solo.joint_pos]), i
        assert (rows[:t] < rb.txt_pos_end).all() and (rows[t:] >= rb.txt_pos_end).all(), i
        assert rows.max() < cos.shape[0] and rows.min() >= 0
    # the text positions really differ between grids (they start at max(h // 2, w // 2)): one shared segment would be wrong
    assert not torch.equal(cos[:n_txt], cos[n_txt:2 * n_txt])
    # one grid: the table IS the single-grid table
    c, s = rope_table_multi((G16,), 9)
    c1, s1 = rope_table(G16, 9)
    assert torch.equal(c, c1) and torch.equal(s, s1)


# ---------------------------------------------------------------------------------------------------------------- 3
def _pipeline(**cfg):
    """A QwenImagePipeline without weights: `batch_key` reads the config, the cache backend and the sample only."""
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline

    class QwenImageTransformer2DModel:                       # (TeaCache looks its coefficients up by this class name)
        teacache = None

    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16))
    return QwenImagePipeline(od_config=OmniDiffusionConfig(**cfg), device="cpu", transformer=QwenImageTransformer2DModel(), vae=vae)


def _sample(grid, cfg, do_cfg=True, **extra):
    return types.SimpleNamespace(sample=dict(grid=grid, cfg=cfg, do_cfg=do_cfg, **extra))


def test_batch_key_drops_grid_and_scale_only_when_asked_and_allowed():
    a, b = _sample(G83, 4.0), _sample(G58, 2.5)
    on, off = _pipeline(mixed_step_batch=True), _pipeline()
    assert on.batch_key(a) == on.batch_key(b)
    assert off.batch_key(a) != off.batch_key(b)
    assert off.batch_key(a) == (G83, True, 4.0, True, None)                      # flag off: the key is exactly what it was
    assert off.batch_key(_sample(G83, 2.5)) != off.batch_key(a)                  # ... a different scale alone splits
    # what a forward still cannot mix keeps its place in the key
    assert on.batch_key(a) != on.batch_key(_sample(G83, 4.0, do_cfg=False))
    assert on.batch_key(a) != on.batch_key(_sample(G83, 4.0, cfg_normalize=False))
    assert on.batch_key(a) != on.batch_key(_sample(G83, 4.0, t_cond=0))
    # samples with condition rows (Edit / Edit-Plus / Layered) keep their grid
    ca, cb = _sample((G16, GODD), 4.0, cond=torch.zeros(45, 64)), _sample((G16, (1, 4, 6)), 4.0, cond=torch.zeros(24, 64))
    assert on.batch_key(ca) != on.batch_key(cb) and on.batch_key(ca) == off.batch_key(ca)
    # TeaCache configured: the grid stays in the key
    tea = _pipeline(mixed_step_batch=True, cache_backend="tea_cache")
    assert tea.transformer.teacache is not None
    assert tea.batch_key(a) != tea.batch_key(b) and tea.batch_key(a) == off.batch_key(a)


def _req(seed, steps, hw, T=3):
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    g = torch.Generator().manual_seed(100 + seed)
    return OmniDiffusionRequest(height=hw, width=hw, num_inference_steps=steps, seed=seed,
                                prompt_embeds=torch.randn(1, T, 8, generator=g), output_type="latent")


def _mixing_fake(**cfg):
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    class Mixing(FakePipeline):
        @staticmethod
        def batch_key(a):
            return ("mixed", a.sample["do_cfg"])

    return Mixing(OmniDiffusionConfig(**cfg))


def test_next_group_token_budget_oldest_first_longest_first():
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    # image rows: 64 px -> 16, 128 px -> 64, 256 px -> 256 (no CFG in the fake: one branch)
    pipe = _mixing_fake(max_step_batch=8, max_step_tokens=340)
    b = ContinuousStepBatcher(pipe)
    reqs = {"s1": _req(1, 3, 64), "L1": _req(2, 2, 256), "m1": _req(3, 3, 128), "L2": _req(4, 2, 256), "s2": _req(5, 1, 64)}
    for k, r in reqs.items():
        b.add(r, k)
    g = b.next_group()
    # FIFO admission while the budget holds: 16 + 256 + 64 = 336 <= 340, L2 (256 more) does not fit and nothing jumps the queue
    assert sorted(a.tag for a in g) == ["L1", "m1", "s1"]
    assert [a.tag for a in g] == ["L1", "m1", "s1"]                              # handed over longest first
    done = dict(b.drain())
    rows = {"s1": 16, "s2": 16, "m1": 64, "L1": 256, "L2": 256}
    for tags, _ in pipe.steps_run:
        assert sum(rows[t] for t in tags) <= 340, tags
        assert [rows[t] for t in tags] == sorted((rows[t] for t in tags), reverse=True), tags
    assert set(done) == set(reqs)
    for k, r in reqs.items():                                                     # results are those of solo runs
        assert torch.equal(done[k].output, FakePipeline().generate([r])[0].output), k
    assert len(pipe.steps_run) < sum(r.num_inference_steps for r in reqs.values())

    # longest first is STABLE by arrival among equal sizes
    pipe = _mixing_fake(max_step_batch=8)
    b = ContinuousStepBatcher(pipe)
    for k, hw in (("a", 64), ("b", 128), ("c", 64), ("d", 128)):
        b.add(_req(1, 1, hw), k)
    assert [a.tag for a in b.next_group()] == ["b", "d", "a", "c"]

    # a request larger than the budget still runs, alone
    pipe = _mixing_fake(max_step_batch=8, max_step_tokens=100)
    b = ContinuousStepBatcher(pipe)
    b.add(_req(1, 2, 256), "big"); b.add(_req(2, 2, 64), "small")
    assert [a.tag for a in b.next_group()] == ["big"]
    done = dict(b.drain())
    assert set(done) == {"big", "small"} and pipe.steps_run[0][0] == ("big",)
    assert ("small",) in [t for t, _ in pipe.steps_run]


def test_defaults_keep_the_round_robin_groups():
    """Both new fields at their defaults: the groups of the existing round-robin scenario (tests/test_engine_host.py) are
    unchanged — per key, FIFO, `max_items` samples, arrival order."""
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    cfg = OmniDiffusionConfig()
    assert cfg.mixed_step_batch is False and cfg.max_step_tokens is None
    pipe = FakePipeline()
    b = ContinuousStepBatcher(pipe, max_items=2)
    assert b.max_tokens is None
    b.add(_req(1, 4, 64), "s1"); b.add(_req(2, 4, 64), "s2"); b.add(_req(3, 2, 64), "s3")
    b.add(_req(4, 3, 128), "L1")
    b.add(_req(5, 3, 256), "X1")
    b.drain()
    order = [tags for tags, _ in pipe.steps_run]
    assert order == [("s1", "s2"), ("L1",), ("X1",)] * 3 + [("s1", "s2"), ("s3",), ("s3",)]


# ---------------------------------------------------------------------------------------------------------------- 4
def test_compact_attention_slot_bound_and_lookup():
    import random

    from vllm_omni_amd.diffusion.batch import attention_compact_slots, attention_slot_lookup

    rng = random.Random(7)
    for Q in (128, 256):
        for _ in range(400):
            B = rng.randint(1, 64)
            lens = [rng.choice([rng.randint(1, 300), rng.randint(1, 20000)]) for _ in range(B)]
            need = sum(-(-n // Q) for n in lens)
            assert need <= sum(lens) // Q + B                                       # the bound covers every real q-block
            slots = attention_compact_slots(lens, Q)
            legacy = B * -(-max(lens) // Q)
            assert slots == 0 or need <= slots < legacy                             # taken only where it is SMALLER
            if slots:
                cu = np.concatenate([[0], np.cumsum(lens)])
                seen = [attention_slot_lookup(cu, Q, s) for s in range(slots)]
                real = [x for x in seen if x is not None]
                assert len(real) == len(set(real)) == need                          # each (item, q-block) exactly once ...
                assert set(real) == {(i, j) for i, n in enumerate(lens) for j in range(-(-n // Q))}
                assert all(x is None for x in seen[need:]) and all(x is not None for x in seen[:need])  # ... spare slots last
                assert all(j * Q < lens[i] for i, j in real)                        # the block has at least one query row
        # equal lengths: the compact bound is never below the legacy grid -> every uniform launch stays the same launch
        for B in range(1, 65):
            for L in list(range(1, 3 * Q + 2)) + [4160, 16448, 320, 6953]:
                assert B * -(-L // Q) <= (B * L) // Q + B
                assert attention_compact_slots([L] * B, Q) == 0
    # the bench shape, a CFG pair at 256x256 with equal prompts: legacy; the mixed group of the GPU test: compact
    assert attention_compact_slots([4160] * 10, 256) == 0 and attention_compact_slots([256 + 7] * 2, 128) == 0
    assert attention_compact_slots([6920, 6065, 1058, 290] * 2, 256) == 28666 // 256 + 8
    assert attention_compact_slots([290, 1058], 128) == 1348 // 128 + 2 == 12               # the pipe kernels' small mix: 12 < 2 * 9
    assert attention_compact_slots([100] * 65, 128) == 0                            # more items than the walk is built for
