"""GPU: TeaCache in mixed step batches (`OmniDiffusionConfig.mixed_step_batch_teacache`, OMNI_FEATURE_TEACACHE_RAGGED): the
TeaCache kernels of omni_dit_forward address every item by its own image-row range, so requests on different token grids
share a forward and still take their own decisions.

  * forced decisions on ONE ragged forward (the kernel test): items of 256 / 192 / 576 image rows with their CFG twins, row
    tiles that straddle items of different sizes, three skip patterns; on the pipe attention kernel's compact grid (small
    model) and once on the w64 kernel's compact grid (full width, one layer).  Checkers: the same forward without TeaCache
    (computed items: bit-equal), every item ALONE on a one-item batch with the same history and the same forced decision
    (skipped items), the module walk of the plug-in surface for the residual (no TeaCache kernel involved);
  * the step batcher end to end: three requests on three grids, two scales, two step counts, a late joiner; never-skip ==
    TeaCache off bit for bit, always-skip and an intermediate threshold against every request served alone;
  * the guard: with the new flag off a mixed group under TeaCache is refused as before, and an equal-grid TeaCache batch
    gives the bits recorded from the commit before this feature (tests/golden/teacache_step_batched_equal_grid.npz)."""
import os

import numpy as np
import pytest
import torch

from _util import GOLDEN_DIR, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
BAR = 4e-3            # one kernel against its checker
SOLO_BAR = 5e-3       # batched against solo final latents (tests/test_gpu_teacache.py, step-batched TeaCache)
MID_THRESH = 0.2      # the default threshold.  On these inputs it gives a mixed pattern (asserted below; measured: 5 / 3 / 5 skipped
                      # of 8 / 6 / 8 forwards per branch), where the existing test's 0.6 skips every forward but the first


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(*shape, device=DEV, generator=g)).to(BF16)


# --------------------------------------------------------------------------------------------- one forward, forced decisions
def _forced_state(m, rb, hist, compute, n0=0):
    """A TeaCache state for `rb` whose item k carries history hist[n0 + k] (prev_mod rows, prev_res) and a forced decision:
    cnt = 1, acc = 1e7 (>= the threshold of 1e6: compute) or 0 (the rescaled distance of one forward stays far below: skip)."""
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.cache.teacache.native import TeaCacheDeviceState

    D = m.inner_dim
    st = TeaCacheDeviceState(TeaCacheConfig(rel_l1_thresh=1e6), rb, D, DEV)
    for k in range(rb.n_items):
        mod, res = hist[n0 + k]
        st.import_item(k, dict(mod=mod.view(-1, D // 32, 32).permute(1, 0, 2), res=res,
                               acc=torch.tensor([1e7 if compute[k] else 0.0], device=DEV),
                               cnt=torch.ones(1, dtype=torch.int32, device=DEV),
                               skip_total=torch.zeros(1, dtype=torch.int32, device=DEV)))
    return st


def _forced_decisions_case(m, heads, grids, txt_lens, patterns, qblk):
    from vllm_omni_amd.diffusion.batch import attention_compact_slots, build_ragged_batch
    from vllm_omni_amd.diffusion.cache.teacache.extractors import extract_qwen_context

    n, R, D, J = len(grids), len(grids) // 2, m.inner_dim, m.joint_attention_dim
    rb = build_ragged_batch(txt_lens, grids, temb_rows=list(range(R)) * 2)
    off, seq = rb.img_offsets, [t + s for t, s in zip(rb.txt_lens, rb.s_imgs)]
    # which attention kernel the launcher picks (attention.hip) and that this shape takes its compact grid: item_skip is
    # then read through the slot lookup
    assert (n * heads * -(-max(seq) // 256) >= 512) == (qblk == 256)
    assert 0 < attention_compact_slots(seq, qblk) < n * -(-max(seq) // qblk)
    lat_r = [_rnd(rb.s_imgs[r], 64, seed=10 + r) for r in range(R)]
    lat = torch.cat(lat_r * 2)                                            # a CFG pair shares its latents
    txt_i = [_rnd(t, J, seed=30 + i) for i, t in enumerate(txt_lens)]
    txt = torch.cat(txt_i)
    sig = torch.tensor([0.6015625, 0.25, 0.90625][:R], device=DEV)
    # history: another scale per item, so that every item has its own relative distance (rows of a neighbour would show)
    hist = [(_rnd(rb.s_imgs[i], D, seed=50 + i, scale=0.5 + 0.25 * i), _rnd(rb.s_imgs[i], D, seed=70 + i)) for i in range(n)]
    prepared = m.prepare_batch(rb)
    plain = m.forward_ragged(prepared, lat, txt, sig).clone()
    # every item alone (a one-item batch: the equal-row path): skipped with this history -> output, accumulator; computed ->
    # the new prev_mod.  The residual of a computed item from the module walk: hidden after the blocks - hidden before them
    solo_skip, solo_acc, solo_mod, solo_res = [], [], [], []
    for i in range(n):
        rb1 = build_ragged_batch([txt_lens[i]], grids[i])
        p1, s1 = m.prepare_batch(rb1), sig[i % R:i % R + 1].clone()
        li = lat_r[i % R].contiguous()
        st1 = _forced_state(m, rb1, hist, [False], n0=i)
        solo_skip.append(m.forward_ragged(p1, li, txt_i[i], s1, teacache=st1).clone())
        assert st1.skip.tolist() == [1]
        solo_acc.append(float(st1.acc[0]))
        st1 = _forced_state(m, rb1, hist, [True], n0=i)
        m.forward_ragged(p1, li, txt_i[i], s1, teacache=st1)
        assert st1.skip.tolist() == [0]
        solo_mod.append(st1.export_item(0)["mod"])
        ctx = extract_qwen_context(m, hidden_states=li[None], encoder_hidden_states=txt_i[i][None], encoder_hidden_states_mask=None,
                                   timestep=s1, img_shapes=[[grids[i]]], txt_seq_lens=[txt_lens[i]], return_dict=False)
        h, _ = ctx.run_transformer_blocks()
        solo_res.append((h.float() - ctx.hidden_states.float())[0])
        print(f"   item {i} ({rb.s_imgs[i]} rows) alone: residual kernel vs module walk {rel_l2(st1.export_item(0)['res'], solo_res[i]):.3e}, "
              f"rescaled distance of the skip run {solo_acc[i]:.4f}")
    for skip in patterns:
        assert len(skip) == n and any(skip) and not all(skip)
        st = _forced_state(m, rb, hist, [not s for s in skip])
        out = m.forward_ragged(prepared, lat, txt, sig, teacache=st).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        assert st.skip.tolist() == [int(s) for s in skip], (st.skip.tolist(), skip)
        assert st.cnt.tolist() == [2] * n and st.skip_total.tolist() == [int(s) for s in skip]
        # the row-tile predicates: a tile is skipped only when every item with a row in it is
        want_tiles = [int(all(skip[i] for i in range(n) if off[i] <= min(256 * t + 255, off[-1] - 1) and off[i + 1] > 256 * t))
                      for t in range(-(-off[-1] // 256))]
        assert st.tile_img.tolist() == want_tiles
        for i in range(n):
            rows = slice(off[i], off[i + 1])
            mod_i, res_i = st.export_item(i)["mod"], st.export_item(i)["res"]
            r_mod = rel_l2(mod_i, solo_mod[i])
            if skip[i]:
                r_out, acc = rel_l2(out[rows], solo_skip[i]), float(st.acc[i])
                print(f"   pattern {''.join('s' if s else 'C' for s in skip)} item {i}: skipped; rows vs the item alone {r_out:.3e}; "
                      f"rescaled distance {acc:.4f} (alone {solo_acc[i]:.4f}); prev_mod vs alone {r_mod:.3e}")
                assert r_out <= BAR, (i, r_out)
                assert torch.equal(res_i, hist[i][1]), i                 # the cached residual of a skipped item is untouched
                # `acc` of a skipped item holds |p(rel)|: the polynomial of its relative distance rel = mean|mod - prev| /
                # mean|prev| (a ratio between 1 and 2.5 with this history: p(rel) = -400 ... -8300).  The item's sums are those
                # of its solo run up to the order of the atomic adds (1e-7); rel is rounded to bf16 (one ulp: at most 2^-7
                # relative) and the polynomial's relative slope rel p'(rel) / p(rel) stays below 5 on [1, 2.5]: |p| within 5 %
                assert abs(acc - solo_acc[i]) <= 0.05 * abs(solo_acc[i]), (i, acc, solo_acc[i])
            else:
                r_res = rel_l2(res_i, solo_res[i])
                print(f"   pattern {''.join('s' if s else 'C' for s in skip)} item {i}: computed; prev_res vs the walk alone {r_res:.3e}; "
                      f"prev_mod vs alone {r_mod:.3e}")
                assert torch.equal(out[rows], plain[rows]), i            # the predicates only remove work
                assert r_res <= BAR, (i, r_res)
                assert float(st.acc[i]) == 0.0
            assert r_mod <= BAR, (i, r_mod)                               # prev <- this forward's modulated input, own rows


def test_forced_decisions_on_one_ragged_forward():
    from test_gpu_teacache import HEADS, _model

    m, _ = _model()
    grids = [(1, 16, 16), (1, 8, 24), (1, 24, 24)] * 2
    from vllm_omni_amd.diffusion.batch import build_ragged_batch

    assert build_ragged_batch([1] * 6, grids).img_offsets == [0, 256, 448, 1024, 1280, 1472, 2048]
    patterns = [[False, True, False, False, True, False],                # only the middle-sized items skip
                [False, False, True, False, False, True],                # only the largest
                [True, True, True, False, True, True]]                   # all but one
    _forced_decisions_case(m, HEADS, grids, [11, 6, 9, 6, 7, 5], patterns, qblk=128)


def test_forced_decisions_on_the_w64_compact_grid_at_full_width():
    from test_gpu_mixed_batch import H, _perturbed_random_model

    m = _perturbed_random_model(1, seed=79)
    grids = [(1, 83, 83), (1, 16, 16)] * 2
    patterns = [[False, True, False, True], [True, False, True, False]]  # the small items skip; then the large ones
    _forced_decisions_case(m, H, grids, [21, 9, 13, 30], patterns, qblk=256)


# ----------------------------------------------------------------------------------------------------------- step batcher
SPEC = [("a", 256, 256, 8, 4.0, 11, 6), ("b", 128, 384, 6, 2.5, 9, 6), ("c", 384, 384, 8, 4.0, 7, 5)]


def _requests():
    from test_gpu_teacache import JOINT
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    out = {}
    for i, (tag, h, w, steps, cfg, tp, tn) in enumerate(SPEC):
        S = (h // 16) * (w // 16)
        kw = dict(height=h, width=w, num_inference_steps=steps, true_cfg_scale=cfg, latents=_rnd(1, S, 64, seed=100 + i),
                  prompt_embeds=_rnd(1, tp, JOINT, seed=200 + i), negative_prompt_embeds=_rnd(1, tn, JOINT, seed=300 + i),
                  output_type="latent")
        out[tag] = lambda kw=kw: OmniDiffusionRequest(**kw)
    return out


def _serve(m, thresh, tags=("a", "b", "c"), **cfg):
    """a and b start together, c joins after two steps (a request alone: `tags` of one).  TeaCache at `thresh` (None: off).
    -> ({tag: final latents}, {tag: [skips pos, skips neg]}, {tag: [cnt pos, cnt neg]}, the image rows of every forward)."""
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    reqs = _requests()
    m.teacache = None if thresh is None else TeaCacheConfig(rel_l1_thresh=thresh)
    pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(max_step_batch=4, **cfg), device=DEV, transformer=m)
    calls, orig, samples = [], m.forward_ragged, {}

    def counted(prepared, *a, **k):
        calls.append(tuple(prepared["batch"].s_imgs))
        return orig(prepared, *a, **k)

    m.forward_ragged = counted
    try:
        b = ContinuousStepBatcher(pipe)
        for t in tags[:2]:
            b.add(reqs[t](), t)
            samples[t] = b.active[-1]
        n_warm = len(calls)
        done = dict(b.step())
        done.update(b.step())
        for t in tags[2:]:
            b.add(reqs[t](), t)
            samples[t] = b.active[-1]
        done.update(b.drain())
        torch.cuda.synchronize()
    finally:
        m.forward_ragged = orig
        m.teacache = None
    for t, o in done.items():
        assert o.error is None, (t, o.error)
    assert set(done) == set(tags)
    tc = {t: a.state.get("tc") for t, a in samples.items()}
    skips = {t: None if v is None else [int(x["skip_total"][0]) for x in v] for t, v in tc.items()}
    cnts = {t: None if v is None else [int(x["cnt"][0]) for x in v] for t, v in tc.items()}
    return {t: o.output.clone() for t, o in done.items()}, skips, cnts, calls[n_warm:]


_SOLO: dict = {}


def _solo(m_seed, m, thresh):
    """Every request served ALONE at this threshold (computed once, shared by the hipGraph and the uncaptured case)."""
    key = (m_seed, thresh)
    if key not in _SOLO:
        lat, skips = {}, {}
        for t, *_ in SPEC:
            o, s, _, _ = _serve(m, thresh, tags=(t,), use_hip_graph=False, mixed_step_batch=True, mixed_step_batch_teacache=True)
            lat[t], skips[t] = o[t], s[t]
        _SOLO[key] = (lat, skips)
    return _SOLO[key]


@pytest.mark.parametrize("graph", [False, True])
def test_step_batcher_mixes_grids_under_teacache(graph):
    from test_gpu_teacache import _model

    m, _ = _model()
    steps = {t: s for t, _, _, s, *_ in SPEC}
    on = dict(use_hip_graph=graph, mixed_step_batch=True, mixed_step_batch_teacache=True)
    # (a) never skip: the latents of the same mixed run with TeaCache off, bit for bit
    plain, _, _, _ = _serve(m, None, use_hip_graph=graph, mixed_step_batch=True)
    never, skips, cnts, calls_on = _serve(m, 1e-12, **on)
    assert skips == {t: [0, 0] for t in steps}
    for t in steps:
        assert torch.equal(never[t], plain[t]), t
    # a sample's history survives every re-composition (c joining, b leaving): the counters run on instead of restarting
    assert cnts == {t: [steps[t]] * 2 for t in steps}
    if not graph:
        # forwards really held several grids, and there were fewer of them than when TeaCache keeps the grid in the key
        _, _, _, calls_off = _serve(m, 1e-12, use_hip_graph=False, mixed_step_batch=True)
        print(f"   forwards: mixed_step_batch_teacache off {len(calls_off)}, on {len(calls_on)}")
        assert any(len(set(c)) > 1 for c in calls_on) and not any(len(set(c)) > 1 for c in calls_off)
        assert len(calls_on) < len(calls_off)
    # (b) always skip: every item computes its first forward only; each request lands where it lands alone
    always, skips, cnts, _ = _serve(m, 1e12, **on)
    assert skips == {t: [steps[t] - 1] * 2 for t in steps} and cnts == {t: [steps[t]] * 2 for t in steps}
    solo_lat, solo_skips = _solo(1234, m, 1e12)
    assert solo_skips == skips
    for t in steps:
        r = rel_l2(always[t], solo_lat[t])
        print(f"   graph={graph} always-skip request {t}: final latents vs the request alone {r:.3e}")
        assert r <= SOLO_BAR, (t, r)
    # (c) an intermediate threshold: a mixed compute / skip pattern, the decisions of the request alone
    mid, skips, cnts, _ = _serve(m, MID_THRESH, **on)
    solo_lat, solo_skips = _solo(1234, m, MID_THRESH)
    for t in steps:
        r = rel_l2(mid[t], solo_lat[t])
        print(f"   graph={graph} thresh={MID_THRESH} request {t}: skips mixed {skips[t]} alone {solo_skips[t]} of {steps[t]} forwards per "
              f"branch; final latents vs alone {r:.3e}")
    assert any(0 < s < steps[t] - 1 for t in steps for s in skips[t]), "threshold did not produce a mixed pattern"
    assert cnts == {t: [steps[t]] * 2 for t in steps}
    for t in steps:
        assert all(abs(a - b) <= 1 for a, b in zip(skips[t], solo_skips[t])), (t, skips[t], solo_skips[t])
        if skips[t] == solo_skips[t]:
            assert rel_l2(mid[t], solo_lat[t]) <= SOLO_BAR, t


# ------------------------------------------------------------------------------------------------------------------ guard
def test_flag_off_keeps_the_refusal_and_the_equal_grid_bits():
    """With `mixed_step_batch_teacache` off nothing moves: a mixed group under TeaCache is refused with the message there was,
    and an equal-grid TeaCache step-batch (the setup of tests/test_gpu_teacache.py::
    test_step_batched_teacache_keeps_per_request_decisions: two 256 x 256 true-CFG requests, 6 steps, rel_l1_thresh 0.6, small
    model) gives the skip counts and the final latents of the commit before this feature.

    Measured with the library built from that commit on one MI355X (three runs, identical): skip counts (pos0, pos1, neg0,
    neg1) = [5, 5, 5, 5]; final latents of both requests: sum -1160.81298828125, sum of magnitudes 32393.046875, recorded as
    bf16 bit patterns in tests/golden/teacache_step_batched_equal_grid.npz (`skips`, `latents`, the figures again in `meta`).
    At rel_l1_thresh 0.2, where the decisions fall near the threshold (a mixed pattern): [3, 3, 3, 3], sum -1161.636474609375, sum
    of magnitudes 32388.814453125 (`skips_mid`, `latents_mid`).  This build on the same machine: the same skip counts and the
    same bits at both thresholds (and at 0.3, 0.15, 0.1 and 0.05: 4 / 3 / 1 / 0 skipped forwards)."""
    from test_gpu_teacache import _loop_inputs, _model
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest
    from vllm_omni_amd.diffusion.step_batcher import ActiveSample

    m, _ = _model()
    m.teacache = TeaCacheConfig(rel_l1_thresh=0.6)
    try:
        pipe = QwenImagePipeline(od_config=OmniDiffusionConfig(mixed_step_batch=True, use_hip_graph=False), device=DEV, transformer=m)
        reqs, group = _requests(), []
        for i, t in enumerate(("a", "b")):
            a = ActiveSample(tag=t, sample=pipe.resolve_request(reqs[t]())[0], seq=i)
            pipe.begin_sample(a)
            group.append(a)
        assert pipe.batch_key(group[0]) != pipe.batch_key(group[1])
        with pytest.raises(NotImplementedError, match="a mixed step-batch cannot run with TeaCache"):
            pipe.denoise_one_step(group)
        pipe = QwenImagePipeline(device=DEV, transformer=m)
        eq = []
        for i in range(2):
            lat, pos, neg = _loop_inputs(6, seed=10 + i)
            eq.append(OmniDiffusionRequest(height=256, width=256, num_inference_steps=6, true_cfg_scale=4.0, latents=lat.to(BF16),
                                           prompt_embeds=pos.to(BF16), negative_prompt_embeds=neg.to(BF16), output_type="latent"))
        runs = {}
        for name, th in (("", 0.6), ("_mid", 0.2)):
            m.teacache = TeaCacheConfig(rel_l1_thresh=th)
            both = pipe.generate(eq, output_type="latent")
            torch.cuda.synchronize()
            runs[name] = (pipe.last_teacache_state.skipped_forwards(), torch.stack([o.output.reshape(256, 64) for o in both]).cpu())
    finally:
        m.teacache = None
    z = np.load(os.path.join(GOLDEN_DIR, "teacache_step_batched_equal_grid.npz"))
    for name, (skips, got) in runs.items():
        want = torch.from_numpy(z["latents" + name].astype(np.int32)).to(torch.int16).view(BF16)
        print(f"   skips {skips} (recorded {z['skips' + name].tolist()}); final latents vs recorded {rel_l2(got, want):.3e}")
        assert skips == z["skips" + name].tolist()
        assert torch.equal(got, want)
    assert all(0 < s < 5 for s in runs["_mid"][0])                      # a mixed compute / skip pattern: decisions near the threshold
