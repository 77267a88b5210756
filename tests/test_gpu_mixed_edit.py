"""GPU: mixed step batches for Edit / Edit-Plus requests (`OmniDiffusionConfig.mixed_step_batch_edit`) and the ragged
CFG + Euler kernel behind them (`omni_cfg_euler_step_ragged`).

  * the kernel: requests of 72 / 272 / 1 / 33 rows (no multiple of 32, one row, boundaries inside a 32-row block) whose items
    carry 70 / 30 / 0 / 5 condition rows in the prediction buffer; checker: `ops.cfg_euler_step_` per request on contiguous
    copies, bit for bit; both `lat_in` destinations, untouched condition rows, two launches, a descriptor that leaves a buffer;
  * forward parity at full width, 2 layers: one ragged forward of three Edit / Edit-Plus items as a CFG pair group against the
    fp32 oracle run per item with that item's own multi-entry `img_shapes`; calibration: the same oracle in bf16;
  * the step batcher end to end on an Edit-Plus pipeline: three requests of different sizes, condition grids, scales and step
    counts, a late joiner; fewer forwards than with the flag off; a hipGraph replay gives the bits of the uncaptured steps;
  * TeaCache with both opt-ins: every request's per-item skip pattern is the pattern of the same request served alone."""
import pytest
import torch

import qwen_image_oracle as O
from _util import cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
H = 24

# (target grid, condition grids): 72 + 70, 272 + 30 and 64 + (45 + 16) rows
EDIT_GROUP = [((1, 9, 8), [(1, 10, 7)]), ((1, 16, 17), [(1, 6, 5)]), ((1, 8, 8), [(1, 5, 9), (1, 4, 4)])]


def _rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (scale * torch.randn(*shape, device=DEV, generator=g)).to(BF16)


def _tokens(grids):
    return sum(f * h * w for f, h, w in grids)


# ------------------------------------------------------------------------------------------------------------- the kernel
K_ROWS, K_COND = [72, 272, 1, 33], [70, 30, 0, 5]
K_SCALES, K_DT = [4.0, 2.5, 1.75, 7.0], [-0.05, -0.125, -0.03, -0.2]


def _kernel_inputs(with_neg):
    from vllm_omni_amd.diffusion.batch import ragged_step_descriptors

    lay = ragged_step_descriptors(K_ROWS, K_COND, with_neg, K_SCALES)
    n_item_rows = lay["item_off"][-1]
    assert lay["total_rows"] == 378 and n_item_rows == (2 if with_neg else 1) * (378 + 105)
    reqs = torch.from_numpy(lay["reqs"].view("<i4").reshape(len(K_ROWS), 8).copy()).to(DEV)
    return (lay, reqs, _rnd(lay["total_rows"], 64, seed=1), _rnd(n_item_rows, 64, seed=2), _rnd(n_item_rows, 64, seed=3),
            torch.tensor(K_DT, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("normalize", [True, False], ids=["normalize", "no_normalize"])
@pytest.mark.parametrize("with_neg", [True, False], ids=["cfg", "no_cfg"])
def test_ragged_step_kernel_is_bit_equal_to_the_per_request_kernel(with_neg, normalize):
    from vllm_omni_amd import ops

    lay, reqs, lat0, pred, lat_in0, dt = _kernel_inputs(with_neg)
    R, q = len(K_ROWS), lay["reqs"]
    want = lat0.clone()
    for r in range(R):                                                   # the checker: one plain launch per request
        o0, o1, n = lay["lat_off"][r], lay["lat_off"][r + 1], K_ROWS[r]
        p = pred[int(q["pos_row"][r]):int(q["pos_row"][r]) + n].clone()
        ng = pred[int(q["neg_row"][r]):int(q["neg_row"][r]) + n].clone() if with_neg else None
        piece = lat0[o0:o1].clone()
        ops.cfg_euler_step_(piece, p, ng, K_SCALES[r], dt[r:r + 1], dt_rows_per_item=0, normalize=normalize)
        want[o0:o1].copy_(piece)
    runs = []
    for _ in range(2):
        lat, lat_in = lat0.clone(), lat_in0.clone()
        ops.cfg_euler_step_ragged_(lat, pred, lat_in, reqs, R, lay["total_rows"], dt, normalize=normalize)
        torch.cuda.synchronize()
        runs.append((lat, lat_in))
    lat, lat_in = runs[0]
    assert torch.isfinite(lat.float()).all() and not torch.equal(lat, lat0)
    assert torch.equal(lat, want)                                        # the per-request kernel's bits
    assert torch.equal(runs[1][0], lat) and torch.equal(runs[1][1], lat_in)      # deterministic
    io = lay["item_off"]
    for i in range((2 if with_neg else 1) * R):
        r = i % R
        o0, o1 = lay["lat_off"][r], lay["lat_off"][r + 1]
        assert torch.equal(lat_in[io[i]:io[i] + K_ROWS[r]], lat[o0:o1]), i                      # the next step's input rows
        assert torch.equal(lat_in[io[i] + K_ROWS[r]:io[i + 1]], lat_in0[io[i] + K_ROWS[r]:io[i + 1]]), i   # condition rows: untouched


def test_ragged_step_kernel_skips_a_request_whose_rows_leave_a_buffer():
    """The host cannot read the device descriptors, so the kernel checks them: a request with a range outside one of the
    buffers is left alone, rows and all; its neighbours are updated as usual."""
    from vllm_omni_amd import ops

    lay, reqs, lat0, pred, lat_in0, dt = _kernel_inputs(True)
    good_lat, good_in = lat0.clone(), lat_in0.clone()
    ops.cfg_euler_step_ragged_(good_lat, pred, good_in, reqs, 4, lay["total_rows"], dt)
    bad = lay["reqs"].copy()
    bad["neg_row"][1] = pred.shape[0] - K_ROWS[1] + 1                    # the last row would lie behind the buffer
    bad["dt_index"][3] = 4                                               # dt has four entries
    lat, lat_in = lat0.clone(), lat_in0.clone()
    ops.cfg_euler_step_ragged_(lat, pred, lat_in, torch.from_numpy(bad.view("<i4").reshape(4, 8).copy()).to(DEV), 4,
                               lay["total_rows"], dt)
    torch.cuda.synchronize()
    lo = lay["lat_off"]
    for r in range(4):
        ref = lat0 if r in (1, 3) else good_lat
        assert torch.equal(lat[lo[r]:lo[r + 1]], ref[lo[r]:lo[r + 1]]), r
    io = lay["item_off"]
    for i in range(8):
        ref = lat_in0 if i % 4 in (1, 3) else good_in
        assert torch.equal(lat_in[io[i]:io[i + 1]], ref[io[i]:io[i + 1]]), i


# ------------------------------------------------------------------------------------------------------------ one forward
def test_forward_parity_of_a_mixed_edit_cfg_group_at_full_width():
    from test_gpu_mixed_batch import _oracle_params, _perturbed_random_model
    from vllm_omni_amd.diffusion.batch import build_ragged_batch

    torch.backends.cuda.matmul.allow_tf32 = False
    m = _perturbed_random_model(2, seed=77)
    P32, Pb = _oracle_params(m), _oracle_params(m, BF16)
    order = [1, 0, 2]                                                        # longest total rows first, as the batcher hands over
    grids = [(EDIT_GROUP[i][0], *EDIT_GROUP[i][1]) for i in order]
    R = len(grids)
    t_pos, t_neg = [64, 290, 20], [11, 37, 5]                                # ragged prompts
    lens, item_grid = t_pos + t_neg, grids * 2                               # pos_0..pos_2, neg_0..neg_2
    rows_r = [torch.cat([_rnd(_tokens(g[:1]), 64, seed=10 + r), _rnd(_tokens(g[1:]), 64, seed=20 + r)]) for r, g in enumerate(grids)]
    rows = rows_r * 2                                                        # a CFG pair shares latents and condition rows
    txt = [_rnd(t, 3584, seed=30 + i) for i, t in enumerate(lens)]
    sig = torch.tensor([0.6015625, 0.25, 0.90625], device=DEV)               # one step index per request, exact in bf16
    rb = build_ragged_batch(lens, item_grid, temb_rows=list(range(R)) * 2)
    assert rb.mixed and rb.s_imgs == [302, 142, 125] * 2
    out = m.forward_ragged(m.prepare_batch(rb), torch.cat(rows), torch.cat(txt), sig).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and out.shape == (sum(rb.s_imgs), 64)
    off, res = rb.img_offsets, []
    with torch.no_grad():
        for i in range(2 * R):
            s1, shapes = sig[i % R:i % R + 1], list(item_grid[i])
            ref = O.dit_forward(P32, rows[i][None].float(), txt[i][None].float(), s1, shapes, num_heads=H)
            eag = O.dit_forward(Pb, rows[i][None], txt[i][None], s1.to(BF16), shapes, num_heads=H)
            got = out[off[i]:off[i + 1]][None]
            S = _tokens(shapes[:1])
            res.append((rel_l2(got, ref), cosine(got, ref), rel_l2(eag, ref), rel_l2(got[:, :S], ref[:, :S])))
            del ref, eag
    for i, (r, c, e, rt) in enumerate(res):
        print(f"   item {i} grids {item_grid[i]} T {lens[i]}: product vs fp32 oracle {r:.3e} cos {c:.6f} (target rows alone {rt:.3e}); "
              f"bf16-eager {e:.3e}")
    for r, c, e, _ in res:
        assert r <= 1e-2 and c >= 0.9995                                     # the forward bar
        assert r <= 1.1 * e                                                  # no further from fp32 than the bf16-eager algorithm


# ------------------------------------------------------------------------------------------------------------ step batcher
def _edit_requests(joint, spec):
    """tag -> dict(request factory, inputs).  Condition latents are handed over packed (`image_latents`): no VAE in the loop."""
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    out = {}
    for i, (tag, k, steps, cfg, tp, tn) in enumerate(spec):
        target, conds = EDIT_GROUP[k]
        S = _tokens([target])
        lat, pos, neg = _rnd(1, S, 64, seed=100 + i), _rnd(1, tp, joint, seed=200 + i), _rnd(1, tn, joint, seed=300 + i)
        cond = [_rnd(_tokens([g]), 64, seed=400 + 10 * i + j) for j, g in enumerate(conds)]
        kw = dict(height=16 * target[1], width=16 * target[2], num_inference_steps=steps, true_cfg_scale=cfg, latents=lat,
                  prompt_embeds=pos, negative_prompt_embeds=neg, output_type="latent",
                  extra={"image_latents": cond, "image_latent_grid": [(g[1], g[2]) for g in conds]})
        out[tag] = dict(grids=[target, *conds], steps=steps, cfg=cfg, lat=lat, pos=pos, neg=neg, cond=torch.cat(cond)[None],
                        req=lambda kw=kw: OmniDiffusionRequest(**kw))
    return out


def _serve(m, spec, tags, join_after, thresh=None, **cfg):
    """tags[:2] start together, the rest joins after `join_after` steps (one tag: the request alone).  TeaCache at `thresh`.
    -> ({tag: final latents}, image rows of every forward, serve states, {tag: [(skip pos, skip neg) per forward]})."""
    from vllm_omni_amd.diffusion.cache.teacache.config import TeaCacheConfig
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit_plus import QwenImageEditPlusPipeline
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    m.teacache = None if thresh is None else TeaCacheConfig(rel_l1_thresh=thresh)
    pipe = QwenImageEditPlusPipeline(od_config=OmniDiffusionConfig(max_step_batch=4, **cfg), device=DEV, transformer=m,
                                     vae=AutoencoderKLQwenImage(device=DEV, with_encoder=True))
    calls, pattern, orig = [], {t: [] for t in tags}, m.forward_ragged

    def counted(prepared, *a, **k):
        calls.append(tuple(prepared["batch"].s_imgs))
        out = orig(prepared, *a, **k)
        tc = k.get("teacache")
        if tc is not None and not torch.cuda.is_current_stream_capturing():
            st = next(s for s in pipe._serve_states.values() if s["prepared"] is prepared)
            skip, R = tc.skip.tolist(), st["R"]
            for r, a_ in enumerate(st["members"]):
                pattern[a_.tag].append((skip[r], skip[R + r]))
        return out

    m.forward_ragged = counted
    try:
        b = ContinuousStepBatcher(pipe)
        for t in tags[:2]:
            b.add(spec[t]["req"](), t)
        done = {}
        for _ in range(join_after):
            done.update(b.step())
        for t in tags[2:]:
            b.add(spec[t]["req"](), t)
        done.update(b.drain())
        torch.cuda.synchronize()
    finally:
        m.forward_ragged = orig
        m.teacache = None
    for t, o in done.items():
        assert o.error is None, (t, o.error)
    assert set(done) == set(tags)
    return {t: o.output.clone() for t, o in done.items()}, calls, dict(pipe._serve_states), pattern


def _oracle_edit_denoise(P, s, dtype):
    """The reference's Edit loop (condition rows behind the latents in every forward, the prediction cut back to the latent rows)
    with the oracle DiT in `dtype`; latents kept in bf16."""
    lat, S = s["lat"], s["lat"].shape[1]
    ts, sig = O.flow_match_sigmas(s["steps"], S)
    x = lat.float()
    for i, t in enumerate(ts):
        s_in = (t.bfloat16() / 1000).bfloat16().float().expand(1).to(lat.device)
        inp = torch.cat([x, s["cond"].float()], dim=1).to(dtype)
        p = O.dit_forward(P, inp, s["pos"].to(dtype), s_in, s["grids"], num_heads=H).float()[:, :S]
        n = O.dit_forward(P, inp, s["neg"].to(dtype), s_in, s["grids"], num_heads=H).float()[:, :S]
        x = O.euler_step(x, O.cfg_combine(p, n, s["cfg"]), float(sig[i]), float(sig[i + 1])).bfloat16().float()
    return x


def test_step_batcher_mixes_edit_requests_end_to_end():
    from test_gpu_mixed_batch import _oracle_params, _perturbed_random_model

    torch.backends.cuda.matmul.allow_tf32 = False
    m = _perturbed_random_model(2, seed=77)
    # (tag, entry of EDIT_GROUP, steps, scale, prompt rows, negative prompt rows): c (Edit-Plus, two pictures) joins late
    spec = _edit_requests(3584, [("a", 0, 4, 4.0, 21, 9), ("b", 1, 3, 2.5, 64, 5), ("c", 2, 2, 3.0, 13, 30)])
    ref, eager = {}, {}
    with torch.no_grad():
        P32 = _oracle_params(m)
        for t, s in spec.items():
            ref[t] = _oracle_edit_denoise(P32, s, torch.float32)
        del P32
        Pb = _oracle_params(m, BF16)
        for t, s in spec.items():
            eager[t] = _oracle_edit_denoise(Pb, s, BF16)
        del Pb
    tags = ("a", "b", "c")
    off, calls_off, keys_off, _ = _serve(m, spec, tags, 1, use_hip_graph=False, mixed_step_batch=True)
    on, calls_on, keys, _ = _serve(m, spec, tags, 1, use_hip_graph=False, mixed_step_batch=True, mixed_step_batch_edit=True)
    graph, calls_g, states_g, _ = _serve(m, spec, tags, 1, use_hip_graph=True, mixed_step_batch=True, mixed_step_batch_edit=True)
    print(f"   forwards: flag off {len(calls_off)}, flag on {len(calls_on)} (hipGraph run: {len(calls_g)} uncaptured calls)")
    for t in tags:
        r_on, r_off, r_e = rel_l2(on[t], ref[t]), rel_l2(off[t], ref[t]), rel_l2(eager[t], ref[t])
        print(f"   request {t} {spec[t]['grids']} {spec[t]['steps']} steps cfg {spec[t]['cfg']}: final latents vs fp32 oracle — "
              f"mixed {r_on:.3e} cos {cosine(on[t], ref[t]):.6f}; flag off {r_off:.3e}; bf16-eager {r_e:.3e}")
    # flag off: one request per forward (no two of them share a grid); flag on: forwards with items of unequal rows, longest first
    assert all(len(set(c)) == 1 and len(c) == 2 for c in calls_off) and len(calls_off) == sum(s["steps"] for s in spec.values())
    assert not any(k[0] == "mixed_edit" for k in keys_off)
    assert any(len(set(c)) > 1 for c in calls_on)
    assert all(list(c[:len(c) // 2]) == sorted(c[:len(c) // 2], reverse=True) for c in calls_on)
    assert len(calls_on) < len(calls_off)
    assert sum(s["steps"] for s in spec.values()) > len(calls_on) >= max(s["steps"] for s in spec.values())
    assert all(k[0] == "mixed_edit" and st["pred_c"] is None for k, st in keys.items())
    # the hipGraph run captured every composition and replayed it: forward_ragged is entered by warm-up + capture only
    assert states_g and all(st["graph"] is not None for st in states_g.values())
    assert len(calls_g) == 2 * len(states_g) and len(states_g) < len(calls_on)
    for t in tags:
        assert torch.isfinite(on[t].float()).all()
        assert rel_l2(on[t], ref[t]) <= 1.1 * rel_l2(eager[t], ref[t]), t
        assert torch.equal(graph[t], on[t]), t                               # a replayed composition == the uncaptured steps


# ----------------------------------------------------------------------------------------------------------------- TeaCache
TEA_SPEC = [("a", 0, 8, 4.0, 11, 6), ("b", 1, 6, 2.5, 9, 6), ("c", 2, 8, 3.0, 7, 5)]


@pytest.mark.parametrize("thresh", [1e-12, 0.2, 1e12], ids=["never_skip", "default_threshold", "always_skip"])
def test_mixed_edit_group_under_teacache_decides_like_each_request_alone(thresh):
    """Both opt-ins, small model: a and b start, c joins after two steps.  Per request and CFG branch the skip / compute decision
    of every forward must be the one the same request takes when it is served alone (its items then have the same rows in a
    one-request group).  1e-12: nothing may be skipped, and the latents are those of the run with TeaCache off; 1e12: everything
    behind the first forward is skipped; 0.2: the default threshold."""
    from test_gpu_teacache import JOINT, _model

    m, _ = _model()
    spec = _edit_requests(JOINT, TEA_SPEC)
    tags = ("a", "b", "c")
    on = dict(use_hip_graph=False, mixed_step_batch=True, mixed_step_batch_edit=True, mixed_step_batch_teacache=True)
    lat, calls, states, pattern = _serve(m, spec, tags, 2, thresh=thresh, **on)
    assert any(len(set(c)) > 1 for c in calls) and all(k[0] == "mixed_edit" for k in states)
    steps = {t: s for t, _, s, *_ in TEA_SPEC}
    for t in tags:
        solo_lat, _, _, solo_pattern = _serve(m, spec, (t,), 0, thresh=thresh, **on)
        r = rel_l2(lat[t], solo_lat[t])
        print(f"   thresh {thresh:g} request {t}: (pos, neg) skips per forward mixed {pattern[t]} alone {solo_pattern[t]}; "
              f"final latents vs alone {r:.3e}")
        assert len(pattern[t]) == steps[t] and pattern[t][0] == (0, 0)
        assert pattern[t] == solo_pattern[t], t
        assert r <= 5e-3, (t, r)              # batched against solo final latents: the bar of tests/test_gpu_teacache_mixed.py
    if thresh == 1e-12:
        assert all(p == (0, 0) for t in tags for p in pattern[t])
        plain, _, _, _ = _serve(m, spec, tags, 2, use_hip_graph=False, mixed_step_batch=True, mixed_step_batch_edit=True)
        for t in tags:
            assert torch.equal(lat[t], plain[t]), t
    if thresh == 1e12:
        assert all(p == (1, 1) for t in tags for p in pattern[t][1:])
