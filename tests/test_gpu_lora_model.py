"""GPU: LoRA adapters on the DiT - merged on the device into copies of the targeted matrices (ops.lora_merge), activated by
pointer.  Small geometry of the existing forward tests (2 layers, 2 heads of 128, joint dim 128).

Parity is against the fp32 oracle whose weights are W + s * B @ A, merged here in fp32 on the CPU and handed to the oracle the way
every other test hands it weights.  Bar: the existing <= 4-layer bar (rel-L2 <= 1e-2, cos >= 0.9995).  The adapters are drawn
large enough that the BASE model's output fails that bar against the merged oracle, so no check passes with the adapter
ignored; lora_B is non-zero (PEFT's zero initialisation would make every check vacuous)."""
import queue

import pytest
import torch

import qwen_image_oracle as O
from _util import bf16_round, cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda:0"
HEADS, JOINT, LAYERS = 2, 128, 2
D = HEADS * 128
GRID, T = (1, 8, 8), 9


def _targets():
    from vllm_omni_amd.diffusion import lora as L

    return L.target_shapes(LAYERS, D, JOINT, 64, 64)


def make_adapter(seed: int, rank: int, *, split_qkv: bool = False, shared_down: bool = False, alpha=None, std=0.06):
    """An adapter on EVERY target (twelve linears per layer and the six global ones), kohya spelling, bf16-exact values.
    split_qkv: q / k / v keys instead of the fused ones (shared_down: all three with one lora_down, i.e. what a fused key means)."""
    g = torch.Generator().manual_seed(seed)
    t = {}
    for mod, (n, k, _) in _targets().items():
        down = bf16_round(torch.randn(rank, k, generator=g) * std)
        up = bf16_round(torch.randn(n, rank, generator=g) * std)
        pieces = [(mod, up, down)]
        for fused, names in ((".to_qkv", ("to_q", "to_k", "to_v")), (".add_kv_proj", ("add_q_proj", "add_k_proj", "add_v_proj"))):
            if split_qkv and mod.endswith(fused):
                downs = [down if shared_down else bf16_round(torch.randn(rank, k, generator=g) * std) for _ in range(3)]
                pieces = [(mod[:-len(fused)] + "." + nm, up[i * D:(i + 1) * D].clone(), downs[i]) for i, nm in enumerate(names)]
        for name, u, d in pieces:
            t["transformer." + name + ".lora_down.weight"], t["transformer." + name + ".lora_up.weight"] = d, u
            if alpha is not None:
                t["transformer." + name + ".alpha"] = torch.tensor(float(alpha))
    return t


def merged_params(Pb: dict, adapters: list) -> dict:
    """fp32 W + sum_i s_i * B_i @ A_i on the CPU.  adapters: [(tensors, weight)]."""
    from vllm_omni_amd.diffusion import lora as L

    out = {k: v.clone().float() for k, v in Pb.items()}
    for tensors, weight in adapters:
        ad = L.parse_adapter("x", tensors, _targets(), D)
        for (mod, row0, rows), (up, down, scale) in ad.updates.items():
            out[mod + ".weight"][row0:row0 + rows] += (scale * weight) * (up.float() @ down.float())
    return out


@pytest.fixture(scope="module")
def world():
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    P = O.make_dit_params(LAYERS, seed=1234, bias_std=0.02, norm_jitter=0.1, num_heads=HEADS, joint_dim=JOINT)
    Pb = {k: bf16_round(v) for k, v in P.items()}
    m = QwenImageTransformer2DModel(num_layers=LAYERS, num_attention_heads=HEADS, joint_attention_dim=JOINT, device=DEV)
    m.load_weights(P.items())
    g = torch.Generator().manual_seed(3)
    lat = bf16_round(torch.randn(1, 64, 64, generator=g))
    txt = bf16_round(torch.randn(1, T, JOINT, generator=g))
    sig = bf16_round(torch.tensor([0.6015625]))
    A = dict(a=make_adapter(1, 8), b=make_adapter(2, 4, alpha=8.0), a_split=make_adapter(3, 8, split_qkv=True),
             f=make_adapter(4, 8), f_split=make_adapter(4, 8, split_qkv=True, shared_down=True))
    return dict(P=P, Pb=Pb, m=m, lat=lat, txt=txt, sig=sig, A=A)


def run(m, w):
    out = m(hidden_states=w["lat"].to(DEV, BF16), encoder_hidden_states=w["txt"].to(DEV, BF16), encoder_hidden_states_mask=None,
            timestep=w["sig"].to(DEV), img_shapes=[[GRID]], txt_seq_lens=[T], return_dict=False)[0]
    torch.cuda.synchronize()
    return out.float().cpu()[0]


def oracle(w, adapters):
    return O.dit_forward(merged_params(w["Pb"], adapters), w["lat"], w["txt"], w["sig"], GRID, num_heads=HEADS)[0]


def fresh(w, **kw):
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    od = OmniDiffusionConfig(**kw) if kw else None
    m = QwenImageTransformer2DModel(od_config=od, num_layers=LAYERS, num_attention_heads=HEADS, joint_attention_dim=JOINT, device=DEV)
    m.load_weights(w["P"].items())
    return m


def test_adapter_parity_against_the_merged_fp32_oracle(world):
    w = world
    m = w["m"]
    base = run(m, w)
    assert rel_l2(base, oracle(w, [])) <= 1e-2                                  # the base model is where it always was
    for name, weight in (("a", 1.0), ("b", 1.0), ("a_split", 0.5)):
        m.load_lora_adapter(name, w["A"][name])
        m.set_lora_adapters([name], weights=[weight])
        assert m.active_lora == ((name, weight),)
        out, ref = run(m, w), oracle(w, [(w["A"][name], weight)])
        r, c = rel_l2(out, ref), cosine(out, ref)
        rb, cb = rel_l2(base, ref), cosine(base, ref)
        print(f"{name} x {weight}: rel_l2 {r:.3e} cos {c:.6f}   (base model vs this oracle: rel_l2 {rb:.3e} cos {cb:.6f})")
        assert r <= 1e-2 and c >= 0.9995
        assert rb > 1e-2 or cb < 0.9995, "the adapter draw is too small to tell an ignored adapter from an applied one"
    m.set_lora_adapters([])


def test_stacked_adapters_against_the_same_oracle(world):
    w = world
    m = w["m"]
    for n in ("a", "b"):
        m.load_lora_adapter(n, w["A"][n])
    m.set_lora_adapters(["a", "b"], weights=[0.7, -0.3])
    out, ref = run(m, w), oracle(w, [(w["A"]["a"], 0.7), (w["A"]["b"], -0.3)])
    m.set_lora_adapters([])
    only_a = oracle(w, [(w["A"]["a"], 0.7)])
    r, c = rel_l2(out, ref), cosine(out, ref)
    print(f"stack a x 0.7 + b x -0.3: rel_l2 {r:.3e} cos {c:.6f}   (oracle with a alone vs both: rel_l2 {rel_l2(only_a, ref):.3e})")
    assert r <= 1e-2 and c >= 0.9995
    assert rel_l2(only_a, ref) > 1e-2 or cosine(only_a, ref) < 0.9995          # b matters: a stack that dropped it would fail


def test_split_and_fused_keys_give_bit_equal_outputs(world):
    w = world
    m = w["m"]
    m.load_lora_adapter("f", w["A"]["f"])
    m.load_lora_adapter("f_split", w["A"]["f_split"])
    m.set_lora_adapters(["f"])
    fused = run(m, w)
    m.set_lora_adapters(["f_split"])
    split = run(m, w)
    m.set_lora_adapters([])
    assert torch.equal(fused, split)
    assert not torch.equal(fused, run(m, w))


def test_deactivation_is_exact_and_parameters_stay_the_base_weights(world):
    w = world
    m = fresh(w)
    sd0 = {k: v.clone().cpu() for k, v in m.state_dict().items()}
    before = run(m, w)
    m.load_lora_adapter("a", w["A"]["a"])
    m.set_lora_adapters(["a"])
    under = run(m, w)
    assert not torch.equal(under, before)
    sd_active = m.state_dict()                                                   # also while the adapter is active
    assert all(torch.equal(sd_active[k].cpu().view(torch.int16), sd0[k].view(torch.int16)) for k in sd0)
    assert m.active_lora == (("a", 1.0),) and torch.equal(run(m, w), under)      # (state_dict dropped the merged set: rebuilt)
    m.set_lora_adapters([])
    assert torch.equal(run(m, w), before)
    sd1 = m.state_dict()
    assert sd1.keys() == sd0.keys() and all(torch.equal(sd1[k].cpu().view(torch.int16), sd0[k].view(torch.int16)) for k in sd0)
    # new base weights under an active adapter: the merged set follows them
    m.set_lora_adapters(["a"])
    run(m, w)
    P2 = O.make_dit_params(LAYERS, seed=77, bias_std=0.02, norm_jitter=0.1, num_heads=HEADS, joint_dim=JOINT)
    m.load_weights(P2.items())
    out = run(m, w)
    ref = O.dit_forward(merged_params({k: bf16_round(v) for k, v in P2.items()}, [(w["A"]["a"], 1.0)]), w["lat"], w["txt"], w["sig"],
                        GRID, num_heads=HEADS)[0]
    assert rel_l2(out, ref) <= 1e-2 and cosine(out, ref) >= 0.9995


@pytest.mark.parametrize("resident,merges", [(2, 2), (1, 3)])
def test_resident_sets_are_reactivated_without_a_merge(world, monkeypatch, resident, merges):
    from vllm_omni_amd import ops

    w = world
    m = fresh(w, max_resident_loras=resident)
    assert m.max_resident_loras == resident
    m.load_lora_adapter("a", w["A"]["a"])
    m.load_lora_adapter("b", w["A"]["b"])
    calls = []
    real = ops.lora_merge
    monkeypatch.setattr(ops, "lora_merge", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    outs = []
    for name in ("a", "b", "a"):
        m.set_lora_adapters([name])
        outs.append(run(m, w))
    per_activation = LAYERS * 14 + 6            # launches of one activation: ten matrices per layer, the two fused ones in 3 ranges
    assert len(calls) == merges * per_activation, (len(calls), per_activation)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])
    gen = m._native_gen
    m.set_lora_adapters(["a"])                  # no change: nothing is invalidated, nothing launched
    assert m._native_gen == gen and len(calls) == merges * per_activation


def _req(w, lora, steps=2, hw=256, seed=5, scale=1.0):
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    g = torch.Generator().manual_seed(seed)
    S = (hw // 16) ** 2
    return OmniDiffusionRequest(height=hw, width=hw, num_inference_steps=steps, true_cfg_scale=4.0, output_type="latent",
                                latents=torch.randn(1, S, 64, generator=g).to(BF16), lora=lora, lora_scale=scale,
                                prompt_embeds=torch.randn(1, 9, JOINT, generator=g).to(BF16),
                                negative_prompt_embeds=torch.randn(1, 5, JOINT, generator=g).to(BF16))


def _pipe(w, m, **cfg):
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline

    return QwenImagePipeline(od_config=OmniDiffusionConfig(**cfg), device=DEV, transformer=m)


def test_captured_step_graph_follows_an_adapter_switch(world):
    """256^2 takes the per-step hipGraph.  a, then b, then none through ONE pipeline whose graph was captured under a: each result
    is the eager result under that request's adapter - the graph was re-captured, no stale pointer was read."""
    w = world
    m = fresh(w)
    m.load_lora_adapter("a", w["A"]["a"])
    m.load_lora_adapter("b", w["A"]["b"])
    graph, eager = _pipe(w, m, use_hip_graph=True), _pipe(w, m, use_hip_graph=False)
    want = {lo: eager.generate([_req(w, lo)], output_type="latent")[0].output.float().cpu() for lo in ("a", "b", None)}
    assert not torch.equal(want["a"], want["b"]) and not torch.equal(want["a"], want[None])
    for lo in ("a", "b", None, "a"):
        got = graph.generate([_req(w, lo)], output_type="latent")[0].output.float().cpu()
        torch.cuda.synchronize()
        assert torch.equal(got, want[lo]), lo
    assert m.active_lora == (("a", 1.0),)
    with pytest.raises(NotImplementedError, match="same LoRA"):
        graph.generate([_req(w, "a"), _req(w, "b")], output_type="latent")
    with pytest.raises(KeyError, match="nope"):
        graph.generate([_req(w, "nope")], output_type="latent")


def test_resident_combinations_keep_their_graphs(world, monkeypatch):
    """max_resident_loras = 2, graph shape: a, b, none are captured once each; going round again replays - no capture, no
    merge - and every result is the eager one.  A kept table comes back with its own generation."""
    from vllm_omni_amd import ops

    w = world
    m = fresh(w, max_resident_loras=2)
    m.load_lora_adapter("a", w["A"]["a"])
    m.load_lora_adapter("b", w["A"]["b"])
    graph, eager = _pipe(w, m, use_hip_graph=True, max_resident_loras=2), _pipe(w, m, use_hip_graph=False, max_resident_loras=2)
    want = {lo: eager.generate([_req(w, lo)], output_type="latent")[0].output.float().cpu() for lo in ("a", "b", None)}
    made = []                                                              # hipGraph captures of the graph pipeline
    keep = graph._keep_captured
    graph._keep_captured = lambda *a: (made.append(1), keep(*a))[1]
    merges = []
    real = ops.lora_merge
    monkeypatch.setattr(ops, "lora_merge", lambda *a, **k: (merges.append(1), real(*a, **k))[1])
    gens = {}
    for rnd in range(2):
        for lo in ("a", "b", None):
            got = graph.generate([_req(w, lo)], output_type="latent")[0].output.float().cpu()
            torch.cuda.synchronize()
            assert torch.equal(got, want[lo]), (rnd, lo)
            assert gens.setdefault(lo, m._native_gen) == m._native_gen
        assert len(made) == 3 and not merges, (rnd, len(made), len(merges))
    assert len(set(gens.values())) == 3
    (st,) = graph._step_state.values()
    assert set(st["graphs"]) == set(gens.values()) == m.live_native_gens()
    # new base weights: every table, set and graph goes
    m.load_weights(w["P"].items())
    graph.generate([_req(w, None)], output_type="latent")
    assert set(st["graphs"]) == {m._native_gen} and not m._lora_sets and len(made) == 4


def test_an_evicted_set_is_freed_although_graphs_were_captured_under_it(world):
    """max_resident_loras = 1 and two adapters alternating on the graph path, at two text lengths (two step states): after every
    switch ONE merged set exists - the evicted one's tensors are gone, also from the state that was not used again - and no
    state holds a graph of a generation that is not live."""
    import gc
    import weakref

    w = world
    m = fresh(w)
    m.load_lora_adapter("a", w["A"]["a"])
    m.load_lora_adapter("b", w["A"]["b"])
    pipe = _pipe(w, m, use_hip_graph=True)
    short = _req(w, "a")
    other = _req(w, "a", seed=6)
    other.prompt_embeds = other.prompt_embeds[:, :7]                        # another text length: another step state
    pipe.generate([short], output_type="latent")
    pipe.generate([other], output_type="latent")
    assert len(pipe._step_state) == 2 and all(len(st["graphs"]) == 1 for st in pipe._step_state.values())
    dead = []
    for lo in ("b", "a", "b"):
        (merged,) = m._lora_sets.values()
        dead.append(weakref.ref(next(iter(merged.values()))))
        del merged
        pipe.generate([_req(w, lo)], output_type="latent")                  # only the first state is used again
        torch.cuda.synchronize()
        gc.collect()
        assert len(m._lora_sets) == 1 and all(r() is None for r in dead), lo
        live = m.live_native_gens()
        assert all(set(st["graphs"]) <= live for st in pipe._step_state.values())
    pipe.remove_lora("b")                                                    # active, nobody uses it: back to the base model
    assert m.active_lora == () and pipe.lora_names() == {"a"} and not m._lora_sets
    assert all(not st["graphs"] or set(st["graphs"]) <= m.live_native_gens() for st in pipe._step_state.values())


def test_fp8_copies_are_quantised_from_the_merged_weights(world):
    w = world
    m = fresh(w)
    m.load_lora_adapter("a", w["A"]["a"])
    bf16_base = run(m, w)
    m.enable_fp8(True)
    fp8_base = run(m, w)
    m.set_lora_adapters(["a"])
    fp8_lora = run(m, w)
    m.enable_fp8(False)
    bf16_lora = run(m, w)
    m.set_lora_adapters([])
    own = rel_l2(fp8_base, bf16_base)                         # the fp8 path's own distance from bf16
    moved = rel_l2(fp8_lora, fp8_base)
    print(f"fp8: own distance from bf16 {own:.3e}; adapter moves the fp8 output by {moved:.3e}; fp8+adapter vs bf16+adapter "
          f"{rel_l2(fp8_lora, bf16_lora):.3e}")
    assert moved > own
    assert rel_l2(fp8_lora, bf16_lora) < rel_l2(fp8_lora, bf16_base)      # and it moved TO the adapter's output


def test_worker_path_serves_adapters_side_by_side(world):
    """Three requests (adapter a, adapter b, none) through the worker's message handler and its continuous step batcher at 256^2,
    2 steps: each final latent is bit-equal to its solo run through the same path, and the number of forwards is the sum of the
    solo runs' - no forward was shared.  An unknown adapter name is that request's error, nobody else's."""
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.worker.gpu_worker import WorkerProc

    w = world
    m = fresh(w)
    m.load_lora_adapter("a", w["A"]["a"])
    m.load_lora_adapter("b", w["A"]["b"])

    def serve(reqs):
        cfg = OmniDiffusionConfig(max_step_batch=4, lora_switch_patience=1)
        pipe = _pipe(w, m, max_step_batch=4, lora_switch_patience=1)
        forwards = []
        real = pipe.denoise_one_step
        pipe.denoise_one_step = lambda group: (forwards.append(tuple(a.tag for a in group)), real(group))[1]
        inbox, outbox = queue.Queue(), queue.Queue()
        wp = serve.wp = WorkerProc(0, cfg, inbox, outbox, pipeline=pipe)
        for tag, r in reqs.items():
            assert wp._handle({"type": "add", "id": tag, "request": r})
        done = {}
        while wp.batcher.has_work():
            wp.batcher.wait_ready()
            for tag, out in wp.batcher.step():
                done[tag] = out
        torch.cuda.synchronize()
        while not outbox.empty():
            msg = outbox.get()
            done[msg["id"]] = msg["output"]
        return done, forwards

    reqs = {"ra": _req(w, "a", seed=1), "rb": _req(w, "b", seed=2), "rn": _req(w, None, seed=3), "bad": _req(w, "nope", seed=4)}
    done, forwards = serve(reqs)
    assert set(done) == set(reqs)
    assert done["bad"].error and "nope" in done["bad"].error and "KeyError" in done["bad"].error
    assert all(len(f) == 1 for f in forwards) and len(forwards) == 3 * 2
    outs = {}
    for tag in ("ra", "rb", "rn"):
        assert done[tag].error is None
        solo, f = serve({tag: reqs[tag]})
        assert len(f) == 2
        outs[tag] = done[tag].output.float().cpu()
        assert torch.equal(outs[tag], solo[tag].output.float().cpu()), tag
    assert m.active_lora in ((), (("a", 1.0),), (("b", 1.0),))
    # the adapters did something: the same request under another adapter gives another latent
    other, _ = serve({"x": _req(w, None, seed=1)})
    assert not torch.equal(other["x"].output.float().cpu(), outs["ra"])
    # "a" is still the active combination after its last request: the engine's remove_lora works all the same
    serve({"ra": reqs["ra"]})
    assert m.active_lora == (("a", 1.0),)
    assert serve.wp._handle({"type": "rpc", "id": 9, "method": "remove_lora", "args": ("a",)})
    assert serve.wp.outbox.get_nowait()["result"] is None and m.active_lora == () and serve.wp.worker.pipeline.lora_names() == {"b"}
