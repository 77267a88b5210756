"""CPU: LoRA adapter files -> merge plan (diffusion/lora.py), the public config / request surface, the binding of the optional
entry point, and the step batcher's adapter rules (tests/_fake_pipeline.py stands in for the pipeline)."""
import ctypes as C

import pytest
import torch

from vllm_omni_amd.diffusion import lora as L

BF16 = torch.bfloat16
D, JOINT, LAYERS = 256, 128, 2
TARGETS = L.target_shapes(LAYERS, D, JOINT, 64, 64)
QKV = "transformer_blocks.0.attn.to_qkv"


def _ab(rows, k, r, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, r, generator=g) * 0.1).to(BF16), (torch.randn(r, k, generator=g) * 0.1).to(BF16)


def _same_plan(p, q):
    assert p.keys() == q.keys()
    for k in p:
        assert torch.equal(p[k][0], q[k][0]) and torch.equal(p[k][1], q[k][1]) and p[k][2] == q[k][2], k


def test_targets_are_the_twelve_linears_per_layer_and_six_global():
    assert len(TARGETS) == LAYERS * 10 + 6
    assert TARGETS[QKV] == (3 * D, D, True) and TARGETS["transformer_blocks.1.img_mlp.net.2"] == (D, 4 * D, True)
    assert TARGETS["transformer_blocks.0.img_mod.1"] == (6 * D, D, False) and TARGETS["txt_in"] == (D, JOINT, False)
    assert TARGETS["time_text_embed.timestep_embedder.linear_1"] == (D, 256, False)


def test_key_spellings_prefixes_and_alpha_give_the_same_plan():
    up, down = _ab(D, D, 8, 1)
    mod = "transformer_blocks.1.attn.to_out.0"
    base = L.parse_adapter("a", {mod + ".lora_A.weight": down, mod + ".lora_B.weight": up}, TARGETS, D).updates
    assert list(base) == [(mod, 0, D)] and base[(mod, 0, D)][2] == 1.0
    for pre in ("", "transformer.", "diffusion_model."):
        kohya = L.parse_adapter("a", {pre + mod + ".lora_down.weight": down, pre + mod + ".lora_up.weight": up}, TARGETS, D)
        _same_plan(base, kohya.updates)
        peft = L.parse_adapter("a", {pre + mod + ".lora_A.weight": down.float(), pre + mod + ".lora_B.weight": up.float()}, TARGETS, D)
        _same_plan(base, peft.updates)
    # alpha: scale = alpha / rank; alpha == rank is the plain plan
    for alpha, want in ((8.0, 1.0), (4.0, 0.5), (16.0, 2.0)):
        got = L.parse_adapter("a", {mod + ".lora_down.weight": down, mod + ".lora_up.weight": up,
                                    mod + ".alpha": torch.tensor(alpha)}, TARGETS, D).updates
        assert got[(mod, 0, D)][2] == want
    # the user weight multiplies it
    ad = L.parse_adapter("a", {mod + ".lora_A.weight": down, mod + ".lora_B.weight": up, mod + ".alpha": torch.tensor(4.0)}, TARGETS, D)
    assert L.stack([(ad, 0.5)])[(mod, 0, D)][2] == 0.25


def test_split_qkv_keys_map_to_row_ranges_of_the_fused_matrices():
    t = {}
    ups = {}
    for pre, names in (("transformer_blocks.0.attn.", ("to_q", "to_k", "to_v")),
                       ("transformer_blocks.1.attn.", ("add_q_proj", "add_k_proj", "add_v_proj"))):
        for i, n in enumerate(names):
            up, down = _ab(D, D, 4, 10 + i)
            t[pre + n + ".lora_A.weight"], t[pre + n + ".lora_B.weight"] = down, up
            ups[pre, i] = up
    plan = L.parse_adapter("a", t, TARGETS, D).updates
    assert sorted(plan) == sorted([(QKV, i * D, D) for i in range(3)] + [("transformer_blocks.1.attn.add_kv_proj", i * D, D) for i in range(3)])
    for i in range(3):
        assert torch.equal(plan[(QKV, i * D, D)][0], ups["transformer_blocks.0.attn.", i])
        assert torch.equal(plan[("transformer_blocks.1.attn.add_kv_proj", i * D, D)][0], ups["transformer_blocks.1.attn.", i])
    # a FUSED key addresses the same three ranges, sharing its down
    upf, downf = _ab(3 * D, D, 4, 20)
    fused = L.parse_adapter("f", {QKV + ".lora_A.weight": downf, QKV + ".lora_B.weight": upf}, TARGETS, D).updates
    assert sorted(fused) == [(QKV, i * D, D) for i in range(3)]
    for i in range(3):
        assert torch.equal(fused[(QKV, i * D, D)][0], upf[i * D:(i + 1) * D]) and torch.equal(fused[(QKV, i * D, D)][1], downf)
    # split keys with one shared down == the fused spelling
    split = {}
    for i, n in enumerate(("to_q", "to_k", "to_v")):
        split[f"transformer_blocks.0.attn.{n}.lora_A.weight"] = downf
        split[f"transformer_blocks.0.attn.{n}.lora_B.weight"] = upf[i * D:(i + 1) * D]
    _same_plan(fused, L.parse_adapter("s", split, TARGETS, D).updates)


def test_stacking_concatenates_along_the_rank_with_the_documented_scales():
    mod = "transformer_blocks.0.img_mlp.net.0.proj"
    u1, d1 = _ab(4 * D, D, 8, 1)
    u2, d2 = _ab(4 * D, D, 4, 2)
    a = L.parse_adapter("a", {mod + ".lora_A.weight": d1, mod + ".lora_B.weight": u1}, TARGETS, D)
    b = L.parse_adapter("b", {mod + ".lora_A.weight": d2, mod + ".lora_B.weight": u2}, TARGETS, D)
    key = (mod, 0, 4 * D)
    # equal scales: bf16 factors untouched, the plain scale argument carries the factor
    up, down, s = L.stack([(a, 0.5), (b, 0.5)])[key]
    assert s == 0.5 and torch.equal(up, torch.cat([u1, u2], 1)) and torch.equal(down, torch.cat([d1, d2], 0))
    # different scales: up pre-scaled in fp32, rounded once; scale 1
    up, down, s = L.stack([(a, 0.7), (b, -0.3)])[key]
    assert s == 1.0 and up.dtype == BF16 and up.shape == (4 * D, 12) and down.shape == (12, D)
    assert torch.equal(up, torch.cat([(u1.float() * 0.7).to(BF16), (u2.float() * -0.3).to(BF16)], 1))
    assert torch.equal(down, torch.cat([d1, d2], 0))
    # an adapter that targets another module only adds its key
    other = L.parse_adapter("c", {"img_in.lora_A.weight": _ab(D, 64, 2, 3)[1], "img_in.lora_B.weight": _ab(D, 64, 2, 3)[0]}, TARGETS, D)
    plan = L.stack([(a, 1.0), (other, 2.0)])
    assert set(plan) == {key, ("img_in", 0, D)} and plan[("img_in", 0, D)][2] == 2.0 and plan[key][2] == 1.0


def test_total_rank_over_256_is_refused_by_name():
    mod = "transformer_blocks.0.attn.to_add_out"
    ads = []
    for i in range(3):
        u, d = _ab(D, D, 100, i)
        ads.append((L.parse_adapter(f"r{i}", {mod + ".lora_A.weight": d, mod + ".lora_B.weight": u}, TARGETS, D), 1.0))
    assert L.stack(ads[:2])[(mod, 0, D)][0].shape[1] == 200
    with pytest.raises(ValueError, match="to_add_out.*256|256.*to_add_out"):
        L.stack(ads)


def test_errors_fire_by_name():
    up, down = _ab(D, D, 4, 1)
    mod = "transformer_blocks.0.attn.to_out.0"
    with pytest.raises(KeyError, match="norm_q"):                                   # not a target
        L.parse_adapter("a", {"transformer_blocks.0.attn.norm_q.lora_A.weight": down,
                              "transformer_blocks.0.attn.norm_q.lora_B.weight": up}, TARGETS, D)
    with pytest.raises(KeyError, match="transformer_blocks.7"):                     # a layer this model does not have
        L.parse_adapter("a", {"transformer_blocks.7.attn.to_q.lora_A.weight": down,
                              "transformer_blocks.7.attn.to_q.lora_B.weight": up}, TARGETS, D)
    with pytest.raises(KeyError, match="lora_magnitude_vector"):                    # DoRA
        L.parse_adapter("a", {mod + ".lora_A.weight": down, mod + ".lora_B.weight": up,
                              mod + ".lora_magnitude_vector": torch.ones(D)}, TARGETS, D)
    with pytest.raises(KeyError, match="hada_w1_a"):                                # LoHa
        L.parse_adapter("a", {mod + ".hada_w1_a": down}, TARGETS, D)
    with pytest.raises(KeyError, match="to_out.0.*lora_B"):                         # missing partner
        L.parse_adapter("a", {mod + ".lora_A.weight": down}, TARGETS, D)
    with pytest.raises(KeyError, match="to_out.0.*lora_A"):
        L.parse_adapter("a", {mod + ".lora_up.weight": up}, TARGETS, D)
    with pytest.raises(KeyError, match="to_out.0"):                                 # an alpha alone
        L.parse_adapter("a", {mod + ".alpha": torch.tensor(4.0)}, TARGETS, D)
    with pytest.raises(ValueError, match="to_out.0"):                               # wrong out rows
        L.parse_adapter("a", {mod + ".lora_A.weight": down, mod + ".lora_B.weight": _ab(2 * D, D, 4, 1)[0]}, TARGETS, D)
    with pytest.raises(ValueError, match="to_out.0"):                               # wrong in columns
        L.parse_adapter("a", {mod + ".lora_A.weight": _ab(D, 2 * D, 4, 1)[1], mod + ".lora_B.weight": up}, TARGETS, D)
    with pytest.raises(ValueError, match="to_out.0"):                               # ranks disagree
        L.parse_adapter("a", {mod + ".lora_A.weight": _ab(D, D, 8, 1)[1], mod + ".lora_B.weight": up}, TARGETS, D)
    with pytest.raises(ValueError, match="to_q"):                                   # a split key carries D rows, not 3 D
        L.parse_adapter("a", {"transformer_blocks.0.attn.to_q.lora_A.weight": down,
                              "transformer_blocks.0.attn.to_q.lora_B.weight": _ab(3 * D, D, 4, 1)[0]}, TARGETS, D)
    with pytest.raises(ValueError, match="given twice"):                            # fused AND split rows of one matrix
        L.parse_adapter("a", {"transformer_blocks.0.attn.to_q.lora_A.weight": down, "transformer_blocks.0.attn.to_q.lora_B.weight": up,
                              QKV + ".lora_A.weight": down, QKV + ".lora_B.weight": _ab(3 * D, D, 4, 1)[0]}, TARGETS, D)
    with pytest.raises(KeyError, match="two down"):                                 # two spellings of one factor
        L.parse_adapter("a", {mod + ".lora_A.weight": down, mod + ".lora_down.weight": down, mod + ".lora_B.weight": up}, TARGETS, D)


def test_target_modules_filter_is_the_only_way_to_drop_keys():
    t = {}
    for n in ("to_q", "to_k", "to_v", "to_out.0"):
        up, down = _ab(D, D, 4, 1)
        t[f"transformer_blocks.0.attn.{n}.lora_A.weight"], t[f"transformer_blocks.0.attn.{n}.lora_B.weight"] = down, up
    t["transformer_blocks.0.attn.norm_q.lora_A.weight"] = down          # not a target: fatal unless filtered away
    t["transformer_blocks.0.attn.norm_q.lora_B.weight"] = up
    with pytest.raises(KeyError, match="norm_q"):
        L.parse_adapter("a", t, TARGETS, D)
    got = L.parse_adapter("a", t, TARGETS, D, target_modules=["to_q", "to_out.0"]).updates
    assert sorted(got) == [("transformer_blocks.0.attn.to_out.0", 0, D), (QKV, 0, D)]
    assert sorted(L.parse_adapter("a", t, TARGETS, D, target_modules=["attn.to_v"]).updates) == [(QKV, 2 * D, D)]
    assert not L.parse_adapter("a", t, TARGETS, D, target_modules=["q"]).updates        # suffix of a NAME, not of a string


def test_adapter_files_safetensors_and_pt(tmp_path):
    from safetensors.torch import save_file

    up, down = _ab(D, D, 4, 1)
    t = {"transformer.transformer_blocks.0.attn.to_out.0.lora_A.weight": down,
         "transformer.transformer_blocks.0.attn.to_out.0.lora_B.weight": up}
    save_file(t, str(tmp_path / "a.safetensors"))
    torch.save(t, str(tmp_path / "a.pt"))
    want = L.parse_adapter("a", t, TARGETS, D).updates
    for f in ("a.safetensors", "a.pt"):
        _same_plan(want, L.parse_adapter("a", L.read_adapter(str(tmp_path / f)), TARGETS, D).updates)
    with pytest.raises(ValueError, match="a.json"):
        L.read_adapter(str(tmp_path / "a.json"))


def test_config_and_request_surface():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    cfg = OmniDiffusionConfig(lora_adapters={"style": "/adapters/style.safetensors"}, max_resident_loras=2)
    assert cfg.lora_adapters == {"style": "/adapters/style.safetensors"} and cfg.max_resident_loras == 2
    assert OmniDiffusionConfig().lora_adapters is None and OmniDiffusionConfig().max_resident_loras == 1
    assert OmniDiffusionConfig().lora_switch_patience == 8
    with pytest.raises(NotImplementedError):                             # the reference's field stays refused
        OmniDiffusionConfig(lora_path="/adapters/x")
    with pytest.raises(ValueError):
        OmniDiffusionConfig(max_resident_loras=0)
    with pytest.raises(TypeError):
        OmniDiffusionConfig(lora_adapters=["/adapters/x"])
    r = OmniDiffusionRequest()
    assert r.lora is None and r.lora_scale == 1.0
    assert L.normalize_combo(None) == () and L.normalize_combo("a", 0.5) == (("a", 0.5),)
    assert L.normalize_combo([("a", 0.7), ("b", -0.3)]) == (("a", 0.7), ("b", -0.3))


def test_entry_point_is_a_feature_pointer_not_a_function():
    from vllm_omni_amd import _native as N

    name = "omni_lora_merge"
    assert name not in N.PROTOTYPES and name in N.FEATURE_PROTOTYPES
    res, args, bit = N.FEATURE_PROTOTYPES[name]
    assert res is C.c_int and bit == 8 == N.FEATURE_LORA_MERGE and len(args) == 2
    assert N.features() & N.FEATURE_LORA_MERGE
    assert N.ABI_VERSION == 14


def test_lora_merge_refuses_a_library_without_the_bit(monkeypatch):
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    monkeypatch.setattr(N, "features", lambda: 7)
    w = torch.zeros(32, 32, dtype=BF16)
    with pytest.raises(N.OmniNativeError, match="OMNI_FEATURE_LORA_MERGE"):
        ops.lora_merge(w, w, torch.zeros(32, 4, dtype=BF16), torch.zeros(4, 32, dtype=BF16), 1.0)


def test_lora_merge_never_falls_back_to_torch_off_gpu():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    w = torch.zeros(32, 32, dtype=BF16)
    with pytest.raises(N.OmniNativeError, match="GPU"):
        ops.lora_merge(w, w.clone(), torch.zeros(32, 4, dtype=BF16), torch.zeros(4, 32, dtype=BF16), 1.0)
    with pytest.raises(N.OmniNativeError, match="do not fit"):
        ops.lora_merge(w, w.clone(), torch.zeros(16, 4, dtype=BF16), torch.zeros(4, 32, dtype=BF16), 1.0)


def test_transformer_adapter_bookkeeping_on_the_host():
    """load / set / delete on a CPU model: names, errors, generations - nothing here touches a kernel."""
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel

    m = QwenImageTransformer2DModel(num_layers=LAYERS, num_attention_heads=2, joint_attention_dim=JOINT, device="cpu")
    up, down = _ab(D, D, 4, 1)
    m.load_lora_adapter("a", {"transformer_blocks.0.attn.to_q.lora_A.weight": down, "transformer_blocks.0.attn.to_q.lora_B.weight": up})
    m.load_lora_adapter("b", {"img_in.lora_A.weight": _ab(D, 64, 2, 3)[1], "img_in.lora_B.weight": _ab(D, 64, 2, 3)[0]})
    assert m.active_lora == ()
    gen = m._native_gen
    m.set_lora_adapters([])
    assert m._native_gen == gen                                             # no change: nothing goes stale
    m.set_lora_adapters(["a", "b"], weights=[0.7, -0.3])
    assert m.active_lora == (("a", 0.7), ("b", -0.3)) and m._native_gen == gen + 1
    with pytest.raises(KeyError, match="nope"):
        m.set_lora_adapters(["nope"])
    with pytest.raises(ValueError, match="twice"):
        m.set_lora_adapters(["a", "a"])
    with pytest.raises(ValueError, match="active"):
        m.delete_lora_adapter("a")
    assert m.active_lora == (("a", 0.7), ("b", -0.3))
    m.set_lora_adapters([])
    assert m.active_lora == () and m._native_gen == gen + 2
    m.delete_lora_adapter("a")
    with pytest.raises(KeyError, match="'a'"):
        m.delete_lora_adapter("a")
    with pytest.raises(KeyError, match="'a'"):
        m.set_lora_adapters(["a"])
    # the parameters are the base weights whatever is loaded: state_dict has no adapter entry
    assert not [k for k in m.state_dict() if "lora" in k]


# ---------------------------------------------------------------------------------------------------- step batcher
def _fake(patience=8, resident_cap=1, **cfg):
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    class LoraFake(FakePipeline):
        """FakePipeline + the adapter hooks the batcher asks for; a merge is counted whenever a non-resident combination runs."""

        def __init__(self, od_config):
            super().__init__(od_config)
            self.resident, self.merges, self.forward_combos = [()], 0, []

        def lora_names(self):
            return {"a", "b"}

        def lora_resident(self, combo):
            return tuple(combo) in self.resident

        def activate_lora(self, combo):
            combo = tuple(combo)
            if combo and combo not in self.resident:
                self.merges += 1
                self.resident = [()] + ([c for c in self.resident if c][-(resident_cap - 1):] if resident_cap > 1 else []) + [combo]
            self.forward_combos.append(combo)

    return LoraFake(OmniDiffusionConfig(max_step_batch=3, lora_switch_patience=patience, **cfg))


def _req(seed, lora=None, steps=6, scale=1.0):
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    return OmniDiffusionRequest(height=64, width=64, num_inference_steps=steps, seed=seed, lora=lora, lora_scale=scale,
                                prompt_embeds=torch.full((1, 3, 4), float(seed)))


def test_batcher_never_mixes_adapters_in_a_forward_and_results_are_solo_results():
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    pl = _fake(patience=2)
    b = ContinuousStepBatcher(pl)
    loras = {0: "a", 1: "b", 2: None, 3: "a", 4: None, 5: [("a", 1.0), ("b", 0.5)]}
    for tag, lo in loras.items():
        b.add(_req(tag + 1, lo), tag=tag)
    out = dict(b.drain())
    combo_of = {t: L.normalize_combo(lo) for t, lo in loras.items()}
    assert len(pl.steps_run) == len(pl.forward_combos)
    for (tags, _steps), combo in zip(pl.steps_run, pl.forward_combos):
        assert {combo_of[t] for t in tags} == {combo}                   # one combination per forward, and it is the activated one
    assert any(len(tags) == 2 for tags, _ in pl.steps_run)              # the two "a" requests and the two base requests DO share
    for tag in loras:                                                    # per-request results: the solo run's
        solo = ContinuousStepBatcher(_fake(), max_items=1)
        solo.add(_req(tag + 1, loras[tag]), tag=0)
        assert torch.equal(out[tag].output, solo.drain()[0][1].output)
    # a weight is part of the combination: "a" at 1.0 and "a" at 0.5 do not share
    pl2 = _fake()
    b2 = ContinuousStepBatcher(pl2)
    b2.add(_req(1, "a"), tag=0)
    b2.add(_req(2, "a", scale=0.5), tag=1)
    b2.drain()
    assert all(len(tags) == 1 for tags, _ in pl2.steps_run)


def test_batcher_unknown_adapter_is_a_keyerror_at_submission():
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    b = ContinuousStepBatcher(_fake())
    with pytest.raises(KeyError, match="nope"):
        b.add(_req(1, "nope"), tag=0)
    with pytest.raises(KeyError, match="zzz"):
        b.add(_req(1, [("a", 1.0), ("zzz", 1.0)]), tag=1)
    assert not b.has_work()


@pytest.mark.parametrize("patience", [0, 3, 8])
def test_patience_bounds_the_wait_of_a_non_resident_key(patience):
    """Adapter a is resident with a long loop; b arrives.  b's first forward comes after at most `patience` further forwards of
    a (and no earlier than that while a has work: the switch is what the rule delays); once b ran, a is the non-resident one."""
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    pl = _fake(patience=patience)
    b = ContinuousStepBatcher(pl)
    b.add(_req(1, "a", steps=40), tag="a")
    b.step()                                                             # a is active now
    assert pl.merges == 1
    b.add(_req(2, "b", steps=40), tag="b")
    first_b = None
    for i in range(40):
        b.step()
        if pl.forward_combos[-1] == (("b", 1.0),):
            first_b = i
            break
    assert first_b == patience, (first_b, patience)
    # from here the two alternate in runs of `patience` forwards (+ the one that switches), never a merge per forward
    b.drain()
    import itertools

    runs = [len(list(g)) for _, g in itertools.groupby(pl.forward_combos)]
    assert pl.merges == len(runs)                                        # one merge per RUN of forwards, not per forward
    assert max(runs[1:-1], default=0) <= patience + 1                    # (the first run includes the forward before b arrived)
    if patience:
        assert pl.merges <= 80 // patience + 2


def test_non_resident_key_runs_at_once_when_no_resident_key_has_work():
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    pl = _fake(patience=1000)
    b = ContinuousStepBatcher(pl)
    b.add(_req(1, "a", steps=3), tag=0)
    b.add(_req(2, "b", steps=3), tag=1)
    assert len(b.drain()) == 2 and len(pl.steps_run) == 6
    # the base model is always resident: with base work present, an adapter waits its patience out
    pl = _fake(patience=4)
    b = ContinuousStepBatcher(pl)
    b.add(_req(1, None, steps=10), tag=0)
    b.add(_req(2, "a", steps=2), tag=1)
    b.drain()
    assert pl.forward_combos[:4] == [()] * 4 and pl.forward_combos[4] == (("a", 1.0),)


def test_resident_combinations_alternate_freely():
    """max_resident_loras = 2: both adapters stay merged, so the keys are served round-robin as keys always were."""
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    pl = _fake(patience=5, resident_cap=2)
    b = ContinuousStepBatcher(pl)
    b.add(_req(1, "a", steps=20), tag=0)
    b.add(_req(2, "b", steps=20), tag=1)
    b.drain()
    assert pl.merges == 2
    first_b = pl.forward_combos.index((("b", 1.0),))
    assert first_b == 5                                                  # b's one merge waited its patience out ...
    both = pl.forward_combos[first_b:first_b + 2 * (20 - first_b)]       # ... and from then on, while a has work, they alternate
    assert all(x != y for x, y in zip(both, both[1:]))


@pytest.mark.parametrize("cfg", [{}, {"mixed_step_batch": True}, {"mixed_step_batch": True, "max_step_tokens": 40}])
def test_without_adapters_the_sequence_of_forwards_is_what_it_was(cfg):
    """lora=None everywhere: the same groups in the same order as a batcher whose pipeline knows nothing about adapters."""
    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.step_batcher import ContinuousStepBatcher

    def run(pl):
        b = ContinuousStepBatcher(pl)
        sizes = [(64, 64), (128, 64), (64, 64), (128, 128), (128, 64), (64, 64), (64, 64)]
        for i, (h, w) in enumerate(sizes):
            r = _req(i + 1, steps=2 + i % 3)
            r.height, r.width = h, w
            b.add(r, tag=i)
            if i % 2:
                b.step()
        outs = dict(b.drain())
        return pl.steps_run, outs

    plain = FakePipeline(OmniDiffusionConfig(max_step_batch=3, **cfg))
    assert not hasattr(plain, "activate_lora")
    seq0, out0 = run(plain)
    seq1, out1 = run(_fake(**cfg))
    assert seq0 == seq1 and len(seq0) > 5
    assert all(torch.equal(out0[k].output, out1[k].output) for k in out0)


# ---------------------------------------------------------------------------------------------------- worker rpc: add / remove
def _rpc(wp, outbox, method, *args):
    assert wp._handle({"type": "rpc", "id": 1, "method": method, "args": args})
    msg = outbox.get_nowait()
    assert msg["type"] == "rpc_result"
    return msg["result"]


def test_worker_rpc_adds_and_removes_adapters_also_while_one_is_still_active(tmp_path):
    """add_lora / remove_lora as the engine sends them, through WorkerProc._handle: the pipeline's own add / remove / activate
    code over a CPU transformer (nothing merges before a forward), the fake's denoising.  After its last request an adapter is
    still the ACTIVE combination: removing it then works and leaves the base model; while a sample in flight names it, removal
    is refused and nothing changes."""
    import queue

    from _fake_pipeline import FakePipeline
    from vllm_omni_amd.diffusion.data import DiffusionOutput, OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image import QwenImagePipeline as P
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.worker.gpu_worker import WorkerProc

    class Pipe(FakePipeline):
        add_lora, remove_lora, lora_names, lora_resident = P.add_lora, P.remove_lora, P.lora_names, P.lora_resident
        activate_lora, _retire_graphs = P.activate_lora, P._retire_graphs

        def __init__(self, od_config):
            super().__init__(od_config)
            self.transformer = QwenImageTransformer2DModel(num_layers=LAYERS, num_attention_heads=2, joint_attention_dim=JOINT,
                                                           device="cpu")
            self._step_state, self._serve_states, self._graph_gens = {}, {}, set()

    up, down = _ab(D, D, 4, 1)
    path = tmp_path / "a.pt"
    torch.save({"transformer_blocks.0.attn.to_q.lora_A.weight": down, "transformer_blocks.0.attn.to_q.lora_B.weight": up}, path)
    cfg = OmniDiffusionConfig(max_step_batch=3)
    pl = Pipe(cfg)
    outbox = queue.Queue()
    wp = WorkerProc(0, cfg, queue.Queue(), outbox, pipeline=pl)
    tr = pl.transformer

    assert _rpc(wp, outbox, "add_lora", "a", str(path)) is None and pl.lora_names() == {"a"}
    bad = _rpc(wp, outbox, "add_lora", "b", str(tmp_path / "missing.pt"))
    assert isinstance(bad, DiffusionOutput) and bad.error and pl.lora_names() == {"a"}
    # one request under "a", served to its end: "a" is still active afterwards (nothing went back to the base model)
    assert wp._handle({"type": "add", "id": "r1", "request": _req(1, "a", steps=3)})
    assert _rpc(wp, outbox, "lora_in_use", "a") == 1
    refused = _rpc(wp, outbox, "remove_lora", "a")                       # in flight: refused, nothing changes
    assert isinstance(refused, DiffusionOutput) and "in flight" in refused.error and pl.lora_names() == {"a"}
    replaced = _rpc(wp, outbox, "add_lora", "a", str(path))             # ... and not replaced under the sample's feet either
    assert isinstance(replaced, DiffusionOutput) and "in flight" in replaced.error
    assert len(wp.batcher.drain()) == 1
    assert tr.active_lora == (("a", 1.0),) and _rpc(wp, outbox, "lora_in_use", "a") == 0
    gen = tr._native_gen
    assert _rpc(wp, outbox, "remove_lora", "a") is None                  # the normal flow: active, but nobody uses it
    assert pl.lora_names() == set() and tr.active_lora == () and tr._native_gen != gen
    gone = _rpc(wp, outbox, "remove_lora", "a")
    assert isinstance(gone, DiffusionOutput) and "KeyError" in gone.error
    assert wp._handle({"type": "add", "id": "r2", "request": _req(2, "a")})           # and the name is unknown to new requests
    msg = outbox.get_nowait()
    assert msg["id"] == "r2" and "KeyError" in msg["output"].error


def test_engine_remove_asks_every_worker_first_and_add_is_all_or_nothing():
    """DiffusionEngine.add_lora / remove_lora over a recorded collective_rpc (no processes): a failed add on one worker removes
    the name from the others; a remove that any worker still needs removes it nowhere."""
    from vllm_omni_amd.diffusion.data import DiffusionOutput
    from vllm_omni_amd.diffusion.diffusion_engine import DiffusionEngine

    class Eng(DiffusionEngine):
        def __init__(self, replies):
            self.sent, self.replies = [], replies

        def collective_rpc(self, method, args=(), kwargs=None, timeout=None, unique_reply_rank=None):
            self.sent.append((method, args))
            return self.replies.get(method, [None, None])

        def __del__(self):
            pass

    e = Eng({})
    e.add_lora("a", "/x")
    e.remove_lora("a")
    assert e.sent == [("add_lora", ("a", "/x")), ("lora_in_use", ("a",)), ("remove_lora", ("a",))]
    e = Eng({"add_lora": [None, DiffusionOutput(error="ValueError: shape\ntraceback")]})
    with pytest.raises(RuntimeError, match="ValueError: shape"):
        e.add_lora("a", "/x")
    assert e.sent == [("add_lora", ("a", "/x")), ("remove_lora", ("a",))]
    e = Eng({"lora_in_use": [0, 2]})
    with pytest.raises(RuntimeError, match="2 sample"):
        e.remove_lora("a")
    assert e.sent == [("lora_in_use", ("a",))]


def test_lora_adapters_config_checks_keys_and_values():
    import pathlib

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    assert OmniDiffusionConfig(lora_adapters={"a": pathlib.Path("/adapters/a.safetensors")}).lora_adapters
    with pytest.raises(TypeError):
        OmniDiffusionConfig(lora_adapters={7: pathlib.Path("/adapters/a.safetensors")})       # a PathLike value excuses no key
    with pytest.raises(TypeError):
        OmniDiffusionConfig(lora_adapters={"a": 7})
