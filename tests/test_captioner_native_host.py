"""CPU: the native captioner (omni_qwen2_text_prefill / omni_qwen2_text_decode_step and their kernels, NativeQwenCaptioner,
`OmniDiffusionConfig.native_captioner`) - everything about it that needs no device.

  1. ABI: the new structs against gcc, feature bit 64, the entry points as data symbols outside `PROTOTYPES`, version still 14,
     the existing structs at their sizes;
  2. every documented refusal of every new symbol, answered BEFORE any launch (made-up pointers);
  3. generation settings: honoured or refused by name, at construction;
  4. the config flag in all four pipelines, and the Layered pipeline's routing of an empty prompt."""
import ctypes as C
import os
import subprocess
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, LAUNCH, ALIGN = 0, -1, -2, -3, -4
P = 0x7F0000010000          # a "device pointer": 16-byte aligned, never dereferenced
ENTRY_POINTS = ("omni_gemv_bf16", "omni_decode_attention", "omni_decode_attention_workspace_bytes", "omni_text_penalized_argmax",
                "omni_qwen2_text_decode_state_bytes", "omni_qwen2_text_prefill", "omni_qwen2_text_decode_step")


# ---------------------------------------------------------------------------------------------------------------- 1
def test_new_structs_match_gcc(tmp_path):
    from vllm_omni_amd import _native as N

    pairs = [("omni_gemv_params", N.GemvParams), ("omni_decode_attn_params", N.DecodeAttnParams),
             ("omni_penalized_argmax_params", N.PenalizedArgmaxParams), ("omni_text_decode_layout", N.TextDecodeLayout),
             ("omni_text_decode_state", N.TextDecodeState)]
    body = ""
    for cname, cls in pairs:
        body += f'  printf("%zu", sizeof({cname}));\n'
        body += "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f, _ in cls._fields_) + '  printf("\\n");\n'
    consts = ("OMNI_FEATURE_TEXT_DECODE", "OMNI_DECODE_ATTN_CHUNK", "OMNI_DECODE_CUR_LEN", "OMNI_DECODE_ROPE_DELTA",
              "OMNI_DECODE_CUR_ID", "OMNI_DECODE_DONE", "OMNI_DECODE_N_GENERATED", "OMNI_DECODE_POS", "OMNI_DECODE_CTRL_WORDS")
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "omni_cdna4.h"\nint main(void) {\n' + body
                   + "".join(f'  printf("%d ", (int){c});\n' for c in consts)
                   + '  printf("\\n%zu %zu %zu\\n", sizeof(omni_text_weights), sizeof(omni_text_batch), sizeof(omni_text_batch_mm));\n'
                   + '  return 0;\n}\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    for (cname, cls), line in zip(pairs, lines):
        out = [int(v) for v in line.split()]
        assert out[0] == C.sizeof(cls), cname
        assert out[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    got = [int(v) for v in lines[len(pairs)].split()]
    assert got == [N.FEATURE_TEXT_DECODE, N.DECODE_ATTN_CHUNK, N.DECODE_CUR_LEN, N.DECODE_ROPE_DELTA, N.DECODE_CUR_ID, N.DECODE_DONE,
                   N.DECODE_N_GENERATED, N.DECODE_POS, N.DECODE_CTRL_WORDS]
    assert got[0] == 64
    # no existing struct changed
    assert [int(v) for v in lines[len(pairs) + 1].split()] == [88, 64, C.sizeof(N.TextBatchMm)]
    assert C.sizeof(N.TextWeights) == 88 and C.sizeof(N.TextBatch) == 64


def test_feature_bit_and_data_symbols():
    from vllm_omni_amd import _native as N

    assert N.features() & N.FEATURE_TEXT_DECODE and N.FEATURE_TEXT_DECODE == 64
    assert N.features() & N.FEATURE_VISION_ENCODER and N.features() & N.FEATURE_TEXT_ENCODER
    assert N.lib().omni_abi_version() == N.ABI_VERSION == 14
    dyn = subprocess.run(["nm", "-D", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kinds = {ln.split()[-1]: ln.split()[-2] for ln in dyn.splitlines() if len(ln.split()) >= 3}
    for name in ENTRY_POINTS:
        assert name not in N.PROTOTYPES and name in N.FEATURE_PROTOTYPES
        assert N.FEATURE_PROTOTYPES[name][2] == N.FEATURE_TEXT_DECODE
        assert kinds[name] in ("D", "R"), (name, kinds[name])          # a data symbol (a const pointer), not text
        assert callable(getattr(N.lib(), name))


# ---------------------------------------------------------------------------------------------------------------- 2
def _tweights(**kw):
    from test_text_encoder_native_host import _weights

    return _weights(**kw)


def _gemv(**kw):
    from vllm_omni_amd import _native as N

    p = N.GemvParams()
    vals = dict(A=P, lda=3584, M=1, N=4608, K=3584, w_k32_blocked=1, W=P, out=P, ldo=4608)
    vals.update(kw)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,want", [
    (dict(A=None), BAD_ARG), (dict(W=None), BAD_ARG), (dict(out=None), BAD_ARG), (dict(M=0), BAD_ARG), (dict(N=0), BAD_ARG),
    (dict(K=0), BAD_ARG), (dict(lda=3576), BAD_ARG), (dict(ldo=4600), BAD_ARG), (dict(res=P, ldres=8), BAD_ARG),
    (dict(w_k32_blocked=2), BAD_ARG),
    (dict(M=9), UNSUPPORTED), (dict(K=3600, lda=3600), UNSUPPORTED), (dict(out_f32=P), UNSUPPORTED),
    (dict(out=None, out_f32=P, res=P, ldres=4608), UNSUPPORTED),
    (dict(A=P + 8), ALIGN), (dict(W=P + 2), ALIGN), (dict(lda=3588), ALIGN),
])
def test_gemv_refusals_before_the_launch(kw, want):
    from vllm_omni_amd import _native as N

    assert N.lib().omni_gemv_bf16(C.byref(_gemv(**kw)), None) == want, kw
    assert N.lib().omni_gemv_bf16(None, None) == BAD_ARG


def _attn(**kw):
    from vllm_omni_amd import _native as N

    p = N.DecodeAttnParams()
    vals = dict(q=P, ldq=4608, k_cache=P, v_cache=P, out=P, ldo=3584, lens=P, len_add=1, n_seq=1, H=28, H_kv=4, head_dim=128,
                capacity=640, softmax_scale=0.088, workspace=P, workspace_bytes=1 << 40)
    vals.update(kw)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,want", [
    (dict(q=None), BAD_ARG), (dict(k_cache=None), BAD_ARG), (dict(v_cache=None), BAD_ARG), (dict(out=None), BAD_ARG),
    (dict(lens=None), BAD_ARG), (dict(workspace=None), BAD_ARG), (dict(n_seq=0), BAD_ARG), (dict(H=0), BAD_ARG),
    (dict(H_kv=0), BAD_ARG), (dict(capacity=0), BAD_ARG), (dict(ldq=3576), BAD_ARG), (dict(ldo=3576), BAD_ARG),
    (dict(workspace_bytes=4096), BAD_ARG),
    (dict(head_dim=64), UNSUPPORTED), (dict(n_seq=9), UNSUPPORTED), (dict(H=30, ldo=4608), UNSUPPORTED), (dict(H=36, ldq=8192, ldo=8192), UNSUPPORTED),
    (dict(q=P + 8), ALIGN), (dict(out=P + 8), ALIGN), (dict(k_cache=P + 8), ALIGN), (dict(v_cache=P + 8), ALIGN),
    (dict(workspace=P + 8), ALIGN), (dict(ldq=4612), ALIGN), (dict(ldo=3588), ALIGN),
])
def test_decode_attention_refusals_before_any_launch(kw, want):
    from vllm_omni_amd import _native as N

    L = N.lib()
    assert L.omni_decode_attention(C.byref(_attn(**kw)), None) == want, kw
    assert L.omni_decode_attention(None, None) == BAD_ARG
    assert L.omni_decode_attention_workspace_bytes(0, 28, 640) == 0 and L.omni_decode_attention_workspace_bytes(1, 28, 0) == 0
    need = L.omni_decode_attention_workspace_bytes(1, 28, 640)
    assert need % 256 == 0 and need >= 28 * 10 * 130 * 4               # (m, l, 128 values) per head and chunk of 64 keys


def _argmax(**kw):
    from vllm_omni_amd import _native as N

    p = N.PenalizedArgmaxParams()
    vals = dict(logits=P, ld=152064, seen=P, seen_stride=152064, ctrl=P, out_tokens=P, vocab=152064, n_seq=1, max_new=512, n_eos=2,
                penalty=1.05)
    vals.update(kw)
    for k, v in vals.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw,want", [
    (dict(logits=None), BAD_ARG), (dict(seen=None), BAD_ARG), (dict(ctrl=None), BAD_ARG), (dict(out_tokens=None), BAD_ARG),
    (dict(vocab=0), BAD_ARG), (dict(n_seq=0), BAD_ARG), (dict(max_new=0), BAD_ARG), (dict(penalty=0.0), BAD_ARG),
    (dict(penalty=-1.0), BAD_ARG), (dict(n_eos=-1), BAD_ARG), (dict(ld=100), BAD_ARG), (dict(seen_stride=100), BAD_ARG),
    (dict(n_seq=9), UNSUPPORTED), (dict(n_eos=9), UNSUPPORTED),
])
def test_penalized_argmax_refusals_before_the_launch(kw, want):
    from vllm_omni_amd import _native as N

    assert N.lib().omni_text_penalized_argmax(C.byref(_argmax(**kw)), None) == want, kw
    assert N.lib().omni_text_penalized_argmax(None, None) == BAD_ARG


def _state(w, **kw):
    from vllm_omni_amd import _native as N

    st = N.TextDecodeState()
    vals = dict(n_seq=1, capacity=640, max_new=512, n_eos=2, eos_ids=(C.c_int32 * 8)(151645, 151643), repetition_penalty=1.05,
                lm_head=P, state=P, state_bytes=1 << 40, workspace=P, workspace_bytes=1 << 40)
    vals.update(kw)
    for k, v in vals.items():
        setattr(st, k, v)
    return st


def _mm_batch(**kw):
    from vllm_omni_amd import _native as N

    b = N.TextBatchMm()
    vals = dict(n_prompts=1, total_rows=96, max_seqlen=96, input_ids=P, cu_seqlens=P, out=P, workspace=P, workspace_bytes=1 << 40,
                row_pos3=P, vision_rows=P, vision_row_of=P, n_vision_rows=24, mrope_section=(C.c_int32 * 3)(16, 24, 24))
    vals.update(kw)
    for k, v in vals.items():
        setattr(b, k, v)
    return b


STATE_REFUSALS = [
    (dict(lm_head=None), BAD_ARG), (dict(state=None), BAD_ARG), (dict(workspace=None), BAD_ARG), (dict(n_seq=0), BAD_ARG),
    (dict(capacity=0), BAD_ARG), (dict(max_new=0), BAD_ARG), (dict(n_eos=-1), BAD_ARG), (dict(repetition_penalty=0.0), BAD_ARG),
    (dict(state_bytes=4096), BAD_ARG), (dict(workspace_bytes=128), BAD_ARG),
    (dict(n_seq=9), UNSUPPORTED), (dict(n_eos=9), UNSUPPORTED),
    (dict(state=P + 8), ALIGN), (dict(workspace=P + 8), ALIGN), (dict(lm_head=P + 8), ALIGN), (dict(logits_out=P + 4), ALIGN),
]


@pytest.mark.parametrize("kw,want", STATE_REFUSALS)
def test_decode_step_and_prefill_refusals_before_any_launch(kw, want):
    from vllm_omni_amd import _native as N

    L, w = N.lib(), _tweights()
    assert L.omni_qwen2_text_decode_step(C.byref(w), C.byref(_state(w, **kw)), None) == want, kw
    assert L.omni_qwen2_text_prefill(C.byref(w), C.byref(_mm_batch()), C.byref(_state(w, **kw)), None) == want, kw


def test_decode_drivers_null_arguments_geometry_and_state_size():
    from vllm_omni_amd import _native as N

    L, w = N.lib(), _tweights()
    st = _state(w)
    assert L.omni_qwen2_text_decode_step(None, C.byref(st), None) == BAD_ARG
    assert L.omni_qwen2_text_decode_step(C.byref(w), None, None) == BAD_ARG
    assert L.omni_qwen2_text_prefill(C.byref(w), None, C.byref(st), None) == BAD_ARG
    assert L.omni_qwen2_text_prefill(C.byref(w), C.byref(_mm_batch()), None, None) == BAD_ARG
    assert L.omni_qwen2_text_prefill(None, C.byref(_mm_batch()), C.byref(st), None) == BAD_ARG
    # the batch and the state must agree; the prompt must fit the cache
    assert L.omni_qwen2_text_prefill(C.byref(w), C.byref(_mm_batch(n_prompts=2)), C.byref(st), None) == BAD_ARG
    assert L.omni_qwen2_text_prefill(C.byref(w), C.byref(_mm_batch()), C.byref(_state(w, capacity=95)), None) == BAD_ARG
    assert L.omni_qwen2_text_prefill(C.byref(w), C.byref(_mm_batch(row_pos3=None)), C.byref(st), None) == BAD_ARG
    for bad in (dict(head_dim=64), dict(num_heads=36, num_kv_heads=4)):             # head size; 9 query heads per K/V head
        wb = _tweights(**bad)
        assert L.omni_qwen2_text_decode_step(C.byref(wb), C.byref(st), None) == UNSUPPORTED, bad
        assert L.omni_qwen2_text_prefill(C.byref(wb), C.byref(_mm_batch()), C.byref(st), None) == UNSUPPORTED, bad
        assert L.omni_qwen2_text_decode_state_bytes(C.byref(wb), 1, 640, 512, None) == 0
    w._keep[1].down_w = None                                            # one missing matrix of one layer
    assert L.omni_qwen2_text_decode_step(C.byref(w), C.byref(st), None) == BAD_ARG
    w = _tweights()
    lay = N.TextDecodeLayout()
    assert L.omni_qwen2_text_decode_state_bytes(None, 1, 640, 512, None) == 0
    assert L.omni_qwen2_text_decode_state_bytes(C.byref(w), 9, 640, 512, None) == 0
    assert L.omni_qwen2_text_decode_state_bytes(C.byref(w), 1, 0, 512, None) == 0
    total = L.omni_qwen2_text_decode_state_bytes(C.byref(w), 1, 640, 512, C.byref(lay))
    cache = 2 * 1 * 4 * 640 * 128 * 2                                   # layers x sequences x K/V heads x positions x 128 bf16
    assert total == lay.total and total % 256 == 0 and total >= 2 * cache + 152064 * 5 + 512 * 4
    assert lay.v_cache - lay.k_cache == cache and lay.seen_stride >= 152064 and lay.ctrl == 0
    offs = [lay.ctrl, lay.out_tokens, lay.seen, lay.k_cache, lay.v_cache, lay.logits, lay.qkv]
    assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    # a state one byte short of that
    assert L.omni_qwen2_text_decode_step(C.byref(w), C.byref(_state(w, state_bytes=total - 1)), None) == BAD_ARG


# ---------------------------------------------------------------------------------------------------------------- 3
def _gc(**kw):
    from transformers import GenerationConfig

    return GenerationConfig(**kw)


def test_generation_settings_taken():
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import check_generation_config

    assert check_generation_config(_gc()) == dict(repetition_penalty=1.0, eos_ids=[])
    assert check_generation_config(_gc(do_sample=False, repetition_penalty=1.3, eos_token_id=7)) == dict(repetition_penalty=1.3, eos_ids=[7])
    # what the Qwen2.5-VL instruct checkpoints ship: sampling with ONE survivor is the penalised argmax
    got = check_generation_config(_gc(do_sample=True, top_k=1, top_p=0.001, temperature=0.1, repetition_penalty=1.05,
                                      eos_token_id=[151645, 151643], pad_token_id=151643, bos_token_id=151643))
    assert got == dict(repetition_penalty=1.05, eos_ids=[151645, 151643])


@pytest.mark.parametrize("kw,field", [
    (dict(num_beams=2), "num_beams"), (dict(do_sample=True, top_k=50), "top_k"), (dict(do_sample=True), "top_k"),
    (dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"), (dict(min_new_tokens=4), "min_new_tokens"),
    (dict(bad_words_ids=[[5]]), "bad_words_ids"), (dict(suppress_tokens=[3]), "suppress_tokens"),
    (dict(eos_token_id=list(range(9))), "eos_token_id"),
])
def test_generation_settings_refused_by_name(kw, field):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import check_generation_config

    with pytest.raises(NotImplementedError, match=rf"generation_config\.{field}\b"):
        check_generation_config(_gc(**kw))


def test_non_positive_penalty_is_refused_by_name():
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import check_generation_config

    with pytest.raises(NotImplementedError, match=r"generation_config\.repetition_penalty"):
        check_generation_config(types.SimpleNamespace(repetition_penalty=0.0))


@pytest.fixture(scope="module")
def small_vl():
    import _vl_factory as F

    return F.make_vl_model(F.SMALL, seed=5).to(torch.bfloat16)


def test_captioner_refuses_at_construction_before_touching_the_model(small_vl):
    import copy

    import _vl_factory as F

    from vllm_omni_amd.diffusion.models.qwen_image import text_encoder as T

    m = copy.deepcopy(small_vl)
    m.generation_config = _gc(num_beams=2)
    with pytest.raises(NotImplementedError, match="num_beams"):
        T.NativeQwenCaptioner.from_hf(m, F.processor(), free_source=True)
    assert len(m.model.visual.blocks) == 2 and len(m.model.language_model.layers) == 2
    m.generation_config = _gc(do_sample=True, top_k=1, repetition_penalty=1.05, eos_token_id=[2, 7])
    cap = T.NativeQwenCaptioner.from_hf(m, F.processor())
    assert len(m.model.language_model.layers) == 2                      # free_source defaults to off: Layered encoding stays HF
    assert cap.repetition_penalty == 1.05 and cap.eos_ids == [2, 7] and type(cap.encoder) is T.NativeQwenEditPromptEncoder
    assert cap.lm_head.shape == (512, 512) and torch.equal(cap.lm_head, m.lm_head.weight) and not cap.encoder.multi_image
    with pytest.raises(ValueError, match="max_new_tokens"):
        cap.prefill("x", None, max_new_tokens=0)


# ---------------------------------------------------------------------------------------------------------------- 4
class _Transformer:
    teacache = None
    use_layer3d_rope = use_additional_t_cond = True


_Transformer.__name__ = "QwenImageTransformer2DModel"


def _pipe(module, name, **cfg):
    import importlib

    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    cls = getattr(importlib.import_module(f"vllm_omni_amd.diffusion.models.qwen_image.{module}"), name)
    vae = types.SimpleNamespace(config=types.SimpleNamespace(latents_mean=[0.0] * 16, latents_std=[1.0] * 16), with_encoder=True)
    return cls(od_config=OmniDiffusionConfig(**cfg), device="cpu", transformer=_Transformer(), vae=vae)


def test_flag_defaults_off_and_only_the_layered_pipeline_takes_it():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig

    assert OmniDiffusionConfig().native_captioner is False
    for module, name in (("pipeline_qwen_image", "QwenImagePipeline"), ("pipeline_qwen_image_edit", "QwenImageEditPipeline"),
                         ("pipeline_qwen_image_edit_plus", "QwenImageEditPlusPipeline")):
        with pytest.raises(NotImplementedError, match="native_captioner"):
            _pipe(module, name, native_captioner=True)
    assert _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline", native_captioner=True).captioner is None


class _FakeCaptioner:
    def __init__(self):
        self.calls = []

    def generate(self, text, picture, max_new_tokens=512):
        self.calls.append((text, picture, max_new_tokens))
        return "a red cube on a table"


class _HFModel:
    """What `get_image_caption` asks of the HF model when the flag is off."""

    def __init__(self):
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def generate(self, input_ids=None, max_new_tokens=None, **kw):
        self.calls.append(max_new_tokens)
        return torch.cat([input_ids, torch.tensor([[11, 12]])], dim=1)


class _Proc:
    def __call__(self, text=None, images=None, padding=True, return_tensors="pt"):
        return _Mapping(input_ids=torch.tensor([[1, 2, 3]]))

    def batch_decode(self, ids, skip_special_tokens=True, clean_up_tokenization_spaces=False):
        return [" ".join(str(int(t)) for t in row) + " " for row in ids]


class _Mapping(dict):
    """A BatchFeature stand-in: `**inputs`, `.input_ids`, `.to(device)`."""

    def __getattr__(self, k):
        return self[k]

    def to(self, dev):
        return self


def test_layered_pipeline_routes_an_empty_prompt():
    from vllm_omni_amd.diffusion.models.qwen_image import pipeline_qwen_image_layered as PL

    picture = torch.zeros(1, 3, 32, 32)
    on = _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline", native_captioner=True)
    with pytest.raises(NotImplementedError, match="no captioner is loaded"):     # the flag never falls back to HF generate
        on.get_image_caption(picture)
    hf = _HFModel()
    on.text_encoder, on._caption_processor = types.SimpleNamespace(model=hf), _Proc()
    on.captioner = fake = _FakeCaptioner()
    assert on.get_image_caption(picture, use_en_prompt=True) == "a red cube on a table"
    assert fake.calls == [(PL.IMAGE_CAPTION_PROMPT_EN, picture, 512)] and hf.calls == []
    on.get_image_caption(picture, use_en_prompt=False)
    assert fake.calls[1][0] == PL.IMAGE_CAPTION_PROMPT_CN
    off = _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline")
    off.text_encoder, off._caption_processor = types.SimpleNamespace(model=hf), _Proc()
    assert off.captioner is None and off.get_image_caption(picture) == "11 12"   # HF generate, prompt trimmed, stripped
    assert hf.calls == [512]


def test_load_text_encoder_builds_the_captioner_only_with_the_flag(small_vl, tmp_path, monkeypatch):
    import copy

    import _vl_factory as F
    import transformers

    from vllm_omni_amd.diffusion.models.qwen_image import text_encoder as T

    m = copy.deepcopy(small_vl)
    proc = F.processor()
    for d in ("text_encoder", "tokenizer", "processor"):
        (tmp_path / d).mkdir()
    monkeypatch.setattr(transformers.Qwen2_5_VLForConditionalGeneration, "from_pretrained", classmethod(lambda cls, *a, **k: m))
    monkeypatch.setattr(transformers.AutoProcessor, "from_pretrained", classmethod(lambda cls, *a, **k: proc))
    monkeypatch.setattr(transformers.AutoTokenizer, "from_pretrained", classmethod(lambda cls, *a, **k: T.ByteTokenizer()))
    off = _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline")
    off.load_text_encoder(str(tmp_path))
    assert off.captioner is None and type(off.text_encoder) is T.QwenPromptEncoder
    on = _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline", native_captioner=True)
    on.load_text_encoder(str(tmp_path))
    assert type(on.captioner) is T.NativeQwenCaptioner and on.captioner.processor is proc
    assert type(on.text_encoder) is T.QwenPromptEncoder and len(m.model.language_model.layers) == 2   # encoding stays HF, whole
    m.generation_config = _gc(num_beams=4)
    bad = _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline", native_captioner=True)
    with pytest.raises(NotImplementedError, match="num_beams"):         # at load, not at the first empty prompt
        bad.load_text_encoder(str(tmp_path))
    (tmp_path / "processor").rmdir()
    with pytest.raises(FileNotFoundError, match="processor"):
        _pipe("pipeline_qwen_image_layered", "QwenImageLayeredPipeline", native_captioner=True).load_text_encoder(str(tmp_path))
