"""GPU: the native Qwen2.5-VL vision tower and Edit prompt encoder - the new row kernels against fp32 torch, the multimodal text
forward against the text-only one, vision tower + language model against the SAME HF model run in fp32, and an Edit request from
a prompt string and a picture with the native encoder against the HF encoder.

Bars (the project's, tests/test_gpu_text_encoder.py):
  row kernels      |err| <= 2^-7 (|ref| + rms(ref)) per element; copies and pad columns bit-exact.
  whole forward    the oracle is HF in fp32 on the same bf16 weights, pictures and tokens, called with EXPLICIT 3-D position_ids
                   (see _vl_factory.py).  d_eager = rel-L2 of HF's own bf16 eager pass against it; d_native <= 1.25 d_eager and
                   cos >= 0.9995, for the vision tower's output alone (HF order) and for the final prompt embeddings.
  pipeline         final latents within the project's <= 4-layer forward bar: rel-L2 <= 1e-2, cos >= 0.9995.
Measured on MI355X: see BASELINE.md section 3."""
import pytest
import torch

import _vl_factory as F
from _util import cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = torch.device("cuda:0")


def elem_close(got, ref, what=""):
    ref, got = ref.float().cpu(), got.float().cpu()
    rms = ref.pow(2).mean().sqrt()
    err = ((got - ref).abs() / (ref.abs() + rms)).max().item()
    print(f"{what}: max scaled err {err:.3e} (bar {2 ** -7:.3e})")
    assert err <= 2 ** -7, f"{what}: max scaled err {err}"


# ------------------------------------------------------------------------------------------------------------ row kernels
def _rope_pad_reference(qkv, H, hd, cos, sin):
    rows = qkv.shape[0]
    x = qkv.float().view(rows, 3, H, hd)
    half = hd // 2
    c, s = cos[:, None, None, :], sin[:, None, None, :]
    lo, hi = x[:, :2, :, :half], x[:, :2, :, half:]
    ref = torch.zeros(rows, 3, H, 128)
    ref[:, :2, :, :half], ref[:, :2, :, half:hd] = lo * c - hi * s, hi * c + lo * s          # apply_rotary_pos_emb_vision
    ref[:, 2, :, :hd] = x[:, 2]
    return ref


@pytest.mark.parametrize("hd", [80, 32])
@pytest.mark.parametrize("H", [4, 16])
@pytest.mark.parametrize("rows", [1, 63, 65, 257])
def test_vision_rope_pad_against_fp32(rows, H, hd):
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(1000 * rows + 10 * H + hd)
    qkv = torch.randn(rows, 3 * H * hd, generator=g).to(BF16)
    ang = torch.rand(rows, hd // 2, generator=g) * 40 - 20
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    ref = _rope_pad_reference(qkv, H, hd, cos, sin)
    got = ops.vision_rope_pad(qkv.to(DEV), H, hd, cos.to(DEV), sin.to(DEV)).cpu().view(rows, 3, H, 128)
    elem_close(got[:, :2, :, :hd], ref[:, :2, :, :hd], f"vision rope rows={rows} H={H} hd={hd}")
    assert torch.equal(got[:, 2, :, :hd], qkv.view(rows, 3, H, hd)[:, 2])      # v: bit for bit
    assert not got[..., hd:].view(torch.int16).any()                          # pad columns: exact (+0) zeros


def test_vision_rope_pad_row_strides():
    """Input rows 64 columns apart from each other's end, output rows inside a wider buffer: nothing outside is touched."""
    from vllm_omni_amd import ops

    rows, H, hd = 37, 4, 80
    g = torch.Generator().manual_seed(5)
    inbuf = torch.randn(rows, 3 * H * hd + 64, generator=g).to(BF16)
    outbuf = torch.full((rows, 3 * H * 128 + 32), 7.0, dtype=BF16)
    ang = torch.rand(rows, hd // 2, generator=g) * 6
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    dout = outbuf.to(DEV)
    ops.vision_rope_pad(inbuf.to(DEV)[:, :3 * H * hd], H, hd, cos.to(DEV), sin.to(DEV), out=dout[:, :3 * H * 128])
    got = dout.cpu()
    ref = _rope_pad_reference(inbuf[:, :3 * H * hd], H, hd, cos, sin)
    view = got[:, :3 * H * 128].reshape(rows, 3, H, 128)
    elem_close(view[:, :2, :, :hd], ref[:, :2, :, :hd], "vision rope row strides")
    assert torch.equal(view[:, 2, :, :hd], inbuf[:, 2 * H * hd:3 * H * hd].reshape(rows, H, hd))
    assert not view[..., hd:].view(torch.int16).any()
    assert torch.equal(got[:, 3 * H * 128:], outbuf[:, 3 * H * 128:])          # the 32 columns behind every output row


def _mrope_reference(qkv, H, Hkv, cos_tab, sin_tab, pos3, section):
    """HF apply_multimodal_rotary_pos_emb restated: cos / sin [3, rows, 128], sections doubled, chunk i from row i % 3."""
    rows = qkv.shape[0]
    cos3 = torch.stack([torch.cat([cos_tab[p], cos_tab[p]], -1) for p in pos3.long()])
    sin3 = torch.stack([torch.cat([sin_tab[p], sin_tab[p]], -1) for p in pos3.long()])
    sec = list(section) * 2
    cos = torch.cat([m[i % 3] for i, m in enumerate(cos3.split(sec, dim=-1))], dim=-1)[:, None, :]
    sin = torch.cat([m[i % 3] for i, m in enumerate(sin3.split(sec, dim=-1))], dim=-1)[:, None, :]
    x = qkv.float().view(rows, H + 2 * Hkv, 128)
    rot = torch.cat((-x[..., 64:], x[..., :64]), dim=-1)
    ref = x.clone()
    ref[:, :H + Hkv] = (x * cos + rot * sin)[:, :H + Hkv]
    return ref


@pytest.mark.parametrize("heads", [(4, 2), (28, 4)])
@pytest.mark.parametrize("rows", [1, 65, 257])
def test_text_mrope_against_fp32_and_bit_equal_to_rope_neox_for_equal_rows(rows, heads):
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import text_rope_tables

    H, Hkv = heads
    sec = [16, 24, 24]
    g = torch.Generator().manual_seed(100 * rows + H)
    qkv = torch.randn(rows, (H + 2 * Hkv) * 128, generator=g).to(BF16)
    pos3 = torch.randint(0, 1101, (3, rows), generator=g, dtype=torch.int32)
    pos3[:, 0] = torch.tensor([0, 1100, 517])                          # unequal rows, both ends of the table
    cos, sin = text_rope_tables(1000000.0, 1101)
    ref = _mrope_reference(qkv, H, Hkv, cos, sin, pos3, sec)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.text_mrope_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), pos3.to(DEV), sec, err=err).cpu().view(rows, -1, 128)
    elem_close(got[:, :H + Hkv], ref[:, :H + Hkv], f"mrope rows={rows} heads={heads}")
    assert torch.equal(got[:, H + Hkv:], qkv.view(rows, -1, 128)[:, H + Hkv:]) and int(err.item()) == 0
    # (the sections matter: with the temporal row everywhere the result differs)
    one = ops.text_rope_neox_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), pos3[0].contiguous().to(DEV)).cpu().view(rows, -1, 128)
    assert not torch.equal(got, one)
    same = pos3[1:2].expand(3, -1).contiguous()
    a = ops.text_mrope_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), same.to(DEV), sec, err=err)
    b = ops.text_rope_neox_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), same[0].contiguous().to(DEV), err=err)
    assert torch.equal(a, b) and int(err.item()) == 0


def test_text_mrope_position_clamp_sets_the_error_word():
    from vllm_omni_amd import ops
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import text_rope_tables

    H, Hkv, rows, sec = 4, 2, 6, [16, 24, 24]
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(rows, 8 * 128, generator=g).to(BF16)
    cos, sin = text_rope_tables(1000000.0, 1101)
    base = torch.tensor([0, 7, 1100, 5, 5, 5], dtype=torch.int32)[None].expand(3, -1)
    for sec_row, col, bad in ((0, 3, 1101), (1, 4, -1), (2, 5, 4000)):   # one bad entry, in each of the three position rows
        pos3 = base.clone()
        pos3[sec_row, col] = bad
        ref = _mrope_reference(qkv, H, Hkv, cos, sin, pos3.clamp(0, 1100), sec)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.text_mrope_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), pos3.to(DEV), sec, err=err).cpu().view(rows, 8, 128)
        assert int(err.item()) != 0, (sec_row, col)
        elem_close(got[:, :6], ref[:, :6], f"mrope clamp row {sec_row}")
        assert torch.equal(got[:, 6:], qkv.view(rows, 8, 128)[:, 6:])
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.text_mrope_(qkv.to(DEV), H, Hkv, cos.to(DEV), sin.to(DEV), base.contiguous().to(DEV), sec, err=err)
    assert int(err.item()) == 0                                          # positions 0 and npos - 1 are inside


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("width", [64, 5120])
@pytest.mark.parametrize("rows", [1, 65, 257])
def test_gelu_erf_against_fp32(rows, width, blocked):
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(rows + width)
    x = (torch.randn(rows, width, generator=g) * 2.5).to(BF16)
    ref = torch.nn.functional.gelu(x.float())                           # nn.GELU(): the exact erf form
    got = ops.gelu_erf(x.to(DEV), out_k32_blocked=blocked)
    if blocked:
        got = ops.k32_blocked_to_rows(got)
    elem_close(got, ref, f"gelu rows={rows} n={width} blocked={blocked}")
    if not blocked:
        d = x.to(DEV)
        assert ops.gelu_erf(d, out=d) is d and torch.equal(d, got)      # in place: the same bits


# ------------------------------------------------------------------------------------------------------------ mm forward
@pytest.fixture(scope="module")
def small_text():
    from test_gpu_text_encoder import _hf_pair

    return _hf_pair(512, 2, 4, 2, 192, seed=21, qk_gain=4.0)


def _text_native(model):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import ByteTokenizer, NativeQwenPromptEncoder

    return NativeQwenPromptEncoder.from_hf(model, ByteTokenizer(), template="ab{}c", drop_idx=2)


def test_mm_forward_without_pictures_is_the_text_forward_bit_for_bit(small_text):
    from vllm_omni_amd import ops

    native = _text_native(small_text[0])
    g = torch.Generator().manual_seed(2)
    lens = [33, 70, 260]
    ids = torch.randint(3, 259, (sum(lens),), generator=g, dtype=torch.int32).to(DEV)
    cu = torch.tensor([0, 33, 103, 363], dtype=torch.int32, device=DEV)
    pos = torch.cat([torch.arange(n, dtype=torch.int32) for n in lens]).to(DEV)
    want = native.encode_packed(ids, cu, pos, 260).clone()
    got = ops.qwen2_text_forward_mm(native._descriptor(), ids, cu, pos[None].expand(3, -1).contiguous(), [16, 24, 24], 260,
                                    native._workspace)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.isfinite(got.float()).all()


def test_bad_vision_row_is_a_zero_row_reported_by_the_next_call_and_never_read(small_text):
    from vllm_omni_amd import ops
    from vllm_omni_amd._native import OmniNativeError

    native = _text_native(small_text[0])
    w = native._descriptor()
    g = torch.Generator().manual_seed(4)
    ids = torch.tensor([5, 6, 7, 8, 9, 10], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 6], dtype=torch.int32, device=DEV)
    pos3 = torch.arange(6, dtype=torch.int32, device=DEV)[None].expand(3, -1).contiguous()
    buf = torch.randn(4, 512, generator=g).to(BF16).to(DEV)
    buf[2] = float("nan")                                              # what lies behind the two vision rows: must not be read
    buf[3] = 0
    vis = buf[:2]
    ws = torch.zeros(ops.qwen2_text_workspace_bytes(w, 6), dtype=torch.uint8, device=DEV)
    run = lambda rows, row_of: ops.qwen2_text_forward_mm(w, ids, cu, pos3, [16, 24, 24], 6, ws, vision_rows=rows,
                                                         vision_row_of=torch.tensor(row_of, dtype=torch.int32, device=DEV))
    good = run(vis, [-1, 0, 1, -1, -1, -1]).clone()
    assert torch.isfinite(good.float()).all()
    assert not torch.equal(good, ops.qwen2_text_forward_mm(w, ids, cu, pos3, [16, 24, 24], 6, ws))     # the vision rows went in
    for bad in (2, -2):                                                # one past the rows; below -1
        out = run(vis, [-1, 0, bad, -1, -1, -1]).clone()                # runs: the row is ZERO (not row 2 of the buffer) ...
        with pytest.raises(OmniNativeError, match="bad argument"):
            run(vis, [-1, 0, 1, -1, -1, -1])                            # ... and the next call over the workspace reports it
        zero = torch.cat([vis, buf[3:4]])                               # the same forward with an explicit zero row 2
        want = run(zero, [-1, 0, 2, -1, -1, -1])                        # (the error word was cleared by the refusal)
        assert torch.equal(out, want) and torch.isfinite(out.float()).all()
    assert torch.equal(run(vis, [-1, 0, 1, -1, -1, -1]), good)


# ------------------------------------------------------------------------------------------------------------ whole encoder
def _encoders(eager, oracle, proc, multi):
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenEditPromptEncoder, QwenEditPromptEncoder

    return (NativeQwenEditPromptEncoder.from_hf(eager, proc, multi_image=multi),
            QwenEditPromptEncoder(F.HFWithPositions(eager), proc, dtype=BF16, multi_image=multi),
            QwenEditPromptEncoder(F.HFWithPositions(oracle), proc, dtype=torch.float32, multi_image=multi))


def _bar(got, eag, ref, what):
    d_native, d_eager, c = rel_l2(got, ref), rel_l2(eag, ref), cosine(got, ref)
    print(f"{what}: d_native {d_native:.4e}  d_eager {d_eager:.4e}  ratio {d_native / d_eager:.3f} (bar 1.25)  cos {c:.6f} (bar 0.9995)")
    assert d_native <= 1.25 * d_eager, (what, d_native, d_eager)
    assert c >= 0.9995, (what, c)


def _check_against_oracle(eager, oracle, native, hf_eager, hf_oracle, prompt, pics, what):
    px = native.processor.image_processor(images=pics, return_tensors="pt")
    pv, thw = px["pixel_values"].to(DEV), px["image_grid_thw"].to(DEV)
    with torch.no_grad():
        ref_v = torch.cat(oracle.model.get_image_features(pv, thw).pooler_output)
        eag_v = torch.cat(eager.model.get_image_features(pv, thw).pooler_output)
    got_v = native.get_image_features(px["pixel_values"], px["image_grid_thw"])
    assert got_v.shape == eag_v.shape and got_v.dtype == BF16
    _bar(got_v, eag_v, ref_v, f"{what}: vision tower")
    image = pics if native.multi_image else pics[0]
    ref, ref_mask = hf_oracle.get_qwen_prompt_embeds(prompt, image=image)
    eag, eag_mask = hf_eager.get_qwen_prompt_embeds(prompt, image=image)
    got, got_mask = native.get_qwen_prompt_embeds(prompt, image=image)
    again, _ = native.get_qwen_prompt_embeds(prompt, image=image)
    torch.cuda.synchronize()
    assert got.shape == eag.shape and got.dtype == eag.dtype == BF16 and got.device == eag.device
    assert torch.equal(got_mask, eag_mask) and torch.equal(got_mask, ref_mask) and got_mask.dtype == eag_mask.dtype
    assert not got[~got_mask.bool()].any()                             # padded rows: exactly zero
    assert torch.equal(got, again)                                     # two identical calls: bit-equal
    _bar(got, eag, ref, f"{what}: prompt embeddings")
    return got


@pytest.fixture(scope="module")
def small_vl():
    return F.hf_pair(F.SMALL, seed=31, device=DEV, qk_gain=4.0)


def test_small_vl_model_edit_plus_two_pictures_against_hf_fp32(small_vl, monkeypatch):
    """Vision 320 / 4 heads of 80 / 420 -> 448 / depth 2 (block 1 attends over whole pictures) / window 112 / out 512; text 512,
    4 / 2 heads of 128, 192, 2 layers.  Grids (16, 22) + (10, 12): 472 patch rows (crossing 64, 128 and 256) in ten ragged
    windows.  The negative prompt after the positive one runs NO second vision forward and equals a fresh encoder's result."""
    from vllm_omni_amd import ops

    eager, oracle = small_vl
    proc = F.processor()
    native, hf_eager, hf_oracle = _encoders(eager, oracle, proc, multi=True)
    pics = F.pictures([(16, 22), (10, 12)])
    calls = []
    real = ops.qwen2_vision_forward
    monkeypatch.setattr(ops, "qwen2_vision_forward", lambda *a, **k: (calls.append(a[1].shape[0]), real(*a, **k))[1])
    got = _check_against_oracle(eager, oracle, native, hf_eager, hf_oracle, "turn the sky purple and keep the house", pics, "small VL")
    assert calls == [472]                                              # features + two encodes of one picture set: one forward
    assert got.shape[0] == 1 and got.shape[2] == 512 and got.shape[1] > 88 + 30
    neg, neg_mask = native.get_qwen_prompt_embeds("blurry", image=pics)
    assert calls == [472]                                              # the negative prompt reuses the vision result
    fresh, _, _ = _encoders(eager, oracle, proc, multi=True)
    neg2, neg_mask2 = fresh.get_qwen_prompt_embeds("blurry", image=pics)
    assert calls == [472, 472]
    assert torch.equal(neg, neg2) and torch.equal(neg_mask, neg_mask2) and not torch.equal(neg[:, -2:], got[:, -2:])
    ref_neg, _ = hf_oracle.get_qwen_prompt_embeds("blurry", image=pics)
    eag_neg, _ = hf_eager.get_qwen_prompt_embeds("blurry", image=pics)
    _bar(neg, eag_neg, ref_neg, "small VL: negative prompt")


def test_small_vl_model_edit_one_picture_against_hf_fp32(small_vl, monkeypatch):
    from vllm_omni_amd import ops

    eager, oracle = small_vl
    native, hf_eager, hf_oracle = _encoders(eager, oracle, F.processor(), multi=False)
    pics = F.pictures([(10, 12)], seed=9)
    calls = []
    real = ops.qwen2_vision_forward
    monkeypatch.setattr(ops, "qwen2_vision_forward", lambda *a, **k: (calls.append(a[1].shape[0]), real(*a, **k))[1])
    _check_against_oracle(eager, oracle, native, hf_eager, hf_oracle, "make the cat orange", pics, "small VL, Edit")
    native.get_qwen_prompt_embeds("blurry", image=pics[0])
    assert calls == [120]
    native.get_qwen_prompt_embeds("blurry", image=F.pictures([(10, 12)], seed=10)[0])           # another picture: a new forward
    assert calls == [120, 120]


def test_real_width_slice_against_hf_fp32():
    """Vision 1280 / 16 heads of 80 / 3420 -> 3456 / out 3584, depth 2; text one layer of 3584 / 28 over 4 heads / 18944; one
    picture of 16 x 22 patches."""
    eager, oracle = F.hf_pair(F.REAL_WIDTH, seed=32, device=DEV)
    native, hf_eager, hf_oracle = _encoders(eager, oracle, F.processor(), multi=False)
    _check_against_oracle(eager, oracle, native, hf_eager, hf_oracle, "a watercolour of a lighthouse at dusk", F.pictures([(16, 22)]),
                          "real width")


# ------------------------------------------------------------------------------------------------------------ pipeline
def test_edit_pipeline_from_prompt_and_picture_native_against_hf_encoder(small_vl):
    """A QwenImageEditPipeline (2-layer DiT at the text model's width) at 64 x 64 / 2 steps with true CFG: the native encoder
    against the HF encoder (on the position wrapper) on the same weights, same picture, same starting latents."""
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_edit import QwenImageEditPipeline
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    native, hf_eager, _ = _encoders(small_vl[0], small_vl[1], F.processor(), multi=False)
    tr = QwenImageTransformer2DModel(num_layers=2, num_attention_heads=2, joint_attention_dim=512, device=DEV)
    tr.init_random_(seed=11)
    vae = AutoencoderKLQwenImage(device=DEV, with_encoder=True).init_random_(seed=12)
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(1, 16, 64, generator=g).to(BF16)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1
    outs = {}
    for name, enc in (("hf", hf_eager), ("native", native)):
        pipe = QwenImageEditPipeline(od_config=OmniDiffusionConfig(use_hip_graph=False), device=DEV, transformer=tr, vae=vae,
                                     text_encoder=enc)
        req = OmniDiffusionRequest(prompt="make the cube red", negative_prompt="blurry", height=64, width=64, num_inference_steps=2,
                                   true_cfg_scale=4.0, latents=lat.clone(), output_type="latent", extra={"image": image})
        res = pipe.generate([req], output_type="latent")[0]
        assert res.error is None, res.error
        outs[name] = res.output.float().cpu()
    e, c = rel_l2(outs["native"], outs["hf"]), cosine(outs["native"], outs["hf"])
    print(f"edit pipeline latents: rel-L2 {e:.4e} (bar 1e-2)  cos {c:.6f} (bar 0.9995)")
    assert torch.isfinite(outs["native"]).all()
    assert e <= 1e-2 and c >= 0.9995, (e, c)
