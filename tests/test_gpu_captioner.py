"""GPU: the native captioner - KV-cache greedy decode of the Qwen2.5-VL text model on the library.

  1. the three kernels alone: the GEMV family against fp64 at the GEMM tests' per-element bar with guarded buffers, decode
     attention against torch SDPA in fp32 (rel-L2 <= 4e-3, the project's attention bar), penalty + argmax + bookkeeping exactly;
  2. prefill: hidden state bit-equal to qwen2_text_forward_mm, cache rows bit-equal to the q|k|v buffer's K / V rows;
  3. cache consistency: step t's logits against a FRESH prefill over the first P + t + 1 tokens (new code against merged code);
  4. teacher-forced parity with HF: 40 logit rows against the fp32 twin, rel-L2 <= 1.25 x HF's own bf16 eager pass, cos >= 0.9995;
     with E = max |HF bf16 - HF fp32| the native argmax scores within 2E of the fp32 maximum and equals the fp32 argmax wherever
     the fp32 top-1 / top-2 gap exceeds 2E (native and eager round in different places at the same precision) - and the test
     asserts that EVERY step is that decisive, so the tokens must be HF's at all 40 steps;
  5. free-running generation with penalty 1.3 (every token within 2E' of the penalised fp32 maximum of its step, at least half
     the steps decisive) and plain greedy (equal to the fp32 HF greedy loop);
  6. stopping: EOS, max_new_tokens under chunk sizes 1 / 5 / 16, a cache one position short;
  7. a Layered request with an empty prompt."""
import pytest
import torch

import _captioner_util as U
import _gemm_check as G
import _vl_factory as F
from _util import cosine, rel_l2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = torch.device("cuda:0")
CHUNK = 64                                                              # N.DECODE_ATTN_CHUNK


# ------------------------------------------------------------------------------------------------------------ 1. GEMV
def _f32_guarded(rows, cols, ld):
    raw = torch.full((1024 + rows * ld + 1024,), -7.5e30, dtype=torch.float32, device=DEV)
    view = raw[1024:1024 + rows * ld].view(rows, ld)[:, :cols]

    def check():
        snap = raw.clone()
        snap[1024:1024 + rows * ld].view(rows, ld)[:, :cols] = -7.5e30
        assert bool((snap == -7.5e30).all()), "fp32 output: an element outside the written region changed"

    return view, check


@pytest.mark.parametrize("blocked", [False, True])
@pytest.mark.parametrize("M,N,K,mode", [(1, 3584, 3584, "plain"), (3, 4608, 3584, "bias"), (1, 3584, 18944, "res"),
                                        (2, 1000, 512, "f32"), (8, 512, 192, "plain")])
def test_gemv_against_fp64(M, N, K, mode, blocked):
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(M * 1000003 + N * 101 + K)
    a = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF16)
    bias = torch.randn(N, generator=g).to(BF16) if mode in ("bias", "f32") else None
    res = torch.randn(M, N, generator=g).to(BF16) if mode == "res" else None
    abuf = torch.zeros(M, K + 64, dtype=BF16, device=DEV)               # a row stride of its own
    abuf[:, :K] = a.to(DEV)
    wd = ops.w_to_k32_blocked(w.to(DEV)) if blocked else w.to(DEV)
    if mode == "res":
        r = G.reference(a, w, None, G.EPI_GATE_RES, res=res, gate=torch.ones(1, N, dtype=BF16), rows_per_item=M)
    else:
        r = G.reference(a, w, bias)
    what = f"gemv M={M} N={N} K={K} {mode} blocked={blocked}"
    if mode == "f32":
        out, check = _f32_guarded(M, N, N + 8)
        ops.gemv_bf16(abuf[:, :K], wd, None if bias is None else bias.to(DEV), out=out, out_f32=True, w_k32_blocked=blocked)
    else:
        out, check = G.guarded(M, N, ld=N + 8, device=DEV)
        if mode == "res":
            out.copy_(res.to(DEV))                                      # the residual aliases the output, as in the decode step
            ops.gemv_bf16(abuf[:, :K], wd, res=out, out=out, w_k32_blocked=blocked)
        else:
            ops.gemv_bf16(abuf[:, :K], wd, None if bias is None else bias.to(DEV), out=out, w_k32_blocked=blocked)
    torch.cuda.synchronize()
    check()
    G.assert_elementwise(out.cpu(), r.ref, r.extra, what)


# ------------------------------------------------------------------------------------------------------------ 1. attention
def _attn_case(H, Hkv, lens, capacity, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(lens)
    q = torch.randn(n, H * 128, generator=g).to(BF16)
    k = torch.randn(n, Hkv, capacity, 128, generator=g).to(BF16)
    v = torch.randn(n, Hkv, capacity, 128, generator=g).to(BF16)
    ref = torch.zeros(n, H * 128)
    for s, L in enumerate(lens):
        qs = q[s].float().view(H, 1, 128)
        ks = k[s, :, :L].float().repeat_interleave(H // Hkv, dim=0)
        vs = v[s, :, :L].float().repeat_interleave(H // Hkv, dim=0)
        ref[s] = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs).reshape(-1)
        k[s, :, L:] = float("nan")                                      # rows past the length: never read
        v[s, :, L:] = float("nan")
    return q, k, v, ref


@pytest.mark.parametrize("heads", [(4, 2), (28, 4)])                    # G = 2 and G = 7
@pytest.mark.parametrize("lens", [[1], [CHUNK - 1], [CHUNK], [CHUNK + 1], [2 * CHUNK + 3], [CHUNK + 1, 1, 2 * CHUNK + 3]])
def test_decode_attention_against_sdpa(heads, lens):
    from vllm_omni_amd import ops

    H, Hkv = heads
    cap = 3 * CHUNK + 8                                                 # more chunks than any length needs, a ragged last one
    q, k, v, ref = _attn_case(H, Hkv, lens, cap, seed=sum(lens) * 7 + H)
    out, check = G.guarded(len(lens), H * 128, ld=H * 128 + 8, device=DEV)
    qbuf = torch.zeros(len(lens), (H + 2 * Hkv) * 128, dtype=BF16, device=DEV)      # q inside a q|k|v row
    qbuf[:, :H * 128] = q.to(DEV)
    ops.decode_attention(qbuf[:, :H * 128], k.to(DEV), v.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), num_heads=H,
                         out=out)
    got = out.cpu().float()
    check()
    again = torch.empty_like(out)
    ops.decode_attention(qbuf[:, :H * 128], k.to(DEV), v.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV) - 1, num_heads=H,
                         len_add=1, out=again)                          # the decode step's form: cur_len + 1
    assert torch.equal(again.cpu().float(), got)
    for s in range(len(lens)):
        e = rel_l2(got[s], ref[s])
        print(f"decode attention H={H} Hkv={Hkv} len={lens[s]}: rel-L2 {e:.3e} (bar 4e-3)")
        assert torch.isfinite(got[s]).all() and e <= 4e-3, (lens[s], e)


def test_decode_attention_skips_a_done_sequence():
    from vllm_omni_amd import ops

    lens = [CHUNK + 1, 5, 2 * CHUNK + 3]
    q, k, v, ref = _attn_case(4, 2, lens, 3 * CHUNK, seed=77)
    out, check = G.guarded(3, 512, device=DEV)
    done = torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV)
    ops.decode_attention(q.to(DEV), k.to(DEV), v.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), num_heads=4, done=done,
                         out=out)
    torch.cuda.synchronize()
    check(written=torch.tensor([True, False, True]))                    # the done sequence's row is not written
    got = out.cpu().float()
    assert rel_l2(got[0], ref[0]) <= 4e-3 and rel_l2(got[2], ref[2]) <= 4e-3


# ------------------------------------------------------------------------------------------------------------ 1. argmax
def _ctrl(n_seq, cur_len, done=None, n_gen=None):
    from vllm_omni_amd import _native as N

    c = torch.zeros(N.DECODE_CTRL_WORDS, N.DECODE_MAX_SEQ, dtype=torch.int32)
    c[N.DECODE_CUR_LEN, :n_seq] = torch.tensor(cur_len, dtype=torch.int32)
    c[N.DECODE_CUR_ID, :n_seq] = -5
    if done is not None:
        c[N.DECODE_DONE, :n_seq] = torch.tensor(done, dtype=torch.int32)
    if n_gen is not None:
        c[N.DECODE_N_GENERATED, :n_seq] = torch.tensor(n_gen, dtype=torch.int32)
    return c


@pytest.mark.parametrize("vocab", [512, 1000, 152064])
def test_penalized_argmax_ties_penalty_eos_and_done(vocab):
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    g = torch.Generator().manual_seed(vocab)
    pen, max_new = 1.5, 6
    x = torch.randn(4, vocab, generator=g)
    seen = torch.zeros(4, vocab + 16, dtype=torch.uint8)
    # 0: the largest logit (positive) was seen -> divided, it loses to a TIE of two unseen ones: the lower index wins
    a, b, top = vocab - 3, vocab // 3, vocab // 2
    x[0, top], x[0, a], x[0, b] = 9.0, 7.0, 7.0
    seen[0, top] = 1
    # 1: every logit negative; the largest was seen -> multiplied, away from zero: the runner-up wins and it is an EOS id
    x[1] = -x[1].abs() - 1.0
    x[1, 5], x[1, vocab - 1] = -0.5, -0.6
    seen[1, 5] = 1
    # 2: done: untouched, whatever its logits;  3: a seen winner that still wins (9 / 1.5 > everything else)
    x[3, 17] = 40.0
    seen[3, 17] = 1
    ctrl = _ctrl(4, [10, 20, 30, 40], done=[0, 0, 1, 0], n_gen=[2, 0, 3, 5])
    out = torch.full((4, max_new), -1, dtype=torch.int32)
    want = []
    for s in range(4):
        p = torch.where(seen[s, :vocab].bool(), torch.where(x[s] < 0, x[s] * pen, x[s] / pen), x[s])
        want.append(int((p == p.max()).nonzero()[0]))
    assert want[0] == b and want[1] == vocab - 1 and want[3] == 17
    d_ctrl, d_out, d_seen = ctrl.to(DEV), out.to(DEV), seen.to(DEV)
    ops.penalized_argmax(x.to(DEV), d_seen, d_ctrl, d_out, penalty=pen, eos_ids=[3, vocab - 1])
    c, o, sn = d_ctrl.cpu(), d_out.cpu(), d_seen.cpu()
    for s, n0, l0 in ((0, 2, 10), (1, 0, 20), (3, 5, 40)):
        assert int(o[s, n0]) == want[s] and int(c[N.DECODE_CUR_ID, s]) == want[s] and int(sn[s, want[s]]) == 1, s
        assert int(c[N.DECODE_N_GENERATED, s]) == n0 + 1 and int(c[N.DECODE_CUR_LEN, s]) == l0 + 1
    assert c[N.DECODE_DONE, :4].tolist() == [0, 1, 1, 1]               # 1: EOS; 2: was done; 3: its sixth token of six
    assert torch.equal(c[:, 2], ctrl[:, 2]) and torch.equal(o[2], out[2]) and torch.equal(sn[2], seen[2])   # done: untouched
    o[0, 2] = o[1, 0] = o[3, 5] = -1
    assert torch.equal(o, out)                                          # nothing else of out_tokens was written
    sn[0, want[0]] = sn[1, want[1]] = 0
    assert torch.equal(sn, seen)
    # again: sequences 1 and 3 are done now and stay as they are; the prefill's form sets cur_len from cu_seqlens
    before = d_ctrl.clone()
    cu = torch.tensor([0, 7, 9, 12, 20], dtype=torch.int32, device=DEV)
    ops.penalized_argmax(x.to(DEV), d_seen, d_ctrl, d_out, penalty=pen, eos_ids=[3, vocab - 1], set_len_cu=cu)
    c2 = d_ctrl.cpu()
    assert torch.equal(c2[:, 1:4], before.cpu()[:, 1:4]) and int(c2[N.DECODE_CUR_LEN, 0]) == 7 and int(c2[N.DECODE_N_GENERATED, 0]) == 4


# ------------------------------------------------------------------------------------------------------------ models
_MODELS = {}


def _setup(geom_name, seed):
    """(eager bf16 HF, its fp32 twin, processor, the picture, the processor's inputs): built once per (geometry, seed)."""
    key = (geom_name, seed)
    if key not in _MODELS:
        # SMALL is built on the CPU and moved: the bars' analysis (every step decisive) was made for the CPU generator's weights
        eager, oracle = F.hf_pair(getattr(F, geom_name), seed=seed, device="cpu" if geom_name == "SMALL" else DEV)
        eager, oracle = eager.to(DEV), oracle.to(DEV)
        proc = U.DecodingProcessor(F.processor())
        pic = F.pictures([U.GRID])[0]
        inputs = proc(text=[U.PROMPT], images=pic, padding=True, return_tensors="pt")
        assert inputs.input_ids.shape == (1, U.P_LEN)
        _MODELS[key] = (eager, oracle, proc, pic, inputs)
    return _MODELS[key]


def _captioner(eager, proc, penalty=1.0, eos=None):
    from transformers import GenerationConfig

    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import NativeQwenCaptioner

    return NativeQwenCaptioner.from_hf(eager, proc, generation_config=GenerationConfig(repetition_penalty=penalty, eos_token_id=eos))


def _forced(seed):
    return torch.randint(3, 380, (1, 40), generator=torch.Generator().manual_seed(seed))[0]


def _teacher_forced(cap, pic, forced, max_new=64):
    """Native logits [1 + len(forced), vocab] (the prefill's row, then one per forced token) and the native argmax of each."""
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    w, st, P = cap.prefill(U.PROMPT, pic, max_new_tokens=max_new)
    rows = [st.logits[0].clone()]
    for t in forced.tolist():
        st.ctrl[N.DECODE_CUR_ID, 0] = t
        ops.qwen2_text_decode_step(w, st)
        rows.append(st.logits[0].clone())
    torch.cuda.synchronize()
    assert P == U.P_LEN and int(st.ctrl[N.DECODE_DONE, 0]) == 0 and int(st.ctrl[N.DECODE_N_GENERATED, 0]) == len(forced) + 1
    assert int(st.ctrl[N.DECODE_CUR_LEN, 0]) == P + len(forced)
    return torch.stack(rows), st.out_tokens[0, :len(forced) + 1].cpu(), st


# ------------------------------------------------------------------------------------------------------------ 2. prefill
def test_prefill_hidden_state_and_cache_are_the_forward_bit_for_bit():
    from vllm_omni_amd import ops

    eager, _, proc, pic, _ = _setup("SMALL", 11)
    cap = _captioner(eager, proc)
    enc = cap.encoder
    x = cap._inputs(U.PROMPT, pic)
    R, D, H, Hkv = x["rows"], 512, 4, 2
    w = enc.text._descriptor()
    for layers in (1, 2):                                               # the q|k|v buffer a forward leaves behind is its LAST layer's
        w.num_layers = layers
        try:
            _, st = cap._decode_state(R, 8)
            cap._state = None
            want = ops.qwen2_text_forward_mm(w, x["ids"], x["cu"], x["pos3"], enc.mrope_section, R, enc.text._workspace,
                                             vision_rows=x["vision_rows"], vision_row_of=x["vision_row_of"]).clone()
            st.k_cache.fill_(7.0)
            st.v_cache.fill_(7.0)
            got = ops.qwen2_text_prefill(w, st, x["ids"], x["cu"], x["pos3"], enc.mrope_section, R, vision_rows=x["vision_rows"],
                                         vision_row_of=x["vision_row_of"])
            torch.cuda.synchronize()
            assert torch.equal(got, want) and torch.isfinite(got.float()).all()
            off = 256 + 2 * ((R * D * 2 + 255) // 256 * 256)            # the workspace: error word, h, xn, then q|k|v
            qkv = enc.text._workspace[off:off + R * (H + 2 * Hkv) * 128 * 2].view(BF16).view(R, H + 2 * Hkv, 128)
            kc, vc = st.k_cache[layers - 1, 0], st.v_cache[layers - 1, 0]                      # [Hkv, capacity, 128]
            assert torch.equal(kc[:, :R].transpose(0, 1), qkv[:, H:H + Hkv]) and torch.equal(vc[:, :R].transpose(0, 1), qkv[:, H + Hkv:])
            assert bool((kc[:, R:] == 7.0).all()) and bool((vc[:, R:] == 7.0).all())           # nothing behind the prompt
            assert st.k_cache.shape[0] == layers
        finally:
            w.num_layers = 2


# ------------------------------------------------------------------------------------------------------------ 3. consistency
def test_every_steps_logits_match_a_fresh_prefill_over_the_same_tokens():
    """The decode attention runs the prefill attention's arithmetic tile for tile (bit-equal outputs on equal inputs); what is left
    between the two paths is the summation order of the GEMV against the MFMA GEMM.  Measured on MI355X: the first 15 steps
    bit-equal, worst scaled error over the 40 steps 7.55e-03 (bar 7.81e-03)."""
    from vllm_omni_amd import ops

    eager, _, proc, pic, _ = _setup("SMALL", 11)
    cap = _captioner(eager, proc)
    forced = _forced(11)
    native, _, _ = _teacher_forced(cap, pic, forced)
    enc = cap.encoder
    x = cap._inputs(U.PROMPT, pic)
    P = x["rows"]
    fresh = _captioner(eager, proc)                                     # its own state: the first one's cache is not touched
    worst = 0.0
    for t in range(len(forced)):
        n = P + t + 1
        ids = torch.cat([x["ids"], forced[:t + 1].to(DEV, torch.int32)])
        tail = (x["max_pos"] + 1 + torch.arange(t + 1, dtype=torch.int32, device=DEV))[None].expand(3, -1)
        pos3 = torch.cat([x["pos3"], tail], dim=1).contiguous()
        row_of = torch.cat([x["vision_row_of"], torch.full((t + 1,), -1, dtype=torch.int32, device=DEV)])
        cu = torch.tensor([0, n], dtype=torch.int32, device=DEV)
        wf, st = fresh._decode_state(n, 4)
        ops.qwen2_text_prefill(wf, st, ids, cu, pos3, enc.mrope_section, n, vision_rows=x["vision_rows"], vision_row_of=row_of)
        worst = max(worst, G.scaled_error(native[t + 1].cpu(), st.logits[0].cpu().double()))
    print(f"cache consistency: worst scaled error over {len(forced)} steps {worst:.3e} (bar {G.U:.3e})")
    assert worst <= G.U


# ------------------------------------------------------------------------------------------------------------ 4. HF parity
def _parity(geom_name, seed):
    eager, oracle, proc, pic, inputs = _setup(geom_name, seed)
    forced = _forced(seed)
    cap = _captioner(eager, proc)
    native, toks, _ = _teacher_forced(cap, pic, forced)
    native = native[:40].float().cpu()                                  # rows P - 1 .. P + 38
    P = U.P_LEN
    ref = U.hf_logits(oracle, F.HFWithPositions(oracle), inputs, forced, DEV)[P - 1:P + 39].cpu()
    eag = U.hf_logits(eager, F.HFWithPositions(eager), inputs, forced, DEV)[P - 1:P + 39].cpu()
    d_native, d_eager, c = rel_l2(native, ref), rel_l2(eag, ref), cosine(native, ref)
    E = float((eag - ref).abs().max())
    top2 = ref.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    print(f"{geom_name} seed {seed}: d_native {d_native:.4e}  d_eager {d_eager:.4e}  ratio {d_native / d_eager:.3f} (bar 1.25)  "
          f"cos {c:.6f} (bar 0.9995)  E {E:.4e}  min gap {float(gap.min()):.4e}  distinct argmax {ref.argmax(1).unique().numel()}")
    assert d_native <= 1.25 * d_eager, (d_native, d_eager)
    assert c >= 0.9995, c
    tok = toks[:40].long()
    score = ref.gather(1, tok[:, None])[:, 0]
    assert bool((score >= top2[:, 0] - 2 * E).all()), "a native token scores more than 2E under the fp32 maximum"
    decisive = gap > 2 * E
    assert torch.equal(tok[decisive], ref.argmax(1)[decisive])
    return decisive


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_teacher_forced_logits_and_tokens_against_hf_fp32(seed):
    decisive = _parity("SMALL", seed)
    assert bool(decisive.all()), "the inputs no longer make every step decisive: the token rule would not bind"


def test_teacher_forced_real_width_slice_against_hf_fp32():
    """One decoder layer at 3584 / 28 query heads over 4 K/V heads (G = 7) / 18944."""
    _parity("REAL_WIDTH", 11)
    _MODELS.pop(("REAL_WIDTH", 11))


# ------------------------------------------------------------------------------------------------------------ 5. free running
def _penalised_rows(model, inputs, g, penalty):
    logits = U.hf_logits(model, F.HFWithPositions(model), inputs, g, DEV)[U.P_LEN - 1:U.P_LEN - 1 + len(g)].cpu()
    prompt = inputs.input_ids[0].tolist()
    return torch.stack([U.penalize(logits[t], prompt + list(g[:t]), penalty) for t in range(len(g))])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_free_running_generation_with_repetition_penalty(seed):
    eager, oracle, proc, pic, inputs = _setup("SMALL", seed)
    g = _captioner(eager, proc, penalty=1.3).generate_ids(U.PROMPT, pic, max_new_tokens=48)
    assert len(g) == 48
    ref, eag = _penalised_rows(oracle, inputs, g, 1.3), _penalised_rows(eager, inputs, g, 1.3)
    E = float((eag - ref).abs().max())
    top2 = ref.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    score = ref.gather(1, torch.tensor(g)[:, None])[:, 0]
    decisive = gap > 2 * E
    print(f"free running seed {seed}: E' {E:.4e}  worst deficit {float((top2[:, 0] - score).max()):.4e}  decisive steps "
          f"{int(decisive.sum())}/48  distinct tokens {len(set(g))}")
    assert bool((score >= top2[:, 0] - 2 * E).all())
    assert int(decisive.sum()) * 2 >= 48, "fewer than half the steps are decisive: the rule would not bind"
    assert torch.equal(torch.tensor(g)[decisive], ref.argmax(1)[decisive])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_plain_greedy_equals_the_hf_fp32_greedy_loop(seed):
    eager, oracle, proc, pic, inputs = _setup("SMALL", seed)
    g = _captioner(eager, proc).generate_ids(U.PROMPT, pic, max_new_tokens=48)
    hf, gaps = [], []
    for _ in range(48):
        row = U.hf_logits(oracle, F.HFWithPositions(oracle), inputs, hf, DEV)[-1]
        t2 = row.topk(2).values
        gaps.append(float(t2[0] - t2[1]))
        hf.append(int(row.argmax()))
    print(f"plain greedy seed {seed}: native {g[:8]}..  hf {hf[:8]}..  min gap {min(gaps):.3e}  distinct {len(set(hf))}")
    assert g == hf


# ------------------------------------------------------------------------------------------------------------ 6. stopping
def test_eos_max_new_tokens_and_chunk_sizes():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    for seed in (11, 12, 13):                                           # the first model whose sequence has such a step
        eager, _, proc, pic, _ = _setup("SMALL", seed)
        free = _captioner(eager, proc, penalty=1.3)
        g = free.generate_ids(U.PROMPT, pic, max_new_tokens=48)
        k = next((i for i in range(3, 48) if g[i] not in g[:i]), None)  # EOS := the token the sequence first emits at step k >= 3
        if k is not None:
            break
    assert k is not None, "no sequence emits a new token at a step >= 3"
    cap = _captioner(eager, proc, penalty=1.3, eos=[g[k], 1])
    for chunk in (1, 5, 16):
        assert cap.generate_ids(U.PROMPT, pic, max_new_tokens=48, chunk=chunk) == g[:k + 1], chunk
        st = cap._state
        assert int(st.ctrl[N.DECODE_N_GENERATED, 0]) == k + 1 and int(st.ctrl[N.DECODE_DONE, 0]) == 1
        assert int(st.ctrl[N.DECODE_CUR_LEN, 0]) == U.P_LEN + k
    snap = st.buffer[:st.layout.logits].clone()                         # control words, out_tokens, seen map, both caches
    ops.qwen2_text_decode_step(cap.encoder.text._descriptor(), st, 3)   # a done sequence neither advances nor writes
    torch.cuda.synchronize()
    words = lambda buf: buf[st.layout.ctrl:st.layout.ctrl + 256].view(torch.int32).view(8, 8)
    words(snap)[N.DECODE_POS, 0] = st.ctrl[N.DECODE_POS, 0]            # (the scratch word every step rewrites: cur_len + rope_delta)
    assert torch.equal(st.buffer[:st.layout.logits], snap) and bool((st.out_tokens[0, k + 1:] == 0).all())
    assert cap.generate(U.PROMPT, pic, max_new_tokens=48) == proc.batch_decode([g[:k]])[0].strip()       # the EOS is dropped
    for chunk in (1, 5, 16):                                            # no EOS in reach: max_new_tokens ends it
        assert free.generate_ids(U.PROMPT, pic, max_new_tokens=7, chunk=chunk) == g[:7], chunk
        assert int(free._state.ctrl[N.DECODE_DONE, 0]) == 1 and int(free._state.ctrl[N.DECODE_CUR_LEN, 0]) == U.P_LEN + 6


def test_a_cache_one_position_short_stops_and_raises_the_error_word():
    from vllm_omni_amd import _native as N
    from vllm_omni_amd import ops

    eager, _, proc, pic, _ = _setup("SMALL", 11)
    cap = _captioner(eager, proc, penalty=1.3)
    g = cap.generate_ids(U.PROMPT, pic, max_new_tokens=8)
    enc = cap.encoder
    x = cap._inputs(U.PROMPT, pic)
    P, w = x["rows"], enc.text._descriptor()
    need_ws = ops.qwen2_text_workspace_bytes(w, P)
    lay = N.TextDecodeLayout()
    import ctypes as C
    cap_short = P + 3                                                   # five tokens need positions P .. P + 3: one short
    total = int(N.lib().omni_qwen2_text_decode_state_bytes(C.byref(w), 1, cap_short, 5, C.byref(lay)))
    raw_state = torch.full((4096 + total + 4096,), 0x5C, dtype=torch.uint8, device=DEV)
    raw_ws = torch.full((4096 + need_ws + 4096,), 0x5C, dtype=torch.uint8, device=DEV)
    raw_ws[4096:4096 + 256] = 0
    ws = raw_ws[4096:4096 + need_ws]
    st = ops.qwen2_decode_state(w, cap.lm_head, ws, 1, cap_short, 5, repetition_penalty=1.3, buffer=raw_state[4096:4096 + total])
    logits_raw = torch.full((1024 + 512 + 1024,), -3.0e30, dtype=torch.float32, device=DEV)
    st.logits = logits_raw[1024:1536].view(1, 512)
    st.desc.logits_out = st.logits.data_ptr()
    ops.qwen2_text_prefill(w, st, x["ids"], x["cu"], x["pos3"], enc.mrope_section, P, vision_rows=x["vision_rows"],
                           vision_row_of=x["vision_row_of"])
    ops.qwen2_text_decode_step(w, st, 3)
    torch.cuda.synchronize()
    assert int(st.ctrl[N.DECODE_DONE, 0]) == 0 and int(st.ctrl[N.DECODE_CUR_LEN, 0]) == cap_short and int(ws[:4].view(torch.int32)) == 0
    assert st.out_tokens[0, :4].tolist() == g[:4]
    snap = st.buffer[:st.layout.logits].clone()
    ops.qwen2_text_decode_step(w, st, 2)                                # the fifth token has no cache position left
    torch.cuda.synchronize()
    assert int(st.ctrl[N.DECODE_DONE, 0]) == 1 and int(st.ctrl[N.DECODE_N_GENERATED, 0]) == 4
    assert int(ws[:4].view(torch.int32)) != 0                           # the error word
    snap[st.layout.ctrl:st.layout.ctrl + 256].view(torch.int32).view(8, 8)[N.DECODE_DONE, 0] = 1
    snap[st.layout.ctrl:st.layout.ctrl + 256].view(torch.int32).view(8, 8)[N.DECODE_POS, 0] = st.ctrl[N.DECODE_POS, 0]
    assert torch.equal(st.buffer[:st.layout.logits], snap)              # nothing but the done flag moved
    for raw, size, what in ((raw_state, total, "state"), (raw_ws, need_ws, "workspace")):
        assert bool((raw[:4096] == 0x5C).all()) and bool((raw[4096 + size:] == 0x5C).all()), f"{what}: a guard band changed"
    assert bool((logits_raw[:1024] == -3.0e30).all()) and bool((logits_raw[1536:] == -3.0e30).all())
    with pytest.raises(N.OmniNativeError, match="omni_qwen2_text_prefill"):     # reported, as always, by the next call - and cleared
        ops.qwen2_text_prefill(w, st, x["ids"], x["cu"], x["pos3"], enc.mrope_section, P, vision_rows=x["vision_rows"],
                               vision_row_of=x["vision_row_of"])
    ops.qwen2_text_prefill(w, st, x["ids"], x["cu"], x["pos3"], enc.mrope_section, P, vision_rows=x["vision_rows"],
                           vision_row_of=x["vision_row_of"])
    torch.cuda.synchronize()
    assert int(st.out_tokens[0, 0]) == g[0]


# ------------------------------------------------------------------------------------------------------------ 7. pipeline
def test_layered_request_with_an_empty_prompt_is_captioned_natively():
    from vllm_omni_amd.diffusion.data import OmniDiffusionConfig
    from vllm_omni_amd.diffusion.models.qwen_image.autoencoder_kl_qwenimage import AutoencoderKLQwenImage
    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_layered import QwenImageLayeredPipeline
    from vllm_omni_amd.diffusion.models.qwen_image.qwen_image_transformer import QwenImageTransformer2DModel
    from vllm_omni_amd.diffusion.models.qwen_image.text_encoder import ByteTokenizer, QwenPromptEncoder
    from vllm_omni_amd.diffusion.request import OmniDiffusionRequest

    eager, _, proc, pic, _ = _setup("SMALL", 11)
    cap = _captioner(eager, proc, penalty=1.3)
    tr = QwenImageTransformer2DModel(num_layers=2, num_attention_heads=2, joint_attention_dim=512, use_additional_t_cond=True,
                                     use_layer3d_rope=True, device=DEV)
    tr.init_random_(seed=11)
    vae = AutoencoderKLQwenImage(device=DEV, with_encoder=True).init_random_(seed=12)
    pipe = QwenImageLayeredPipeline(od_config=OmniDiffusionConfig(use_hip_graph=False, native_captioner=True), device=DEV,
                                    transformer=tr, vae=vae, text_encoder=QwenPromptEncoder(eager, ByteTokenizer(), dtype=BF16))
    pipe.captioner, pipe.caption_max_new_tokens = cap, 24
    g = torch.Generator().manual_seed(4)
    lat = torch.randn(1, 3 * 16, 64, generator=g).to(BF16)
    image = torch.rand(1, 3, 64, 64, generator=g) * 2 - 1

    def run(prompt):
        req = OmniDiffusionRequest(prompt=prompt, negative_prompt="blurry", height=64, width=64, num_inference_steps=2,
                                   true_cfg_scale=4.0, latents=lat.clone(), output_type="latent",
                                   extra={"image": image, "prompt_image": pic, "layers": 2, "use_en_prompt": True})
        res = pipe.generate([req], output_type="latent")[0]
        assert res.error is None, res.error
        return req, res.output.float().cpu()

    from vllm_omni_amd.diffusion.models.qwen_image.pipeline_qwen_image_layered import IMAGE_CAPTION_PROMPT_EN

    caption = cap.generate(IMAGE_CAPTION_PROMPT_EN, pic, max_new_tokens=24)
    assert caption and caption == caption.strip()
    req, auto = run("")
    assert req.prompt == caption                                        # the request was captioned by the library
    _, given = run(caption)
    e, c = rel_l2(auto, given), cosine(auto, given)
    print(f"layered pipeline, caption {caption[:40]!r}..: rel-L2 {e:.4e} (bar 1e-2)  cos {c:.6f} (bar 0.9995)")
    assert torch.isfinite(auto).all() and e <= 1e-2 and c >= 0.9995, (e, c)
