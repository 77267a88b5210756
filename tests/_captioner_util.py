"""Shared by the native captioner's tests (not collected): the stub processor with a `batch_decode`, the caption prompt of the
tests, and HF run over a whole sequence with explicit 3-D positions."""
import torch

import vl_stubs as V

PROMPT = "<|im_start|>user\n<|vision_start|><|image_pad|><|vision_end|>describe<|im_end|>\n<|im_start|>assistant\n"
GRID = (8, 12)                      # one picture of 8 x 12 patches: 24 picture tokens, a prompt of 96
P_LEN = 96
SPECIAL = frozenset({0, 1, 2, 499, V.IMAGE_TOKEN, V.VISION_START, V.VISION_END, V.IM_START, V.IM_END})


class DecodingProcessor:
    """`StubVLProcessor` plus the `batch_decode` a captioner ends with: token t reads "w<t>", special tokens can be skipped."""

    def __init__(self, stub, special=SPECIAL):
        self.stub, self.special = stub, frozenset(special)
        self.image_processor = stub.image_processor

    def __call__(self, *a, **k):
        return self.stub(*a, **k)

    def batch_decode(self, rows, skip_special_tokens=False, clean_up_tokenization_spaces=False):
        return [" " + " ".join(f"w{int(t)}" for t in row if not (skip_special_tokens and int(t) in self.special)) + " " for row in rows]


def hf_logits(model, positions_of, inputs, extra_ids, device):
    """fp32 logits [len, vocab] of ONE full-sequence forward of `model` over the processor's prompt followed by `extra_ids`, with
    explicit position_ids = get_rope_index(...) (see _vl_factory.py)."""
    ids = torch.cat([inputs.input_ids, torch.as_tensor(extra_ids, dtype=torch.long).view(1, -1)], dim=1).to(device)
    mask = torch.ones_like(ids)
    thw = inputs.image_grid_thw.to(device)
    with torch.no_grad():
        pos = positions_of.positions(ids, mask, thw)
        out = model(input_ids=ids, attention_mask=mask, position_ids=pos, pixel_values=inputs.pixel_values.to(device),
                    image_grid_thw=thw)
    return out.logits[0].float()


def penalize(logits_row, seen_ids, penalty):
    """HF RepetitionPenaltyLogitsProcessor on one row."""
    x = logits_row.clone()
    idx = torch.as_tensor(sorted(set(int(i) for i in seen_ids)), dtype=torch.long, device=x.device)
    v = x[idx]
    x[idx] = torch.where(v < 0, v * penalty, v / penalty)
    return x
