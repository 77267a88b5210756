"""Ragged, token-major batch descriptors for the native DiT runner (host logic, no GPU needed).

The reference runs one request at a time (`reqs[0]`, vllm_omni/diffusion/worker/gpu_worker.py:128-130) and
zero-pads unequal prompts when B > 1 (pipeline_qwen_image.py:386-392), after which padded text rows ARE
attended to (the block ignores encoder_hidden_states_mask, qwen_image_transformer.py:545).  Parity target is
therefore per-request B=1 semantics; this module lets several requests (and the two true-CFG branches of one
request) share a DiT forward WITHOUT padding: rows of all items are concatenated, and small int32 maps tell the
kernels which item / joint row / RoPE position every token belongs to.

Item i contributes T_i text rows and S_i image rows (S_i = the tokens of item i's latent grid; the items of a forward
may sit on DIFFERENT grids, see `build_ragged_batch`).  Three row spaces:
  image stream  [n_img_rows]  item-major                 (residual stream `hidden_states`)
  text stream   [n_txt_rows]  item-major                 (residual stream `encoder_hidden_states`)
  joint         [n_joint_rows] per item [text_i ; image_i]  (q/k/v/attention; reference order, :412-416)
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch


@dataclass
class RaggedBatch:
    txt_lens: list[int]
    s_imgs: list[int]             # image rows of every item
    temb_rows: list[int]          # item -> row of the timestep-embedding table (items may share one)
    n_temb: int
    grids: tuple                  # per item: (frames, h/16, w/16) latent token grid, or a tuple of such triples (target +
                                  # condition images on one sequence axis)
    txt_pos_end: int              # rope table rows [0, txt_pos_end) are text positions
    img_start: int = 0            # first image token of the grid held by this batch (sequence-parallel chunk)
    cu_seqlens: np.ndarray = field(repr=False, default=None)
    img_item: np.ndarray = field(repr=False, default=None)
    txt_item: np.ndarray = field(repr=False, default=None)
    img_joint_row: np.ndarray = field(repr=False, default=None)
    txt_joint_row: np.ndarray = field(repr=False, default=None)
    joint_pos: np.ndarray = field(repr=False, default=None)

    @property
    def n_items(self) -> int:
        return len(self.txt_lens)

    @property
    def mixed(self) -> bool:
        """Do the items sit on more than one grid?"""
        return any(g != self.grids[0] for g in self.grids)

    @property
    def distinct_grids(self) -> tuple:
        """The grids of this batch in order of first appearance (the segment order of the RoPE table)."""
        return tuple(dict.fromkeys(self.grids))

    @property
    def n_txt_pos(self) -> int:
        """Text positions per distinct grid: the RoPE table holds one text segment of this length for each of them."""
        return self.txt_pos_end // len(self.distinct_grids)

    @property
    def s_img(self) -> int:
        """Image rows per item of a batch on ONE grid; a mixed batch has no such number (use `s_imgs`)."""
        if self.mixed:
            raise ValueError("items of this batch sit on different grids: there is no common s_img, use s_imgs")
        return self.s_imgs[0]

    @property
    def grid(self) -> tuple:
        """The grid of a batch on ONE grid; a mixed batch has no such grid (use `grids`)."""
        if self.mixed:
            raise ValueError("items of this batch sit on different grids: there is no common grid, use grids")
        return self.grids[0]

    @property
    def n_img_rows(self) -> int:
        return int(sum(self.s_imgs))

    @property
    def img_offsets(self) -> list[int]:
        """First image-stream row of every item, and the total behind the last."""
        offs = [0]
        for s in self.s_imgs:
            offs.append(offs[-1] + s)
        return offs

    @property
    def n_txt_rows(self) -> int:
        return int(sum(self.txt_lens))

    @property
    def n_joint_rows(self) -> int:
        return self.n_img_rows + self.n_txt_rows

    @property
    def max_seqlen(self) -> int:
        return max(t + s for t, s in zip(self.txt_lens, self.s_imgs))

    def device_maps(self, device) -> dict[str, torch.Tensor]:
        names = ("cu_seqlens", "img_item", "txt_item", "img_joint_row", "txt_joint_row", "joint_pos")
        return {n: torch.from_numpy(getattr(self, n)).to(device) for n in names}


def _per_item_grids(grid, n: int):
    """`grid` as a tuple of n normalised per-item grids.  A LIST with one entry per item is the per-item form; anything else
    (a triple, a tuple of triples: the Edit pipelines' multi-entry grid) is one grid that every item sits on."""
    from .models.qwen_image.rope import normalize_grids

    def one(g):
        g = normalize_grids(g)
        return g[0] if len(g) == 1 else g               # one image: the plain (f, h, w) triple; several: a tuple of triples

    if isinstance(grid, list) and grid and all(isinstance(g, (list, tuple)) for g in grid):
        if len(grid) != n:
            raise ValueError(f"{len(grid)} per-item grids for {n} items")
        return tuple(tuple(one(tuple(g))) for g in grid)
    return (tuple(one(grid)),) * n


def build_ragged_batch(txt_lens: list[int], grid, temb_rows: list[int] | None = None,
                       txt_pos_end: int | None = None, img_rows: tuple[int, int] | None = None) -> RaggedBatch:
    """Build the int32 row maps for items with text lengths `txt_lens`.  `grid`: one latent grid common to all items, or a
    LIST of grids, one per item (requests of different resolutions in one forward).
    `img_rows = (start, count)`: every item holds only that slice of the grid's image tokens (a sequence-parallel rank's
    chunk, reference qwen_image_transformer.py:735-738,772-781); RoPE positions stay those of the full grid.  One grid only.

    RoPE positions (`joint_pos`, rows of models/qwen_image/rope.py `rope_table_multi`): the table of a forward is laid out
    [text segment of distinct grid 0 | text segment of grid 1 | ... | image segment of grid 0 | image segment of grid 1 | ...],
    every text segment `n_txt` rows long (n_txt = the `txt_pos_end` argument, default the longest prompt), because the text
    positions of an item start behind ITS grid's half-extent.  The batch's `txt_pos_end` is the end of the last text segment,
    so "rows below txt_pos_end are text positions" holds for any number of grids; with one grid the layout is the
    single-grid table's."""
    if not txt_lens or any(t <= 0 for t in txt_lens):
        raise ValueError("every item needs at least one text token")
    from .models.qwen_image.rope import grid_tokens

    n = len(txt_lens)
    grids = _per_item_grids(grid, n)
    distinct = tuple(dict.fromkeys(grids))
    totals = [grid_tokens(g) for g in grids]
    if img_rows is None:
        img_start, s_imgs = 0, totals
    else:
        if len(distinct) != 1:
            raise ValueError("img_rows (a sequence-parallel chunk) needs one grid for all items")
        img_start, s_imgs = int(img_rows[0]), [int(img_rows[1])] * n
        if img_start < 0 or s_imgs[0] <= 0 or img_start + s_imgs[0] > totals[0]:
            raise ValueError("img_rows outside the token grid")
    temb_rows = list(range(n)) if temb_rows is None else list(temb_rows)
    if len(temb_rows) != n:
        raise ValueError("temb_rows must have one entry per item")
    tmax = max(txt_lens)
    n_txt = tmax if txt_pos_end is None else txt_pos_end
    if n_txt < tmax:
        raise ValueError("txt_pos_end smaller than the longest prompt")
    # table row of the first text / image position of every distinct grid
    seg = {g: k for k, g in enumerate(distinct)}
    txt_pos_end = n_txt * len(distinct)
    img_seg0, o = {}, txt_pos_end
    for g in distinct:
        img_seg0[g] = o
        o += grid_tokens(g)
    seq = np.asarray([t + s for t, s in zip(txt_lens, s_imgs)], dtype=np.int64)
    cu = np.zeros(n + 1, dtype=np.int32)
    cu[1:] = np.cumsum(seq)
    img_item = np.repeat(np.asarray(temb_rows, dtype=np.int32), s_imgs)
    txt_item = np.repeat(np.asarray(temb_rows, dtype=np.int32), txt_lens)
    img_joint = np.concatenate([cu[i] + txt_lens[i] + np.arange(s_imgs[i], dtype=np.int32) for i in range(n)])
    txt_joint = np.concatenate([cu[i] + np.arange(txt_lens[i], dtype=np.int32) for i in range(n)])
    joint_pos = np.empty(int(cu[-1]), dtype=np.int32)
    for i in range(n):
        joint_pos[cu[i]: cu[i] + txt_lens[i]] = seg[grids[i]] * n_txt + np.arange(txt_lens[i], dtype=np.int32)
        joint_pos[cu[i] + txt_lens[i]: cu[i + 1]] = img_seg0[grids[i]] + img_start + np.arange(s_imgs[i], dtype=np.int32)
    return RaggedBatch(txt_lens=list(txt_lens), s_imgs=list(s_imgs), temb_rows=temb_rows, n_temb=max(temb_rows) + 1,
                       grids=grids, txt_pos_end=txt_pos_end, img_start=img_start, cu_seqlens=cu,
                       img_item=img_item.astype(np.int32), txt_item=txt_item.astype(np.int32),
                       img_joint_row=img_joint.astype(np.int32), txt_joint_row=txt_joint.astype(np.int32),
                       joint_pos=joint_pos)


# ---- the step update of a group whose requests differ in target rows AND carry condition rows (Edit / Edit-Plus): host model
# of omni_cfg_euler_req (include/omni_cdna4.h).  Item order of the forward: pos_0..pos_{R-1}, neg_0..neg_{R-1}; item i holds
# [target rows of its request ; that request's condition rows].
CFG_EULER_RAGGED_MAX_REQS = 64
CFG_EULER_REQ_DTYPE = np.dtype([("lat_row", "<i4"), ("rows", "<i4"), ("pos_row", "<i4"), ("neg_row", "<i4"),
                                ("dst_row", "<i4", (2,)), ("dt_index", "<i4"), ("cfg_scale", "<f4")])


def ragged_step_descriptors(target_rows: list[int], cond_rows: list[int], do_cfg: bool, scales: list[float]) -> dict:
    """Row layout of one step of R requests, request r with target_rows[r] latent rows and cond_rows[r] condition rows:
      lat_off   [R + 1]        request r's rows of the latent state `lat`  (the state holds target rows only)
      item_off  [n_items + 1]  item i's rows of the forward's input `lat_in` and output `pred`: target rows, then condition rows
      reqs      [R] omni_cfg_euler_req records: where request r's predictions start in `pred` (the first target_rows[r] rows of
                its items), where its updated rows go in `lat_in` (the same rows: the next step's input), its dt entry r, its scale
      total_rows               sum of the target rows (sizes the kernel launch)."""
    R = len(target_rows)
    if not 0 < R <= CFG_EULER_RAGGED_MAX_REQS:
        raise ValueError(f"{R} requests: the ragged step update takes 1 .. {CFG_EULER_RAGGED_MAX_REQS}")
    if len(cond_rows) != R or len(scales) != R:
        raise ValueError("one condition row count and one scale per request")
    if any(int(s) < 1 for s in target_rows) or any(int(c) < 0 for c in cond_rows):
        raise ValueError("every request needs at least one target row (condition rows may be none)")
    lat_off = [0]
    for s in target_rows:
        lat_off.append(lat_off[-1] + int(s))
    item_off = [0]
    for _ in range(2 if do_cfg else 1):
        for s, c in zip(target_rows, cond_rows):
            item_off.append(item_off[-1] + int(s) + int(c))
    reqs = np.zeros(R, dtype=CFG_EULER_REQ_DTYPE)
    for r in range(R):
        neg = item_off[R + r] if do_cfg else -1
        reqs[r] = (lat_off[r], int(target_rows[r]), item_off[r], neg, (item_off[r], neg), r, float(scales[r]))
    return dict(lat_off=lat_off, item_off=item_off, reqs=reqs, total_rows=lat_off[-1])


# ---- the compact attention grid for items of unequal length: host model of csrc/common.h (omni_attn_compact_slots,
# omni_attn_slot_lookup).  The kernels do this on the device; these functions state the same rule for tests and tools.
ATTN_COMPACT_MAX_ITEMS = 64


def attention_compact_slots(seq_lens: list[int], qblk: int) -> int:
    """Slots per head of the compact grid, or 0 when the launch keeps the legacy grid of len(seq_lens) * ceil(max / qblk)
    workgroups per head.  The bound sum // qblk + B needs only integers the host has (n_joint_rows, n_items, max_seqlen); it
    covers sum_i ceil(len_i / qblk) because every ceil adds less than one, and for equal lengths it is never below the legacy
    grid, so such launches never change."""
    B = len(seq_lens)
    if B > ATTN_COMPACT_MAX_ITEMS or sum(seq_lens) <= 0:
        return 0
    slots = sum(seq_lens) // qblk + B
    legacy = B * -(-max(seq_lens) // qblk)
    return slots if slots < legacy else 0


def attention_slot_lookup(cu_seqlens, qblk: int, slot: int):
    """slot -> (item, q-block) by the walk over cu_seqlens the kernels do; None for a slot behind the last real block."""
    for i in range(len(cu_seqlens) - 1):
        nb = -(-(int(cu_seqlens[i + 1]) - int(cu_seqlens[i])) // qblk)
        if slot < nb:
            return i, slot
        slot -= nb
    return None
