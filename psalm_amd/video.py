"""Video object tracking: the reference's DAVIS loop with memory (psalm/eval/eval_davis.py:388-480, `--with_memory`) as a stateful object.

    trk = VideoTracker(model)                     # a region-task PSALM, precision "f16x3" or "fp32"
    for inputs in clip:                           # what eval_davis.py:421-428 hands eval_video, batch 1
        out = trk.step(input_ids=..., attention_mask=..., images=..., vp_images=..., seg_info=..., labels=...)
        out["fused"]                              # (H, W) uint8 DAVIS label map of this frame

Per frame the reference feeds the last accepted frame and the masks predicted on it back as the visual prompt, calls eval_video, picks one query
per object, checks the picks pairwise for IoU > 0.4, paints the label map and replaces the memory if the check passed.  Written against
`PSALM.eval_video` that loop runs Swin + projector twice per frame (the second pass recomputes what the previous step computed), pulls all Q
full-resolution masks to the host, and pushes the resized prompt masks back only for `nonzero()` to run on the host again.  Here the state stays
on the device:

  * the memory frame's projector tokens are kept (copied out of the step that computed them): a memory-path step runs ONE vision pass;
  * pick, label map, pair counts and the memory flag are kernels (psalm_video_pick / psalm_video_fuse);
  * the picked masks are resized with the frame's own transforms right away (psalm_mask_resize_nearest_pad = `apply_segmentation`), so the next
    step finds its prompt masks, their per-row pixel counts and their pixel totals ready;
  * the region points are selected on the device (psalm_mask_select_points) from R * n integer ranks: the reference's point sampler reads only
    `nonzero.shape[0]`, so the host needs the R totals, not the masks.

ONE read-back per step: a block of 1 + 4 R + 2 R^2 32-bit words (flag, pixel counts of the picked and of the resized masks, picks, scores, pair
counts).  No full-resolution mask crosses the bus unless the caller reads `out`.  Launches are eager (no hipGraph), batch 1.

Without a dataset record (no `instances`, no `vp_images`, no ground truth) a track begins with `start` -- click, box, scribble or mask prompts on
frame 0 in the grammar of `PSALM.segment(regions=)`, drawn and sampled on the device -- or with `adopt` (masks on an encoded ImageSession), and goes
on with `track(images, seg_info)`.  The tracker keeps that ORIGIN prompt the way it keeps the memory (frame 0's projector tokens + the resized prompt
masks), so a frame prompted from it while the memory is empty runs one vision pass too and reads no mask on the host.

Deviation from the reference: when a picked mask is empty -- or has no pixel left after the resize to the model's input size -- the memory is NOT
replaced (`empty_updates` counts these).  The reference replaces it and then fails in `torch.randint(0, 0, ...)` on the next frame.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from .model import PSALM
from .session import ImageSession, default_region_index_sampler  # noqa: F401  (the sampler lives next to its point-sampler twin; re-exported here)
from .config import REGION_TOKEN_INDEX
from .preprocess import nearest_pad_tables

MAX_OBJECTS = 32          # one bit per object in psalm_video_fuse's per-pixel set
TOPK = 10                 # eval_davis.py:446


class _Memory:
    """What the tracker keeps of the last accepted frame: its projector tokens, the picked masks ALREADY resized and padded with that frame's
    transforms (R, S, S) uint8 + per-row pixel counts (R, S), the pixel totals (host ints) and the fill numbers."""
    __slots__ = ("tokens", "masks", "row_cnt", "counts", "fill")

    def __init__(self, tokens, masks, row_cnt, counts, fill):
        self.tokens, self.masks, self.row_cnt, self.counts, self.fill = tokens, masks, row_cnt, counts, fill


class VideoTracker:
    """See the module docstring.  State: `_mem` (None or the last accepted frame, ~ n_img * hidden * 4 + R * S * S bytes on the device), `_origin`
    (None or the prompt `start` / `adopt` was given, in the same form) with the tracking prompt's ids, the clip
    name, small cached device tables (resize index tables per geometry, fill numbers), and the counters
        memory_frames      steps prompted from memory
        prompt_frames      steps prompted from the caller's vp_images / vp_region_masks
        rejected_updates   steps whose picks failed the IoU check (memory kept)
        empty_updates      steps whose memory update was skipped because a picked mask was empty (the deviation above)."""

    def __init__(self, model: PSALM):
        if model.seg_task != "region":
            raise ValueError(f"VideoTracker needs a region-task model (seg_task = {model.seg_task!r})")
        if model.precision not in ("f16x3", "fp32") or model.llm_products != 3:
            raise NotImplementedError("VideoTracker: precision 'f16x3' (llm_products = 3) or 'fp32'")
        if model.cfg.md_queries < TOPK:
            raise ValueError(f"VideoTracker: the pick reads each object's {TOPK} best of Q scores, Q = {model.cfg.md_queries}")
        self.model, self.ops = model, model.ops
        self._tabs = {}
        self._fills = {}
        self.reset()
        self.memory_frames = self.prompt_frames = self.rejected_updates = self.empty_updates = 0

    def reset(self):
        """Forget the memory: the next step is prompted by the caller's visual prompt (a new clip).  The origin prompt of `start` / `adopt` goes
        with it: `track` needs a new one."""
        self._mem: Optional[_Memory] = None
        self._video = None
        self._origin: Optional[_Memory] = None
        self._prompt = None                                 # (input_ids, attention_mask, canvas (H, W)) of the track begun by start / adopt

    # ------------------------------------------------------------------ small cached device tables
    def _tables(self, transforms):
        h, w, nh, nw = [int(v) for v in transforms["resize"]]
        ph, pw = [int(v) for v in transforms["pad"]]
        key = (h, w, nh, nw, ph, pw)
        t = self._tabs.get(key)
        if t is None:
            if len(self._tabs) >= 16:
                self._tabs.clear()
            rows, cols = nearest_pad_tables(*key)
            t = self._tabs[key] = (torch.from_numpy(rows).to(self.ops.device), torch.from_numpy(cols).to(self.ops.device))
        return t

    def _fill_dev(self, fill):
        key = tuple(fill)
        t = self._fills.get(key)
        if t is None:
            if len(self._fills) >= 64:
                self._fills.clear()
            t = self._fills[key] = torch.tensor(key, dtype=torch.int32).to(self.ops.device)
        return t

    @staticmethod
    def _fill_list(v) -> List[int]:
        fill = [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
        if len(fill) > MAX_OBJECTS:
            raise ValueError(f"VideoTracker: {len(fill)} objects, at most {MAX_OBJECTS}")
        if len(fill) == 0:
            raise ValueError("VideoTracker: no object (empty vp_fill_number)")
        if any(x < 0 or x > 255 for x in fill):
            raise ValueError(f"VideoTracker: fill numbers {fill} outside 0..255 (the fused label map is uint8)")
        return fill

    # ------------------------------------------------------------------ pick, IoU check, fuse, memory update (eval_davis.py:433-480)
    def _observe(self, tokens, pred_masks, scores, fill, transforms):
        """The frame's bookkeeping.  tokens (n_img, hidden) fp32: the frame's projector tokens; pred_masks (Q, H, W) fp32 of 0 / 1 and scores (Q, R):
        `instances.pred_masks` / `.scores` of the frame; fill: R fill numbers; transforms: the frame's resize / pad record.  Returns the extra
        keys of `step` (without `used_memory`) and replaces the memory when the picks pass."""
        o = self.ops
        fill = self._fill_list(fill)
        R = len(fill)
        if scores.dim() != 2 or scores.shape[1] != R:
            raise ValueError(f"VideoTracker: scores of shape {tuple(scores.shape)} for {R} objects")      # eval_davis.py:438
        Q = int(scores.shape[0])
        if Q < TOPK:
            raise ValueError(f"VideoTracker: the pick reads each object's {TOPK} best of Q scores, Q = {Q}")
        if pred_masks.shape[0] != Q:
            raise ValueError("VideoTracker: one mask per query")
        Hh, Ww = int(pred_masks.shape[1]), int(pred_masks.shape[2])
        if tuple(int(v) for v in transforms["resize"][:2]) != (Hh, Ww):
            raise ValueError(f"VideoTracker: masks of {(Hh, Ww)} for transforms of an image of {tuple(transforms['resize'][:2])}")
        row_tab, col_tab = self._tables(transforms)
        # the step's ONE read-back: [flag | nonzero (R) | resized nonzero (R) | pick_query (R) | pick_score (R, fp32 bits) | inter (R,R) | union (R,R)]
        blk = o.zeros(1 + 4 * R + 2 * R * R, dtype=torch.int32)
        v_flag, v_nz, v_rnz, v_q = blk[0:1], blk[1:1 + R], blk[1 + R:1 + 2 * R], blk[1 + 2 * R:1 + 3 * R]
        v_s = blk[1 + 3 * R:1 + 4 * R].view(torch.float32)
        v_in = blk[1 + 4 * R:1 + 4 * R + R * R].view(R, R)
        v_un = blk[1 + 4 * R + R * R:].view(R, R)
        o.video_pick(scores.contiguous(), v_q, v_s)
        picked, fused, _, _, _, _ = o.video_fuse(pred_masks.contiguous(), v_q, self._fill_dev(fill), v_in, v_un, v_nz, v_flag)
        masks, row_cnt = o.mask_resize_nearest_pad(picked, row_tab, col_tab, total=v_rnz)
        keep = o.empty(*tokens.shape, dtype=tokens.dtype)
        o.copy_(keep, tokens)
        host = blk.cpu().numpy()
        ok = bool(host[0] == 1)
        nz, rnz = host[1:1 + R], host[1 + R:1 + 2 * R]
        updated = False
        if not ok:
            self.rejected_updates += 1                      # "memory is wrong, using origin visual prompt" (eval_davis.py:479-480)
        elif (nz == 0).any() or (rnz == 0).any():
            self.empty_updates += 1
        else:
            self._mem = _Memory(keep, masks, row_cnt, [int(x) for x in rnz], fill)
            updated = True
        extra = {}
        if getattr(self.model, "mask_boxes", False):        # where each object is: (x0, y0, x1, y1) of its picked mask, zeros when it is empty
            extra["boxes"] = o.mask_boxes(picked)[0]        # (the areas are the `nonzero` counts the read-back has brought already)
        return {**extra, "picked_masks": picked, "fused": fused,
                "picked_query": torch.from_numpy(host[1 + 2 * R:1 + 3 * R].astype(np.int64)),
                "picked_scores": torch.from_numpy(host[1 + 3 * R:1 + 4 * R].copy().view(np.float32)),
                "pair_inter": torch.from_numpy(host[1 + 4 * R:1 + 4 * R + R * R].reshape(R, R).copy()),
                "pair_union": torch.from_numpy(host[1 + 4 * R + R * R:].reshape(R, R).copy()),
                "memory_updated": updated}

    # ------------------------------------------------------------------ one frame
    @torch.no_grad()
    def step(self, input_ids=None, attention_mask=None, images=None, vp_images=None, seg_info=None, labels=None,
             region_index_sampler: Callable = default_region_index_sampler):
        """One frame (batch 1), with the arguments eval_davis.py:421-428 passes to eval_video: `seg_info[0]["instances"]` carries `vp_region_masks`
        (prompt masks on `vp_images`), `vp_fill_number` and `gt_masks`; `seg_info[0]["transforms"]` the frame's resize / pad record
        (ImagePreprocessor).  The tracker resets itself when the parent directory of `seg_info[0]["file_name"]` changes (eval_davis.py:390-398).

        Returns what `eval_video` returns for the frame (`instances`, `gt`, `mask_pred`) plus
            picked_masks (R,H,W) uint8, fused (H,W) uint8            on the device, private copies
            boxes (R,4) float32                                      on the device, only with the model's `mask_boxes` switch on: (x0, y0, x1, y1)
                                                                     of each picked mask, zeros for an empty one
            picked_query (R) int64, picked_scores (R) float32,
            pair_inter / pair_union (R,R) int32                      on the host (they arrive with the step's one read-back)
            used_memory, memory_updated                              bools.
        Memory path (memory non-empty and as many objects as the memory has, eval_davis.py:401-415): the <region> features are pooled from the memory
        frame's projector tokens at points drawn on the memory masks after `apply_segmentation`; the fill numbers are the memory's.  Otherwise the
        caller's `vp_images` / `vp_region_masks` are used as eval_video uses them (:417-419).  `region_index_sampler(m, n)`: n ranks into the m
        non-zero pixels of a prompt mask (default: the reference's sampler on the global torch RNG).
        Deviation from the reference: an empty picked mask (before or after the resize to the input size) leaves the memory unchanged."""
        m, o = self.model, self.ops
        if images is None or images.dim() != 4 or images.shape[0] != 1 or seg_info is None or len(seg_info) != 1:
            raise ValueError("VideoTracker.step: one frame per call (batch 1)")
        info = seg_info[0]
        inst = info["instances"]
        name = info.get("file_name")
        video = str(name).split("/")[-2] if name is not None and "/" in str(name) else None      # eval_davis.py:390
        if name is not None and video != self._video:
            if self._video is not None:                     # (no clip seen yet: nothing to forget)
                self.reset()
            self._video = video
        fill = self._fill_list(inst.vp_fill_number)
        mem = self._mem
        use_memory = mem is not None and len(fill) == len(mem.fill)
        images = images.to(m.device, torch.float32).contiguous()
        stages: dict = {}
        if use_memory:
            fill = mem.fill                                                      # eval_davis.py:414
            R, n = len(fill), m.cfg.region_points
            idx = torch.stack([region_index_sampler(c, n) for c in mem.counts]).to(torch.int32)
            blob, layout, meta = m._prepare(input_ids, attention_mask, images, seg_info, None, None, None, None, None, None, video=True,
                                            region_counts=[R], extra_arrays={"region_idx": idx.numpy()})
            dv = m._views(torch.from_numpy(blob).to(m.device), layout)
            pts = o.mask_select_points(mem.masks, mem.row_cnt, dv["region_idx"].view(R, n))
            results = m._forward_device(images, dv, meta, stages=stages, vp_tokens=mem.tokens, region_pts=pts)
            self.memory_frames += 1
        else:
            if vp_images is None:
                raise ValueError("VideoTracker.step: vp_images is needed while the memory is empty")
            vp = vp_images.to(m.device, torch.float32).contiguous()
            blob, layout, meta = m._prepare(input_ids, attention_mask, images, seg_info, None, None, None, None, None,
                                            lambda nz, k: region_index_sampler(nz.shape[0], k), video=True)
            dv = m._views(torch.from_numpy(blob).to(m.device), layout)
            results = m._forward_device(images, dv, meta, stages=stages, vp_images=vp)
            self.prompt_frames += 1
        out = m._finalize(results[0], info)
        res = out["instances"]
        out.update(self._observe(stages["image_tokens"], res.pred_masks, res.scores, fill, info["transforms"]))
        out["used_memory"] = use_memory
        return out

    # ------------------------------------------------------------------ tracks that begin with a prompt instead of a dataset record
    def _track_prompt(self, who, input_ids, attention_mask, R):
        """the tracking prompt (1, T) with R <region> tokens"""
        if not torch.is_tensor(input_ids) or input_ids.dim() not in (1, 2) or (input_ids.dim() == 2 and input_ids.shape[0] != 1):
            raise ValueError(f"VideoTracker.{who}: one prompt, input_ids (1, T) (batch 1)")
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
            attention_mask = attention_mask[None] if attention_mask is not None and attention_mask.dim() == 1 else attention_mask
        n_tok = int((input_ids == REGION_TOKEN_INDEX).sum())
        if n_tok != R:
            raise ValueError(f"VideoTracker.{who}: {R} regions for {n_tok} <region> tokens in input_ids")
        return input_ids, attention_mask

    def _fill_for(self, who, fill, R):
        fill = self._fill_list(list(range(1, R + 1)) if fill is None else fill)
        if len(fill) != R:
            raise ValueError(f"VideoTracker.{who}: {len(fill)} fill numbers for {R} regions")
        return fill

    @staticmethod
    def _frame_info(who, images, seg_info):
        if images is None or images.dim() != 4 or images.shape[0] != 1 or seg_info is None or len(seg_info) != 1:
            raise ValueError(f"VideoTracker.{who}: one frame per call (batch 1)")
        info = seg_info[0]
        if not isinstance(info, dict) or info.get("transforms") is None:
            raise ValueError(f"VideoTracker.{who}: seg_info[0]['transforms'] (the frame's resize / pad record) is needed")
        return info

    @torch.no_grad()
    def start(self, input_ids, images, seg_info, regions, attention_mask=None, fill=None,
              region_index_sampler: Callable = default_region_index_sampler):
        """Frame 0 of a track (batch 1), prompted by GEOMETRY on the frame itself: `regions` is the flat list of R region prompts of the one prompt
        `input_ids` ((1, T) with R <region> tokens), in the grammar of `PSALM.segment(regions=)` -- {"points"} / {"scribble"} (+ "radius"),
        {"box"}, {"mask"}, {"rle"} in integer pixels of the ORIGINAL frame, the (h, w) of `seg_info[0]["transforms"]["resize"]`.  `fill`: R fill
        numbers in 0..255, default 1..R.  `seg_info[0]` needs no `instances`.

        The prompt is drawn, dilated and resized + padded with the frame's tables on the device (one launch each), ONE read-back brings the R pixel
        totals, `region_index_sampler(m, n)` is called per region in order, and the <region> features pool from the frame's own projector tokens:
        one Swin + projector pass.  The result equals, bit for bit, `step` on a fresh tracker with `vp_images = images`,
        `vp_region_masks = apply_segmentation(mask, transforms)` of the same prompts and `vp_fill_number = fill`; it has the keys of `step`
        without `gt`.  The tracker keeps the prompt (frame 0's tokens, the resized masks, their counts, `fill`) as the ORIGIN of the track next to
        the memory, and `input_ids` / `attention_mask` for `track`.  Calling `start` again (a re-prompt on a later frame) replaces origin and memory
        and resets no counter; a call that raises leaves the tracker as it was."""
        m, o = self.model, self.ops
        info = self._frame_info("start", images, seg_info)
        if not isinstance(regions, (list, tuple)):
            raise ValueError("VideoTracker.start: regions is a list with one region prompt per <region> token")
        R = len(regions)
        input_ids, attention_mask = self._track_prompt("start", input_ids, attention_mask, R)
        fill = self._fill_for("start", fill, R)
        tr = info["transforms"]
        images = images.to(m.device, torch.float32).contiguous()
        canvas = (int(images.shape[2]), int(images.shape[3]))
        try:
            rp = m._region_prompt_plan(None, input_ids, [info], [list(regions)], transforms=tr, canvas=canvas)
        except ValueError as e:
            raise ValueError(f"VideoTracker.start: {e}") from None
        extra = {k: v for k, v in rp["arrays"].items() if k != "region_img"}                  # (_prepare writes the image index itself)
        blob, layout, meta = m._prepare(input_ids, attention_mask, images, [info], None, None, None, None, None, None, video=True,
                                        region_counts=[R], extra_arrays=extra)
        dv = m._views(torch.from_numpy(blob).to(m.device), layout)
        total = o.zeros(R, dtype=torch.int32)
        masks, row_cnt = m._region_prompt_masks(None, rp, dv, total, tables=self._tables(tr))
        counts = total.cpu().tolist()                                                         # the ONE read-back in front of the model pass
        try:
            idx = m._region_prompt_ranks(rp, counts, region_index_sampler)
        except ValueError as e:
            raise ValueError(f"VideoTracker.start: {e}") from None
        pts = o.mask_select_points(masks, row_cnt, idx.to(m.device))
        stages: dict = {}
        results = m._forward_device(images, dv, meta, stages=stages, region_pts=pts)          # (<region> features from the frame's OWN tokens)
        out = m._finalize(results[0], info, gt_optional=True)
        out.pop("gt", None)
        res = out["instances"]
        tokens = stages["image_tokens"]
        keep = o.empty(*tokens.shape, dtype=tokens.dtype)
        o.copy_(keep, tokens)
        self._origin = _Memory(keep, masks, row_cnt, [int(c) for c in counts], fill)
        self._prompt = (input_ids, attention_mask, canvas)
        self._mem = None
        self.prompt_frames += 1
        out.update(self._observe(tokens, res.pred_masks, res.scores, fill, tr))
        out["used_memory"] = False
        return out

    @torch.no_grad()
    def track(self, images, seg_info, region_index_sampler: Callable = default_region_index_sampler):
        """The next frame (batch 1) of the track begun by `start` / `adopt`: `seg_info[0]` carries the frame's geometry (`transforms`, `height` /
        `width`, `padding_mask`) and needs no `instances`; no `vp_images`.  With a non-empty memory this is the memory path of `step`; while the
        memory is empty (the picks of the start frame were rejected or came out empty) the frame is prompted from the kept origin through the
        same code -- its tokens as `vp_tokens`, points selected on its masks on the device -- and counts as a prompt frame.  One vision pass either
        way; `region_index_sampler(m, n)` is drawn per region, in order.  Returns the keys of `step` without `gt`.  `file_name` is not read: a
        new clip begins with `start` or `reset()`."""
        m, o = self.model, self.ops
        if self._origin is None:
            raise ValueError("VideoTracker.track: no track to go on with (call start or adopt first)")
        info = self._frame_info("track", images, seg_info)
        input_ids, attention_mask, canvas = self._prompt
        if (int(images.shape[2]), int(images.shape[3])) != canvas:
            raise ValueError(f"VideoTracker.track: a frame of {tuple(images.shape[2:])}, the track began on {canvas} (the kept tokens are of that size)")
        mem = self._mem
        use_memory = mem is not None and len(mem.fill) == len(self._origin.fill)
        src = mem if use_memory else self._origin
        fill = src.fill
        images = images.to(m.device, torch.float32).contiguous()
        R, n = len(fill), m.cfg.region_points
        idx = torch.stack([region_index_sampler(c, n) for c in src.counts]).to(torch.int32)
        blob, layout, meta = m._prepare(input_ids, attention_mask, images, [info], None, None, None, None, None, None, video=True,
                                        region_counts=[R], extra_arrays={"region_idx": idx.numpy()})
        dv = m._views(torch.from_numpy(blob).to(m.device), layout)
        pts = o.mask_select_points(src.masks, src.row_cnt, dv["region_idx"].view(R, n))
        stages: dict = {}
        results = m._forward_device(images, dv, meta, stages=stages, vp_tokens=src.tokens, region_pts=pts)
        if use_memory:
            self.memory_frames += 1
        else:
            self.prompt_frames += 1
        out = m._finalize(results[0], info, gt_optional=True)
        out.pop("gt", None)
        res = out["instances"]
        out.update(self._observe(stages["image_tokens"], res.pred_masks, res.scores, fill, info["transforms"]))
        out["used_memory"] = use_memory
        return out

    @torch.no_grad()
    def adopt(self, session, masks, input_ids, attention_mask=None, fill=None):
        """Go on from an image session's result: `session` is an ImageSession of this model (and weights version) whose `seg_info` has `transforms`,
        `masks` (R, h, w) uint8 / bool on the device or the host at the session's ORIGINAL size -- `out["picked_masks"]` of
        `segment(session, ids, regions=..., pick=True)`, or any masks of that size (non-zero = set; the bytes are kept as they are).  They are resized
        with the session's tables (psalm_mask_resize_nearest_pad; one read-back of the R totals), `session.image_tokens` are copied, and the result
        becomes both memory and origin of the track: the next `track` is a memory step, equal to `step` with the session's image as `vp_images`
        and `apply_segmentation(mask, transforms)` as `vp_region_masks`.  `input_ids` (1, T): the tracking prompt with R <region> tokens; `fill`
        as in `start`.  Runs no model pass and changes no counter; a call that raises leaves the tracker as it was."""
        m, o = self.model, self.ops
        if not isinstance(session, ImageSession) or session.model is not m:
            raise ValueError("VideoTracker.adopt: this session was made by another model (or replica)")
        if session.version != m._weights_version:
            raise ValueError("VideoTracker.adopt: the model's weights were prepared again after this session was made; encode the image again")
        tr = session.seg_info.get("transforms") if isinstance(session.seg_info, dict) else None
        if tr is None:
            raise ValueError("VideoTracker.adopt: the session's seg_info['transforms'] (the resize / pad record of its image) is needed")
        h, w, nh, nw = [int(v) for v in tr["resize"]]
        canvas = (int(session.images.shape[2]), int(session.images.shape[3]))
        if (nh + int(tr["pad"][0]), nw + int(tr["pad"][1])) != canvas:
            raise ValueError(f"VideoTracker.adopt: the session's transforms lead to {(nh + int(tr['pad'][0]), nw + int(tr['pad'][1]))}, "
                             f"its image is {canvas}")
        if not torch.is_tensor(masks):
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (h, w):
            raise ValueError(f"VideoTracker.adopt: masks of shape {tuple(masks.shape)} for an image of {(h, w)} (R, h, w)")
        if masks.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"VideoTracker.adopt: masks of dtype {masks.dtype} (uint8 or bool)")
        R = int(masks.shape[0])
        input_ids, attention_mask = self._track_prompt("adopt", input_ids, attention_mask, R)
        fill = self._fill_for("adopt", fill, R)
        masks = masks.to(m.device).contiguous()
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else masks
        row_tab, col_tab = self._tables(tr)
        total = o.zeros(R, dtype=torch.int32)
        small, row_cnt = o.mask_resize_nearest_pad(masks, row_tab, col_tab, total=total)
        keep = o.empty(*session.image_tokens.shape, dtype=session.image_tokens.dtype)
        o.copy_(keep, session.image_tokens)
        counts = [int(c) for c in total.cpu().tolist()]
        for r, c in enumerate(counts):
            if c <= 0:
                raise ValueError(f"VideoTracker.adopt: region {r}: no pixel of the mask is left after the resize to the model's input size")
        self._origin = self._mem = _Memory(keep, small, row_cnt, counts, fill)
        self._prompt = (input_ids, attention_mask, canvas)
