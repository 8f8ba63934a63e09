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

Deviation from the reference: when a picked mask is empty -- or has no pixel left after the resize to the model's input size -- the memory is NOT
replaced (`empty_updates` counts these).  The reference replaces it and then fails in `torch.randint(0, 0, ...)` on the next frame.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from .model import PSALM, default_region_index_sampler  # noqa: F401  (the sampler lives next to its point-sampler twin; re-exported here)
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
    """See the module docstring.  State: `_mem` (None or the last accepted frame, ~ n_img * hidden * 4 + R * S * S bytes on the device), the clip
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
        """Forget the memory: the next step is prompted by the caller's visual prompt (a new clip)."""
        self._mem: Optional[_Memory] = None
        self._video = None

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
        return {"picked_masks": picked, "fused": fused,
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
