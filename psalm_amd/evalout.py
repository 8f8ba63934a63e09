"""Evaluator-facing outputs computed on the device.

The reference's evaluators start every image with `.cpu().numpy()` of the model's full-resolution outputs -- `sem_seg` (133,H,W) fp32 =
558 MB and `instances.pred_masks` (100,H,W) fp32 = 419 MB at 1024^2 -- and then reduce them on the host to a label map, a confusion
matrix, a PNG, run-length codes or a few intersection / union counts.  These functions produce those SMALL results on the GPU (kernels in
csrc/evalout.hip) in exactly the evaluators' arithmetic, so only KBs..MBs cross PCIe and the metric meters can be combined across ranks
with one tiny RCCL all-reduce (`psalm_amd.dist.reduce_metrics`, the role of AverageMeter.all_reduce, referring_segmentation.py:58-79).

    semantic_labels(sem_seg)                      panoptic_evaluation.py:125        -> (H,W) int32 labels
    ConfusionMatrix(C, ignore).update(pred, gt)   panoptic_evaluation.py:127-134    -> (C+1,C+1) int64 on the device
    panoptic_png_rgb(panoptic_ids)                panoptic_evaluation.py:204 (id2rgb) -> (H,W,3) uint8, ready for the PNG encoder
    masks_to_rle(pred_masks)                      region_segmentation.py:282 (pycocotools mask.encode) -> [{"size": [h,w], "counts": bytes}]
    iou_counts(pred_masks, gt_masks, pairs)       referring_segmentation.py:101-113 (intersectionAndUnionGPU, K=2) -> intersection, union
    fuse_masks_by_score(pred_masks, scores, thr)  eval_grefcoco.py:113-131,277-285 (gRefCOCO: union of the candidates above thr, else top-1)
    IoUMeters                                     referring_segmentation.py:139-177 + :58-79 (cIoU / gIoU bookkeeping + all-reduce)
    mask_boxes(masks) / label_boxes(labels, n)    llava_phi.py:319,395,438-440 (the commented-out `BitMasks(..).get_bounding_boxes()`) -> boxes, areas
    mask_pair_counts(masks_a, masks_b)            COCO mask matching / DAVIS J: the prediction x ground-truth overlap matrix on bit planes
    mask_nms(masks, scores, iou_thr)              greedy mask NMS under an exact rational IoU threshold (PSALM.segment_everything's rule)
    mask_components(masks, connectivity)          a mask's connected parts as instances: labels in scipy.ndimage.label's numbering, count, box / area table
    clean_masks(masks, min_island, max_hole)      SAM-style post-processing: fill holes up to N pixels, then drop islands below N pixels
    mask_outlines(masks, connectivity)            a mask's boundary as closed rings of lattice corners (COCO polygons as they stand), holes as rings
    outline_polygons(out, holes)                  mask_outlines' tables on the host: per mask a list of flat [x0, y0, x1, y1, ...] lists
    fill_polygons(rings, vertices, shape)         the way back: integer polygons -> masks, even-odd over pixel centres (fills an outline to its mask)
    mask_distance(masks, to, border)              exact squared Euclidean distance maps (scipy distance_transform_edt squared) of masks on the device
    mask_centers(masks)                           a click from a mask: the set pixel deepest inside, [y, x, dist2] per mask
    mask_boundaries(masks)                        DAVIS seg2bmap at the mask's own size
    boundary_counts(pred, gt, pairs, bound)       DAVIS f_measure's integers per pair; boundary_f(counts) -> precision, recall, F; davis_bound(shape)
    JFMeters                                      DAVIS J&F bookkeeping beside IoUMeters (J from iou_counts, F from boundary_counts) + all-reduce
    label_pair_counts(gt, gt_ids, pred, pred_ids) panopticapi pq_compute_single_core's np.unique(gt * 256^3 + pred): the overlap table of two id maps
    PanopticQuality(categories).update(...)       panoptic_evaluation.py:179-221 + panopticapi pq_compute: PQ / SQ / RQ without the PNG round trip
    coco_instance_records(instances, image_id)    detectron2 instances_to_coco_json (instance_evaluation.py) -> the COCO result records
"""
from __future__ import annotations

import math
from ctypes import c_long
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip_ops as H


def _ops(ops):
    return ops if ops is not None else H.get_ops()


def _on_device(o, t: torch.Tensor, dtypes, what: str) -> torch.Tensor:
    """The kernels read raw pointers: a tensor of another dtype would be misread (or read out of bounds), a host tensor -- the reference's
    evaluators habitually hold `.cpu()` copies -- would hand the GPU a host address.  Reject the former, move the latter."""
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        raise H.PsalmHipError(f"{what}: dtype {getattr(t, 'dtype', type(t))} not supported (expected one of {', '.join(str(d) for d in dtypes)})")
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t.to(o.device).contiguous()


def semantic_labels(sem_seg: torch.Tensor, ops=None) -> torch.Tensor:
    """`sem_seg.argmax(dim=0)` for a (C,H,W) float32 class map -> (H,W) int32 (first maximal class on ties, as torch)."""
    o = _ops(ops)
    if sem_seg.dim() != 3:
        raise H.PsalmHipError("semantic_labels: (C,H,W) class map")
    sem_seg = _on_device(o, sem_seg, (torch.float32,), "semantic_labels")
    C, Hh, Ww = sem_seg.shape
    out = o.empty(Hh, Ww, dtype=torch.int32)
    o._check(o.lib.psalm_semantic_labels(o._p(sem_seg), o._p(out), C, c_long(Hh * Ww), o._stream()), "psalm_semantic_labels")
    return out


class ConfusionMatrix:
    """my_SemSegEvaluator's `_conf_matrix` (panoptic_evaluation.py:127-134) kept on the device: rows = prediction, columns = ground truth,
    last row / column = the ignore bucket.  `update` takes int32 label maps (the prediction from `semantic_labels`)."""

    def __init__(self, num_classes: int, ignore_label: int = 255, ops=None):
        self.ops = _ops(ops)
        self.num_classes, self.ignore_label = num_classes, ignore_label
        self.conf = torch.zeros(num_classes + 1, num_classes + 1, dtype=torch.int64, device=self.ops.device)

    def update(self, pred: torch.Tensor, gt: torch.Tensor) -> None:
        o = self.ops
        gt = gt.to(o.device, torch.int32).contiguous()
        if pred.shape != gt.shape or pred.dtype != torch.int32:
            raise H.PsalmHipError("ConfusionMatrix.update: int32 label maps of equal shape")
        pred = pred.to(o.device).contiguous()
        o._check(o.lib.psalm_confusion_accumulate(o._p(pred), o._p(gt), c_long(pred.numel()), self.num_classes, self.ignore_label,
                                                  o._p(self.conf), o._stream()), "psalm_confusion_accumulate")

    def miou(self) -> Tuple[np.ndarray, float]:
        """Per-class IoU and mIoU as my_SemSegEvaluator.evaluate derives them from the matrix (detectron2 SemSegEvaluator.evaluate)."""
        conf = self.conf.cpu().numpy().astype(np.float64)
        tp = conf.diagonal()[:-1]
        pos_gt = conf[:-1, :-1].sum(0)
        pos_pred = conf[:-1, :-1].sum(1)
        union = pos_gt + pos_pred - tp
        valid = pos_gt > 0
        iou = np.where(union > 0, tp / np.maximum(union, 1), np.nan)
        return iou, float(np.nansum(iou[valid]) / max(valid.sum(), 1))


def panoptic_png_rgb(panoptic_ids: torch.Tensor, ops=None) -> torch.Tensor:
    """panopticapi `id2rgb`: id -> (id % 256, id // 256 % 256, id // 65536 % 256); (H,W) int32 -> (H,W,3) uint8 on the device."""
    o = _ops(ops)
    Hh, Ww = panoptic_ids.shape
    out = o.empty(Hh, Ww, 3, dtype=torch.uint8)
    o._check(o.lib.psalm_panoptic_rgb(o._p(panoptic_ids.to(o.device, torch.int32).contiguous()), o._p(out), c_long(Hh * Ww), o._stream()), "psalm_panoptic_rgb")
    return out


def rle_counts_to_string(counts: Sequence[int]) -> bytes:
    """pycocotools maskApi.c rleToString: LEB128-like, 5 data bits + continuation bit per char, chars 48..111, counts after the third
    stored as differences to the count two positions earlier."""
    out = bytearray()
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(ch + 48)
    return bytes(out)


def masks_to_rle(masks: torch.Tensor, ops=None) -> List[dict]:
    """Binary masks (n,H,W) float32 | uint8 (nonzero = foreground) -> COCO RLE dicts, == `mask.encode(np.asfortranarray(m))` of pycocotools.
    The device finds the run boundaries (column-major); only those (4 bytes per run) are copied to the host."""
    o = _ops(ops)
    if masks.dim() != 3:
        raise H.PsalmHipError("masks_to_rle: (n,H,W) float32 / uint8 / bool masks")
    masks = _on_device(o, masks, (torch.float32, torch.uint8, torch.bool), "masks_to_rle")
    n, Hh, Ww = masks.shape
    if n == 0:
        return []
    u8 = 1 if masks.dtype == torch.uint8 else 0
    col_cnt = o.empty(n, Ww, dtype=torch.int32)
    col_off = o.empty(n, Ww, dtype=torch.int32)
    total = o.empty(n, dtype=torch.int32)
    o._check(o.lib.psalm_mask_rle_count(o._p(masks), u8, n, Hh, Ww, o._p(col_cnt), o._p(col_off), o._p(total), o._stream()), "psalm_mask_rle_count")
    tot = total.cpu().numpy().astype(np.int64)                 # the one sync: n small integers
    base = np.concatenate(([0], np.cumsum(tot)[:-1]))
    pos = o.empty(max(int(tot.sum()), 1), dtype=torch.int32)
    o._check(o.lib.psalm_mask_rle_emit(o._p(masks), u8, n, Hh, Ww, o._p(col_off), o._p(torch.from_numpy(base).to(o.device)), o._p(pos), o._stream()),
             "psalm_mask_rle_emit")
    pos = pos.cpu().numpy().astype(np.int64)
    out = []
    for i in range(n):
        b = pos[base[i]: base[i] + tot[i]]
        counts = np.diff(np.concatenate(([0], b, [Hh * Ww])))  # run lengths, starting with the zeros run (0 if the mask starts with 1)
        out.append({"size": [Hh, Ww], "counts": rle_counts_to_string(counts.tolist())})
    return out


def iou_counts(pred_masks: torch.Tensor, gt_masks: torch.Tensor, pairs: Sequence[Tuple[int, int]], ops=None):
    """intersectionAndUnionGPU(pred, gt, K=2, ignore_index=255) for each (prediction index, target index) pair, on the device:
    pred_masks (n,H,W) float32|uint8 (nonzero = 1), gt_masks (m,H,W) uint8 with 255 = ignore.
    Returns (intersection (P,2), union (P,2), target (P,2)) int64 tensors on the device (classes: background, foreground)."""
    o = _ops(ops)
    if pred_masks.dim() != 3 or gt_masks.dim() != 3:
        raise H.PsalmHipError("iou_counts: (n,H,W) predictions and (m,H,W) targets")
    pred_masks = _on_device(o, pred_masks, (torch.float32, torch.uint8, torch.bool), "iou_counts")
    gt = gt_masks.to(o.device, torch.uint8).contiguous()
    if tuple(pred_masks.shape[1:]) != tuple(gt.shape[1:]):
        raise H.PsalmHipError("iou_counts: prediction / target size mismatch")
    P = len(pairs)
    n, m = pred_masks.shape[0], gt.shape[0]
    if any(not (0 <= int(p) < n and 0 <= int(t) < m) for p, t in pairs):
        raise H.PsalmHipError(f"iou_counts: pair index out of range (predictions {n}, targets {m})")
    pi = torch.tensor([p for p, _ in pairs], dtype=torch.int32, device=o.device)
    ti = torch.tensor([t for _, t in pairs], dtype=torch.int32, device=o.device)
    counts = torch.zeros(P, 6, dtype=torch.int64, device=o.device)
    HW = int(pred_masks.shape[1] * pred_masks.shape[2])
    o._check(o.lib.psalm_iou_counts(o._p(pred_masks), 1 if pred_masks.dtype == torch.uint8 else 0, o._p(gt), o._p(pi), o._p(ti), P, c_long(HW),
                                    o._p(counts), o._stream()), "psalm_iou_counts")
    inter, outp, tgt = counts[:, 0:2], counts[:, 2:4], counts[:, 4:6]
    return inter, outp + tgt - inter, tgt


def fuse_masks_by_score(pred_masks: torch.Tensor, scores: torch.Tensor, thr: float = 0.6, ops=None) -> torch.Tensor:
    """gRefCOCO's fused prediction (psalm/eval/eval_grefcoco.py:113-131: `compute_metric` + `fuse_masks` :277-285) on the device: the
    union of the candidate masks whose score exceeds `thr`; when none does, the top-1 candidate (the reference's fall-back).
    pred_masks (n,H,W) float32|uint8|bool (nonzero = 1), scores (n) -> (H,W) uint8.  Feed the result to `iou_counts` / `IoUMeters`
    (the no-object target, union == 0 -> accuracy 1, is IoUMeters.update's rule, eval_grefcoco.py:147-148)."""
    o = _ops(ops)
    if pred_masks.dim() != 3 or scores.dim() != 1 or scores.shape[0] != pred_masks.shape[0] or not (1 <= pred_masks.shape[0] <= 1024):
        raise H.PsalmHipError("fuse_masks_by_score: (n,H,W) masks and (n) scores, 1 <= n <= 1024")
    pred_masks = _on_device(o, pred_masks, (torch.float32, torch.uint8, torch.bool), "fuse_masks_by_score")
    sc = _on_device(o, scores, (torch.float32,), "fuse_masks_by_score")
    n, Hh, Ww = pred_masks.shape
    out = torch.empty(Hh, Ww, dtype=torch.uint8, device=o.device)
    from ctypes import c_float
    o._check(o.lib.psalm_fuse_masks(o._p(pred_masks), 1 if pred_masks.dtype == torch.uint8 else 0, o._p(sc), n, c_long(Hh * Ww), c_float(float(thr)),
                                    o._p(out), o._stream()), "psalm_fuse_masks")
    return out


def mask_boxes(masks: torch.Tensor, ops=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Where each mask is and how large: masks (n,H,W) float32 (set: > 0) | uint8 | bool (set: != 0) -> (boxes (n,4) float32, areas (n) int32) on
    the device.  detectron2's `BitMasks.get_bounding_boxes` -- the line the reference comments out as slow on the host (llava_phi.py:319,395,
    438-440): (x_min, y_min, x_max + 1, y_max + 1) over the set pixels, zeros for an empty mask; area = set pixels.  Nothing is read back."""
    o = _ops(ops)
    if not torch.is_tensor(masks) or masks.dim() != 3:
        raise H.PsalmHipError("mask_boxes: (n,H,W) float32 / uint8 / bool masks")
    return o.mask_boxes(_on_device(o, masks, (torch.float32, torch.uint8, torch.bool), "mask_boxes"))


def label_boxes(labels: torch.Tensor, n_ids: int, ops=None) -> torch.Tensor:
    """An id map (H,W) int32 | uint8 -- `panoptic_seg[0]`, the tracker's `fused` -- -> (n_ids,5) int32 on the device: [x0, y0, x1, y1, area] of
    the pixels of every id in [0, n_ids), n_ids <= 256 (the box convention of `mask_boxes`; zeros for an id that does not occur; other values
    are ignored)."""
    o = _ops(ops)
    if not torch.is_tensor(labels) or labels.dim() != 2:
        raise H.PsalmHipError("label_boxes: an (H,W) int32 / uint8 id map")
    return o.label_boxes(_on_device(o, labels, (torch.int32, torch.uint8), "label_boxes"), n_ids)


def _bit_planes(o, masks, what):
    if not torch.is_tensor(masks) or masks.dim() != 3:
        raise H.PsalmHipError(f"{what}: (n,H,W) float32 / uint8 / bool masks")
    masks = _on_device(o, masks, (torch.float32, torch.uint8, torch.bool), what)
    if not 1 <= masks.shape[0] <= o.MASK_PAIRS_MAX:
        raise H.PsalmHipError(f"{what}: {masks.shape[0]} masks (1..{o.MASK_PAIRS_MAX})")
    return masks, o.mask_pack_bits(masks)


def mask_pair_counts(masks_a: torch.Tensor, masks_b: Optional[torch.Tensor] = None, ops=None):
    """All-pairs mask overlap on the device: masks_a (na,H,W), masks_b (nb,H,W) float32 (set: > 0) | uint8 | bool (set: != 0), masks_b=None: a
    against itself; 1 <= na, nb <= 1024 -> (inter (na,nb) int32 = pixels set in both, areas_a (na) int32, areas_b (nb) int32).  The masks are
    packed into bit planes once (psalm_mask_pack_bits) and every pair is a popcount over 64-pixel words (psalm_mask_pair_counts).
    `iou = inter / (areas_a[:, None] + areas_b[None] - inter)` gives the prediction x ground-truth matrix of COCO mask matching and DAVIS J
    without moving a mask."""
    o = _ops(ops)
    a, (bits_a, areas_a) = _bit_planes(o, masks_a, "mask_pair_counts")
    if masks_b is None:
        return o.mask_pair_counts(bits_a), areas_a, areas_a
    b, (bits_b, areas_b) = _bit_planes(o, masks_b, "mask_pair_counts")
    if tuple(a.shape[1:]) != tuple(b.shape[1:]):
        raise H.PsalmHipError(f"mask_pair_counts: masks of {tuple(a.shape[1:])} against masks of {tuple(b.shape[1:])}")
    return o.mask_pair_counts(bits_a, bits_b), areas_a, areas_b


def iou_fraction(iou_thr) -> Tuple[int, int]:
    """The NMS threshold as the rational the kernels compare with: a (num, den) pair as it is, a float through
    `Fraction(iou_thr).limit_denominator(4096)` (0.7 -> 7/10); it must lie in (0, 1] with a denominator <= 4096 (ValueError otherwise)."""
    from fractions import Fraction
    if isinstance(iou_thr, (tuple, list)):
        if len(iou_thr) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in iou_thr):
            raise ValueError(f"iou_thr {iou_thr!r}: a float or a (num, den) pair of integers")
        num, den = int(iou_thr[0]), int(iou_thr[1])
    else:
        v = float(iou_thr)
        if not 0.0 < v <= 1.0:                                        # (NaN fails both comparisons)
            raise ValueError(f"iou_thr {iou_thr!r} outside (0, 1]")
        f = Fraction(v).limit_denominator(4096)
        num, den = f.numerator, f.denominator
    if not 0 < num <= den <= 4096:
        raise ValueError(f"iou_thr {iou_thr!r} = {num}/{den}: outside (0, 1] or a denominator above 4096")
    return num, den


def mask_nms(masks: torch.Tensor, scores: torch.Tensor, iou_thr=0.7, min_area: int = 1, min_score: Optional[float] = None, ops=None) -> dict:
    """Greedy mask NMS on the device: masks (n,H,W) float32 | uint8 | bool, scores (n) float32 without NaN, 1 <= n <= 1024.  Candidates are
    walked by descending score (equal scores: the lower index first); one with fewer than `min_area` pixels or a score below `min_score` is
    filtered; one whose IoU with an already kept candidate EXCEEDS the threshold is suppressed by the first such candidate.  The rule is the
    rational `Fraction(iou_thr).limit_denominator(4096)` (0.7 is 7/10; or give `iou_thr=(num, den)`) and it is strict: an IoU equal to the
    threshold does not suppress; the comparison is made in integers.
    -> {"kept": (K) int64 indices by descending score, "keep": (n) int32 1 kept / 0 suppressed / -1 filtered, "owner": (n) int32 the kept
    candidate that stands for each (-1: filtered), "areas": (n) int32, "inter": (n,n) int32}, on the device.  One read-back: the `kept` block."""
    o = _ops(ops)
    num, den = iou_fraction(iou_thr)
    masks, (bits, areas) = _bit_planes(o, masks, "mask_nms")
    n = masks.shape[0]
    if not torch.is_tensor(scores) or scores.dim() != 1 or scores.shape[0] != n:
        raise H.PsalmHipError(f"mask_nms: (n) float32 scores for {n} masks")
    sc = _on_device(o, scores, (torch.float32,), "mask_nms")
    inter = o.mask_pair_counts(bits)
    kept, keep, owner = o.mask_nms(inter, areas, sc, num, den, min_area=min_area, min_score=min_score)
    K = int(kept.cpu()[0])                                            # the one read-back
    kept = o.to_i64(kept[1:1 + K]) if K else torch.empty(0, dtype=torch.int64, device=o.device)
    return {"kept": kept, "keep": keep, "owner": owner, "areas": areas, "inter": inter}


def _planes(o, masks, what):
    if not torch.is_tensor(masks) or masks.dim() != 3:
        raise H.PsalmHipError(f"{what}: (n,H,W) float32 / uint8 / bool masks")
    masks = _on_device(o, masks, (torch.float32, torch.uint8, torch.bool), what)
    if masks.shape[0] > 65535:
        raise H.PsalmHipError(f"{what}: {masks.shape[0]} masks (at most 65535)")
    return masks


def mask_components(masks: torch.Tensor, connectivity: int = 8, max_components: int = 256, ops=None) -> dict:
    """A mask's connected parts as instances -- a referring or semantic mask that covers three separate objects is three components: masks
    (n,H,W) float32 (set: > 0) | uint8 | bool (set: != 0), up to 65535 of them, on host or device -> {"labels": (n,H,W) int32, 0 off the mask and
    1 + rank on it, the plane's components ranked by their lowest row-major pixel (the numbering of scipy.ndimage.label, structure = the full
    3 x 3 for connectivity 8, the cross for 4); "count": (n) int32; "table": (n, max_components, 6) int32 = [x0, y0, x1, y1, area, border] per
    component (the box convention of `label_boxes`; border = 1 when it touches the image border; zeros beyond `count`; components beyond
    max_components are labelled and counted, not tabled)}, on the device.  Nothing is read back."""
    o = _ops(ops)
    labels, count, table = o.mask_components(_planes(o, masks, "mask_components"), connectivity=connectivity, max_components=max_components)
    return {"labels": labels, "count": count, "table": table}


def clean_masks(masks: torch.Tensor, min_island: int = 0, max_hole: int = 0, connectivity: int = 8, ops=None) -> dict:
    """What every click-to-mask tool does to its results: masks (n,H,W) float32 (set: > 0) | uint8 | bool, up to 65535, on host or device ->
    {"masks": (n,H,W) uint8 of 0 / 1, "areas": (n) int32 of the cleaned masks, "removed": (n) int32, "filled": (n) int32 pixels changed}, on the
    device.  First the holes -- components of the unset pixels, under the complementary connectivity, that do not touch the image border -- of
    at most `max_hole` pixels are filled; then the components of the set pixels with fewer than `min_island` pixels are dropped (a ring whose
    hole was filled is judged as the blob it became; a mask may become empty).  A parameter of 0 skips its step.  Nothing is read back."""
    o = _ops(ops)
    out, areas, filled, removed = o.mask_clean(_planes(o, masks, "clean_masks"), connectivity=connectivity, min_island=min_island, max_hole=max_hole)
    return {"masks": out, "areas": areas, "removed": removed, "filled": filled}


def mask_outlines(masks: torch.Tensor, connectivity: int = 8, ops=None) -> dict:
    """Masks as polygons -- what an annotation tool, a viewer's overlay or a COCO `segmentation` list wants -- traced on the device: masks (n,H,W)
    float32 (set: > 0) | uint8 | bool (set: != 0), up to 65535, on host or device, (H + 1) * (W + 1) * 4 < 2^31 -> {"ring_count": (n) int32,
    "vertex_count": (n) int32, "rings": (R,4) int32 = [mask, first vertex offset, vertex count, signed area], "vertices": (V,2) int32 = (x, y)}, on
    the device.  Pixel (py, px) covers [px, px + 1] x [py, py + 1]; the boundary between set and unset pixels is walked with the set pixel on the
    right and split into closed rings, joined at a diagonal contact under connectivity 8, separated under 4; a ring lists its corners only, from
    its row-major lowest vertex; a mask's rings come in the order of those vertices.  area > 0: an outer boundary (as many as
    `mask_components` counts), area < 0: a hole; a mask's areas add up to its pixels.  `fill_polygons` gives the masks back bit for bit.  Read
    back: the per-mask edge / corner totals that size the work, and the ring counts -- nothing proportional to H * W."""
    o = _ops(ops)
    ring_count, vertex_count, rings, vertices = o.mask_outlines(_planes(o, masks, "mask_outlines"), connectivity=connectivity)
    return {"ring_count": ring_count, "vertex_count": vertex_count, "rings": rings, "vertices": vertices}


def outline_polygons(out: dict, holes: bool = False) -> List[List[List[int]]]:
    """`mask_outlines`' result on the host: per mask a list of flat [x0, y0, x1, y1, ...] lists -- COCO polygons -- of its outer rings (area > 0),
    or with holes=True of all its rings in table order.  Reads back the ring and vertex tables."""
    n = int(out["ring_count"].shape[0])
    rings = out["rings"].cpu().numpy()
    verts = out["vertices"].cpu().numpy()
    polys: List[List[List[int]]] = [[] for _ in range(n)]
    for row, off, cnt, area in rings.tolist():
        if holes or area > 0:
            polys[row].append(verts[off:off + cnt].reshape(-1).tolist())
    return polys


def fill_polygons(rings, vertices, shape, ops=None) -> torch.Tensor:
    """Integer polygons -> masks on the device: rings (R,4) int32 = [mask, first vertex offset, vertex count, anything], vertices (V,2) int32 =
    (x, y) lattice points within [0, W] x [0, H] (tensors or arrays, host or device), shape = (m, H, W) -> (m,H,W) uint8 of 0 / 1.  Even-odd over
    pixel centres: pixel (py, px) is set iff an odd number of ring edges cross the row y = py + 1/2 strictly right of x = px + 1/2 (in integers;
    no ties).  Holes are rings; rings may cross; a ring given twice cancels.  `fill_polygons(out["rings"], out["vertices"], masks.shape)` of
    `mask_outlines`' result is the masks' 0 / 1 planes."""
    o = _ops(ops)
    tabs = []
    for t, cols, what in ((rings, 4, "rings"), (vertices, 2, "vertices")):
        if not torch.is_tensor(t):
            a = np.asarray(t)
            t = torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros((0, cols), np.int32)))
        if t.dim() != 2 or t.shape[1] != cols or t.dtype not in (torch.int32, torch.int64):
            raise H.PsalmHipError(f"fill_polygons: {what} ({'RV'[cols == 2]},{cols}) integers, got {t.dtype} {tuple(t.shape)}")
        tabs.append(t.to(torch.int32).to(o.device).contiguous())
    return o.mask_fill_polygons(tabs[0], tabs[1], tuple(shape))


def mask_distance(masks: torch.Tensor, to: str = "unset", border: bool = False, ops=None) -> torch.Tensor:
    """How far each pixel is from the mask's edge, exactly: masks (n,H,W) float32 (set: > 0) | uint8 | bool (set: != 0), up to 65535, on host or
    device, 1 <= H, W <= 16384 -> (n,H,W) int32 on the device, the SQUARED Euclidean distance to the nearest seed pixel.  to="unset": the seeds are
    the unset pixels -- the inside distance, `scipy.ndimage.distance_transform_edt(mask) ** 2`, 0 off the mask; to="set": the set pixels,
    `distance_transform_edt(~mask) ** 2`.  border=True: every position outside the image is a seed too (the transform of the plane padded with
    seeds all round, cropped back).  A plane without any seed gives 2^30 everywhere.  `dist2 <= r * r` erodes (to="unset") or dilates (to="set")
    by a disc of any radius; `dist2.amax()` is how thick a mask is.  Nothing is read back."""
    o = _ops(ops)
    return o.mask_distance(_planes(o, masks, "mask_distance"), to=to, border=border)


def mask_centers(masks: torch.Tensor, ops=None) -> torch.Tensor:
    """A click from a mask -- the point every interactive tool uses: masks (n,H,W) as `mask_distance` takes them -> (n,3) int32 on the device =
    [y, x, dist2] of the set pixel deepest inside, the first maximum (row-major) of `mask_distance(masks, border=True)` over the set pixels, the
    image border counted as outside; [-1, -1, 0] for an empty mask.  Every pixel with (y' - y)^2 + (x' - x)^2 < dist2 is inside the image and
    set.  (y, x) is a valid {"points": [(y, x)]} prompt for `segment` / `VideoTracker.start` when the masks are in the original image's pixels.
    Nothing is read back."""
    o = _ops(ops)
    return o.mask_centers(_planes(o, masks, "mask_centers"))


def mask_boundaries(masks: torch.Tensor, ops=None) -> torch.Tensor:
    """DAVIS's `seg2bmap` at the mask's own size: masks (n,H,W) as `mask_distance` takes them -> (n,H,W) uint8 of 0 / 1 on the device: a pixel
    that differs from its right, lower or lower-right neighbour (the last row looks right only, the last column down only, the last pixel is
    0).  Nothing is read back."""
    o = _ops(ops)
    return o.mask_boundaries(_planes(o, masks, "mask_boundaries"))


def davis_bound(shape, bound_th: float = 0.008) -> int:
    """DAVIS's boundary tolerance in pixels for masks of `shape` = (H, W): `bound_th` itself if >= 1, else ceil(bound_th * hypot(H, W))."""
    Hh, Ww = int(shape[-2]), int(shape[-1])
    return int(bound_th) if bound_th >= 1 else int(math.ceil(bound_th * math.hypot(Hh, Ww)))


def boundary_counts(pred_masks: torch.Tensor, gt_masks: torch.Tensor, pairs: Sequence[Tuple[int, int]], bound: int, ops=None) -> torch.Tensor:
    """The integers of DAVIS's boundary measure F (`f_measure`, without void pixels) for each (prediction index, target index) pair, on the
    device: pred_masks (n,H,W), gt_masks (m,H,W) as `mask_distance` takes them, `bound` an integer number of pixels, 0 <= bound <= 32767
    (`davis_bound(shape)`) -> (P,4) int64 = [n_fg, n_gt, fg_match, gt_match]: the boundary pixels (`mask_boundaries`) of the prediction and of
    the target, the prediction boundary pixels within `bound` of the target's boundary (dy^2 + dx^2 <= bound^2, the disc of
    `cv2.dilate(., disk(bound))`), and the mirror image.  Only the planes the pairs name are processed, each once.  `boundary_f` turns the
    counts into precision, recall and F.  Nothing is read back."""
    o = _ops(ops)
    pred_masks = _planes(o, pred_masks, "boundary_counts")
    gt_masks = _planes(o, gt_masks, "boundary_counts")
    if tuple(pred_masks.shape[1:]) != tuple(gt_masks.shape[1:]):
        raise H.PsalmHipError(f"boundary_counts: predictions of {tuple(pred_masks.shape[1:])} against targets of {tuple(gt_masks.shape[1:])}")
    n, m = int(pred_masks.shape[0]), int(gt_masks.shape[0])
    pairs = [(int(p), int(t)) for p, t in pairs]
    if any(not (0 <= p < n and 0 <= t < m) for p, t in pairs):
        raise H.PsalmHipError(f"boundary_counts: pair index out of range (predictions {n}, targets {m})")
    up, ut = sorted({p for p, _ in pairs}), sorted({t for _, t in pairs})
    rp, rt = {p: i for i, p in enumerate(up)}, {t: i for i, t in enumerate(ut)}
    tab = torch.tensor(up + ut + [rp[p] for p, _ in pairs] + [rt[t] for _, t in pairs], dtype=torch.int32).to(o.device)      # one small upload
    a, b, P = len(up), len(up) + len(ut), len(pairs)
    return o.boundary_counts(pred_masks, gt_masks, tab[b:b + P], tab[b + P:], bound, pred_index=tab[:a], gt_index=tab[a:b])


def boundary_f(counts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`boundary_counts`' (P,4) integers -> (precision, recall, F), float64 arrays on the host, with DAVIS's special cases: no prediction
    boundary but a target one: P = 1, R = 0; the reverse: P = 0, R = 1; neither: P = R = 1; else P = fg_match / n_fg, R = gt_match / n_gt;
    F = 0 if P + R == 0 else 2 P R / (P + R).  Reads back the 4 P integers."""
    c = (counts.cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)).astype(np.int64).reshape(-1, 4)
    n_fg, n_gt, fg_m, gt_m = (c[:, k].astype(np.float64) for k in range(4))
    prec = np.where(n_fg > 0, fg_m / np.maximum(n_fg, 1), 1.0)
    rec = np.where(n_gt > 0, gt_m / np.maximum(n_gt, 1), 1.0)
    prec = np.where((n_fg > 0) & (n_gt == 0), 0.0, prec)
    rec = np.where((n_fg == 0) & (n_gt > 0), 0.0, rec)
    s = prec + rec
    f = np.where(s == 0, 0.0, 2 * prec * rec / np.where(s == 0, 1.0, s))
    return prec, rec, f


def coco_instance_records(instances, image_id, category_ids: Optional[Sequence[int]] = None, ops=None, segmentation: str = "rle") -> List[dict]:
    """detectron2's `instances_to_coco_json`, the records the reference's instance evaluator collects (instance_evaluation.py): per instance
    {"image_id", "category_id", "bbox": [x, y, w, h] floats from `pred_boxes` (BoxMode XYXY_ABS -> XYWH_ABS), "score", "segmentation": COCO RLE
    with its counts as str}.  category_ids: the contiguous class index -> dataset category id table (the evaluator's reverse id mapping).
    Only the small arrays (boxes, scores, classes, run boundaries) are read back; the boxes are real under `PSALM.mask_boxes = True`.
    segmentation="polygon": the COCO polygon form instead -- a list of flat [x0, y0, x1, y1, ...] lists, the outer rings of `mask_outlines`
    (connectivity 8; COCO polygons cannot say holes: a consumer that fills them gets the mask with its holes closed)."""
    if segmentation not in ("rle", "polygon"):
        raise ValueError(f"coco_instance_records: segmentation = {segmentation!r} ('rle' or 'polygon')")
    n = len(instances)
    if n == 0:
        return []
    boxes = instances.pred_boxes.detach().cpu().numpy().astype(np.float64)
    boxes[:, 2] -= boxes[:, 0]
    boxes[:, 3] -= boxes[:, 1]
    scores = instances.scores.detach().cpu().tolist()
    classes = instances.pred_classes.detach().cpu().tolist() if hasattr(instances, "pred_classes") else [0] * n
    if segmentation == "polygon":
        polys = outline_polygons(mask_outlines(instances.pred_masks, ops=ops))
    else:
        rles = masks_to_rle(instances.pred_masks, ops=ops)
    out = []
    for k in range(n):
        rle = polys[k] if segmentation == "polygon" else {"size": rles[k]["size"], "counts": rles[k]["counts"].decode("utf-8")}
        out.append({"image_id": image_id, "category_id": int(category_ids[classes[k]]) if category_ids is not None else int(classes[k]),
                    "bbox": boxes[k].tolist(), "score": float(scores[k]), "segmentation": rle})
    return out


class IoUMeters:
    """The three AverageMeters of the referring / region evaluation loops (referring_segmentation.py:139-177: intersection, union,
    acc_iou) fed from device-side counts; `all_reduce()` = AverageMeter.all_reduce (:58-79) as ONE small SUM all-reduce."""

    def __init__(self):
        self.sum = torch.zeros(7, dtype=torch.float64)         # [I0, I1, U0, U1, acc0, acc1, n]

    def update(self, inter: torch.Tensor, union: torch.Tensor) -> None:
        """inter / union (P,2) for the evaluator's top-1 prediction of each of P samples (compute_metric, :139-171)."""
        i, u = inter.double().cpu(), union.double().cpu()
        acc = i / (u + 1e-5)
        acc[u == 0] = 1.0                                       # no-object target (:158)
        self.sum[0:2] += i.sum(0)
        self.sum[2:4] += u.sum(0)
        self.sum[4:6] += acc.sum(0)
        self.sum[6] += i.shape[0]

    def all_reduce(self, device=None) -> None:
        """SUM over ranks in float64 (pixel counts pass 2^24 within a few images).  `device`: where the collective runs; by default the
        current GPU under the nccl (RCCL) backend -- which reduces device tensors only, as the reference's AverageMeter.all_reduce knows
        (`.cuda()` first) -- and the host otherwise (gloo)."""
        import torch.distributed as dist
        from .dist import reduce_metrics
        if device is None and dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            device = torch.device("cuda", torch.cuda.current_device())
        t = self.sum.to(device) if device is not None else self.sum.clone()
        self.sum = reduce_metrics(t).double().cpu()

    def results(self) -> dict:
        ciou = float(self.sum[1] / (self.sum[3] + 1e-10))      # iou_class[1], region_segmentation.py:286-287
        giou = float(self.sum[5] / max(float(self.sum[6]), 1e-5))
        return {"ciou": ciou, "giou": giou, "n": int(self.sum[6])}


class JFMeters:
    """DAVIS's J&F beside `IoUMeters`: per (prediction, target) pair J = intersection / union of the foreground (1 where the union is empty)
    and F = `boundary_f` of the pair's `boundary_counts`; `results()` gives their means over the pairs seen, `all_reduce()` sums the meters
    over ranks as ONE small all-reduce (`psalm_amd.dist.reduce_metrics`)."""

    def __init__(self):
        self.sum = torch.zeros(3, dtype=torch.float64)         # [sum J, sum F, n]

    def update(self, inter: torch.Tensor, union: torch.Tensor, bcounts: torch.Tensor) -> None:
        """inter / union: (P) foreground pixel counts, or the (P,2) tensors of `iou_counts` (the foreground column is taken); bcounts (P,4) of
        `boundary_counts` for the same pairs."""
        i, u = inter.double().cpu(), union.double().cpu()
        if i.dim() == 2:
            i, u = i[:, 1], u[:, 1]
        j = torch.where(u == 0, torch.ones_like(u), i / torch.where(u == 0, torch.ones_like(u), u))
        f = boundary_f(bcounts)[2]
        if f.shape[0] != j.shape[0]:
            raise ValueError(f"JFMeters.update: {j.shape[0]} overlap counts against {f.shape[0]} boundary counts")
        self.sum[0] += j.sum()
        self.sum[1] += float(f.sum())
        self.sum[2] += j.shape[0]

    def all_reduce(self, device=None) -> None:
        """SUM over ranks, as IoUMeters.all_reduce."""
        import torch.distributed as dist
        from .dist import reduce_metrics
        if device is None and dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            device = torch.device("cuda", torch.cuda.current_device())
        t = self.sum.to(device) if device is not None else self.sum.clone()
        self.sum = reduce_metrics(t).double().cpu()

    def results(self) -> dict:
        n = max(float(self.sum[2]), 1.0)
        j, f = float(self.sum[0]) / n, float(self.sum[1]) / n
        return {"J": j, "F": f, "J&F": (j + f) / 2, "n": int(self.sum[2])}


def _id_map(o, m, what: str) -> torch.Tensor:
    """An id map for the pair-count kernel: a tensor or array on host or device, (H,W) of any integer type (held as int32) or the panoptic PNG's
    (H,W,3) uint8 -> contiguous on the device."""
    if isinstance(m, np.ndarray):
        if m.dtype == np.uint32:
            m = m.astype(np.int64)
        m = torch.from_numpy(np.ascontiguousarray(m))
    if not torch.is_tensor(m):
        raise H.PsalmHipError(f"{what}: a tensor or array, got {type(m)}")
    if m.dim() == 3 and m.shape[2] == 3 and m.dtype == torch.uint8:
        return m.to(o.device).contiguous()
    if m.dim() != 2 or m.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint8):
        raise H.PsalmHipError(f"{what}: an (H,W) integer id map or its (H,W,3) uint8 rgb form, got {m.dtype} {tuple(m.shape)}")
    return m.to(o.device, torch.int32).contiguous()


def _sorted_ids(ids, what: str) -> Tuple[np.ndarray, np.ndarray]:
    """any integer sequence -> (the ids ascending as int32, the permutation that sorts them); duplicates, values <= 0 or >= 2^31, more than 1023:
    ValueError"""
    ids = ids.cpu().tolist() if torch.is_tensor(ids) else ids.tolist() if isinstance(ids, np.ndarray) else list(ids)
    if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in ids):
        raise ValueError(f"{what}: a flat sequence of integers")
    if len(ids) > H.Ops.LABEL_PAIRS_MAX_IDS:
        raise ValueError(f"{what}: {len(ids)} ids (at most {H.Ops.LABEL_PAIRS_MAX_IDS})")
    if any(not 0 < int(v) < 2 ** 31 for v in ids):
        raise ValueError(f"{what}: ids must lie in [1, 2^31 - 1] (0 is VOID)")
    v = np.array([int(x) for x in ids], dtype=np.int64)
    order = np.argsort(v, kind="stable")
    s = v[order]
    if (np.diff(s) == 0).any():
        raise ValueError(f"{what}: an id is listed twice")
    return s.astype(np.int32), order.astype(np.int64)


def label_pair_counts(gt, gt_ids, pred, pred_ids, ops=None):
    """The overlap table of two id maps -- what panopticapi gets from `np.unique(gt * 256^3 + pred, return_counts=True)` -- on the device: gt, pred on
    host or device, (H,W) integers or the PNG's (H,W,3) uint8 (id = R + 256 G + 65536 B); gt_ids / pred_ids: any integer sequences of distinct ids
    in [1, 2^31 - 1], at most 1023 each (ValueError otherwise) -> (counts (G+2, P+2) int32 on the device, gt_order, pred_order).  The ids are sorted
    here: row 1 + k counts the pixels of `gt_ids[gt_order[k]]`, row 0 the value 0 (VOID), the last row every other value; columns likewise for
    `pred`.  The table sums to H * W.  Nothing is read back."""
    o = _ops(ops)
    gs, g_order = _sorted_ids(gt_ids, "label_pair_counts gt_ids")
    ps, p_order = _sorted_ids(pred_ids, "label_pair_counts pred_ids")
    tab = torch.from_numpy(np.concatenate((gs, ps))).to(o.device)                                           # one small upload
    counts = o.label_pair_counts(_id_map(o, gt, "label_pair_counts gt"), tab[:gs.size], _id_map(o, pred, "label_pair_counts pred"), tab[gs.size:],
                                 check=False)
    return counts, g_order, p_order


class PanopticQuality:
    """PQ / SQ / RQ of COCO panoptic -- panopticapi's `pq_compute` -- kept on the device beside `ConfusionMatrix`, without the PNG round trip of
    my_coco_panoptic_evaluator (panoptic_evaluation.py:179-221).  categories: {dataset category id: isthing}; a dict of panopticapi's records
    ({id: {"isthing": ..}}) is taken too.  `update` per image (two launches, no read-back), `results()` once at the end."""

    def __init__(self, categories: dict, ops=None):
        self.ops = _ops(ops)
        self.categories = {int(k): bool(v["isthing"] if isinstance(v, dict) else v) for k, v in categories.items()}
        C = len(self.categories)
        if not 1 <= C <= H.Ops.PQ_MAX_CATEGORIES:
            raise ValueError(f"PanopticQuality: {C} categories (1..{H.Ops.PQ_MAX_CATEGORIES})")
        self._slot = {c: i for i, c in enumerate(self.categories)}
        dev = self.ops.device
        self.stat = torch.zeros(C, 3, dtype=torch.int64, device=dev)      # [tp, fp, fn]
        self.iou = torch.zeros(C, dtype=torch.float64, device=dev)
        self.notes = torch.zeros(4, dtype=torch.int64, device=dev)        # [images, unlisted gt pixels, unlisted pred pixels, empty listed preds]

    def _cat_slot(self, cat, what):
        try:
            return self._slot[int(cat)]
        except KeyError:
            raise ValueError(f"PanopticQuality.update: {what} category {cat!r} is not one of the meter's categories") from None

    def update(self, pred, pred_segments_info, gt, gt_segments_info, category_ids: Optional[Sequence[int]] = None) -> None:
        """One image: pred = `result["panoptic_seg"][0]` with its `segments_info` list ({"id", "category_id", ..}; category_ids: the contiguous class
        index -> dataset category id table, as in `coco_instance_records`), gt = the ground truth's id map or its RGB PNG array with the COCO panoptic
        JSON's records ({"id", "category_id", "iscrowd"}).  One small upload (sorted id tables, category slots, crowd flags, each prediction's crowd
        slot), `psalm_label_pair_counts`, `psalm_pq_accumulate`; nothing is read back.  A category outside the meter's: ValueError."""
        o = self.ops
        gs, g_order = _sorted_ids([s["id"] for s in gt_segments_info], "PanopticQuality.update gt ids")
        ps, p_order = _sorted_ids([s["id"] for s in pred_segments_info], "PanopticQuality.update prediction ids")
        G, P = gs.size, ps.size
        g_slot_of = np.empty(G, np.int64)
        g_slot_of[g_order] = 1 + np.arange(G)                            # JSON position -> gt slot
        g_cat = np.array([self._cat_slot(s["category_id"], "ground-truth") for s in gt_segments_info], dtype=np.int64).reshape(-1)
        g_crowd = np.array([1 if int(s.get("iscrowd", 0)) == 1 else 0 for s in gt_segments_info], dtype=np.int64).reshape(-1)
        crowd_slot = {}                                                  # panopticapi's crowd_labels_dict: the LAST crowd segment of a category wins
        for k in range(G):
            if g_crowd[k]:
                crowd_slot[int(g_cat[k])] = int(g_slot_of[k])
        p_cat = np.array([self._cat_slot(category_ids[int(s["category_id"])] if category_ids is not None else s["category_id"], "prediction")
                          for s in pred_segments_info], dtype=np.int64).reshape(-1)
        p_crowd = np.array([crowd_slot.get(int(c), -1) for c in p_cat], dtype=np.int64).reshape(-1)
        tab = torch.from_numpy(np.concatenate((gs, ps, g_cat[g_order], g_crowd[g_order], p_cat[p_order], p_crowd[p_order])).astype(np.int32)).to(o.device)
        cut = np.cumsum([0, G, P, G, G, P, P]).tolist()
        t_gs, t_ps, t_gcat, t_gcrowd, t_pcat, t_pcrowd = (tab[a:b] for a, b in zip(cut[:-1], cut[1:]))
        counts = o.label_pair_counts(_id_map(o, gt, "PanopticQuality.update gt"), t_gs, _id_map(o, pred, "PanopticQuality.update pred"), t_ps, check=False)
        o.pq_accumulate(counts, t_gcat, t_gcrowd, t_pcat, t_pcrowd, self.stat, self.iou, self.notes)

    def all_reduce(self, device=None) -> None:
        """SUM over ranks as ONE small all-reduce (`psalm_amd.dist.reduce_metrics`) of a (C,4) float64 [tp, fp, fn, iou] block plus the notes; the
        counts stay exact below 2^53.  `device` as in IoUMeters.all_reduce."""
        import torch.distributed as dist
        from .dist import reduce_metrics
        if device is None and dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
            device = torch.device("cuda", torch.cuda.current_device())
        C = len(self.categories)
        t = torch.cat((self.stat.double(), self.iou[:, None]), dim=1).reshape(-1)
        t = torch.cat((t, self.notes.double()))
        t = reduce_metrics(t.to(device) if device is not None else t.clone()).double().to(self.ops.device)
        block = t[:4 * C].reshape(C, 4)
        self.stat = block[:, :3].round().to(torch.int64).contiguous()
        self.iou = block[:, 3].contiguous()
        self.notes = t[4 * C:].round().to(torch.int64).contiguous()

    def results(self, strict: bool = True) -> dict:
        """panopticapi's `pq_compute` result from ONE read-back of the accumulators: {"All" | "Things" | "Stuff": {"pq", "sq", "rq", "n"}, "per_class":
        {category id: {"pq", "sq", "rq"}}, "notes": {"images", "unlisted_gt_pixels", "unlisted_pred_pixels", "empty_pred_segments"}} in
        `pq_average`'s arithmetic (a class with tp + fp + fn == 0 is left out of n and reads 0; sq = 0 when tp == 0; a group without any class gives
        0 where panopticapi divides by zero).  strict=True: pixels of a prediction id that its segments_info does not list raise, as panopticapi
        does."""
        C = len(self.categories)
        flat = torch.cat((self.stat.double().reshape(-1), self.iou, self.notes.double())).cpu().numpy()      # the one read-back (counts < 2^53)
        stat = np.rint(flat[:3 * C]).astype(np.int64).reshape(C, 3)
        iou = flat[3 * C:4 * C]
        notes = np.rint(flat[4 * C:]).astype(np.int64)
        note = {"images": int(notes[0]), "unlisted_gt_pixels": int(notes[1]), "unlisted_pred_pixels": int(notes[2]), "empty_pred_segments": int(notes[3])}
        if strict and note["unlisted_pred_pixels"]:
            raise ValueError(f"PanopticQuality: {note['unlisted_pred_pixels']} prediction pixels carry an id that segments_info does not list")
        out = {"per_class": {}, "notes": note}
        for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
            pq = sq = rq = 0.0
            n = 0
            for cat, thing in self.categories.items():
                if isthing is not None and thing != isthing:
                    continue
                k = self._slot[cat]
                tp, fp, fn, s = int(stat[k, 0]), int(stat[k, 1]), int(stat[k, 2]), float(iou[k])
                if tp + fp + fn == 0:
                    res = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
                else:
                    n += 1
                    res = {"pq": s / (tp + 0.5 * fp + 0.5 * fn), "sq": s / tp if tp != 0 else 0.0, "rq": tp / (tp + 0.5 * fp + 0.5 * fn)}
                    pq, sq, rq = pq + res["pq"], sq + res["sq"], rq + res["rq"]
                if isthing is None:
                    out["per_class"][cat] = res
            out[name] = {"pq": pq / n if n else 0.0, "sq": sq / n if n else 0.0, "rq": rq / n if n else 0.0, "n": n}
        return out


def compact_results(result: dict, gt_sem: Optional[torch.Tensor] = None, conf: Optional[ConfusionMatrix] = None, ops=None,
                    pq: Optional[PanopticQuality] = None, gt_panoptic=None, category_ids: Optional[Sequence[int]] = None) -> dict:
    """What the reference's panoptic / semantic / instance evaluators keep of ONE eval_seg result (panoptic_evaluation.py:114-145,179-222;
    instance masks as COCO RLE, region_segmentation.py:282), produced on the device, so that KBs..MBs instead of ~1 GB cross PCIe:
        "sem_labels"   (H,W) int32          from result["sem_seg"]           (+ conf.update(labels, gt_sem) when both are given)
        "panoptic_rgb" (H,W,3) uint8, "segments_info"   from result["panoptic_seg"]
        "instances"    {"rle": [...], "scores": (n,), "pred_classes": (n,)}  from result["instances"]
                       (+ "boxes" (n,4), "areas" (n,) when the result was made under `PSALM.mask_boxes = True`)
    Keys follow what the result holds (semantic-only / instance-only tasks give the matching subset).
    pq + gt_panoptic = (ground-truth id map or RGB PNG array, its segments_info): when both are given and the result holds `panoptic_seg`, the
    image is scored on the device as well -- `pq.update(pan, info, *gt_panoptic, category_ids=category_ids)`; nothing else changes."""
    o = _ops(ops)
    out = {}
    if "sem_seg" in result:
        out["sem_labels"] = semantic_labels(result["sem_seg"].contiguous(), ops=o)
        if conf is not None and gt_sem is not None:
            conf.update(out["sem_labels"], gt_sem)
    if "panoptic_seg" in result:
        pan, info = result["panoptic_seg"]
        out["panoptic_rgb"] = panoptic_png_rgb(pan, ops=o)
        out["segments_info"] = info
        if pq is not None and gt_panoptic is not None:
            pq.update(pan, info, gt_panoptic[0], gt_panoptic[1], category_ids=category_ids)
    if "instances" in result and getattr(result["instances"], "pred_masks", None) is not None:
        inst = result["instances"]
        out["instances"] = {"rle": masks_to_rle(inst.pred_masks, ops=o), "scores": inst.scores}
        if hasattr(inst, "pred_classes"):
            out["instances"]["pred_classes"] = inst.pred_classes
        if hasattr(inst, "pred_areas"):
            out["instances"]["boxes"], out["instances"]["areas"] = inst.pred_boxes, inst.pred_areas
    return out
