"""Helpers of the `PSALM.mask_boxes` tests (tests/test_29_mask_boxes_model_emu.py, tests/test_30_mask_boxes_gpu.py).  The tiny synthetic model's own
masks are empty, so its outputs would compare zeros with zeros: the post-processing is driven with CRAFTED predictor outputs instead -- mask logits
of +8 inside a few rectangles and discs and -8 outside at the decoder's resolution, class / SEG / region logits under which several queries
survive -- through `PSALM._postprocess` + `_finalize` at a canvas of 96 with an original size of (60, 80): the crop to 72 x 96 and the resize are
not the identity.  The oracle is numpy on the very masks (id map) the library returned; every comparison is exact."""
import numpy as np
import torch

from interactive_util import image_of, model_for
from psalm_amd import evalout as E

CANVAS, ORIG = 96, (60, 80)
LOW = CANVAS // 4                 # the decoder's mask resolution
VALID = 72 // 4                   # rows of it that lie inside the un-padded box (the image is resized to 72 x 96, then padded to 96 x 96)
TASKS = ("semantic", "instance", "panoptic", "referring", "region")
# Every query gets a blob but one in six.  (The selecting tasks rank their candidates by class probability alone, LP:428, so the empty query is selected
# with its class like the others; in the panoptic task it has a thing class, 0, and passes the thing filter.)
EMPTY = 0


def nonempty(Q):
    return [q for q in range(Q) if q % 6 != EMPTY]
N_CLASSES = {"semantic": 5, "instance": 5, "panoptic": 5}
THING = [1, 1, 0, 0, 1]
NEW_LAUNCHES = ("psalm_mask_boxes", "psalm_label_boxes")


def np_box(m):
    """detectron2 BitMasks.get_bounding_boxes on one mask: ([x0, y0, x1, y1], area), zeros when no pixel is set"""
    m = m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)
    ys, xs = np.nonzero(m > 0 if m.dtype.kind == "f" else m != 0)
    if len(ys) == 0:
        return [0, 0, 0, 0], 0
    return [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1], len(ys)


def np_boxes(masks):
    got = [np_box(m) for m in masks]
    return np.array([b for b, _ in got], np.float32).reshape(-1, 4), np.array([a for _, a in got], np.int32)


def blob_logits(Q, nonempty):
    """(Q, LOW, LOW) float32 of -8 with +8 inside one blob per query of `nonempty`: rectangles and discs of several sizes inside the valid rows,
    some touching the image's edges"""
    yy, xx = np.mgrid[:LOW, :LOW]
    out = np.full((Q, LOW, LOW), -8.0, np.float32)
    for i, q in enumerate(nonempty):
        if i % 2 == 0:
            y0, x0 = (2 * i) % (VALID - 6), (5 * i) % (LOW - 8)
            out[q, y0:y0 + 4 + i % 3, x0:x0 + 5 + i % 4] = 8.0
        else:
            cy, cx, r = 3 + (3 * i) % (VALID - 6), 4 + (7 * i) % (LOW - 8), 2 + i % 3
            out[q][((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) & (yy < VALID)] = 8.0
    if len(nonempty) > 2:
        out[list(nonempty)[2], 0, :] = 8.0                       # the whole first row: a box as wide as the image
    return out


def crafted_outputs(model, task, K=3):
    """what `PSALM.predictor` returns for one image, with the crafted logits"""
    Q, dev = model.cfg.md_queries, model.device
    r = {"pred_masks": torch.from_numpy(blob_logits(Q, nonempty(Q))).to(dev), "pred_class_name_logits": None, "pred_SEG_logits": None,
         "pred_region_logits": None}
    if task in N_CLASSES:
        C = N_CLASSES[task]
        cls = np.zeros((Q, C + 1), np.float32)
        for q in range(Q):
            cls[q, (2 * q) % C] = 8.0
        r["pred_class_name_logits"] = torch.from_numpy(cls).to(dev)
    elif task == "referring":
        r["pred_SEG_logits"] = torch.linspace(-2.0, 3.0, Q).view(Q, 1).contiguous().to(dev)
    else:
        reg = np.full((K, Q), -3.0, np.float32) + np.arange(Q, dtype=np.float32) * 0.01
        reg[0, 2], reg[1, 5] = 4.0, 4.0
        reg[2, :] = -200.0                                       # sigmoid = 0: every score of region 2 is 0 and its pick, the first arg-max, is query 0 = EMPTY
        r["pred_region_logits"] = torch.from_numpy(reg).to(dev)
    return r


def post(model, task, r, info, calls=None):
    """`_postprocess` (+ the launch names, when `calls` is a list) -> the un-finalized result"""
    if task == "panoptic":
        model.is_thing_list = THING
    lib = model.ops.lib
    lib.calls = [] if calls is not None else None
    try:
        res = model._postprocess(r, model._post_sizes(CANVAS, CANVAS, info, model.cfg.size_divisibility))
        if calls is not None:
            calls.extend(lib.calls)
    finally:
        lib.calls = None
    return res


class HostTrips:
    """counts the device-to-host reads of a block: Tensor.cpu / .item / .tolist / .numpy on a tensor (on the emulator they are no-ops that are
    called all the same)"""

    def __enter__(self):
        self.n = 0
        self._saved = {k: getattr(torch.Tensor, k) for k in ("cpu", "item")}
        for k, fn in self._saved.items():
            def counted(t, *a, _fn=fn, **kw):
                self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, counted)
        return self

    def __exit__(self, *exc):
        for k, fn in self._saved.items():
            setattr(torch.Tensor, k, fn)


def check_condition(masks):
    """the condition of these tests: at least half of the compared masks are non-empty and at least one is empty"""
    areas = [int((m != 0).sum()) for m in masks]
    assert sum(a > 0 for a in areas) * 2 >= len(areas) and any(a == 0 for a in areas), areas


def task_case(kind, precision, task, native=True, queries=None):
    """Switch on: boxes / areas (panoptic: each segment's area / bbox) equal numpy's on the returned masks, through the native post-processing call
    (native = True, where the task and mode have one) or the op-level sequence; COCO records; one host round trip for panoptic.  Switch off: zeros,
    no new field, no new launch."""
    if queries is None:
        model = model_for(kind, precision, task)
    else:                                                        # (64 < Q <= 128: the size at which the panoptic task has a native call)
        from test_14_video_tracker_emu import model_for as model_with
        model = model_with(kind, precision, task, md_queries=queries)
    _, info = image_of(model.cfg, orig=ORIG, size=CANVAS)
    r = crafted_outputs(model, task)
    gt_opt = task == "region"
    saved = (model.mask_boxes, model.c_stages)
    try:
        model.c_stages = native
        model.mask_boxes = False
        calls_off = []
        res = post(model, task, r, info, calls_off)
        with HostTrips() as trips_off:
            off = model._finalize(res, info, gt_optional=gt_opt)
        assert not any(n in calls_off for n in NEW_LAUNCHES)
        model.mask_boxes = True
        calls_on = []
        res = post(model, task, r, info, calls_on)
        with HostTrips() as trips_on:
            on = model._finalize(res, info, gt_optional=gt_opt)
    finally:
        model.mask_boxes, model.c_stages = saved
    on["_calls"] = calls_on
    if task == "semantic":
        assert calls_on == calls_off and set(on) == set(off) | {"_calls"} and "instances" not in on
        return on
    assert trips_on.n == trips_off.n and (task != "panoptic" or trips_on.n == 1)         # panoptic: the one round trip, table included
    assert calls_on.count("psalm_mask_boxes") == 1 and calls_on.count("psalm_label_boxes") == (1 if task == "panoptic" else 0)
    assert [c for c in calls_on if c not in NEW_LAUNCHES] == calls_off
    ion, ioff = on["instances"], off["instances"]
    # off: today's result
    assert not ioff.has("pred_areas") and not hasattr(ioff, "pred_areas")
    assert ioff.pred_boxes.dtype == torch.float32 and not ioff.pred_boxes.any() and tuple(ioff.pred_boxes.shape) == (len(ioff), 4)
    assert set(ion.get_fields()) == set(ioff.get_fields()) | {"pred_areas"}
    for k, v in ioff.get_fields().items():
        if k != "pred_boxes":
            assert torch.equal(ion.get_fields()[k].cpu(), v.cpu()), k
    # on: numpy on the returned masks
    masks = ion.pred_masks.cpu()
    assert tuple(masks.shape[1:]) == ORIG
    check_condition(masks)
    wb, wa = np_boxes(masks)
    assert ion.pred_boxes.dtype == torch.float32 and ion.pred_areas.dtype == torch.int32 and ion.pred_boxes.device == ion.pred_masks.device
    assert np.array_equal(ion.pred_boxes.cpu().numpy(), wb), (ion.pred_boxes.cpu().numpy(), wb)
    assert np.array_equal(ion.pred_areas.cpu().numpy(), wa)
    if task == "panoptic":
        pan, segs = on["panoptic_seg"]
        _, segs_off = off["panoptic_seg"]
        assert len(segs) >= 2 and all("area" not in s and "bbox" not in s for s in segs_off)
        assert [{k: v for k, v in s.items() if k not in ("area", "bbox")} for s in segs] == segs_off
        for s in segs:
            (x0, y0, x1, y1), a = np_box(pan.cpu() == s["id"])
            assert a > 0 and s["area"] == a and s["bbox"] == [x0, y0, x1 - x0, y1 - y0], s
            assert all(type(v) is int for v in s["bbox"] + [s["area"]])
    if task in ("instance", "panoptic"):
        cat = [10 * (c + 1) for c in range(N_CLASSES[task])]
        recs = E.coco_instance_records(ion, image_id=17, category_ids=cat, ops=model.ops)
        rles = E.masks_to_rle(ion.pred_masks, ops=model.ops)
        assert len(recs) == len(ion)
        for k, rec in enumerate(recs):
            x0, y0, x1, y1 = wb[k].tolist()
            assert rec["image_id"] == 17 and rec["category_id"] == cat[int(ion.pred_classes[k])] and rec["score"] == float(ion.scores[k])
            assert rec["bbox"] == [x0, y0, x1 - x0, y1 - y0] and all(type(v) is float for v in rec["bbox"])
            assert rec["segmentation"] == {"size": rles[k]["size"], "counts": rles[k]["counts"].decode("utf-8")}
        comp_on, comp_off = E.compact_results(on, ops=model.ops), E.compact_results(off, ops=model.ops)
        assert "boxes" not in comp_off["instances"] and "areas" not in comp_off["instances"]
        assert comp_on["instances"]["boxes"] is ion.pred_boxes and comp_on["instances"]["areas"] is ion.pred_areas
    return on


def pick_case(kind, precision="fp32"):
    """`_region_pick` on a crafted region result: picked_boxes / picked_areas are the picked queries' rows (one of them the empty query)"""
    model = model_for(kind, precision, "region")
    _, info = image_of(model.cfg, orig=ORIG, size=CANVAS)
    r = crafted_outputs(model, "region")
    saved = model.mask_boxes
    try:
        model.mask_boxes = False
        off = model._region_pick(post(model, "region", r, info))
        model.mask_boxes = True
        calls = []
        res = post(model, "region", r, info, calls)
        lib = model.ops.lib
        lib.calls = []
        on = model._region_pick(res)
        pick_calls, lib.calls = lib.calls, None
        out = model._finalize(res, info, gt_optional=True)
    finally:
        model.mask_boxes = saved
        model.ops.lib.calls = None
    assert set(off) == {"picked_query", "picked_scores", "picked_masks"} and set(on) == set(off) | {"picked_boxes", "picked_areas"}
    assert pick_calls.count("psalm_mask_boxes") == 1 and pick_calls.count("psalm_mask_gather_u8") == 1
    for k in off:
        assert torch.equal(on[k].cpu(), off[k].cpu()), k
    q = on["picked_query"].tolist()
    assert q == [2, 5, EMPTY]
    check_condition(on["picked_masks"].cpu())                                             # (3 picks: two blobs and the empty query)
    wb, wa = np_boxes(on["picked_masks"].cpu())
    pb, pa = on["picked_boxes"], on["picked_areas"]
    assert pb.dtype == torch.float32 and pa.dtype == torch.int32 and pb.device == on["picked_masks"].device and tuple(pb.shape) == (3, 4)
    assert np.array_equal(pb.cpu().numpy(), wb) and np.array_equal(pa.cpu().numpy(), wa)
    assert torch.equal(pb.cpu(), out["instances"].pred_boxes.cpu()[q]) and torch.equal(pa.cpu(), out["instances"].pred_areas.cpu()[q])
    return on


def observe_case(kind, precision="fp32"):
    """crafted discs (and one empty object) through `VideoTracker._observe`: `boxes` of the picked masks; the read-back block is unchanged"""
    from psalm_amd import VideoTracker
    from psalm_amd.synthetic import video_clip_inputs
    from test_14_video_tracker_emu import crafted, disc, frame_tokens
    model = model_for(kind, precision, "region")
    f0 = video_clip_inputs(model.cfg, 1, 3, orig=ORIG)[0]
    tr = f0["seg_info"][0]["transforms"]
    h, w = tr["resize"][:2]
    discs = [disc(h, w, 20, 22, 9), np.zeros((h, w), np.uint8), disc(h, w, 50, 70, 14)]          # the last one is cut by two image edges
    tok = frame_tokens(model, f0["images"])
    saved = model.mask_boxes
    lib = model.ops.lib
    outs, calls, trips = {}, {}, {}
    try:
        for flag in (False, True):
            model.mask_boxes = flag
            lib.calls = []
            with HostTrips() as t:
                outs[flag] = VideoTracker(model)._observe(tok, *crafted(model, discs, (3, 7, 9)), [1, 2, 3], tr)
            calls[flag], trips[flag], lib.calls = lib.calls, t.n, None
    finally:
        model.mask_boxes = saved
        lib.calls = None
    off, on = outs[False], outs[True]
    assert "boxes" not in off and set(on) == set(off) | {"boxes"} and "psalm_mask_boxes" not in calls[False]
    assert [c for c in calls[True] if c != "psalm_mask_boxes"] == calls[False] and calls[True].count("psalm_mask_boxes") == 1
    assert trips[True] == trips[False] == 1                                                # the step's one read-back
    for k, v in off.items():
        assert (torch.equal(on[k].cpu(), v.cpu()) if torch.is_tensor(v) else on[k] == v), k
    picked = on["picked_masks"].cpu()
    assert np.array_equal(picked.numpy(), np.stack(discs))
    check_condition(picked)
    wb, _ = np_boxes(picked)
    assert on["boxes"].dtype == torch.float32 and on["boxes"].device == on["picked_masks"].device
    assert np.array_equal(on["boxes"].cpu().numpy(), wb) and wb[1].tolist() == [0, 0, 0, 0] and wb[2].tolist()[2:] == [80.0, 60.0]
    return on


def e2e_case(kind, precision="fp32"):
    """One call per session path on the tiny model with the switch on (its own masks are empty: this shows the plumbing -- keys, shapes, dtypes,
    device -- and that whatever comes back is consistent with the returned masks)."""
    from click_track_util import geometry, prompts_for
    from interactive_util import prompts_of, regions_for
    from psalm_amd import VideoTracker
    from psalm_amd.synthetic import make_inputs, video_clip_inputs

    def consistent(inst):
        wb, wa = np_boxes(inst.pred_masks.cpu())
        assert inst.pred_boxes.device == inst.pred_masks.device and inst.pred_areas.dtype == torch.int32
        assert np.array_equal(inst.pred_boxes.cpu().numpy(), wb) and np.array_equal(inst.pred_areas.cpu().numpy(), wa)

    pan = model_for(kind, precision, "panoptic")
    reg = model_for(kind, precision, "region")
    saved = (pan.mask_boxes, reg.mask_boxes)
    try:
        pan.mask_boxes = reg.mask_boxes = True
        out = pan.eval_seg(**make_inputs(pan.cfg, "panoptic", size=CANVAS, batch=1, seed=4, num_classes=9))[0]
        consistent(out["instances"])
        for s in out["panoptic_seg"][1]:
            (x0, y0, x1, y1), a = np_box(out["panoptic_seg"][0].cpu() == s["id"])
            assert s["area"] == a and s["bbox"] == [x0, y0, x1 - x0, y1 - y0]
        image, info = image_of(reg.cfg, orig=ORIG, size=CANVAS)
        ids, am = prompts_of(reg.cfg, CANVAS)
        sess = reg.encode_image(image, [info])
        outs = reg.segment(sess, ids, am, regions=regions_for(*ORIG))
        for o_, R in zip(outs, (1, 3)):
            consistent(o_["instances"])
            wb, wa = np_boxes(o_["picked_masks"].cpu())
            assert tuple(o_["picked_boxes"].shape) == (R, 4) and o_["picked_boxes"].device == o_["picked_masks"].device
            assert np.array_equal(o_["picked_boxes"].cpu().numpy(), wb) and np.array_equal(o_["picked_areas"].cpu().numpy(), wa)
        clip = video_clip_inputs(reg.cfg, 2, 2, orig=ORIG)
        trk = VideoTracker(reg)
        trk.start(clip[0]["input_ids"], clip[0]["images"], geometry(clip[0]), regions=prompts_for(2, *ORIG, reg.device),
                  attention_mask=clip[0]["attention_mask"])
        got = trk.track(clip[1]["images"], geometry(clip[1]))
        consistent(got["instances"])
        assert got["boxes"].dtype == torch.float32 and tuple(got["boxes"].shape) == (2, 4) and got["boxes"].device == got["picked_masks"].device
        assert np.array_equal(got["boxes"].cpu().numpy(), np_boxes(got["picked_masks"].cpu())[0])
    finally:
        pan.mask_boxes, reg.mask_boxes = saved
