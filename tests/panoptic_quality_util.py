"""Helpers of the panoptic-quality tests (tests/test_46_label_pairs_kernels.py, test_47_panoptic_quality_emu.py, test_48_panoptic_quality_gpu.py).

The oracle restates panopticapi's `pq_compute_single_core` and `pq_average` literally -- dicts, `np.unique(gt.astype(np.uint64) * 256**3 + pred,
return_counts=True)`, a float `iou > 0.5` -- on numpy copies of the maps.  Where it departs from panopticapi, so that the bookkeeping can be
compared too: a segment's area is counted from its map (panopticapi trusts the JSON's `area` for the ground truth); pixels of an id that no record
lists are totalled in `notes` instead of raising KeyError; a listed prediction without a pixel is totalled and passed over instead of raising; a
group without any class averages to 0 instead of dividing by zero.  The pair-count oracle is a second, independent one (np.searchsorted +
np.bincount), because ids beyond 2^24 and negative values do not survive the `* 256**3` packing.  Every comparison of the tests is exact."""
import numpy as np
import torch

OFFSET = 256 ** 3
VOID = 0
HAND_CATEGORIES = {1: True, 2: True, 3: False}


# ---------------------------------------------------------------------------------------------------------------- oracles
def np_rgb2id(a):
    a = np.asarray(a)
    if a.ndim == 3:
        a = a.astype(np.int64)
        return a[..., 0] + 256 * a[..., 1] + 65536 * a[..., 2]
    return a.astype(np.int64)


def np_id2rgb(ids):
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=-1).astype(np.uint8)


def np_slots(m, ids_sorted):
    """slot of every pixel under the ascending table: 0 = VOID, 1 + k = ids_sorted[k], n + 1 = anything else"""
    m = np_rgb2id(m)
    t = np.asarray(ids_sorted, np.int64)
    n = t.size
    k = np.searchsorted(t, m)
    hit = (k < n) & (t[np.minimum(k, max(n - 1, 0))] == m) if n else np.zeros(m.shape, bool)
    return np.where(m == 0, 0, np.where(hit, 1 + k, n + 1))


def np_pair_counts(gt, gt_ids_sorted, pred, pred_ids_sorted):
    G, P = len(gt_ids_sorted), len(pred_ids_sorted)
    a, b = np_slots(gt, gt_ids_sorted), np_slots(pred, pred_ids_sorted)
    return np.bincount((a * (P + 2) + b).reshape(-1), minlength=(G + 2) * (P + 2)).reshape(G + 2, P + 2).astype(np.int32)


def new_stat(categories):
    return {c: {"tp": 0, "fp": 0, "fn": 0, "iou": 0.0} for c in categories}, {"images": 0, "unlisted_gt_pixels": 0, "unlisted_pred_pixels": 0,
                                                                               "empty_pred_segments": 0}


def pq_single(stat, notes, gt, gt_segments_info, pred, pred_segments_info):
    """pq_compute_single_core for one image, added to `stat` / `notes` in place.  The records' category_id are dataset ids (keys of stat)."""
    pan_gt, pan_pred = np_rgb2id(gt), np_rgb2id(pred)
    gt_segms = {el["id"]: dict(el) for el in gt_segments_info}
    pred_segms = {el["id"]: dict(el) for el in pred_segments_info}
    for segms, pan, note in ((gt_segms, pan_gt, "unlisted_gt_pixels"), (pred_segms, pan_pred, "unlisted_pred_pixels")):
        labels, labels_cnt = np.unique(pan, return_counts=True)
        for el in segms.values():
            el["area"] = 0
        for label, label_cnt in zip(labels.tolist(), labels_cnt.tolist()):
            if label in segms:
                segms[label]["area"] = label_cnt
            elif label != VOID:
                notes[note] += label_cnt
    notes["images"] += 1
    for label in [k for k, el in pred_segms.items() if el["area"] == 0]:
        notes["empty_pred_segments"] += 1
        del pred_segms[label]

    pan_gt_pred = pan_gt.astype(np.uint64) * OFFSET + pan_pred.astype(np.uint64)
    gt_pred_map = {}
    labels, labels_cnt = np.unique(pan_gt_pred, return_counts=True)
    for label, intersection in zip(labels.tolist(), labels_cnt.tolist()):
        gt_pred_map[(label // OFFSET, label % OFFSET)] = intersection

    gt_matched, pred_matched = set(), set()
    for (gt_label, pred_label), intersection in gt_pred_map.items():
        if gt_label not in gt_segms:
            continue
        if pred_label not in pred_segms:
            continue
        if gt_segms[gt_label].get("iscrowd", 0) == 1:
            continue
        if gt_segms[gt_label]["category_id"] != pred_segms[pred_label]["category_id"]:
            continue
        union = pred_segms[pred_label]["area"] + gt_segms[gt_label]["area"] - intersection - gt_pred_map.get((VOID, pred_label), 0)
        iou = intersection / union
        if iou > 0.5:
            stat[gt_segms[gt_label]["category_id"]]["tp"] += 1
            stat[gt_segms[gt_label]["category_id"]]["iou"] += iou
            gt_matched.add(gt_label)
            pred_matched.add(pred_label)

    crowd_labels_dict = {}
    for gt_label, gt_info in gt_segms.items():
        if gt_label in gt_matched:
            continue
        if gt_info.get("iscrowd", 0) == 1:
            crowd_labels_dict[gt_info["category_id"]] = gt_label
            continue
        stat[gt_info["category_id"]]["fn"] += 1

    for pred_label, pred_info in pred_segms.items():
        if pred_label in pred_matched:
            continue
        intersection = gt_pred_map.get((VOID, pred_label), 0)
        if pred_info["category_id"] in crowd_labels_dict:
            intersection += gt_pred_map.get((crowd_labels_dict[pred_info["category_id"]], pred_label), 0)
        if intersection / pred_info["area"] > 0.5:
            continue
        stat[pred_info["category_id"]]["fp"] += 1


def pq_average(stat, categories, isthing):
    pq, sq, rq, n = 0, 0, 0, 0
    per_class_results = {}
    for label, label_isthing in categories.items():
        if isthing is not None:
            if label_isthing != isthing:
                continue
        iou, tp, fp, fn = stat[label]["iou"], stat[label]["tp"], stat[label]["fp"], stat[label]["fn"]
        if tp + fp + fn == 0:
            per_class_results[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
            continue
        n += 1
        pq_class = iou / (tp + 0.5 * fp + 0.5 * fn)
        sq_class = iou / tp if tp != 0 else 0
        rq_class = tp / (tp + 0.5 * fp + 0.5 * fn)
        per_class_results[label] = {"pq": pq_class, "sq": sq_class, "rq": rq_class}
        pq += pq_class
        sq += sq_class
        rq += rq_class
    if n == 0:
        return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class_results
    return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class_results


def pq_results(stat, notes, categories):
    """pq_compute's result in the shape of PanopticQuality.results()"""
    out = {"notes": dict(notes)}
    for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
        out[name], per_class = pq_average(stat, categories, isthing)
        if isthing is None:
            out["per_class"] = per_class
    return out


def oracle_of(scenes, categories):
    stat, notes = new_stat(categories)
    for sc in scenes:
        pq_single(stat, notes, to_np(sc["gt"]), sc["gt_info"], to_np(sc["pred"]), sc["pred_info"])
    return stat, notes


def to_np(m):
    return m.cpu().numpy() if torch.is_tensor(m) else np.asarray(m)


def stat_arrays(stat, notes, categories):
    """the oracle's dicts as the device accumulators: stat (C,3) int64, iou (C) float64, notes (4) int64"""
    s = np.array([[stat[c]["tp"], stat[c]["fp"], stat[c]["fn"]] for c in categories], np.int64).reshape(-1, 3)
    i = np.array([stat[c]["iou"] for c in categories], np.float64)
    n = np.array([notes[k] for k in ("images", "unlisted_gt_pixels", "unlisted_pred_pixels", "empty_pred_segments")], np.int64)
    return s, i, n


def kernel_tables(scene, categories):
    """The small tables `psalm_pq_accumulate` takes, built here independently of evalout: sorted ids, category slots, crowd flags, crowd slots."""
    slot = {c: k for k, c in enumerate(categories)}
    g = sorted(scene["gt_info"], key=lambda s: s["id"])
    p = sorted(scene["pred_info"], key=lambda s: s["id"])
    gs, ps = [s["id"] for s in g], [s["id"] for s in p]
    crowd = {}
    for s in scene["gt_info"]:                                  # JSON order: the later crowd segment of a category wins
        if s.get("iscrowd", 0) == 1:
            crowd[s["category_id"]] = 1 + gs.index(s["id"])
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    return {"gt_ids": i32(gs), "pred_ids": i32(ps), "gt_cat": i32([slot[s["category_id"]] for s in g]),
            "gt_crowd": i32([1 if s.get("iscrowd", 0) == 1 else 0 for s in g]), "pred_cat": i32([slot[s["category_id"]] for s in p]),
            "pred_crowd_slot": i32([crowd.get(s["category_id"], -1) for s in p])}


# ---------------------------------------------------------------------------------------------------------------- cases
def hand_case():
    gt = np.array([[10, 10, 10, 20, 20, 20], [10, 10, 10, 20, 20, 20], [30, 30, 30, 30, 0, 0], [30, 30, 30, 30, 0, 0]], np.int32)
    pred = np.array([[1, 1, 1, 1, 2, 2], [1, 1, 0, 0, 2, 2], [3, 3, 3, 3, 4, 4], [3, 3, 3, 5, 4, 4]], np.int32)
    gt_info = [{"id": 10, "category_id": 1, "iscrowd": 0}, {"id": 20, "category_id": 2, "iscrowd": 1}, {"id": 30, "category_id": 3, "iscrowd": 0}]
    pred_info = [{"id": 1, "category_id": 1}, {"id": 2, "category_id": 2}, {"id": 3, "category_id": 3}, {"id": 4, "category_id": 1},
                 {"id": 5, "category_id": 3}]
    return {"gt": gt, "gt_info": gt_info, "pred": pred, "pred_info": pred_info}


HAND_STAT = {1: {"tp": 1, "fp": 0, "fn": 0, "iou": 5 / 7}, 2: {"tp": 0, "fp": 0, "fn": 0, "iou": 0.0}, 3: {"tp": 1, "fp": 1, "fn": 0, "iou": 7 / 8}}


def check_oracle_on_hand_case():
    stat, notes = oracle_of([hand_case()], HAND_CATEGORIES)
    assert stat == HAND_STAT, stat
    assert notes == {"images": 1, "unlisted_gt_pixels": 0, "unlisted_pred_pixels": 0, "empty_pred_segments": 0}
    res = pq_results(stat, notes, HAND_CATEGORIES)
    assert res["All"]["pq"] == (5 / 7 + 7 / 12) / 2 and res["All"]["n"] == 2
    assert res["Things"]["pq"] == 5 / 7 and res["Stuff"]["pq"] == 7 / 12 and res["Stuff"]["rq"] == 2 / 3
    return stat, notes


def scene(gt, gt_info, pred, pred_info):
    return {"gt": np.asarray(gt, np.int32), "gt_info": gt_info, "pred": np.asarray(pred, np.int32), "pred_info": pred_info}


def edge_cases():
    """name -> (scene, categories): the knife edges of the rule"""
    cats = {7: True, 8: False}
    seg = lambda i, c, crowd=0: {"id": i, "category_id": c, "iscrowd": crowd}
    out = {}
    # IoU exactly 1/2: a gt of 2 pixels, a prediction of 1 pixel inside it -> no match: FN + FP
    out["iou_half"] = (scene([[5, 5, 0]], [seg(5, 7)], [[9, 0, 0]], [seg(9, 7)]), cats)
    # a false-positive share of exactly 1/2 on VOID: it is NOT forgiven
    out["fp_half"] = (scene([[0, 0, 5, 5]], [seg(5, 8)], [[9, 9, 9, 9]], [seg(9, 7)]), cats)
    # ... and just above 1/2 it is
    out["fp_forgiven"] = (scene([[0, 0, 0, 5, 5]], [seg(5, 8)], [[9, 9, 9, 9, 9]], [seg(9, 7)]), cats)
    # a listed gt without a pixel: FN
    out["gt_no_pixel"] = (scene([[5, 5, 5]], [seg(5, 7), seg(6, 8)], [[9, 9, 9]], [seg(9, 7)]), cats)
    # a listed prediction without a pixel: notes only
    out["pred_no_pixel"] = (scene([[5, 5, 5]], [seg(5, 7)], [[9, 9, 9]], [seg(9, 7), seg(4, 8), seg(11, 7)]), cats)
    # two crowd segments of one category: the later one in JSON order (id 3, listed after id 6) is the one that forgives
    g = [[6, 6, 6, 6, 3, 3, 3, 3]]
    p = [[1, 1, 1, 1, 2, 2, 2, 2]]
    out["two_crowds"] = (scene(g, [seg(6, 7, 1), seg(3, 7, 1)], p, [seg(1, 7), seg(2, 7)]), cats)
    out["two_crowds_other_order"] = (scene(g, [seg(3, 7, 1), seg(6, 7, 1)], p, [seg(1, 7), seg(2, 7)]), cats)
    # unlisted ids on both sides
    out["unlisted"] = (scene([[5, 5, 77, 77]], [seg(5, 7)], [[9, 9, 9, 88]], [seg(9, 7)]), cats)
    return out


def voronoi(rng, H, W, n):
    """(H,W) int64 of region indices 0..n-1 around n random sites"""
    ys, xs = rng.integers(0, H, n), rng.integers(0, W, n)
    yy, xx = np.mgrid[:H, :W]
    return np.argmin((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2, axis=-1)


def random_scene(rng, H, W, categories, n_gt=5, n_pred=6, big_ids=False):
    """A ground truth of Voronoi regions, some crowd, some VOID, some listed without a pixel; a prediction that is the ground truth shifted, with a
    few regions re-split, its categories mostly right."""
    cats = list(categories)
    top = 2 ** 24 - 1 if big_ids else 400
    g_reg = voronoi(rng, H, W, n_gt)
    g_ids = rng.choice(np.arange(1, top), n_gt + 1, replace=False).astype(np.int64)
    gt = g_ids[g_reg]
    if rng.random() < 0.7:
        gt[g_reg == 0] = 0                                      # a VOID region
    g_cat = rng.choice(cats, n_gt + 1)
    gt_info = [{"id": int(g_ids[k]), "category_id": int(g_cat[k]), "iscrowd": int(rng.random() < 0.25)} for k in range(n_gt + 1) if 0 < k < n_gt or rng.random() < 0.5]   # (region 0 may go unlisted; id n_gt has no pixel)
    rng.shuffle(gt_info)
    shifted = np.roll(g_reg, (int(rng.integers(-1, 2)), int(rng.integers(-2, 3))), axis=(0, 1))
    split = voronoi(rng, H, W, n_pred)
    p_reg = np.where(rng.random(n_gt)[shifted] < 0.6, shifted, n_gt + split)
    uniq = np.unique(p_reg)
    p_ids = rng.choice(np.arange(1, top), uniq.size + 1, replace=False).astype(np.int64)
    lut = np.zeros(n_gt + n_pred, np.int64)
    lut[uniq] = p_ids[:uniq.size]
    pred = lut[p_reg]
    if rng.random() < 0.5:
        pred[split == 0] = 0
    pred_info = []
    for k, r in enumerate(uniq.tolist()):
        right = r < n_gt and rng.random() < 0.8
        pred_info.append({"id": int(p_ids[k]), "category_id": int(g_cat[r]) if right else int(rng.choice(cats))})
    if rng.random() < 0.3:
        pred_info.append({"id": int(p_ids[-1]), "category_id": int(rng.choice(cats))})          # listed, no pixel
    rng.shuffle(pred_info)
    return scene(gt, gt_info, pred, pred_info)


def random_scenes(n, seed=0, H=9, W=13, categories=None, **kw):
    rng = np.random.default_rng(seed)
    categories = categories or RANDOM_CATEGORIES
    return [random_scene(rng, H, W, categories, **kw) for _ in range(n)]


RANDOM_CATEGORIES = {11: True, 12: True, 13: False, 17: False, 40: True}


# ---------------------------------------------------------------------------------------------------------------- checks shared by emu / gpu
def assert_results_equal(got, want):
    assert got["notes"] == want["notes"], (got["notes"], want["notes"])
    for k in ("All", "Things", "Stuff"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["per_class"] == want["per_class"]


def meter_for(ops, categories):
    from psalm_amd import evalout as E
    return E.PanopticQuality(categories, ops=ops)


def feed(meter, sc, device=None, rgb=False, **kw):
    gt, pred = torch.from_numpy(np_id2rgb(sc["gt"]) if rgb else sc["gt"]), torch.from_numpy(sc["pred"])
    if device is not None:
        gt, pred = gt.to(device), pred.to(device)
    meter.update(pred, sc["pred_info"], gt, sc["gt_info"], **kw)


def meter_case(ops, scenes, categories, on_device=True, rgb=False):
    """a meter fed the scenes == the oracle fed the scenes: integers exact, floats =="""
    m = meter_for(ops, categories)
    for sc in scenes:
        feed(m, sc, ops.device if on_device else None, rgb=rgb)
    stat, notes = oracle_of(scenes, categories)
    s, i, n = stat_arrays(stat, notes, categories)
    assert np.array_equal(m.stat.cpu().numpy(), s) and np.array_equal(m.notes.cpu().numpy(), n)
    assert np.array_equal(m.iou.cpu().numpy().view(np.int64), i.view(np.int64))
    assert_results_equal(m.results(strict=False), pq_results(stat, notes, categories))
    return m


def derived_ground_truth(pan, segs, category_ids):
    """A ground truth derived from a panoptic result: the id map shifted by (2, 3) (VOID where the shift leaves the image), the first two segments
    merged into one, the last one marked crowd; dataset category ids through `category_ids`."""
    pan = to_np(pan).astype(np.int32)
    gt = np.zeros_like(pan)
    gt[2:, 3:] = pan[:-2, :-3]
    ids = [s["id"] for s in segs]
    assert len(ids) >= 3
    gt[gt == ids[1]] = ids[0]
    info = [{"id": 100 + s["id"], "category_id": int(category_ids[s["category_id"]]), "iscrowd": int(s["id"] == ids[-1])} for s in segs if s["id"] != ids[1]]
    return np.where(gt > 0, gt + 100, 0).astype(np.int32), info


def real_result_case(kind, precision="fp32"):
    """`panoptic_seg` of the crafted-predictor case of tests/mask_boxes_util.py against a ground truth derived from it: the meter == the oracle on
    `.cpu()` copies, directly and through compact_results(pq=, gt_panoptic=)."""
    import mask_boxes_util as MB
    from psalm_amd import evalout as E
    on = MB.task_case(kind, precision, "panoptic")
    pan, segs = on["panoptic_seg"]
    cat_ids = [10 * (c + 1) for c in range(MB.N_CLASSES["panoptic"])]
    categories = {c: bool(t) for c, t in zip(cat_ids, MB.THING)}
    gt, gt_info = derived_ground_truth(pan, segs, cat_ids)
    ops = MB.model_for(kind, precision, "panoptic").ops
    stat, notes = new_stat(categories)
    pq_single(stat, notes, gt, gt_info, to_np(pan), [dict(s, category_id=cat_ids[s["category_id"]]) for s in segs])
    assert sum(v["tp"] for v in stat.values()) >= 1 and notes["unlisted_pred_pixels"] == 0
    want = pq_results(stat, notes, categories)
    gt_dev = torch.from_numpy(gt).to(ops.device)
    m = E.PanopticQuality(categories, ops=ops)
    m.update(pan, segs, gt_dev, gt_info, category_ids=cat_ids)
    assert_results_equal(m.results(), want)
    m2 = E.PanopticQuality(categories, ops=ops)
    plain = E.compact_results(on, ops=ops)
    comp = E.compact_results(on, ops=ops, pq=m2, gt_panoptic=(gt_dev, gt_info), category_ids=cat_ids)
    assert set(comp) == set(plain) and torch.equal(comp["panoptic_rgb"].cpu(), plain["panoptic_rgb"].cpu())
    assert_results_equal(m2.results(), want)
    m3 = E.PanopticQuality(categories, ops=ops)                                   # the ground truth as the PNG's RGB array
    m3.update(pan, segs, np_id2rgb(gt), gt_info, category_ids=cat_ids)
    assert_results_equal(m3.results(), want)
    return want


def hand_meter_case(kind):
    from ops_backend import make_ops
    ops = make_ops(kind)
    m = meter_case(ops, [hand_case()], HAND_CATEGORIES)
    res = m.results()
    assert res["All"] == {"pq": (5 / 7 + 7 / 12) / 2, "sq": (5 / 7 + 7 / 8) / 2, "rq": (1.0 + 2 / 3) / 2, "n": 2}
    assert res["Things"]["pq"] == 5 / 7 and res["Things"]["n"] == 1 and res["Stuff"] == {"pq": 7 / 12, "sq": 7 / 8, "rq": 2 / 3, "n": 1}
    assert res["per_class"][2] == {"pq": 0.0, "sq": 0.0, "rq": 0.0} and res["notes"]["images"] == 1
    meter_case(ops, [hand_case()], HAND_CATEGORIES, on_device=False)             # host maps are moved
    meter_case(ops, [hand_case()], HAND_CATEGORIES, rgb=True)                    # the ground truth as the PNG's RGB array
    rec = meter_for(ops, {c: {"isthing": int(t), "name": str(c)} for c, t in HAND_CATEGORIES.items()})               # panopticapi's category records
    feed(rec, hand_case(), ops.device)
    assert_results_equal(rec.results(), res)
    return res


def random_meter_case(kind, n=12, shape=(33, 65), big=(130, 70)):
    """meters fed several images == the oracle fed the same images; the last scene at the larger size, ids up to 2^24 - 1 through RGB"""
    from ops_backend import make_ops
    ops = make_ops(kind)
    scenes = random_scenes(n, seed=47, H=shape[0], W=shape[1], n_gt=9, n_pred=11)
    meter_case(ops, scenes[:1], RANDOM_CATEGORIES)
    meter_case(ops, scenes[:2], RANDOM_CATEGORIES)                               # two images == the oracle fed both
    meter_case(ops, scenes, RANDOM_CATEGORIES)
    large = random_scenes(2, seed=48, H=big[0], W=big[1], n_gt=30, n_pred=40, big_ids=True)
    meter_case(ops, large, RANDOM_CATEGORIES, rgb=True)


def identity_case(kind):
    """pred == gt (no crowd, everything listed): pq = sq = rq = 1 for every class present"""
    from ops_backend import make_ops
    ops = make_ops(kind)
    rng = np.random.default_rng(5)
    reg = voronoi(rng, 33, 65, 7)
    cats = list(RANDOM_CATEGORIES)
    info = [{"id": 3 + 5 * k, "category_id": cats[k % 4], "iscrowd": 0} for k in range(7)]
    ids = (3 + 5 * reg).astype(np.int32)
    sc = scene(ids, info, ids, [{"id": s["id"], "category_id": s["category_id"]} for s in info])
    res = meter_case(ops, [sc], RANDOM_CATEGORIES).results()
    for c in cats[:4]:
        assert res["per_class"][c] == {"pq": 1.0, "sq": 1.0, "rq": 1.0}
    assert res["per_class"][cats[4]] == {"pq": 0.0, "sq": 0.0, "rq": 0.0}
    assert res["All"] == {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": 4}


def strict_case(kind):
    import pytest
    from ops_backend import make_ops
    ops = make_ops(kind)
    sc = hand_case()
    sc["pred_info"] = sc["pred_info"][:-1]                                       # id 5 is in the map and not in the records
    m = meter_for(ops, HAND_CATEGORIES)
    feed(m, sc, ops.device)
    with pytest.raises(ValueError, match="does not list"):
        m.results()
    res = m.results(strict=False)
    assert res["notes"]["unlisted_pred_pixels"] == 1
    stat, notes = oracle_of([sc], HAND_CATEGORIES)
    assert_results_equal(res, pq_results(stat, notes, HAND_CATEGORIES))
    with pytest.raises(ValueError, match="not one of"):                          # a category the meter does not know
        m.update(torch.from_numpy(sc["pred"]), [{"id": 1, "category_id": 99}], torch.from_numpy(sc["gt"]), sc["gt_info"])
    with pytest.raises(ValueError, match="twice"):
        m.update(torch.from_numpy(sc["pred"]), [{"id": 1, "category_id": 1}] * 2, torch.from_numpy(sc["gt"]), sc["gt_info"])
    assert int(m.notes.cpu()[0]) == 1                                            # the refused updates left the meter alone


def category_ids_case(kind):
    """predictions carry contiguous class indices; category_ids maps them to the dataset's ids"""
    from ops_backend import make_ops
    ops = make_ops(kind)
    sc = hand_case()
    table = [3, 1, 2]                                                            # contiguous index -> dataset id
    contiguous = dict(sc, pred_info=[dict(s, category_id=table.index(s["category_id"])) for s in sc["pred_info"]])
    m = meter_for(ops, HAND_CATEGORIES)
    feed(m, contiguous, ops.device, category_ids=table)
    stat, notes = oracle_of([sc], HAND_CATEGORIES)
    assert_results_equal(m.results(), pq_results(stat, notes, HAND_CATEGORIES))


def all_reduce_case(kind):
    """Two meters summed by hand -- what the SUM all-reduce does -- against one meter over all images: integers exact; the iou sums within
    rtol 1e-12 (fewer than 1000 additions, each off by at most 2^-53 relative, in another order).  Without a process group all_reduce leaves a
    meter as it is."""
    from ops_backend import make_ops
    ops = make_ops(kind)
    scenes = random_scenes(8, seed=49, H=33, W=65, n_gt=9, n_pred=11)
    one, a, b = (meter_for(ops, RANDOM_CATEGORIES) for _ in range(3))
    for k, sc in enumerate(scenes):
        feed(one, sc, ops.device)
        feed(a if k < 5 else b, sc, ops.device)
    before = (a.stat.clone(), a.iou.clone(), a.notes.clone())
    a.all_reduce()
    assert a.stat.dtype == torch.int64 and a.notes.dtype == torch.int64 and a.iou.dtype == torch.float64 and a.stat.device == before[0].device
    assert torch.equal(a.stat, before[0]) and torch.equal(a.iou, before[1]) and torch.equal(a.notes, before[2])
    a.stat, a.iou, a.notes = a.stat + b.stat, a.iou + b.iou, a.notes + b.notes
    assert torch.equal(a.stat.cpu(), one.stat.cpu()) and torch.equal(a.notes.cpu(), one.notes.cpu())
    assert int(one.stat.sum()) < 1000
    np.testing.assert_allclose(a.iou.cpu().numpy(), one.iou.cpu().numpy(), rtol=1e-12, atol=0)
    ra, ro = a.results(strict=False), one.results(strict=False)
    assert ra["All"]["n"] == ro["All"]["n"] and ra["notes"] == ro["notes"]
    np.testing.assert_allclose(ra["All"]["pq"], ro["All"]["pq"], rtol=1e-12, atol=0)
    feed(a, scenes[0], ops.device)                                               # the reduced meter goes on accumulating
    assert int(a.notes.cpu()[0]) == len(scenes) + 1
