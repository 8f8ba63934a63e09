"""Cases of segment_everything(min_island=, max_hole=, connectivity=) shared by tests/test_37_segment_everything_clean_emu.py and
tests/test_38_segment_everything_clean_gpu.py (kind: "emu" | "hip").  The yardstick is the numpy pipeline on `segment`'s picks: the cleanup
oracle of tests/components_util.py, then the oracle of tests/everything_util.py (pack, pair counts, NMS, paint, boxes).  Every comparison is for
equality."""
import numpy as np
import pytest
import torch

from components_util import np_clean_many
from everything_util import (DTYPES, assert_everything, assert_same_prompts, bits_np, discs, grid_clicks, np_boxes, np_nms, np_pack, np_paint,
                             np_pair_counts, prompt_ids, session_for)
from interactive_util import model_for, rank_sampler


def oracle_everything_clean(prompts, num, den, min_area, min_score, min_island, max_hole, connectivity):
    """what segment_everything must return under cleaning, in numpy, from what segment(regions=..., pick=True) returned"""
    pm = np.concatenate([p["picked_masks"].cpu().numpy() for p in prompts])
    sc = np.concatenate([p["picked_scores"].cpu().numpy() for p in prompts])
    qq = np.concatenate([p["picked_query"].cpu().numpy() for p in prompts])
    R, Hh, Ww = pm.shape
    cleaned, areas, filled, removed = np_clean_many(pm != 0, min_island, max_hole, connectivity)
    flags = cleaned.reshape(R, -1) != 0
    words = np_pack(flags)
    assert np.array_equal(areas, flags.sum(1))
    kept, keep, owner = np_nms(np_pair_counts(flags, flags), areas, sc, num, den, min_area, min_score)
    idx = kept[1:1 + kept[0]].astype(np.int64)
    boxes, kareas = np_boxes(flags[idx].reshape(-1, Hh, Ww))
    return {"masks": cleaned[idx] != 0, "scores": sc[idx], "queries": qq[idx], "regions": idx, "areas": kareas, "boxes": boxes,
            "labels": np_paint(flags, kept).reshape(Hh, Ww), "owner": owner.astype(np.int64), "keep": keep,
            "cleaned": np.stack([removed, filled], 1).astype(np.int32), "_words": words}


def assert_everything_clean(out, want, device):
    assert_everything(out, want, device)
    c = out["cleaned"]
    assert c.dtype == torch.int32 and c.device.type == device.type and c.is_contiguous()
    assert np.array_equal(c.cpu().numpy(), want["cleaned"]), (c.cpu().numpy(), want["cleaned"])


def defaults_case(kind):
    """min_island = max_hole = 0 is the call without them: equal tensors for every key, no `cleaned`, the same launches of the device step in the
    same order"""
    model, sess, info = session_for(kind)
    ids, am = prompt_ids(model.cfg, (5, 7))
    lib = model.ops.lib
    runs = []
    for kw in ({}, {"min_island": 0, "max_hole": 0, "connectivity": 4}):
        lib.calls = []
        try:
            out = model.segment_everything(sess, ids, am, grid=(3, 4), min_area=0, region_index_sampler=rank_sampler, **kw)
            runs.append((out, list(lib.calls)))
        finally:
            lib.calls = None
    (a, calls_a) = runs[0]
    assert "psalm_mask_clean" not in calls_a and "psalm_mask_components" not in calls_a
    for b, calls_b in runs[1:]:
        assert set(a) == set(b) == set(DTYPES) | {"prompts"}
        for k in DTYPES:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
        assert_same_prompts(b["prompts"], a["prompts"])
        # launch for launch: everything from the first pack on (in front of it run a built the session's prefix cache and run b found it)
        assert calls_b[calls_b.index("psalm_mask_pack_bits"):] == calls_a[calls_a.index("psalm_mask_pack_bits"):]


def planted_prompts(model, counts=(5, 7), shape=(70, 150)):
    """Picks that are not the tiny model's (its masks are empty at any size, so they hold neither speck nor hole): overlapping discs with
    planted specks (1 .. 3 pixels, away from the disc or not) and pin-holes (1 .. 2 pixels inside the disc), as two prompts of 5 and 7 regions;
    the last region of each prompt picks the first one's query: an exact duplicate."""
    Q, prompts = model.cfg.md_queries, []
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(17)
    H, W = shape
    for b, k in enumerate(counts):
        m = discs(Q, H, W, 40 + b, rmin=15, rmax=45).astype(np.float32)
        for q in range(Q):
            for _ in range(6):                                     # specks: a pixel, a domino or an L of three
                y, x = rng.integers(1, H - 1), rng.integers(1, W - 1)
                m[q, y, x] = 1
                if rng.random() < 0.5:
                    m[q, y, x + 1] = 1
                    if rng.random() < 0.5:
                        m[q, y + 1, x] = 1
            ys, xs = np.nonzero(m[q, 1:-1, 1:-2])
            for j in rng.integers(0, len(ys), 5):                  # pin-holes
                m[q, ys[j] + 1, xs[j] + 1] = 0
                if rng.random() < 0.5:
                    m[q, ys[j] + 1, xs[j] + 2] = 0
        masks = torch.from_numpy(m).to(model.device)
        scores = torch.rand(Q, k, generator=g)
        scores[:, k - 1] = scores[:, 0]
        p = model._region_pick({"_pending": ("region", scores.to(model.device), masks, None)})
        p["instances"] = type("I", (), {"scores": scores, "pred_masks": masks})()
        prompts.append(p)
    return prompts, counts


def planted_case(kind, thr=(3, 10), min_area=1, min_score=None, min_island=4, max_hole=2, connectivity=8):
    """the device step on planted picks == the numpy pipeline; at least one click loses a speck and one gets a hole filled"""
    model = model_for(kind, "fp32")
    prompts, counts = planted_prompts(model)
    lib = model.ops.lib
    lib.calls = []
    try:
        out = model._everything_dedup(prompts, counts, thr[0], thr[1], min_area, min_score, min_island, max_hole, connectivity)
        calls = list(lib.calls)
    finally:
        lib.calls = None
    want = oracle_everything_clean(prompts, thr[0], thr[1], min_area, min_score, min_island, max_hole, connectivity)
    assert_everything_clean(out, want, model.device)
    if min_island:
        assert want["cleaned"][:, 0].max() > 0
    if max_hole:
        assert want["cleaned"][:, 1].max() > 0
    raw = np.concatenate([p["picked_masks"].cpu().numpy() for p in prompts]) != 0
    assert (raw.reshape(len(raw), -1).sum(1) != np_clean_many(raw, min_island, max_hole, connectivity)[1]).any()
    assert calls.count("psalm_mask_clean") == len(counts) and calls.count("psalm_mask_pack_bits") == 1
    for name in ("psalm_mask_pair_counts", "psalm_mask_nms", "psalm_mask_paint_bits"):
        assert calls.count(name) == 1, (name, calls.count(name))
    assert (want["keep"] == 1).sum() >= 2 and (want["keep"] == 0).sum() >= 1, want["keep"]
    # the packed words of the cleaned buffer, through the public op: the same planes give the oracle's words
    cleaned, areas, filled, removed = model.ops.mask_clean(
        torch.cat([p["picked_masks"] for p in prompts]), connectivity=connectivity, min_island=min_island, max_hole=max_hole)
    assert np.array_equal(bits_np(model.ops.mask_pack_bits(cleaned)[0]), want["_words"])
    return out, want


def model_path_case(kind, precision="fp32"):
    """through the public call on the tiny region model: segment_everything(min_island=, max_hole=) == the numpy pipeline on the picks of
    `segment` with the same clicks (the tiny model's masks are empty: nothing changes, `cleaned` is zero, the path is the cleaning one)"""
    from psalm_amd.evalout import iou_fraction
    model, sess, info = session_for(kind, precision)
    h, w = info["transforms"]["resize"][:2]
    counts = (5, 7)
    ids, am = prompt_ids(model.cfg, counts)
    out = model.segment_everything(sess, ids, am, grid=(3, 4), min_area=0, min_island=3, max_hole=2, connectivity=4,
                                   region_index_sampler=rank_sampler)
    want_prompts = model.segment(sess, ids, am, regions=grid_clicks(h, w, 3, 4, counts), region_index_sampler=rank_sampler, pick=True)
    assert_same_prompts(out["prompts"], want_prompts)
    want = oracle_everything_clean(want_prompts, *iou_fraction(0.7), 0, None, 3, 2, 4)
    assert_everything_clean(out, want, model.device)
    assert tuple(out["cleaned"].shape) == (12, 2)


def errors_case(kind):
    model, sess, info = session_for(kind)
    ids, am = prompt_ids(model.cfg, (12,))
    builds, hits = sess.prefix_builds, sess.prefix_hits
    for kw, match in (({"min_island": -1}, "min_island"), ({"max_hole": -2}, "max_hole"), ({"min_island": 1.5}, "min_island"),
                      ({"max_hole": True}, "max_hole"), ({"min_island": 3, "connectivity": 6}, "connectivity"), ({"connectivity": 0}, "connectivity"),
                      ({"connectivity": None}, "connectivity")):
        with pytest.raises(ValueError, match=match):
            model.segment_everything(sess, ids, am, grid=(3, 4), region_index_sampler=rank_sampler, **kw)
    assert (sess.prefix_builds, sess.prefix_hits) == (builds, hits)                   # none of these reached the pipeline
