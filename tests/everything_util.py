"""Helpers of the segment-everything tests (tests/test_33_mask_pairs_kernels.py, test_34_segment_everything_emu.py, test_35_segment_everything_gpu.py):
the numpy oracle of csrc/maskpairs.hip -- pack into plane-flat bit words, all-pairs intersections, greedy NMS under the integer IoU rule, the
label map -- and the cases the emulator and the GPU tests share.  Everything is integer-exact: every comparison is for equality."""
import copy

import numpy as np
import pytest
import torch

from interactive_util import image_of, model_for, rank_sampler
from psalm_amd.config import IMAGE_TOKEN_INDEX, REGION_TOKEN_INDEX, SEG_TOKEN_INDEX
from psalm_amd.preprocess import nearest_pad_tables


# ---------------------------------------------------------------------------------------------------- the numpy oracle
def np_set(masks):
    """(n, ...) array -> bool: float32 is set when > 0 (NaN, -0.0, negatives are not), everything else when != 0"""
    masks = np.asarray(masks)
    if masks.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return masks > 0
    return masks != 0


def np_pack(flags):
    """bool (m, HW) -> uint64 (m, nw): word w, bit b = pixel 64 w + b; the last word's tail is zero"""
    m, HW = flags.shape
    nw = (HW + 63) // 64
    padded = np.zeros((m, nw * 64), np.uint8)
    padded[:, :HW] = flags
    return np.packbits(padded.reshape(m, nw, 8, 8), axis=-1, bitorder="little").reshape(m, nw, 8).copy().view("<u8").reshape(m, nw)


def np_pair_counts(a, b):
    """bool (ma, HW), (mb, HW) -> int32 (ma, mb) pixels set in both"""
    return (a.astype(np.int64) @ b.astype(np.int64).T).astype(np.int32)


def np_nms(inter, areas, scores, num, den, min_area=1, min_score=None):
    """the rule of psalm_mask_nms in Python integers -> (kept (m + 1), keep (m), owner (m)) int32"""
    m = len(areas)
    order = sorted(range(m), key=lambda i: (-float(scores[i]), i))
    keep, owner, kept = np.full(m, -1, np.int32), np.full(m, -1, np.int32), []
    for i in order:
        if int(areas[i]) < min_area or (min_score is not None and float(scores[i]) < np.float32(min_score)):
            continue
        by = next((j for j in kept
                   if den * int(inter[i][j]) > num * (int(areas[i]) + int(areas[j]) - int(inter[i][j]))), None)
        if by is None:
            keep[i], owner[i] = 1, i
            kept.append(i)
        else:
            keep[i], owner[i] = 0, by
    block = np.full(m + 1, -1, np.int32)
    block[0] = len(kept)
    block[1:1 + len(kept)] = kept
    return block, keep, owner


def np_paint(flags, kept):
    """bool (m, HW), kept block -> int32 (HW): 1 + the first k whose row kept[1 + k] holds the pixel, 0 for none"""
    labels = np.zeros(flags.shape[1], np.int32)
    for k in range(int(kept[0]) - 1, -1, -1):
        labels[flags[kept[1 + k]]] = k + 1
    return labels


def np_boxes(flags_hw):
    """bool (K, H, W) -> (boxes (K, 4) float32 in the mask_boxes convention, areas (K) int32)"""
    boxes, areas = np.zeros((len(flags_hw), 4), np.float32), np.zeros(len(flags_hw), np.int32)
    for i, m in enumerate(flags_hw):
        ys, xs = np.nonzero(m)
        if len(ys):
            boxes[i] = [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]
        areas[i] = len(ys)
    return boxes, areas


def bits_np(t):
    """an int64 bit tensor -> uint64 numpy"""
    return t.cpu().numpy().view(np.uint64)


def discs(n, H, W, seed, rmin=4, rmax=None):
    """n planes with one random disc each (uint8 0 / 1); neighbouring seeds overlap a lot"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    rmax = rmax or max(rmin + 1, min(H, W) // 3)
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        cy, cx, r = g.integers(0, H), g.integers(0, W), g.integers(rmin, rmax)
        out[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return out


# ---------------------------------------------------------------------------------------------------- segment_everything cases (kind: "emu" | "hip")
def prompt_ids(cfg, counts, seed=4):
    """len(counts) prompts on one image with counts[b] <region> tokens each, built as synthetic.video_clip_inputs builds its one prompt -- text,
    <image>, text, the <region> tokens, text, <seg>, text -- with one leading text for all (segment's rule), right-padded"""
    g = torch.Generator(device="cpu")
    g.manual_seed(3000 + seed)

    def txt(n):
        return torch.randint(5, cfg.vocab_size, (n,), generator=g).tolist()

    head = txt(3) + [IMAGE_TOKEN_INDEX]
    rows = [head + txt(2) + [REGION_TOKEN_INDEX] * k + txt(2) + [SEG_TOKEN_INDEX] + txt(1) for k in counts]
    T = max(len(r) for r in rows)
    ids = torch.zeros(len(rows), T, dtype=torch.int64)
    am = torch.zeros(len(rows), T, dtype=torch.bool)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.tensor(r)
        am[b, :len(r)] = True
    return ids, am


def grid_clicks(h, w, gy, gx, counts, radius=None):
    """the clicks segment_everything(grid=(gy, gx)) makes, as `regions` of segment: row-major cells dealt to the prompts by their token counts"""
    extra = {} if radius is None else {"radius": radius}
    flat = [dict(points=[((2 * i + 1) * h // (2 * gy), (2 * j + 1) * w // (2 * gx))], **extra) for i in range(gy) for j in range(gx)]
    out, g0 = [], 0
    for k in counts:
        out.append(flat[g0:g0 + k])
        g0 += k
    return out


def oracle_everything(prompts, num, den, min_area=1, min_score=None):
    """what segment_everything must return, in numpy, from what segment(regions=..., pick=True) returned"""
    pm = np.concatenate([p["picked_masks"].cpu().numpy() for p in prompts])
    sc = np.concatenate([p["picked_scores"].cpu().numpy() for p in prompts])
    qq = np.concatenate([p["picked_query"].cpu().numpy() for p in prompts])
    R, Hh, Ww = pm.shape
    flags = pm.reshape(R, -1) != 0
    areas = flags.sum(1).astype(np.int32)
    kept, keep, owner = np_nms(np_pair_counts(flags, flags), areas, sc, num, den, min_area, min_score)
    idx = kept[1:1 + kept[0]].astype(np.int64)
    boxes, kareas = np_boxes(flags[idx].reshape(-1, Hh, Ww))
    return {"masks": pm[idx] != 0, "scores": sc[idx], "queries": qq[idx], "regions": idx, "areas": kareas, "boxes": boxes,
            "labels": np_paint(flags, kept).reshape(Hh, Ww), "owner": owner.astype(np.int64), "keep": keep}


DTYPES = {"masks": torch.uint8, "scores": torch.float32, "queries": torch.int64, "regions": torch.int64, "areas": torch.int32,
          "boxes": torch.float32, "labels": torch.int32, "owner": torch.int64, "keep": torch.int32}


def assert_everything(out, want, device):
    for k, dt in DTYPES.items():
        assert out[k].dtype == dt and out[k].device.type == device.type, (k, out[k].dtype, out[k].device)
        got = out[k].cpu().numpy()
        w = want[k].astype(got.dtype) if k == "masks" else want[k]
        assert got.shape == w.shape and np.array_equal(got, w), (k, got, w)


def assert_same_prompts(got, want):
    """two lists of segment results: the same bits"""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert set(a) == set(b)
        assert torch.equal(a["mask_pred"].cpu(), b["mask_pred"].cpu())
        assert torch.equal(a["instances"].pred_masks.cpu(), b["instances"].pred_masks.cpu())
        assert torch.equal(a["instances"].scores.cpu(), b["instances"].scores.cpu())
        for k in ("picked_query", "picked_scores", "picked_masks"):
            assert torch.equal(a[k].cpu(), b[k].cpu()), k


def session_for(kind, precision="fp32", seed=4):
    model = model_for(kind, precision)
    img, info = image_of(model.cfg, orig=(60, 80), size=96, seed=seed)
    return model, model.encode_image(img, info), info


def equality_case(kind, counts, precision="fp32", iou_thr=0.7, min_area=1, min_score=None):
    """segment_everything(grid=(3, 4)) == the numpy oracle on segment(regions=<the same clicks>, pick=True) of a second call under the same
    sampler, in every key; out["prompts"] == that segment call bit for bit; one read-back-free launch of each post-step kernel"""
    from psalm_amd.evalout import iou_fraction
    model, sess, info = session_for(kind, precision)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompt_ids(model.cfg, counts)
    assert sum(counts) == 12
    lib = model.ops.lib
    lib.calls = []
    try:
        out = model.segment_everything(sess, ids, am, grid=(3, 4), iou_thr=iou_thr, min_area=min_area, min_score=min_score,
                                       region_index_sampler=rank_sampler)
        calls = lib.calls
    finally:
        lib.calls = None
    want_prompts = model.segment(sess, ids, am, regions=grid_clicks(h, w, 3, 4, counts), region_index_sampler=rank_sampler, pick=True)
    assert_same_prompts(out["prompts"], want_prompts)
    want = oracle_everything(want_prompts, *iou_fraction(iou_thr), min_area=min_area, min_score=min_score)
    assert_everything(out, want, model.device)
    K = len(want["regions"])
    assert calls.count("psalm_mask_pack_bits") == len(counts)
    for name in ("psalm_mask_pair_counts", "psalm_mask_nms", "psalm_mask_paint_bits"):
        assert calls.count(name) == 1, (name, calls.count(name))
    assert calls.count("psalm_mask_unpack_bits") == (1 if K else 0)
    return out, want


def same_click_twice_case(kind):
    """the SAME click as two tokens with identical geometry: both columns of the scores are bit-identical, both pick the same query, so the
    second click is a duplicate of the first -- whatever the synthetic weights predict"""
    model, sess, info = session_for(kind)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompt_ids(model.cfg, (2,))
    click = {"points": [(h // 2, w // 2)]}
    out = model.segment_everything(sess, ids, am, grid=None, regions=[[click, dict(click)]], region_index_sampler=rank_sampler)
    sc = out["prompts"][0]["instances"].scores.cpu().numpy()
    assert sc.shape[1] == 2 and np.array_equal(sc[:, 0], sc[:, 1]), "the two clicks' score columns differ: the prompt side is not deterministic"
    q = out["prompts"][0]["picked_query"].tolist()
    assert q[0] == q[1]
    area = int((out["prompts"][0]["picked_masks"][0] != 0).sum())           # the read-back area decides which structure is due
    if area > 0:
        assert out["keep"].tolist() == [1, 0] and out["owner"].tolist() == [0, 0]
        assert out["regions"].tolist() == [0] and out["areas"].tolist() == [area] and tuple(out["masks"].shape[:1]) == (1,)
        assert int(out["labels"].max()) == 1
    else:
        assert out["keep"].tolist() == [-1, -1] and out["owner"].tolist() == [-1, -1]
        assert out["regions"].tolist() == [] and tuple(out["masks"].shape) == (0,) + tuple(out["labels"].shape)
        assert int(out["labels"].max()) == 0
    return area


def crafted_picks_case(kind, thr=(3, 10), min_area=1, min_score=None):
    """the device step of segment_everything on picks that are not this tiny model's (its masks are empty and its scores zero): two prompts of
    5 and 7 regions over overlapping discs at (70, 150), two regions picking the same query -- the oracle keeps several and suppresses several"""
    model = model_for(kind, "fp32")
    Q, counts, prompts = model.cfg.md_queries, (5, 7), []
    g = torch.Generator().manual_seed(5)
    for b, k in enumerate(counts):
        masks = torch.from_numpy(discs(Q, 70, 150, 40 + b, rmin=15, rmax=45)).float().to(model.device)
        scores = torch.rand(Q, k, generator=g)
        scores[:, k - 1] = scores[:, 0]                          # the last region picks the first one's query: an exact duplicate
        p = model._region_pick({"_pending": ("region", scores.to(model.device), masks, None)})
        p["instances"] = type("I", (), {"scores": scores, "pred_masks": masks})()
        prompts.append(p)
    out = model._everything_dedup(prompts, counts, thr[0], thr[1], min_area, min_score)
    want = oracle_everything(prompts, thr[0], thr[1], min_area, min_score)
    assert_everything(out, want, model.device)
    keep = want["keep"]
    assert (keep == 1).sum() >= 2 and (keep == 0).sum() >= 1, keep
    owner = want["owner"]                                       # the duplicates share their originals' owner and are never kept themselves
    assert owner[4] == owner[0] and owner[11] == owner[5] and keep[4] < 1 and keep[11] < 1
    return want


def errors_case(kind):
    model, sess, info = session_for(kind)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompt_ids(model.cfg, (12,))
    good = grid_clicks(h, w, 3, 4, (12,))
    model.segment(sess, ids, am, regions=good, region_index_sampler=rank_sampler)      # the prefix cache exists from here on
    builds, hits = sess.prefix_builds, sess.prefix_hits

    def fails(match, ids_=ids, **kw):
        kw.setdefault("region_index_sampler", rank_sampler)
        with pytest.raises(ValueError, match=match):
            model.segment_everything(sess, ids_, am if ids_ is ids else None, **kw)

    fails("either `grid` or `regions`", grid=(3, 4), regions=good)
    fails("either `grid` or `regions`", grid=None)
    fails("gy \\* gx", grid=(3, 3))
    fails("gy \\* gx", grid=(12,))
    fails("gy \\* gx", grid=(0, 12))
    for bad in (0.0, 1.5, -0.2, float("nan"), (0, 3), (4, 3), (1, 5000)):
        fails("iou_thr", grid=(3, 4), iou_thr=bad)
    fails("radius", grid=None, regions=good, radius=3)
    no_tokens = ids.clone()
    no_tokens[no_tokens == REGION_TOKEN_INDEX] = 7
    fails("0 <region> tokens", ids_=no_tokens, grid=(1, 1))
    too_many = torch.cat((ids[:, :1], torch.full((1, 1025), REGION_TOKEN_INDEX, dtype=ids.dtype), ids[:, 1:]), 1)
    too_many[too_many == REGION_TOKEN_INDEX] = torch.where(torch.arange(12 + 1025) < 1025, REGION_TOKEN_INDEX, 7)
    fails("1025 <region> tokens", ids_=too_many, grid=(25, 41))
    assert (sess.prefix_builds, sess.prefix_hits) == (builds, hits)                   # none of these reached the pipeline
    # what segment(regions=) raises, with segment's text; the counters move as in one segment call that fails there
    fails("prompt 0, region 0: radius 17", grid=(3, 4), radius=17)
    fails("prompt 0: 11 region prompts for 12", grid=None, regions=[good[0][:11]])
    bad = [list(good[0])]
    bad[0][5] = {"points": [(h, 0)]}
    c0 = (sess.prefix_builds, sess.prefix_hits)
    fails("prompt 0, region 5: pixel", grid=None, regions=bad)
    c1 = (sess.prefix_builds, sess.prefix_hits)
    with pytest.raises(ValueError, match="prompt 0, region 5: pixel"):
        model.segment(sess, ids, am, regions=bad, region_index_sampler=rank_sampler)
    c2 = (sess.prefix_builds, sess.prefix_hits)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (c2[0] - c1[0], c2[1] - c1[1])
    # a region without a pixel is found BEHIND the prefix cache (segment's one read-back): again the counters of one segment call
    tall = copy.copy(sess)
    _, info2 = image_of(model.cfg, orig=(300, 200))
    tall.seg_info = info2
    rows, cols = nearest_pad_tables(*info2["transforms"]["resize"], *info2["transforms"]["pad"])
    y = next(v for v in range(300) if v not in set(rows.tolist()))
    lost = [[{"points": [(y, int(cols[3]))], "radius": 0}] + grid_clicks(300, 200, 3, 4, (12,))[0][1:]]
    c0 = (tall.prefix_builds, tall.prefix_hits)
    with pytest.raises(ValueError, match="prompt 0, region 0: no pixel"):
        model.segment_everything(tall, ids, am, grid=None, regions=lost, region_index_sampler=rank_sampler)
    c1 = (tall.prefix_builds, tall.prefix_hits)
    with pytest.raises(ValueError, match="prompt 0, region 0: no pixel"):
        model.segment(tall, ids, am, regions=lost, region_index_sampler=rank_sampler)
    c2 = (tall.prefix_builds, tall.prefix_hits)
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (c2[0] - c1[0], c2[1] - c1[1]) and c1 != c0
    # a model of another task
    from psalm_amd.synthetic import fix_indices, session_inputs
    other = model_for(kind, "fp32", task="referring")
    rinp = fix_indices(session_inputs(other.cfg, "referring", 1))
    rsess = other.encode_image(rinp["images"][:1], info)
    with pytest.raises(ValueError, match="region task"):
        other.segment_everything(rsess, rinp["input_ids"], rinp["attention_mask"], grid=(1, 1))
    with pytest.raises(ValueError, match="another model"):
        model.segment_everything(rsess, ids, am, grid=(3, 4))


def unchanged_case(kind):
    """segment(regions=...) returns after the new calls what it returned before them"""
    model, sess, info = session_for(kind)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompt_ids(model.cfg, (5, 7))
    regions = grid_clicks(h, w, 3, 4, (5, 7))
    before = model.segment(sess, ids, am, regions=regions, region_index_sampler=rank_sampler)
    model.segment_everything(sess, ids, am, grid=(3, 4), region_index_sampler=rank_sampler)
    model.segment_everything(sess, ids, am, grid=None, regions=regions, iou_thr=(1, 2), min_area=3, region_index_sampler=rank_sampler)
    after = model.segment(sess, ids, am, regions=regions, region_index_sampler=rank_sampler)
    assert_same_prompts(after, before)
