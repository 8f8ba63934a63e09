"""Oracles for csrc/distance.hip in plain numpy, written from the contract and not from the kernels: the brute-force squared distance map (a
broadcast over the seed list), seg2bmap's rules shift by shift, the centre as the first arg-max of the masked border map, boundary counts and
DAVIS's F from those.  Plus the session cases of tests/test_44 / test_45 (the tiny region model of tests/everything_util.py)."""
import math

import numpy as np

FAR = 1 << 30


def np_dist2(flags, to="unset", border=False):
    """flags (H,W) bool -> (H,W) int32: min over the seeds of dy^2 + dx^2; FAR without a seed"""
    flags = np.asarray(flags, bool)
    H, W = flags.shape
    seeds = np.argwhere(flags if to == "set" else ~flags).astype(np.int32)         # (int32 holds 2 * 16383^2)
    yy, xx = np.indices((H, W), dtype=np.int32)
    out = np.full((H, W), FAR, np.int32)
    for k in range(0, len(seeds), 256):                               # (chunks keep the broadcast small)
        s = seeds[k:k + 256]
        d = (yy[None] - s[:, 0, None, None]) ** 2 + (xx[None] - s[:, 1, None, None]) ** 2
        out = np.minimum(out, d.min(0))
    return np.minimum(out, np_border2(H, W)) if border else out


def np_border2(H, W):
    """the squared distance to the nearest position outside the image"""
    yy, xx = np.indices((H, W), dtype=np.int32)
    return np.minimum(np.minimum(yy + 1, H - yy), np.minimum(xx + 1, W - xx)) ** 2


def np_bmap(flags):
    """DAVIS seg2bmap at the mask's own size"""
    m = np.asarray(flags, bool)
    e, s, se = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    e[:, :-1] = m[:, 1:]
    s[:-1, :] = m[1:, :]
    se[:-1, :-1] = m[1:, 1:]
    b = (m ^ e) | (m ^ s) | (m ^ se)
    b[-1, :] = m[-1, :] ^ e[-1, :]
    b[:, -1] = m[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def np_center(flags):
    """[y, x, dist2] of the first maximum of the border=True inside map over the set pixels; [-1, -1, 0] for an empty mask"""
    flags = np.asarray(flags, bool)
    if not flags.any():
        return np.array([-1, -1, 0], np.int32)
    d = np.where(flags, np_dist2(flags, "unset", True), -1)
    p = int(np.argmax(d))                                             # the first maximum: the lowest row-major index
    return np.array([p // flags.shape[1], p % flags.shape[1], d.reshape(-1)[p]], np.int32)


def np_boundary_counts(pred, gt, bound):
    """[n_fg, n_gt, fg_match, gt_match] of one pair"""
    bp, bg = np_bmap(pred), np_bmap(gt)
    dp, dg = np_dist2(bp, "set"), np_dist2(bg, "set")
    b2 = int(bound) * int(bound)
    return np.array([bp.sum(), bg.sum(), (bp & (dg <= b2)).sum(), (bg & (dp <= b2)).sum()], np.int64)


def np_boundary_f(c):
    """DAVIS f_measure's last lines on one pair's integers -> (precision, recall, F) as Python floats (float64)"""
    n_fg, n_gt, fg_match, gt_match = (int(v) for v in c)
    if n_fg == 0 and n_gt > 0:
        p, r = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        p, r = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        p, r = 1.0, 1.0
    else:
        p, r = fg_match / n_fg, gt_match / n_gt
    return p, r, (0.0 if p + r == 0 else 2 * p * r / (p + r))


def disc_inside(flags, cy, cx, d2):
    """every pixel with (y - cy)^2 + (x - cx)^2 < d2 is inside the image and set"""
    H, W = flags.shape
    r = math.isqrt(max(int(d2) - 1, 0)) + 1
    if cy - r < -1 or cx - r < -1 or cy + r > H or cx + r > W:        # a pixel of the open disc may lie outside: look at it exactly
        for y in range(cy - r, cy + r + 1):
            for x in range(cx - r, cx + r + 1):
                if (y - cy) ** 2 + (x - cx) ** 2 < d2 and not (0 <= y < H and 0 <= x < W):
                    return False
    yy, xx = np.indices((H, W))
    return bool(flags[(yy - cy) ** 2 + (xx - cx) ** 2 < d2].all())


# ---------------------------------------------------------------------------------------------------- session cases (emu and MI355X)
def _imports():
    import torch
    from everything_clean_util import planted_prompts
    from everything_util import DTYPES, assert_same_prompts, prompt_ids, session_for
    from interactive_util import assert_same_prediction, model_for, prompts_of, rank_sampler, regions_for
    return dict(torch=torch, planted_prompts=planted_prompts, DTYPES=DTYPES, assert_same_prompts=assert_same_prompts, model_for=model_for,
                prompt_ids=prompt_ids, rank_sampler=rank_sampler, session_for=session_for, assert_same_prediction=assert_same_prediction,
                prompts_of=prompts_of, regions_for=regions_for)


def assert_centers_equal(centers, planes):
    """the device table against the oracle on the call's own masks; the open disc lies inside each mask"""
    got = centers.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (len(planes), 3)
    want = np.stack([np_center(p) for p in planes]) if len(planes) else np.zeros((0, 3), np.int32)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for (cy, cx, d2), p in zip(got.tolist(), planes):
        if p.any():
            assert p[cy, cx] and disc_inside(p, cy, cx, d2)


CENTER_CALLS = {"psalm_mask_distance", "psalm_mask_centers"}


def everything_centers_case(kind, **extra):
    """the device step behind segment_everything on planted picks (real shapes): with centers=True every other key and every launch in front
    are those of the call without it; `centers` equals evalout.mask_centers of the returned masks and the oracle"""
    from psalm_amd import evalout as E
    u = _imports()
    torch = u["torch"]
    model = u["model_for"](kind, "fp32")
    prompts, counts = u["planted_prompts"](model)
    lib = model.ops.lib
    runs = []
    for kw in ({}, {"centers": True}):
        lib.calls = []
        try:
            runs.append((model._everything_dedup(prompts, counts, 3, 10, 1, None, extra.get("min_island", 0), extra.get("max_hole", 0), 8,
                                                 outlines=extra.get("outlines", False), **kw), list(lib.calls)))
        finally:
            lib.calls = None
    (a, calls_a), (b, calls_b) = runs
    assert "centers" not in a and set(b) == set(a) | {"centers"}
    for k in a:
        if k == "outlines":
            for kk in a[k]:
                assert torch.equal(a[k][kk].cpu(), b[k][kk].cpu()), kk
        else:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
    assert calls_b[:len(calls_a)] == calls_a and set(calls_b[len(calls_a):]) == CENTER_CALLS
    assert not any(c in CENTER_CALLS for c in calls_a)
    planes = b["masks"].cpu().numpy() != 0
    assert len(planes) >= 2 and b["centers"].device.type == model.device.type
    assert torch.equal(b["centers"].cpu(), E.mask_centers(b["masks"], ops=model.ops).cpu())
    assert_centers_equal(b["centers"], planes)
    assert b["centers"].cpu().numpy()[:, 2].max() > 4                 # planted blobs: real depth
    return b


def public_centers_case(kind, precision="fp32"):
    """segment_everything(centers=True) and segment / segment_many(centers=True) on the tiny model: the new key equals evalout.mask_centers of
    the call's own masks, every other key is the one of the call without the argument; non-bool values raise"""
    import pytest
    from psalm_amd import evalout as E
    u = _imports()
    torch = u["torch"]
    model, sess, info = u["session_for"](kind, precision)
    ids, am = u["prompt_ids"](model.cfg, (5, 7))
    kw = dict(grid=(3, 4), min_area=0, region_index_sampler=u["rank_sampler"])
    a = model.segment_everything(sess, ids, am, **kw)
    b = model.segment_everything(sess, ids, am, centers=True, **kw)
    assert set(a) == set(u["DTYPES"]) | {"prompts"} and set(b) == set(a) | {"centers"}
    for k in u["DTYPES"]:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    u["assert_same_prompts"](b["prompts"], a["prompts"])
    assert torch.equal(b["centers"].cpu(), E.mask_centers(b["masks"], ops=model.ops).cpu())
    assert_centers_equal(b["centers"], b["masks"].cpu().numpy() != 0)
    c = model.segment_everything(sess, ids, am, centers=True, outlines=True, min_island=3, max_hole=2, **kw)
    d = model.segment_everything(sess, ids, am, outlines=True, min_island=3, max_hole=2, **kw)
    assert set(c) == set(d) | {"centers"}
    for k in set(d) - {"prompts", "outlines"}:
        assert torch.equal(c[k].cpu(), d[k].cpu()), k
    for k in d["outlines"]:
        assert torch.equal(c["outlines"][k].cpu(), d["outlines"][k].cpu()), k
    assert torch.equal(c["centers"].cpu(), E.mask_centers(c["masks"], ops=model.ops).cpu())
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="centers"):
            model.segment_everything(sess, ids, am, centers=bad, **kw)
    h, w = info["transforms"]["resize"][:2]
    ids, am = u["prompts_of"](model.cfg)
    regions = u["regions_for"](h, w)
    plain = model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"])
    for call in (lambda **kw: model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"], **kw),
                 lambda **kw: model.segment_many([(sess, dict(input_ids=ids, attention_mask=am, regions=regions))],
                                                 region_index_sampler=u["rank_sampler"], **kw)[0]):
        got = call(centers=True)
        for g, p in zip(got, plain):
            assert set(g) == set(p) | {"picked_centers"} and "picked_centers" not in p
            u["assert_same_prediction"](g, p)
            for k in ("picked_query", "picked_scores", "picked_masks"):
                assert torch.equal(g[k].cpu(), p[k].cpu()), k
            assert torch.equal(g["picked_centers"].cpu(), E.mask_centers(g["picked_masks"], ops=model.ops).cpu())
            assert_centers_equal(g["picked_centers"], g["picked_masks"].cpu().numpy() != 0)
        with pytest.raises(ValueError, match="centers"):
            call(centers=1)
    both = model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"], centers=True, outlines=True)
    for g, p in zip(both, got):
        assert set(g) == set(p) | {"picked_outlines"} and torch.equal(g["picked_centers"].cpu(), p["picked_centers"].cpu())
    none = model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"], centers=True, pick=False)
    assert all("picked_centers" not in g for g in none)


def click_round_trip_case(kind, precision="fp32"):
    """centres of planted masks, in the original image's pixels, fed back as {"points": [(y, x)]} prompts: `segment` takes them, and each
    click lies on the mask it came from"""
    from psalm_amd import evalout as E
    u = _imports()
    torch = u["torch"]
    model, sess, info = u["session_for"](kind, precision)
    h, w = info["transforms"]["resize"][:2]
    from everything_util import discs
    masks = discs(3, h, w, 44, rmin=4, rmax=min(h, w) // 3)
    masks[2] = 0
    masks[2, 1:4, w - 5:w - 1] = 1                                    # a small mask near a corner
    centers = E.mask_centers(torch.from_numpy(masks), ops=model.ops).cpu().tolist()
    for k, (cy, cx, d2) in enumerate(centers):
        assert d2 >= 1 and masks[k, cy, cx] != 0
    ids, am = u["prompts_of"](model.cfg)                              # prompt 0: one region, prompt 1: three
    regions = [[{"points": [tuple(centers[0][:2])]}], [{"points": [tuple(c[:2])]} for c in centers]]
    res = model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"], centers=True)
    assert [tuple(r["picked_centers"].shape) for r in res] == [(1, 3), (3, 3)]
    assert all(tuple(r["picked_masks"].shape[1:]) == (h, w) for r in res)
