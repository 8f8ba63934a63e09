"""Helpers of the interactive-session tests (tests/test_24_interactive_session_emu.py, tests/test_25_interactive_session_gpu.py): region prompts given as
geometry (`regions=` of PSALM.segment / segment_many) against the host path they replace -- the prompt drawn in numpy, enhance_with_circles,
apply_segmentation, `instances.region_masks`, `region_points` under the same sampler.  Both sides run the same kernels behind the points, so every
comparison is bit for bit."""
import copy

import numpy as np
import pytest
import torch

from ops_backend import make_ops
from psalm_amd.config import PsalmConfig
from psalm_amd.model import PSALM
from psalm_amd.preprocess import apply_segmentation, enhance_with_circles, nearest_pad_tables, rle_to_mask
from psalm_amd.synthetic import RegionInstances, fix_indices, make_state_dict, session_inputs, video_clip_inputs

_MODELS = {}


def model_for(kind, precision, task="region"):
    key = (kind, precision, task)
    if key not in _MODELS:
        cfg = PsalmConfig.tiny(task)
        _MODELS[key] = PSALM(cfg, make_state_dict(cfg, seed=12), ops=make_ops(kind), precision=precision)
    return _MODELS[key]


class GtOnly:
    """an `instances` entry that carries ground truth and no region masks"""

    def __init__(self, gt_masks):
        self.gt_masks = gt_masks


def image_of(cfg, orig=(60, 80), size=96, seed=4):
    """(image (1, 3, size, size), geometry entry of seg_info: padding_mask / height / width / transforms) of video_clip_inputs' first frame"""
    f = video_clip_inputs(cfg, 1, 1, size=size, orig=orig, seed=seed)[0]
    info = {k: v for k, v in f["seg_info"][0].items() if k in ("padding_mask", "height", "width", "transforms")}
    return f["images"], info


def prompts_of(cfg, size=96):
    """two prompts with 1 and 3 <region> tokens: (input_ids, attention_mask) of session_inputs(cfg, "region", 2)"""
    inp = fix_indices(session_inputs(cfg, "region", 2, size=size))
    return inp["input_ids"], inp["attention_mask"]


def line(y0, x0, y1, x1, n):
    t = np.linspace(0.0, 1.0, n)
    return sorted(set(zip(np.round(y0 + (y1 - y0) * t).astype(int).tolist(), np.round(x0 + (x1 - x0) * t).astype(int).tolist())))


def blob(h, w, seed=0):
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    m[h // 3:h // 3 + 9, w // 4:w // 4 + 14] = rng.integers(0, 2, (9, 14))
    m[h // 3, w // 4] = 7                                       # any non-zero pixel counts
    return m


def regions_for(h, w, mask_as="numpy", device=None):
    """prompt 0: one point prompt; prompt 1: box + scribble + mask"""
    m = blob(h, w)
    if mask_as == "bool_tensor":
        m = torch.from_numpy(m != 0)
        m = m.to(device) if device is not None else m
    return [[{"points": [(h // 2, w // 2), (3, w - 2)]}],
            [{"box": (h // 6, w // 4, h // 2, w)}, {"scribble": line(5, 5, h - 10, w - 10, 40)}, {"mask": m}]]


def mask_of(rp, h, w):
    """the (h, w) uint8 region mask the dataset mapper would hand apply_segmentation for one region prompt"""
    m = np.zeros((h, w), np.uint8)
    if "box" in rp:
        y0, x0, y1, x1 = rp["box"]
        m[y0:y1, x0:x1] = 1
        return m
    if "mask" in rp or "rle" in rp:
        src = rle_to_mask(rp["rle"]) if "rle" in rp else rp["mask"]
        src = src.cpu().numpy() if torch.is_tensor(src) else np.asarray(src)
        return (src != 0).astype(np.uint8)
    kind = "points" if "points" in rp else "scribble"
    for y, x in rp[kind]:
        m[y, x] = 1
    return enhance_with_circles(m, rp.get("radius", 10 if kind == "points" else 5))


def host_infos(info, regions, gts=None):
    """per prompt the geometry entry + `instances` with the host-prepared region masks (and ground truth: the host path cannot run without)"""
    tr = info["transforms"]
    h, w = tr["resize"][:2]
    out = []
    for b, entry in enumerate(regions):
        rm = torch.from_numpy(np.stack([apply_segmentation(mask_of(rp, h, w), tr) for rp in entry]))
        d = dict(info)
        d["instances"] = RegionInstances(rm, gts[b] if gts is not None else rm.clone().float())
        out.append(d)
    return out


def rank_sampler(m, n):
    """deterministic ranks that reach the first and the last pixel"""
    return torch.cat((torch.tensor([0, m - 1]), (torch.arange(n - 2) * 7919 + 11) % m))


class CountingSampler:
    """ranks that depend on how many regions were drawn before: two runs agree only if they draw in the same order"""

    def __init__(self):
        self.calls = []

    def __call__(self, m, n):
        self.calls.append(int(m))
        return (torch.arange(n) * 7919 + 13 * len(self.calls)) % m


def as_point_sampler(s):
    return lambda nz, k: s(nz.shape[0], k)


def assert_same_prediction(got, want):
    assert torch.equal(got["mask_pred"].cpu(), want["mask_pred"].cpu())
    assert torch.equal(got["instances"].pred_masks.cpu(), want["instances"].pred_masks.cpu())
    assert torch.equal(got["instances"].scores.cpu(), want["instances"].scores.cpu())


def assert_picks(out, n_regions):
    sc = out["instances"].scores.cpu().numpy()
    assert sc.shape[1] == n_regions
    q = out["picked_query"].cpu()
    assert q.dtype == torch.int64 and q.tolist() == sc.argmax(0).tolist()              # (numpy: the first occurrence of the maximum)
    assert out["picked_scores"].dtype == torch.float32 and np.array_equal(out["picked_scores"].cpu().numpy(), sc.max(0))
    pm = out["picked_masks"]
    assert pm.dtype == torch.uint8 and pm.shape == (n_regions,) + tuple(out["instances"].pred_masks.shape[1:])
    assert torch.equal(pm.cpu().float(), out["instances"].pred_masks.cpu()[q])


# ---------------------------------------------------------------------------------------------------- cases (kind: "emu" | "hip")
def equality_case(kind, precision, batch_decoder):
    """section 3 of the contract + the launch count + picks + the absence of `gt`"""
    model = model_for(kind, precision)
    cfg = model.cfg
    img, info = image_of(cfg)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompts_of(cfg)
    regions = regions_for(h, w, "bool_tensor" if batch_decoder else "numpy", model.device)
    old = model.batch_decoder
    model.batch_decoder = batch_decoder
    lib = model.ops.lib
    try:
        sess = model.encode_image(img, info)
        want = model.segment(sess, ids, am, seg_info=host_infos(info, regions), region_point_sampler=as_point_sampler(rank_sampler))
        lib.calls = []
        try:
            got = model.segment(sess, ids, am, regions=regions, region_index_sampler=rank_sampler)
            calls = lib.calls
        finally:
            lib.calls = None
    finally:
        model.batch_decoder = old
    for name in ("psalm_mask_rasterize", "psalm_mask_dilate_disc", "psalm_mask_resize_nearest_pad", "psalm_mask_select_points"):
        assert calls.count(name) == 1, (name, calls.count(name))
    assert len(got) == 2
    for b, k in enumerate((1, 3)):
        assert_same_prediction(got[b], want[b])
        assert "gt" not in got[b] and "gt" in want[b]
        assert_picks(got[b], k)
    return got


def ground_truth_case(kind, precision="fp32"):
    """`gt` is present and what the host path returns when the prompt's seg_info carries instances.gt_masks; pick=False adds no keys; an RLE prompt"""
    model = model_for(kind, precision)
    img, info = image_of(model.cfg)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompts_of(model.cfg)
    regions = regions_for(h, w)
    m = np.asfortranarray(blob(h, w, seed=3) != 0)
    flat = m.reshape(-1, order="F")
    runs = np.diff(np.flatnonzero(np.r_[True, flat[1:] != flat[:-1], True]))
    regions[0][0] = {"rle": {"size": [h, w], "counts": ([0] if flat[0] else []) + runs.tolist()}}
    assert np.array_equal(rle_to_mask(regions[0][0]["rle"]), m.astype(np.uint8))
    g = torch.Generator().manual_seed(1)
    gts = [(torch.rand(k, 96, 96, generator=g) < 0.3).float() for k in (1, 3)]
    sess = model.encode_image(img, info)
    want = model.segment(sess, ids, am, seg_info=host_infos(info, regions, gts), region_point_sampler=as_point_sampler(rank_sampler))
    infos = [dict(info, instances=GtOnly(gt)) for gt in gts]
    got = model.segment(sess, ids, am, seg_info=infos, regions=regions, region_index_sampler=rank_sampler, pick=False)
    for a, b in zip(got, want):
        assert_same_prediction(a, b)
        assert torch.equal(a["gt"].cpu(), b["gt"].cpu())
        assert set(a) == set(b)                                 # no picked_* keys
    # the predictor outputs (postprocess=False), the region logits behind the scores among them
    want = model.segment(sess, ids, am, seg_info=host_infos(info, regions, gts), region_point_sampler=as_point_sampler(rank_sampler), postprocess=False)
    got = model.segment(sess, ids, am, regions=regions, region_index_sampler=rank_sampler, postprocess=False)
    for a, b in zip(got, want):
        assert set(a) == set(b) and float(b["pred_region_logits"].abs().max()) > 0
        assert torch.equal(a["pred_masks"], b["pred_masks"]) and torch.equal(a["pred_region_logits"], b["pred_region_logits"])


def pick_case(kind):
    """the pick on scores and masks that are not this tiny model's (its masks are empty and its scores zero): first arg-max per region, that query's mask"""
    model = model_for(kind, "fp32")
    g = torch.Generator().manual_seed(2)
    scores = torch.rand(model.cfg.md_queries, 3, generator=g)
    scores[[2, 5], 1] = 2.0
    masks = (torch.rand(model.cfg.md_queries, 17, 23, generator=g) < 0.4).float()
    out = model._region_pick({"_pending": ("region", scores.to(model.device), masks.to(model.device), None)})
    out["instances"] = type("I", (), {"scores": scores, "pred_masks": masks})()
    assert_picks(out, 3)
    assert out["picked_query"].tolist()[1] == 2


def segment_many_case(kind, precision):
    """two sessions with different original sizes in one segment_many call == the loop of segment(regions=...) under the same sampler sequence"""
    model = model_for(kind, precision)
    cfg = model.cfg
    ids, am = prompts_of(cfg)
    reqs = []
    for orig, seed in (((60, 80), 4), ((80, 60), 5)):
        img, info = image_of(cfg, orig=orig, seed=seed)
        h, w = info["transforms"]["resize"][:2]
        reqs.append((model.encode_image(img, info), {"input_ids": ids, "attention_mask": am, "regions": regions_for(h, w)}))
    s1 = CountingSampler()
    want = [model.segment(sess, kw["input_ids"], kw["attention_mask"], regions=kw["regions"], region_index_sampler=s1) for sess, kw in reqs]
    s2 = CountingSampler()
    lib = model.ops.lib
    lib.calls = []
    try:
        got = model.segment_many(reqs, region_index_sampler=s2)
        calls = lib.calls
    finally:
        lib.calls = None
    assert s1.calls == s2.calls and len(s1.calls) == 8
    for name in ("psalm_mask_rasterize", "psalm_mask_dilate_disc", "psalm_mask_resize_nearest_pad", "psalm_mask_select_points"):
        assert calls.count(name) == 2, (name, calls.count(name))                       # once per request
    for gr, wr in zip(got, want):
        for a, b in zip(gr, wr):
            assert_same_prediction(a, b)
            assert "gt" not in a
            for k in ("picked_query", "picked_scores", "picked_masks"):
                assert torch.equal(a[k].cpu(), b[k].cpu()), k


def unchanged_case(kind, precision):
    """segment without `regions` returns after a `regions` call what it returned before one"""
    model = model_for(kind, precision)
    img, info = image_of(model.cfg)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompts_of(model.cfg)
    regions = regions_for(h, w)
    infos = host_infos(info, regions)
    sess = model.encode_image(img, info)
    torch.manual_seed(9)
    before = model.segment(sess, ids, am, seg_info=infos)
    model.segment(sess, ids, am, regions=regions, region_index_sampler=rank_sampler)
    torch.manual_seed(9)
    after = model.segment(sess, ids, am, seg_info=infos)
    for a, b in zip(after, before):
        assert_same_prediction(a, b)
        assert torch.equal(a["gt"].cpu(), b["gt"].cpu()) and set(a) == set(b)


def errors_case(kind, precision="fp32"):
    model = model_for(kind, precision)
    cfg = model.cfg
    img, info = image_of(cfg)
    h, w = info["transforms"]["resize"][:2]
    ids, am = prompts_of(cfg)
    sess = model.encode_image(img, info)
    good = regions_for(h, w)

    def swap(b, j, rp):
        r = [list(e) for e in good]
        r[b][j] = rp
        return r

    def fails(match, regions=good, session=sess, **kw):
        with pytest.raises(ValueError, match=match):
            model.segment(session, ids, am, regions=regions, region_index_sampler=rank_sampler, **kw)

    fails("prompt 1: 2 region prompts for 3", [good[0], good[1][:2]])
    fails("one list of region prompts per prompt", good[:1])
    fails("prompt 1, region 2: .*exactly one of", swap(1, 2, {}))
    fails("prompt 0, region 0: .*exactly one of", swap(0, 0, {"points": [(1, 1)], "box": (0, 0, 2, 2)}))
    fails("prompt 1, region 1: unknown keys", swap(1, 1, {"scribble": [(1, 1)], "colour": 3}))
    fails("prompt 1, region 0: unknown keys", swap(1, 0, {"box": (0, 0, 2, 2), "radius": 3}))
    fails(f"prompt 0, region 0: pixel .* outside the image of .*{h}, {w}", swap(0, 0, {"points": [(h, 0)]}))
    fails("prompt 1, region 1: pixel", swap(1, 1, {"scribble": [(0, 0), (0, -1)]}))
    fails("prompt 1, region 0: box", swap(1, 0, {"box": (0, 0, h + 1, w)}))
    fails("prompt 1, region 0: box", swap(1, 0, {"box": (5, 5, 5, 9)}))
    fails("prompt 0, region 0: radius 17", swap(0, 0, {"points": [(1, 1)], "radius": 17}))
    fails("prompt 0, region 0: radius -1", swap(0, 0, {"points": [(1, 1)], "radius": -1}))
    fails("prompt 1, region 2: a mask of shape", swap(1, 2, {"mask": np.zeros((w, h), np.uint8)}))
    fails("prompt 1, region 2: no pixel", swap(1, 2, {"mask": np.zeros((h, w), np.uint8)}))
    fails("prompt 0: regions given together with", seg_info=host_infos(info, good))
    bare = copy.copy(sess)                                      # (shallow: the session's tensors, another geometry entry)
    bare.seg_info = {k: v for k, v in info.items() if k != "transforms"}
    fails("transforms", session=bare)
    bare.seg_info = None
    fails("transforms", session=bare)
    # a pixel that the down-scaling resize drops: 300 x 200 -> 96 x 64 reads one source row in three
    _, info2 = image_of(cfg, orig=(300, 200))
    tall = copy.copy(sess)
    tall.seg_info = info2
    rows, cols = nearest_pad_tables(*info2["transforms"]["resize"], *info2["transforms"]["pad"])
    y = next(v for v in range(300) if v not in set(rows.tolist()))
    lost = swap(0, 0, {"points": [(y, int(cols[3]))], "radius": 0})
    lost[1] = regions_for(300, 200)[1]
    fails("prompt 0, region 0: no pixel of the prompt is left after the resize", lost, session=tall)
    with pytest.raises(ValueError, match="request 1: prompt 0, region 0: radius"):
        model.segment_many([(sess, {"input_ids": ids, "attention_mask": am, "regions": good}),
                            (sess, {"input_ids": ids, "attention_mask": am, "regions": swap(0, 0, {"points": [(1, 1)], "radius": 99})})])
    with pytest.raises(ValueError, match="one kind per call"):
        model.segment_many([(sess, {"input_ids": ids, "attention_mask": am, "regions": good}),
                            (sess, {"input_ids": ids, "attention_mask": am, "seg_info": host_infos(info, good)})])
    # regions on a model of another task
    other = model_for(kind, precision, task="referring")
    rinp = fix_indices(session_inputs(other.cfg, "referring", 1))
    rsess = other.encode_image(rinp["images"][:1], info)
    with pytest.raises(ValueError, match="region task"):
        other.segment(rsess, rinp["input_ids"], rinp["attention_mask"], token_refer_id=rinp["token_refer_id"],
                      refer_embedding_indices=rinp["refer_embedding_indices"], regions=[[]])
