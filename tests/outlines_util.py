"""Helpers of the outline tests (tests/test_40_mask_outlines_kernels.py, test_41_outline_sessions_emu.py, test_42_outline_sessions_gpu.py): a
plain sequential oracle of csrc/outlines.hip, written from the definitions alone (include/psalm_hip.h) -- a tracer that WALKS every ring edge by
edge, and a filler that evaluates the even-odd rule pixel by pixel -- and the model-level cases shared by the emulated and the GPU sessions.
Everything is integers: every comparison is for equality."""
import numpy as np

from components_util import np_set  # noqa: F401  (re-exported: the set test of the planes)

# direction -> (dx, dy): +x, +y (down), -x, -y; "left" of d is (d + 3) % 4 (heading +x, left is -y)
STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))


def _edge_exists(f, H, W, x, y, d):
    """the crack edge that leaves vertex (x, y) in direction d: the pixel on its right is set, the one on its left is not"""
    def px(py, qx):
        return 0 <= py < H and 0 <= qx < W and bool(f[py, qx])
    if d == 0:
        return px(y, x) and not px(y - 1, x)                         # heading +x: right is below
    if d == 1:
        return px(y, x - 1) and not px(y, x)                         # heading +y: right is -x
    if d == 2:
        return px(y - 1, x - 1) and not px(y, x - 1)                 # heading -x: right is above
    return px(y - 1, x) and not px(y - 1, x - 1)                     # heading -y: right is +x


def np_outlines(flags, connectivity=8):
    """bool (H, W) -> [(vertices [(x, y), ...], signed area)]: the rings of the plane, each from its row-major lowest vertex, ordered by it"""
    assert connectivity in (4, 8)
    f = np.asarray(flags, bool)
    H, W = f.shape
    order = (3, 0, 1) if connectivity == 8 else (1, 0, 3)             # turns relative to the heading: left, straight, right / right, straight, left
    seen = set()
    rings = []
    for y in range(H + 1):                                            # row-major over the start vertices: a ring is met first at its lowest vertex
        for x in range(W + 1):
            for d in range(4):
                if (x, y, d) in seen or not _edge_exists(f, H, W, x, y, d):
                    continue
                walk = []
                cx, cy, cd = x, y, d
                while (cx, cy, cd) not in seen:
                    seen.add((cx, cy, cd))
                    walk.append((cx, cy, cd))
                    cx, cy = cx + STEP[cd][0], cy + STEP[cd][1]
                    for t in order:
                        nd = (cd + t) % 4
                        if _edge_exists(f, H, W, cx, cy, nd):
                            cd = nd
                            break
                    else:
                        raise AssertionError("an edge without a successor")
                assert (cx, cy, cd) == (x, y, d), "the walk did not close on its first edge"
                n = len(walk)
                corners = [(walk[i][0], walk[i][1]) for i in range(n) if walk[i - 1][2] != walk[i][2]]
                assert corners[0] == (x, y)
                a2 = sum(corners[i][0] * corners[(i + 1) % len(corners)][1] - corners[(i + 1) % len(corners)][0] * corners[i][1] for i in range(len(corners)))
                assert a2 % 2 == 0
                rings.append((corners, a2 // 2))
    return rings


def np_fill(rings, H, W):
    """[ring, ...] with ring = [(x, y), ...] integer vertices -> bool (H, W) by the even-odd rule over pixel centres, in Python integers"""
    out = np.zeros((H, W), bool)
    edges = []
    for ring in rings:
        ring = [(int(x), int(y)) for x, y in ring]
        for i in range(len(ring)):
            (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % len(ring)]
            if y0 == y1:
                continue
            if y0 > y1:
                x0, y0, x1, y1 = x1, y1, x0, y0
            edges.append((x0, y0, x1, y1))
    for py in range(H):
        row = [e for e in edges if 2 * e[1] <= 2 * py + 1 < 2 * e[3]]
        if not row:
            continue
        for px in range(W):
            k = sum(1 for x0, y0, x1, y1 in row if 2 * x0 * (y1 - y0) + (2 * py + 1 - 2 * y0) * (x1 - x0) > (2 * px + 1) * (y1 - y0))
            out[py, px] = k & 1
    return out


def np_tables(planes, connectivity=8):
    """bool (m, H, W) -> (ring_count (m), vertex_count (m), rings (R, 4), vertices (V, 2)) int32 in the layout of psalm_mask_outlines"""
    rc, vc, rings, verts = [], [], [], []
    for row, f in enumerate(planes):
        rs = np_outlines(f, connectivity)
        rc.append(len(rs))
        vc.append(sum(len(r[0]) for r in rs))
        for corners, area in rs:
            rings.append([row, len(verts), len(corners), area])
            verts.extend(corners)
    return (np.array(rc, np.int32).reshape(-1), np.array(vc, np.int32).reshape(-1), np.array(rings, np.int32).reshape(-1, 4),
            np.array(verts, np.int32).reshape(-1, 2))


def tables_of(polys_per_plane):
    """[[ring, ...] per plane] with ring = [(x, y), ...] -> (rings (R, 4), vertices (V, 2)) int32, area column 0"""
    rings, verts = [], []
    for row, polys in enumerate(polys_per_plane):
        for ring in polys:
            rings.append([row, len(verts), len(ring), 0])
            verts.extend((int(x), int(y)) for x, y in ring)
    return np.array(rings, np.int32).reshape(-1, 4), np.array(verts, np.int32).reshape(-1, 2)


def assert_outlines_equal(out, planes, connectivity):
    """a dict of mask_outlines' tensors == the oracle's tables of the bool planes"""
    want = np_tables(planes, connectivity)
    for name, w in zip(("ring_count", "vertex_count", "rings", "vertices"), want):
        g = out[name].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), name


# ---------------------------------------------------------------------------------------------------- model-level cases (kind: "emu" | "hip")
def _imports():
    import torch
    from everything_clean_util import planted_prompts
    from everything_util import DTYPES, assert_same_prompts, prompt_ids, session_for
    from interactive_util import assert_same_prediction, model_for, prompts_of, rank_sampler, regions_for
    return locals()


def everything_outlines_case(kind, connectivity=8):
    """the device step on planted picks (overlapping discs with specks and pin-holes at (70, 150)): `outlines` == the oracle on the returned
    `masks`; every other key equals the call without it, the launches in front of the outline step too"""
    u = _imports()
    torch = u["torch"]
    model = u["model_for"](kind, "fp32")
    prompts, counts = u["planted_prompts"](model)
    lib = model.ops.lib
    runs = []
    for kw in ({}, {"outlines": True}):
        lib.calls = []
        try:
            runs.append((model._everything_dedup(prompts, counts, 3, 10, 1, None, 0, 0, connectivity, **kw), list(lib.calls)))
        finally:
            lib.calls = None
    (a, calls_a), (b, calls_b) = runs
    assert set(a) == set(u["DTYPES"]) and set(b) == set(a) | {"outlines"}
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].cpu(), b[k].cpu()), k
    assert calls_b[:len(calls_a)] == calls_a and set(calls_b[len(calls_a):]) == {"psalm_mask_outline_totals", "psalm_mask_outlines"}
    assert not any("outline" in c for c in calls_a)
    planes = b["masks"].cpu().numpy() != 0
    assert len(planes) >= 2 and set(b["outlines"]) == {"ring_count", "vertex_count", "rings", "vertices"}
    assert all(v.device.type == model.device.type for v in b["outlines"].values())
    assert_outlines_equal(b["outlines"], planes, connectivity)
    assert b["outlines"]["ring_count"].cpu().numpy().max() > 1      # specks and pin-holes: more than one ring per mask
    return b


def public_call_case(kind, precision="fp32"):
    """segment_everything(outlines=True) and segment(outlines=True) on the tiny model: the new keys equal the oracle on the call's own masks, every
    other key is the one of the call without the argument; the default call's key set is today's"""
    u = _imports()
    torch = u["torch"]
    model, sess, info = u["session_for"](kind, precision)
    ids, am = u["prompt_ids"](model.cfg, (5, 7))
    a = model.segment_everything(sess, ids, am, grid=(3, 4), min_area=0, region_index_sampler=u["rank_sampler"])
    b = model.segment_everything(sess, ids, am, grid=(3, 4), min_area=0, region_index_sampler=u["rank_sampler"], outlines=True, connectivity=4)
    assert set(a) == set(u["DTYPES"]) | {"prompts"} and set(b) == set(a) | {"outlines"}
    for k in u["DTYPES"]:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
    u["assert_same_prompts"](b["prompts"], a["prompts"])
    assert_outlines_equal(b["outlines"], b["masks"].cpu().numpy() != 0, 4)
    h, w = info["transforms"]["resize"][:2]
    ids, am = u["prompts_of"](model.cfg)
    regions = u["regions_for"](h, w)
    plain = model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"])
    for call in (lambda **kw: model.segment(sess, ids, am, regions=regions, region_index_sampler=u["rank_sampler"], **kw),
                 lambda **kw: model.segment_many([(sess, dict(input_ids=ids, attention_mask=am, regions=regions))],
                                                 region_index_sampler=u["rank_sampler"], **kw)[0]):
        got = call(outlines=True)
        for g, p in zip(got, plain):
            assert set(g) == set(p) | {"picked_outlines"} and "picked_outlines" not in p
            u["assert_same_prediction"](g, p)
            for k in ("picked_query", "picked_scores", "picked_masks"):
                assert torch.equal(g[k].cpu(), p[k].cpu()), k
            assert_outlines_equal(g["picked_outlines"], g["picked_masks"].cpu().numpy() != 0, 8)
        assert all("picked_outlines" not in g for g in call(outlines=True, pick=False))


def polygon_regions(model, h, w):
    """prompt 0: a triangle; prompt 1: a ring with a hole, the outline of a blob fed back from mask_outlines (all its rings), a box.  Returns the
    `regions` with polygons and the same with {"mask": np_fill(polygon)} in their place; vertices are (y, x), the oracle's rings (x, y)"""
    import torch
    from interactive_util import blob
    from psalm_amd import evalout as E
    tri = [(2, 3), (h, w // 2), (h // 2, w)]                          # touches the lattice's last row and column
    holed = [[(5, 4), (5, w - 6), (h - 7, w - 6), (h - 7, 4)], [(15, 20), (h - 20, 20), (h - 20, w - 30), (15, w - 30)]]
    m = blob(h, w) != 0
    out = E.mask_outlines(torch.from_numpy(m)[None], connectivity=4, ops=model.ops)
    back = [[(y, x) for x, y in zip(flat[0::2], flat[1::2])] for flat in E.outline_polygons(out, holes=True)[0]]
    assert len(back) > 1 and np.array_equal(np_fill([[(x, y) for y, x in r] for r in back], h, w), m)

    def filled(rings):
        return np_fill([[(x, y) for y, x in r] for r in rings], h, w).astype(np.uint8)
    polys = [[{"polygon": tri}], [{"polygon": holed}, {"polygon": back}, {"box": (h // 6, w // 4, h // 2, w)}]]
    masks = [[{"mask": filled([tri])}], [{"mask": filled(holed)}, {"mask": filled(back)}, {"box": (h // 6, w // 4, h // 2, w)}]]
    assert filled([tri]).any() and filled(holed)[h // 2, w // 2] == 0 and filled(holed)[6, 5] == 1
    return polys, masks


def polygon_prompt_case(kind, precision="fp32"):
    """a polygon prompt gives, tensor for tensor, the results of the same call with {"mask": np_fill(polygon)}: segment, segment_many"""
    u = _imports()
    torch = u["torch"]
    model, sess, info = u["session_for"](kind, precision)
    h, w = info["transforms"]["resize"][:2]
    ids, am = u["prompts_of"](model.cfg)
    polys, masks = polygon_regions(model, h, w)
    lib = model.ops.lib
    lib.calls = []
    try:
        got = model.segment(sess, ids, am, regions=polys, region_index_sampler=u["rank_sampler"])
        calls = list(lib.calls)
    finally:
        lib.calls = None
    assert calls.count("psalm_mask_fill_polygons") == 3               # one per polygon region, into its plane
    want = model.segment(sess, ids, am, regions=masks, region_index_sampler=u["rank_sampler"])
    many = model.segment_many([(sess, dict(input_ids=ids, attention_mask=am, regions=polys)), (sess, dict(input_ids=ids, attention_mask=am, regions=masks))],
                              region_index_sampler=u["rank_sampler"])
    for res in (got, many[0], many[1]):
        for g, p in zip(res, want):
            assert set(g) == set(p)
            u["assert_same_prediction"](g, p)
            for k in ("picked_query", "picked_scores", "picked_masks"):
                assert torch.equal(g[k].cpu(), p[k].cpu()), k


def polygon_tracker_case(kind, precision="fp32", orig=(60, 80)):
    """VideoTracker.start(regions=polygons) == start(regions=masks of np_fill): the shared prompt plan takes polygons there too"""
    from click_track_util import assert_same_track, geometry
    from interactive_util import CountingSampler, model_for
    from psalm_amd import VideoTracker
    from psalm_amd.synthetic import video_clip_inputs
    model = model_for(kind, precision)
    f0 = video_clip_inputs(model.cfg, 1, 3, orig=orig)[0]
    h, w = f0["seg_info"][0]["transforms"]["resize"][:2]
    polys, masks = polygon_regions(model, h, w)
    res = []
    for regions in (polys[1], masks[1]):
        s = CountingSampler()
        trk = VideoTracker(model)
        res.append((trk.start(f0["input_ids"], f0["images"], geometry(f0), regions=regions, attention_mask=f0["attention_mask"], region_index_sampler=s),
                    s.calls, trk._origin.masks.cpu()))
    assert res[0][1] == res[1][1] and len(res[0][1]) == 3
    assert res[0][2].equal(res[1][2])
    assert_same_track(res[0][0], res[1][0])


def polygon_errors_case(kind):
    import pytest
    u = _imports()
    model, sess, info = u["session_for"](kind)
    h, w = info["transforms"]["resize"][:2]
    ids, am = u["prompts_of"](model.cfg)
    ok = [{"box": (0, 0, 4, 4)}, {"box": (0, 0, 4, 4)}]
    tri = [(1, 1), (1, 9), (9, 1)]
    for bad, match in (({"polygon": [(1, 1), (5, 5)]}, "prompt 1, region 0: a polygon ring of 2 vertices"),
                       ({"polygon": [tri, [(2, 2), (3, 3)]]}, "prompt 1, region 0: a polygon ring of 2 vertices"),
                       ({"polygon": [(1, 1), (h + 1, 3), (4, 4)]}, "prompt 1, region 0: vertex .* outside"),
                       ({"polygon": [(1, 1), (3, w + 1), (4, 4)]}, "prompt 1, region 0: vertex .* outside"),
                       ({"polygon": [(1, 1), (-1, 3), (4, 4)]}, "prompt 1, region 0: vertex .* outside"),
                       ({"polygon": [(1, 1), (2.5, 3), (4, 4)]}, "prompt 1, region 0: y 2.5 is not an integer"),
                       ({"polygon": [(1, 1), (2, True), (4, 4)]}, "prompt 1, region 0: x True is not an integer"),
                       ({"polygon": [(1, 1), (2, 3, 4), (4, 4)]}, "prompt 1, region 0: .* is not a \\(y, x\\) vertex"),
                       ({"polygon": []}, "prompt 1, region 0: a polygon is a ring"),
                       ({"polygon": tri, "box": (0, 0, 4, 4)}, "prompt 1, region 0: .*exactly one of"),
                       ({"polygon": tri, "radius": 3}, "prompt 1, region 0: unknown keys")):
        with pytest.raises(ValueError, match=match):
            model.segment(sess, ids, am, regions=[[{"points": [(3, 3)]}], [bad] + ok], region_index_sampler=u["rank_sampler"])
    assert "polygon" in model.REGION_PROMPT_KEYS
    cap = model.REGION_POLYGON_MAX_VERTICES
    try:
        type(model).REGION_POLYGON_MAX_VERTICES = 5
        with pytest.raises(ValueError, match="prompt 1, region 1: the polygon prompts of one call hold more than 5 vertices"):
            model.segment(sess, ids, am, regions=[[{"points": [(3, 3)]}], [{"polygon": tri}, {"polygon": tri}, ok[0]]], region_index_sampler=u["rank_sampler"])
    finally:
        type(model).REGION_POLYGON_MAX_VERTICES = cap


class _Instances:
    def __init__(self, masks, boxes, scores, classes):
        self.pred_masks, self.pred_boxes, self.scores, self.pred_classes = masks, boxes, scores, classes

    def __len__(self):
        return int(self.pred_masks.shape[0])


def coco_records_case(kind):
    """coco_instance_records(segmentation="polygon"): the outer rings as COCO polygons; the default stays RLE"""
    import pytest
    import torch
    from everything_util import discs
    from ops_backend import make_ops
    from psalm_amd import evalout as E
    o = make_ops(kind)
    m = discs(4, 40, 52, 9, rmin=4, rmax=15)
    m[:, 20, 21] ^= 1                                                 # a pin-hole or a speck
    m[0, 5:15, 5:15] = 1
    m[0, 9, 9] = 0                                                    # a hole for certain: a ring that the COCO polygons leave out
    m[3] = 0                                                          # an empty mask: no polygon
    inst = _Instances(torch.from_numpy(m), torch.tensor([[1., 2., 5., 9.]] * 4), torch.tensor([.9, .8, .7, .6]), torch.tensor([0, 2, 1, 1]))
    rec = E.coco_instance_records(inst, 7, category_ids=[10, 20, 30], ops=o, segmentation="polygon")
    polys = E.outline_polygons(E.mask_outlines(inst.pred_masks, ops=o))
    allr = E.outline_polygons(E.mask_outlines(inst.pred_masks, ops=o), holes=True)
    for k in range(4):
        want = [[c for v in corners for c in v] for corners, a in np_outlines(m[k] != 0, 8) if a > 0]
        assert rec[k]["segmentation"] == polys[k] == want and all(isinstance(c, int) for p in polys[k] for c in p)
        assert allr[k] == [[c for v in corners for c in v] for corners, a in np_outlines(m[k] != 0, 8)]
        assert rec[k]["image_id"] == 7 and rec[k]["category_id"] == [10, 30, 20, 20][k] and rec[k]["bbox"] == [1.0, 2.0, 4.0, 7.0]
    assert rec[3]["segmentation"] == [] and any(len(a) > len(p) for a, p in zip(allr, polys))
    default = E.coco_instance_records(inst, 7, category_ids=[10, 20, 30], ops=o)
    assert default == E.coco_instance_records(inst, 7, category_ids=[10, 20, 30], ops=o, segmentation="rle")
    assert all(set(r["segmentation"]) == {"size", "counts"} for r in default)
    with pytest.raises(ValueError, match="segmentation"):
        E.coco_instance_records(inst, 7, ops=o, segmentation="mask")
    # the public functions take host tensors of the three dtypes; fill_polygons takes arrays
    for t in (torch.from_numpy(m), torch.from_numpy(m).float(), torch.from_numpy(m) != 0):
        out = E.mask_outlines(t, connectivity=4, ops=o)
        assert_outlines_equal(out, m != 0, 4)
        assert np.array_equal(E.fill_polygons(out["rings"], out["vertices"], m.shape, ops=o).cpu().numpy(), m)
        assert np.array_equal(E.fill_polygons(out["rings"].cpu().numpy(), out["vertices"].cpu().tolist(), m.shape, ops=o).cpu().numpy(), m)
    assert not E.fill_polygons([], [], (2, 3, 4), ops=o).cpu().numpy().any()
    from psalm_amd.hip_ops import PsalmHipError
    with pytest.raises(PsalmHipError):
        E.mask_outlines(torch.zeros(3, 4), ops=o)
    with pytest.raises(PsalmHipError):
        E.mask_outlines(torch.zeros(1, 3, 4), connectivity=6, ops=o)
    with pytest.raises(PsalmHipError):
        E.fill_polygons(np.zeros((1, 4), np.float32), np.zeros((3, 2), np.int32), (1, 3, 4), ops=o)
