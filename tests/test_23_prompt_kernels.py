"""The region-prompt kernels (csrc/prompts.hip: psalm_mask_rasterize, psalm_mask_dilate_disc, psalm_region_best, psalm_mask_gather_u8) and their
chain into psalm_mask_resize_nearest_pad / psalm_mask_select_points, against the host formulas of the dataset mapper they replace
(psalm_amd/preprocess.py enhance_with_circles / apply_segmentation, model.region_points' expression).  Integer work: every comparison is exact.
Runs on the host emulation and, marked gpu, on the MI355X."""
import numpy as np
import pytest
import torch

from ops_backend import make_ops, ops  # noqa: F401  (fixture: "emu" on the CPU, "hip" marked gpu)
from psalm_amd.hip_ops import PsalmHipError
from psalm_amd.preprocess import apply_segmentation, enhance_with_circles, nearest_pad_tables


def _dev(ops, a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(ops.device)


def brute_discs(mask, radius):
    """the reference's loop restated: for every pixel equal to 1 a full-image map of sqrt(dx^2 + dy^2) <= radius, OR-ed together"""
    h, w = mask.shape
    yy, xx = np.mgrid[:h, :w]
    out = np.zeros((h, w), bool)
    for cy, cx in zip(*np.nonzero(mask == 1)):
        out |= np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2) <= radius
    return out.astype(np.uint8)


def _dilate(ops, planes, radii, max_radius=None):
    max_radius = max([0] + [r for r in radii]) if max_radius is None else max_radius
    out = ops.mask_dilate_disc(_dev(ops, planes), _dev(ops, np.asarray(radii, np.int32)), max_radius)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- dilation
def _small_plane():
    m = np.zeros((70, 150), np.uint8)
    for y, x in ((0, 0), (0, 149), (69, 0), (69, 149), (33, 63), (34, 64), (20, 127), (21, 128)):
        m[y, x] = 1
    m[50, 40] = 2                                   # neither of these seeds a disc
    m[10, 100] = 255
    return m


def test_dilate_small_plane_all_radii(ops):
    """70 x 150 (no multiple of 64, wider than two 64-bit words), seeds at the corners and astride the word boundaries, radii 0 / 1 / 5 / 10 / 16 and a
    plane that is copied"""
    m = _small_plane()
    radii = [0, 1, 5, 10, 16, -1]
    got = _dilate(ops, np.stack([m] * 6), radii)
    counts = []
    for i, r in enumerate(radii[:5]):
        want = enhance_with_circles(m, r)
        assert np.array_equal(want, brute_discs(m, r)), r
        assert np.array_equal(got[i], want), r
        counts.append(int(want.sum()))
    assert counts == [8, 28, 296, 1052, 2529]
    assert np.array_equal(got[5], m) and got[5, 50, 40] == 2 and got[5, 10, 100] == 255


def test_dilate_across_tiles(ops):
    """200 x 600 with 40 random seeds: several tiles in both directions"""
    rng = np.random.default_rng(23)
    m = np.zeros((200, 600), np.uint8)
    m[rng.integers(0, 200, 40), rng.integers(0, 600, 40)] = 1
    got = _dilate(ops, np.stack([m, m]), [10, 16])
    assert np.array_equal(got[0], enhance_with_circles(m, 10)) and np.array_equal(got[1], enhance_with_circles(m, 16))
    assert np.array_equal(got[1], brute_discs(m, 16))


def test_dilate_edge_cases(ops):
    ones = np.ones((1, 20, 70), np.uint8)
    assert np.array_equal(_dilate(ops, ones, [5]), ones)
    assert not _dilate(ops, np.zeros((1, 20, 70), np.uint8), [5]).any()
    # a radius below max_radius in the same call (the halo is max_radius rows, the disc the plane's own)
    m = _small_plane()
    assert np.array_equal(_dilate(ops, m[None], [5], max_radius=16)[0], enhance_with_circles(m, 5))
    t = _dev(ops, ones)
    rad = _dev(ops, np.asarray([5], np.int32))
    with pytest.raises(PsalmHipError):
        ops.mask_dilate_disc(t, rad, 17)
    with pytest.raises(PsalmHipError):
        ops.mask_dilate_disc(t, rad, 5, out=t)


# ---------------------------------------------------------------------------------------------------- rasterize
def test_rasterize(ops):
    R, h, w = 3, 37, 53
    prims = np.asarray([[0, 0, 0, 0, 0, 0], [0, 0, 36, 52, 0, 0], [0, 0, 36, 52, 0, 0],
                        [1, 1, 5, 7, 20, 53], [1, 1, 30, 2, 31, 3]], np.int32)
    want = np.zeros((R, h, w), np.uint8)
    want[0, 0, 0] = want[0, 36, 52] = 1
    want[1, 5:20, 7:53] = 1
    want[1, 30:31, 2:3] = 1
    out = _dev(ops, np.full((R, h, w), 0xAB, np.uint8))
    got = ops.mask_rasterize(_dev(ops, prims), R, h, w, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy(), want)
    assert not want[2].any()
    out = _dev(ops, np.full((R, h, w), 0xAB, np.uint8))
    assert not ops.mask_rasterize(_dev(ops, np.zeros((0, 6), np.int32)), R, h, w, out=out).cpu().numpy().any()


def test_rasterize_writes_nothing_outside(ops):
    """primitives (or parts of them) outside the image or with a region outside [0, R) are dropped: the buffer is one guard plane longer"""
    R, h, w = 2, 9, 11
    prims = np.asarray([[0, 0, -1, 3, 0, 0], [0, 0, 9, 3, 0, 0], [0, 0, 3, 11, 0, 0], [0, 0, 3, -1, 0, 0], [2, 0, 1, 1, 0, 0], [-1, 1, 0, 0, 9, 11],
                        [1, 1, -4, -4, 3, 2], [1, 1, 7, 9, 50, 60], [1, 2, 0, 0, 9, 11]], np.int32)
    buf = _dev(ops, np.full((R + 1, h, w), 0xAB, np.uint8))
    ops.mask_rasterize(_dev(ops, prims), R, h, w, out=buf[:R])
    got = buf.cpu().numpy()
    want = np.zeros((R, h, w), np.uint8)
    want[1, 0:3, 0:2] = 1
    want[1, 7:9, 9:11] = 1
    assert np.array_equal(got[:R], want) and (got[R] == 0xAB).all()


# ---------------------------------------------------------------------------------------------------- region_best / gather
def test_region_best(ops):
    rng = np.random.default_rng(7)
    s = rng.random((100, 5)).astype(np.float32)
    s[[3, 7], 2] = 2.0                               # equal maxima: the lower query
    s[99, 4] = 3.0
    q, v = ops.region_best(_dev(ops, s))
    assert q.dtype == torch.int32 and q.cpu().tolist() == np.argmax(s, 0).tolist() and q.cpu().tolist()[2] == 3
    assert np.array_equal(v.cpu().numpy(), s.max(0))
    one = rng.random((1, 4)).astype(np.float32)
    q, v = ops.region_best(_dev(ops, one))
    assert q.cpu().tolist() == [0, 0, 0, 0] and np.array_equal(v.cpu().numpy(), one[0])
    with pytest.raises(PsalmHipError):
        ops.region_best(_dev(ops, np.zeros((1025, 2), np.float32)))


def test_mask_gather_u8(ops):
    rng = np.random.default_rng(8)
    m = rng.standard_normal((6, 13, 41)).astype(np.float32)
    m[2, 0, 0] = 0.0
    got = ops.mask_gather_u8(_dev(ops, m), _dev(ops, np.asarray([4, 2, 2, 0], np.int32)))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), (m[[4, 2, 2, 0]] > 0).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------- the chain
def _line(y0, x0, y1, x1, n):
    t = np.linspace(0.0, 1.0, n)
    return sorted(set(zip(np.round(y0 + (y1 - y0) * t).astype(int).tolist(), np.round(x0 + (x1 - x0) * t).astype(int).tolist())))


def _chain(ops, h, w, S, specs, n=8, seed=0):
    """specs: per region ("points" | "scribble" | "box", geometry, radius).  rasterize -> dilate -> resize + pad -> select against the host path:
    apply_segmentation(enhance_with_circles(mask, radius)) and (nonzero() / [S, S])[ranks].float().  Returns (source totals, resized totals)."""
    from psalm_amd.synthetic import resized_box
    nh, nw = resized_box(h, w, S)
    tr = {"resize": (h, w, nh, nw), "pad": (S - nh, S - nw)}
    R = len(specs)
    prims, radii, host = [], [], []
    for r, (kind, geo, rad) in enumerate(specs):
        m = np.zeros((h, w), np.uint8)
        if kind == "box":
            y0, x0, y1, x1 = geo
            prims.append([r, 1, y0, x0, y1, x1])
            m[y0:y1, x0:x1] = 1
        else:
            for y, x in geo:
                prims.append([r, 0, y, x, 0, 0])
                m[y, x] = 1
            m = enhance_with_circles(m, rad)
        radii.append(rad)
        host.append(m)
    want = np.stack([apply_segmentation(m, tr) for m in host])
    rows, cols = nearest_pad_tables(h, w, nh, nw, S - nh, S - nw)
    raw = ops.mask_rasterize(_dev(ops, np.asarray(prims, np.int32)), R, h, w)
    dil = ops.mask_dilate_disc(raw, _dev(ops, np.asarray(radii, np.int32)), max([0] + radii))
    assert np.array_equal(dil.cpu().numpy(), np.stack(host))
    total = torch.zeros(R, dtype=torch.int32).to(ops.device)
    out, row_cnt = ops.mask_resize_nearest_pad(dil, _dev(ops, rows), _dev(ops, cols), total=total)
    assert np.array_equal(out.cpu().numpy(), want)
    totals = total.cpu().tolist()
    assert totals == want.astype(bool).sum((1, 2)).tolist() and min(totals) > 0
    rng = np.random.default_rng(seed)
    idx = np.stack([np.r_[0, t - 1, rng.integers(0, t, n - 2)] for t in totals]).astype(np.int32)
    pts = ops.mask_select_points(out, row_cnt, _dev(ops, idx))
    wh = torch.tensor([S, S])[None]
    pts_want = torch.stack([(torch.from_numpy(want[r]).nonzero() / wh)[torch.from_numpy(idx[r]).long()].float() for r in range(R)])
    assert torch.equal(pts.cpu(), pts_want)
    return [int(m.sum()) for m in host], totals


def test_chain_upscaling_with_pad_rows(ops):
    """60 x 80 into a 96 canvas: 72 x 96 real, 24 pad rows"""
    src, dst = _chain(ops, 60, 80, 96, [("points", [(30, 40)], 10), ("scribble", _line(5, 5, 50, 70, 40), 5), ("box", (10, 20, 35, 80), -1),
                                        ("points", [(0, 0), (59, 79)], 3)])
    assert all(d > s for s, d in zip(src, dst))


def test_chain_downscaling_loses_pixels(ops):
    """300 x 200 into 96: a thin (radius 0) scribble loses pixels in the resize"""
    src, dst = _chain(ops, 300, 200, 96, [("scribble", _line(10, 10, 280, 150, 300), 0), ("points", [(150, 100)], 10), ("box", (0, 0, 300, 200), -1)])
    assert dst[0] < src[0] and dst[2] == 96 * 64


@pytest.mark.gpu
def test_chain_real_size():
    """480 x 640 into 1024^2: point, scribble of 300 pixels, box"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    scribble = _line(100, 50, 400, 600, 2000)[:300]
    assert len(scribble) == 300
    _chain(make_ops("hip"), 480, 640, 1024, [("points", [(240, 320)], 10), ("scribble", scribble, 5), ("box", (100, 200, 480, 640), -1)], n=32)
