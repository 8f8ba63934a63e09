"""csrc/distance.hip -- psalm_mask_distance / psalm_mask_centers / psalm_mask_boundaries / psalm_boundary_counts -- and their evalout surface
against the numpy oracles of tests/distance_util.py.  Integer results: every comparison of device results is np.array_equal.  Runs on the host
emulation of the kernel sources and, marked gpu, on the MI355X.  The plane with ONE seed in a corner at (130, 70) has only long-range distances
(a windowed column search fails it); (5, 200) has four ballot words with a ragged last one (the carry across words)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from distance_util import FAR, disc_inside, np_bmap, np_boundary_counts, np_border2, np_boundary_f, np_center, np_dist2
from ops_backend import ops  # noqa: F401  (fixture)
from psalm_amd import evalout as E
from psalm_amd.hip_ops import PsalmHipError

DTYPES = [torch.float32, torch.uint8, torch.bool]
IDS = ["f32", "u8", "bool"]
SHAPES = [(1, 1), (1, 67), (67, 1), (33, 65), (70, 86), (5, 200), (130, 70)]
MODES = [("unset", False), ("unset", True), ("set", False), ("set", True)]


# ---------------------------------------------------------------------------------------------------- planes
@functools.lru_cache(maxsize=None)
def case_planes(H, W):
    g = np.random.default_rng(H * 1000 + W)
    yy, xx = np.indices((H, W))
    planes = [np.zeros((H, W), bool), np.ones((H, W), bool)]
    for cy, cx in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):   # a single set pixel in each corner
        p = np.zeros((H, W), bool)
        p[cy, cx] = True
        planes.append(p)
    lone = np.ones((H, W), bool)                                      # a single UNSET pixel in a corner: every inside distance is long-range
    lone[H - 1, 0] = False
    frame = np.zeros((H, W), bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    r = max(min(H, W) // 2, 1)
    disc = (yy - (r - 1)) ** 2 + (xx - (r - 1)) ** 2 <= (r - 1) ** 2 + 1          # touches the top and the left border
    planes += [lone, (yy + xx) % 2 == 0, frame, disc, xx < 64]
    planes += [g.random((H, W)) < p for p in (0.02, 0.5, 0.98)]
    planes = np.stack(planes)
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def case_dist2(H, W, to, border):
    if border:                                                        # (the plain maps are computed once)
        out = np.minimum(case_dist2(H, W, to, False), np_border2(H, W)[None])
    else:
        out = np.stack([np_dist2(p, to) for p in case_planes(H, W)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_centers(H, W):
    return np.stack([np_center(p) for p in case_planes(H, W)])


@functools.lru_cache(maxsize=None)
def case_bmaps(H, W):
    return np.stack([np_bmap(p) for p in case_planes(H, W)])


def dev(ops, flags, dtype, seed=1):
    """bool planes as a device tensor of `dtype`; float32 planes carry every kind of unset value (NaN, -0.0, negatives) and of set value"""
    flags = np.asarray(flags, bool)
    if dtype == torch.float32:
        g = np.random.default_rng(seed)
        on = g.choice(np.array([1e-30, 2.0, np.inf], np.float32), size=flags.shape)
        off = g.choice(np.array([np.nan, -0.0, 0.0, -1.5, -np.inf], np.float32), size=flags.shape)
        return torch.from_numpy(np.where(flags, on, off).astype(np.float32)).to(ops.device)
    if dtype == torch.uint8:
        return torch.from_numpy(np.where(flags, np.uint8(1 + 254 * (flags.sum() % 2)), np.uint8(0))).to(ops.device)
    return torch.from_numpy(flags.copy()).to(ops.device)


def same(got, want, what=""):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:5].tolist())


# ---------------------------------------------------------------------------------------------------- the oracle itself
def random_planes(seed, count=200):
    g = np.random.default_rng(seed)
    for _ in range(count):
        H, W = g.integers(1, 41, 2)
        yield g.random((H, W)) < g.choice([0.02, 0.3, 0.5, 0.9, 0.98])


def test_oracle_equals_scipy_edt():
    ndi = pytest.importorskip("scipy.ndimage")
    for k, f in enumerate(random_planes(43)):
        if not f.all():
            assert np.array_equal(np_dist2(f, "unset"), np.rint(ndi.distance_transform_edt(f) ** 2).astype(np.int32)), k
        if f.any():
            assert np.array_equal(np_dist2(f, "set"), np.rint(ndi.distance_transform_edt(~f) ** 2).astype(np.int32)), k


def test_oracle_border_map_is_the_padded_plane_cropped():
    for k, f in enumerate(random_planes(44)):
        for to in ("unset", "set"):
            pad = np.full((f.shape[0] + 2, f.shape[1] + 2), to == "set")      # seeds all round
            pad[1:-1, 1:-1] = f
            assert np.array_equal(np_dist2(f, to, True), np_dist2(pad, to)[1:-1, 1:-1]), (k, to)
    assert (np_dist2(np.ones((3, 4), bool), "unset") == FAR).all() and (np_dist2(np.zeros((3, 4), bool), "set") == FAR).all()
    assert np_dist2(np.ones((3, 5), bool), "unset", True).tolist() == [[1, 1, 1, 1, 1], [1, 4, 4, 4, 1], [1, 1, 1, 1, 1]]


def test_oracle_center_disc_lies_inside_the_mask():
    for k, f in enumerate(random_planes(45)):
        cy, cx, d2 = np_center(f).tolist()
        if not f.any():
            assert (cy, cx, d2) == (-1, -1, 0)
            continue
        assert f[cy, cx] and d2 >= 1 and disc_inside(f, cy, cx, d2), k
        assert not disc_inside(f, cy, cx, d2 + 1), k                  # ... and no larger disc does: d2 is the distance to a seed
    assert np_center(np.ones((5, 7), bool)).tolist() == [2, 2, 9]     # ties: the lowest row-major index


def test_oracle_bmap_on_hand_cases():
    assert np_bmap(np.ones((1, 1), bool)).tolist() == [[False]]
    assert np_bmap(np.array([[0, 1, 1, 0]], bool)).astype(int).tolist() == [[1, 0, 1, 0]]
    sq = np.zeros((4, 4), bool)
    sq[1:3, 1:3] = True
    assert np_bmap(sq).astype(int).tolist() == [[1, 1, 1, 0], [1, 0, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]]
    assert np_boundary_f([0, 3, 0, 0]) == (1.0, 0.0, 0.0) and np_boundary_f([3, 0, 0, 0]) == (0.0, 1.0, 0.0)
    assert np_boundary_f([0, 0, 0, 0]) == (1.0, 1.0, 1.0) and np_boundary_f([4, 2, 2, 1]) == (0.5, 0.5, 0.5)


# ---------------------------------------------------------------------------------------------------- distance maps
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_distance_maps_equal_the_oracle(ops, dtype, shape):
    H, W = shape
    t = dev(ops, case_planes(H, W), dtype)
    for to, border in MODES:
        same(ops.mask_distance(t, to=to, border=border), case_dist2(H, W, to, border), (to, border))
    if shape == (130, 70):
        want = case_dist2(H, W, "unset", False)
        assert want[6, 0, W - 1] == (H - 1) ** 2 + (W - 1) ** 2 and want[1].min() == FAR      # the lone seed: the plane's diagonal; no seed: FAR


@pytest.mark.parametrize("shape", [(33, 65), (5, 200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_index_list_chunking_and_workspace_poison(ops, shape):
    H, W = shape
    planes = case_planes(H, W)
    n = len(planes)
    index = [3, 0, 0, -1, n, 2, 3, 10, 1, 6]                          # repeats, reorders, entries outside [0, n): the empty plane
    picked = np.stack([planes[r] if 0 <= r < n else np.zeros((H, W), bool) for r in index])
    idx = torch.tensor(index, dtype=torch.int32, device=ops.device)
    t = dev(ops, planes, torch.float32)
    for to, border in MODES:
        want = np.stack([np_dist2(p, to, border) for p in picked])
        same(ops.mask_distance(t, index=idx, to=to, border=border), want)
        same(ops.mask_distance(t, index=idx, to=to, border=border, max_workspace_bytes=1), want)            # one row per chunk
        same(ops.mask_distance(t, to=to, border=border, max_workspace_bytes=1), case_dist2(H, W, to, border))
    same(ops.mask_centers(t, index=idx), np.stack([np_center(p) for p in picked]))
    same(ops.mask_centers(t, index=idx, max_workspace_bytes=1), np.stack([np_center(p) for p in picked]))
    same(ops.mask_boundaries(t, index=idx), np.stack([np_bmap(p) for p in picked]).astype(np.uint8))
    # the workspace's previous contents do not matter: the library's own entry on a workspace of 0xFF bytes and on one of zeros
    u8 = dev(ops, planes, torch.uint8)
    fn = ops._cdll_raw.psalm_mask_distance_workspace
    fn.restype = ctypes.c_long
    nbytes = fn(n, H, W)
    assert nbytes >= n * (H * W + 2 * (H + 2) * W) * 2
    for to, border in MODES:
        outs = []
        for fill in (0xFF, 0x00):
            ws = torch.full((nbytes + 256,), fill, dtype=torch.uint8, device=ops.device)
            off = (-ws.data_ptr()) % 256
            out = torch.full((n, H, W), -7, dtype=torch.int32, device=ops.device)
            rc = ops.lib.psalm_mask_distance(ops._p(u8), 1, n, H, W, ctypes.c_void_p(0), n, int(to == "set"), int(border), ops._p(out),
                                             ctypes.c_void_p(ws.data_ptr() + off), ctypes.c_long(nbytes), ops._stream())
            assert rc == 0
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], case_dist2(H, W, to, border))
    none = ops.mask_distance(torch.zeros(0, 5, 7, dtype=torch.uint8, device=ops.device))
    assert tuple(none.shape) == (0, 5, 7) and none.dtype == torch.int32
    assert tuple(ops.mask_centers(t, index=idx[:0]).shape) == (0, 3) and tuple(ops.mask_boundaries(t, index=idx[:0]).shape) == (0, H, W)


# ---------------------------------------------------------------------------------------------------- centres
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_centers_equal_the_oracle_and_their_discs_lie_inside(ops, dtype, shape):
    H, W = shape
    planes = case_planes(H, W)
    t = dev(ops, planes, dtype)
    got = ops.mask_centers(t)
    same(got, case_centers(H, W))
    same(ops.mask_centers(t, dist2=ops.mask_distance(t, border=True)), case_centers(H, W))
    same(E.mask_centers(t.cpu() if dtype != torch.bool else t, ops=ops), case_centers(H, W))
    masks = t.cpu().numpy()
    for k, (cy, cx, d2) in enumerate(got.cpu().tolist()):
        if not planes[k].any():
            assert (cy, cx, d2) == (-1, -1, 0)                        # the empty plane's row
            continue
        assert masks[k, cy, cx] > 0 and d2 >= 1 and disc_inside(planes[k], cy, cx, d2), k


def test_center_ties_go_to_the_lowest_index(ops):
    m = np.zeros((3, 20, 40), bool)
    m[0, 2:9, 3:10] = m[0, 2:9, 25:32] = True                         # two equal squares side by side: the left one's centre
    m[1, 11:18, 3:10] = m[1, 2:9, 25:32] = True                       # the upper one, though it lies to the right
    m[2, 5:10, 5:12] = True                                           # a 5 x 7 rectangle: three pixels at depth 3, the first one
    got = ops.mask_centers(torch.from_numpy(m).to(ops.device)).cpu().tolist()
    assert got == [[5, 6, 16], [5, 28, 16], [7, 7, 9]]
    assert got == [np_center(p).tolist() for p in m]


# ---------------------------------------------------------------------------------------------------- boundary maps and counts
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_boundary_maps_equal_the_oracle(ops, dtype, shape):
    H, W = shape
    t = dev(ops, case_planes(H, W), dtype)
    same(ops.mask_boundaries(t), case_bmaps(H, W).astype(np.uint8))
    same(E.mask_boundaries(t, ops=ops), case_bmaps(H, W).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def pair_case():
    """masks at (70, 86) and the pairs: identical, a mask and its one-pixel shift, a mask and an empty one (both ways), both empty, disjoint
    blobs, noise against a blob"""
    H, W = 70, 86
    yy, xx = np.indices((H, W))
    blob = (yy - 30) ** 2 + (xx - 35) ** 2 <= 18 ** 2
    blob[25:32, 30:38] = False                                        # with a hole
    shifted = np.roll(blob, 1, axis=1)
    small = (yy - 60) ** 2 + (xx - 75) ** 2 <= 6 ** 2                 # disjoint from blob, touches no border
    empty = np.zeros((H, W), bool)
    noise = np.random.default_rng(7).random((H, W)) < 0.5
    pred = np.stack([blob, shifted, empty, small, noise])
    gt = np.stack([blob, empty, small, np.ones((H, W), bool)])
    pairs = [(0, 0), (1, 0), (0, 1), (2, 0), (2, 1), (3, 0), (0, 2), (4, 0), (1, 3), (0, 0)]
    return pred, gt, pairs


@functools.lru_cache(maxsize=None)
def pair_counts(bound):
    pred, gt, pairs = pair_case()
    return np.stack([np_boundary_counts(pred[p], gt[t], bound) for p, t in pairs])


@pytest.mark.parametrize("bound", [0, 1, 3, "davis"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_boundary_counts_and_f(ops, dtype, bound):
    pred, gt, pairs = pair_case()
    if bound == "davis":
        bound = E.davis_bound((70, 86))
        assert bound == 1 and E.davis_bound((480, 854)) == 8 and E.davis_bound((1, 9, 9), 5) == 5 and E.davis_bound((70, 86), 0.05) == 6
    want = pair_counts(bound)
    got = E.boundary_counts(dev(ops, pred, dtype), dev(ops, gt, torch.uint8 if dtype == torch.float32 else torch.float32), pairs, bound, ops=ops)
    assert got.dtype == torch.int64 and got.device.type == ops.device.type
    same(got, want)
    assert want[0, 0] == want[0, 1] == want[0, 2] == want[0, 3] > 0 and want[2].tolist()[1:] == [0, 0, 0] and want[4].tolist() == [0, 0, 0, 0]
    if bound == 0:
        assert 0 < want[1, 2] < want[1, 0]                            # the shift: some boundary pixels coincide, not all
    if bound >= 1:
        assert want[1, 2] == want[1, 0] and want[1, 3] == want[1, 1]  # ... and all of them lie within one pixel
    assert want[6].tolist()[2:] == [0, 0]                             # disjoint blobs, further apart than any bound here
    prec, rec, f = E.boundary_f(got)
    assert prec.dtype == rec.dtype == f.dtype == np.float64
    for k, c in enumerate(want):
        p, r, ff = np_boundary_f(c)
        assert abs(prec[k] - p) <= 1e-12 and abs(rec[k] - r) <= 1e-12 and abs(f[k] - ff) <= 1e-12, k
    assert (prec[0], rec[0], f[0]) == (1.0, 1.0, 1.0)
    assert (prec[2], rec[2], f[2]) == (0.0, 1.0, 0.0) and (prec[3], rec[3], f[3]) == (1.0, 0.0, 0.0) and (prec[4], rec[4], f[4]) == (1.0, 1.0, 1.0)


def test_boundary_counts_on_every_shape(ops):
    """the pair list over the case planes of the smallest shapes: planes in several pairs, every plane's maps made once"""
    for H, W in ((1, 1), (1, 67), (67, 1), (5, 200)):
        planes = case_planes(H, W)
        n = len(planes)
        pairs = [(k, (k * 5 + 3) % n) for k in range(n)] + [(2, 2), (n - 1, 0)]
        want = np.stack([np_boundary_counts(planes[p], planes[t], 2) for p, t in pairs])
        t = dev(ops, planes, torch.bool)
        same(E.boundary_counts(t, t, pairs, 2, ops=ops), want, (H, W))
    assert tuple(E.boundary_counts(t, t, [], 2, ops=ops).shape) == (0, 4)


def test_boundary_f_special_cases_and_jf_meters(ops):
    p, r, f = E.boundary_f(torch.tensor([[0, 5, 0, 0], [5, 0, 0, 0], [0, 0, 0, 0], [4, 8, 1, 6], [3, 3, 0, 0]]))
    assert p.tolist() == [1.0, 0.0, 1.0, 0.25, 0.0] and r.tolist() == [0.0, 1.0, 1.0, 0.75, 0.0]
    assert f.tolist() == [0.0, 0.0, 1.0, 2 * 0.25 * 0.75 / (0.25 + 0.75), 0.0]
    m = E.JFMeters()
    # pair 0: J = 30 / 40, F from (P, R) = (1 / 2, 1 / 4) = 1 / 3; pair 1: an empty union, J = 1, no boundaries at all, F = 1
    m.update(torch.tensor([30, 0]), torch.tensor([40, 0]), torch.tensor([[8, 8, 4, 2], [0, 0, 0, 0]]))
    res = m.results()
    assert res["n"] == 2 and res["J"] == (0.75 + 1.0) / 2 and abs(res["F"] - (1 / 3 + 1.0) / 2) <= 1e-15
    assert abs(res["J&F"] - (res["J"] + res["F"]) / 2) <= 1e-15
    m.update(torch.tensor([[100, 10]]), torch.tensor([[120, 20]]), torch.tensor([[2, 2, 2, 2]]))      # iou_counts' (P,2) form: the foreground column
    res = m.results()
    assert res["n"] == 3 and abs(res["J"] - (0.75 + 1.0 + 0.5) / 3) <= 1e-15 and abs(res["F"] - (1 / 3 + 2.0) / 3) <= 1e-15
    m.all_reduce()                                                    # no process group: the sums stay
    assert m.results() == res
    # J from the device's own counts: iou_counts and boundary_counts on one pair list
    pred, gt, pairs = pair_case()
    pairs = pairs[:2]
    tp, tg = torch.from_numpy(pred), torch.from_numpy(gt.astype(np.uint8))
    inter, union, _ = E.iou_counts(tp, tg, pairs, ops=ops)
    m = E.JFMeters()
    m.update(inter, union, E.boundary_counts(tp, tg, pairs, 1, ops=ops))
    j = [(pred[a] & gt[b]).sum() / (pred[a] | gt[b]).sum() for a, b in pairs]
    fs = [np_boundary_f(np_boundary_counts(pred[a], gt[b], 1))[2] for a, b in pairs]
    res = m.results()
    assert abs(res["J"] - np.mean(j)) <= 1e-12 and abs(res["F"] - np.mean(fs)) <= 1e-12 and res["n"] == 2


# ---------------------------------------------------------------------------------------------------- errors
def test_error_returns(ops):
    m = torch.ones(2, 8, 9, dtype=torch.uint8, device=ops.device)
    for fn in (ops.mask_distance, ops.mask_centers, ops.mask_boundaries, lambda t: ops.boundary_counts(t, t, pi, pi, 1)):
        pi = torch.zeros(1, dtype=torch.int32, device=ops.device)
        with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
            fn(m.to(torch.int32))
        with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
            fn(m[0])
        for shape in ((1, 0, 9), (1, 8, 0)):
            with pytest.raises(PsalmHipError, match="1 <= H, W <= 16384"):
                fn(torch.zeros(shape, dtype=torch.uint8, device=ops.device))
        with pytest.raises(PsalmHipError, match="1 <= H, W <= 16384"):
            fn(torch.zeros(1, 1, 16385, dtype=torch.uint8, device=ops.device))
        with pytest.raises(PsalmHipError, match="1 <= H, W <= 16384"):
            fn(torch.zeros(1, 16385, 1, dtype=torch.uint8, device=ops.device))
    for bad in ("inside", "Unset", None, 0):
        with pytest.raises(PsalmHipError, match="to = "):
            ops.mask_distance(m, to=bad)
        with pytest.raises(PsalmHipError, match="to = "):
            E.mask_distance(m, to=bad, ops=ops)
    with pytest.raises(PsalmHipError, match="border"):
        ops.mask_distance(m, border=1)
    with pytest.raises(PsalmHipError, match="index"):
        ops.mask_distance(m, index=torch.zeros(2, dtype=torch.int64, device=ops.device))
    with pytest.raises(PsalmHipError, match="max_workspace_bytes"):
        ops.mask_distance(m, max_workspace_bytes=-1)
    with pytest.raises(PsalmHipError, match="out"):
        ops.mask_distance(m, out=torch.zeros(2, 8, 8, dtype=torch.int32, device=ops.device))
    with pytest.raises(PsalmHipError, match="dist2"):
        ops.mask_centers(m, dist2=torch.zeros(2, 8, 9, dtype=torch.float32, device=ops.device))
    for bad in (-1, 32768, 1.5, True, None):
        with pytest.raises(PsalmHipError, match="0 <= bound <= 32767"):
            E.boundary_counts(m, m, [(0, 1)], bad, ops=ops)
    for pairs in ([(0, 2)], [(2, 0)], [(-1, 0)], [(0, 0), (1, -1)]):
        with pytest.raises(PsalmHipError, match="pair index out of range"):
            E.boundary_counts(m, m, pairs, 1, ops=ops)
    with pytest.raises(PsalmHipError, match="against targets"):
        E.boundary_counts(m, m[:, :, :8].contiguous(), [(0, 0)], 1, ops=ops)
    with pytest.raises(PsalmHipError, match="not supported"):
        E.boundary_counts(m, m.to(torch.int32), [(0, 0)], 1, ops=ops)
    for fn in (E.mask_distance, E.mask_centers, E.mask_boundaries):
        with pytest.raises(PsalmHipError):
            fn(torch.zeros(3, 4), ops=ops)
        with pytest.raises(PsalmHipError, match="not supported"):
            fn(torch.zeros(1, 3, 4, dtype=torch.float64), ops=ops)
    if not ops.is_emu:
        with pytest.raises(PsalmHipError, match="GPU tensors"):
            ops.mask_distance(m.cpu())
    # the library's own error codes
    raw = ops._cdll_raw
    wd, wb = raw.psalm_mask_distance_workspace, raw.psalm_boundary_counts_workspace
    wd.restype = wb.restype = ctypes.c_long
    assert wd(-1, 8, 8) == -1 and wd(65536, 8, 8) == -1 and wd(1, 0, 8) == -1 and wd(1, 8, 0) == -1 and wd(1, 16385, 8) == -1 and wd(1, 8, 16385) == -1
    assert wd(0, 8, 8) == 0 and wd(1, 16384, 16384) > 0 and wd(2, 8, 9) % 256 == 0
    assert wb(1, -1, 8, 8) == -1 and wb(1, 1, 0, 8) == -1 and wb(1, 1, 8, 16385) == -1 and wb(65535, 1, 8, 8) == -1 and wb(0, 0, 8, 8) == 0
    assert wb(2, 3, 8, 9) >= 2 * 5 * 72 + wd(5, 8, 9)
    p, L, null = ops._p, ctypes.c_long, ctypes.c_void_p(0)
    ws = ops._aligned_ws("test_43", 1 << 16)
    out = ops.empty(2, 8, 9, dtype=torch.int32)

    def dist(H=8, W=9, to=0, border=0, mm=2, ws_ptr=None, ws_bytes=1 << 16):
        return ops.lib.psalm_mask_distance(p(m), 1, 2, H, W, null, mm, to, border, p(out), p(ws) if ws_ptr is None else ws_ptr, L(ws_bytes), ops._stream())

    assert dist() == 0 and (out.cpu().numpy() == FAR).all()
    assert dist(border=1) == 0 and out.cpu()[0].tolist() == np_dist2(np.ones((8, 9), bool), "unset", True).tolist()
    assert dist(H=0) == -1 and b"1 <= H, W <= 16384" in ops.lib.psalm_last_error()
    assert dist(W=16385) == -1 and b"1 <= H, W <= 16384" in ops.lib.psalm_last_error()
    assert dist(to=2) == -1 and b"to_set" in ops.lib.psalm_last_error()
    assert dist(border=2) == -1 and dist(mm=1) == -1 and dist(mm=0, W=9) == -1
    assert dist(ws_bytes=100) == -1 and b"workspace" in ops.lib.psalm_last_error()
    assert dist(ws_ptr=ctypes.c_void_p(ws.data_ptr() + 64)) == -1 and b"256-byte aligned" in ops.lib.psalm_last_error()
    counts = ops.empty(1, 4, dtype=torch.int64)
    pi = torch.zeros(1, dtype=torch.int32, device=ops.device)

    def count(bound=1, H=8, W=9, ws_bytes=1 << 16):
        return ops.lib.psalm_boundary_counts(p(m), 1, 2, null, 2, p(m), 1, 2, null, 2, H, W, p(pi), p(pi), 1, bound, p(counts), p(ws), L(ws_bytes), ops._stream())

    assert count() == 0 and counts.cpu().tolist() == [[0, 0, 0, 0]]
    assert count(bound=-1) == -1 and b"0 <= bound <= 32767" in ops.lib.psalm_last_error()
    assert count(bound=32768) == -1 and count(bound=32767) == 0
    assert count(H=16385) == -1 and count(ws_bytes=100) == -1
    cen, slots = ops.empty(2, 3, dtype=torch.int32), ops.empty(2, dtype=torch.int64)
    assert ops.lib.psalm_mask_centers(p(m), 1, 2, 0, 9, null, 2, p(out), p(slots), p(cen), ops._stream()) == -1
    assert ops.lib.psalm_mask_centers(p(m), 1, 2, 8, 9, null, 1, p(out), p(slots), p(cen), ops._stream()) == -1
    assert ops.lib.psalm_mask_boundaries(p(m), 1, 2, 8, 16385, null, 2, p(m), ops._stream()) == -1
    # a pair index outside the planes, given to the library itself: counted as nothing
    pi[0] = 5
    assert count() == 0 and counts.cpu().tolist() == [[0, 0, 0, 0]]
