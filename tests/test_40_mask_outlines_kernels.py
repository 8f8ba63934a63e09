"""csrc/outlines.hip -- psalm_mask_outline_totals / psalm_mask_outlines / psalm_mask_fill_polygons -- against the sequential oracle of
tests/outlines_util.py.  Integer results: every comparison is np.array_equal.  Runs on the host emulation of the kernel sources and, marked gpu,
on the MI355X -- where the checkerboard and the spiral at (70, 86) are the test that no launch reads what another block of it writes (the
emulation runs one block at a time and cannot show that)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from components_util import np_components
from ops_backend import ops  # noqa: F401  (fixture)
from outlines_util import np_fill, np_outlines, np_tables, tables_of
from psalm_amd.hip_ops import PsalmHipError

DTYPES = [torch.float32, torch.uint8, torch.bool]
IDS = ["f32", "u8", "bool"]
CONN = [4, 8]
SHAPES = [(1, 1), (1, 67), (67, 1), (33, 65), (70, 86)]             # (70, 86): 3 x 3 ragged 32-tiles, 6177 vertices -- several scan blocks


# ---------------------------------------------------------------------------------------------------- planes
def spiral(H, W):
    """a one-pixel-wide path that winds inwards with pitch 2: one ring, as long as a ring of the plane can be"""
    m = np.zeros((H, W), bool)
    k = 0
    while True:
        t, l, b, r = 2 * k, 2 * k, H - 1 - 2 * k, W - 1 - 2 * k
        if b - t < 2 or r - l < 2:
            break
        m[t, l:r + 1] = m[t:b + 1, r] = m[b, l:r + 1] = True
        m[t + 2:b + 1, l] = True                                      # the left stroke stops short of the top: the loop stays open ...
        m[t + 2, l:l + 3] = True                                      # ... and runs into the next loop's top row
        k += 1
    return m


def comb(H, W):
    m = np.zeros((H, W), bool)
    m[:, 0::2] = True
    m[-1] = True
    return m


def nested(H, W):
    m = np.zeros((H, W), bool)
    for k in range(4):                                                # four rings, walls and gaps two pixels thick
        m[4 * k:H - 4 * k, 4 * k:W - 4 * k] = True
        m[4 * k + 2:H - 4 * k - 2, 4 * k + 2:W - 4 * k - 2] = False
    return m


@functools.lru_cache(maxsize=None)
def case_planes(H, W):
    g = np.random.default_rng(H * 1000 + W)
    yy, xx = np.indices((H, W))
    planes = [np.zeros((H, W), bool), np.ones((H, W), bool), (yy + xx) % 2 == 0, spiral(H, W), comb(H, W), yy == xx, nested(H, W)]
    planes += [g.random((H, W)) < p for p in (0.3, 0.41, 0.59, 0.8)]
    planes = np.stack(planes)
    planes.setflags(write=False)
    return planes


@functools.lru_cache(maxsize=None)
def case_tables(H, W, conn):
    return np_tables(case_planes(H, W), conn)


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


def check_tables(got, want):
    for name, g, w in zip(("ring_count", "vertex_count", "rings", "vertices"), got, want):
        g = g.cpu().numpy()
        assert g.dtype == np.int32 and g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:5].tolist())


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_properties_on_random_planes():
    """sum of the signed areas = set pixels; outer rings = components; holes = components of the padded complement under the complementary
    connectivity, minus the outside; fill(outlines(f)) == f; first vertices distinct and sorted"""
    g = np.random.default_rng(40)
    for k in range(300):
        H, W = g.integers(1, 41, 2)
        if k % 3:
            H, W = min(H, 16), min(W, 16)                             # (the filler is plain Python: most planes small)
        f = g.random((H, W)) < g.choice([0.3, 0.41, 0.59, 0.8])
        for conn in CONN:
            rings = np_outlines(f, conn)
            assert sum(a for _, a in rings) == f.sum(), (k, conn)
            assert sum(1 for _, a in rings if a > 0) == np_components(f, conn)[1], (k, conn)
            pad = np.ones((H + 2, W + 2), bool)
            pad[1:-1, 1:-1] = ~f
            assert sum(1 for _, a in rings if a < 0) == np_components(pad, 4 if conn == 8 else 8)[1] - 1, (k, conn)
            assert all(a != 0 for _, a in rings)
            firsts = [(c[0][1], c[0][0]) for c, _ in rings]
            assert firsts == sorted(set(firsts)), (k, conn)
            assert all(c[0] == min(c, key=lambda v: (v[1], v[0])) and c.count(c[0]) == 1 for c, _ in rings)
            assert np.array_equal(np_fill([c for c, _ in rings], H, W), f), (k, conn)


def test_oracle_outer_rings_equal_scipy_label():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(41)
    for k in range(300):
        H, W = g.integers(1, 41, 2)
        f = g.random((H, W)) < g.choice([0.3, 0.41, 0.59, 0.8])
        for conn in CONN:
            n = ndi.label(f, structure=np.ones((3, 3)) if conn == 8 else None)[1]
            assert sum(1 for _, a in np_outlines(f, conn) if a > 0) == n, (k, conn)


def test_oracle_on_hand_cases():
    assert np_outlines(np.ones((1, 1), bool), 8) == [([(0, 0), (1, 0), (1, 1), (0, 1)], 1)]
    diag = np.eye(2, dtype=bool)
    assert np_outlines(diag, 8) == [([(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)], 2)]
    assert np_outlines(diag, 4) == [([(0, 0), (1, 0), (1, 1), (0, 1)], 1), ([(1, 1), (2, 1), (2, 2), (1, 2)], 1)]
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    ring[2, 2] = True
    for conn in CONN:
        got = np_outlines(ring, conn)
        assert [a for _, a in got] == [25, -9, 1]
        assert got[1][0] == [(1, 1), (1, 4), (4, 4), (4, 1)]          # a hole runs the other way round
    assert np_fill([[(0, 0), (4, 0), (0, 4)]], 4, 4).astype(int).tolist() == [[1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------------- kernel against oracle
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_outlines_and_fill_round_trip(ops, dtype, conn, shape):
    """empty, full, checkerboard, spiral, comb, diagonal, nested rings and noise at four densities in ONE call (edge totals from 0 to the most a
    plane can have): the oracle's tables; filling them gives the planes back; outer rings and areas agree with mask_components / mask_boxes"""
    H, W = shape
    planes = case_planes(H, W)
    want = case_tables(H, W, conn)
    t = dev(ops, planes, dtype)
    got = ops.mask_outlines(t, connectivity=conn)
    check_tables(got, want)
    if shape == (70, 86):
        assert want[0][3] == 1 and planes[3].sum() > 2500             # the spiral: ONE ring around thousands of pixels, two edges and more each
        assert want[0][2] == (H * W // 2 if conn == 4 else 1 + (H - 2) * (W - 2) // 2)       # checkerboard: a ring per pixel / one + a hole per unset inner pixel
    filled = ops.mask_fill_polygons(got[2], got[3], planes.shape)
    assert filled.dtype == torch.uint8 and np.array_equal(filled.cpu().numpy(), planes.astype(np.uint8))
    rings = got[2].cpu().numpy()
    outer = np.bincount(rings[rings[:, 3] > 0, 0], minlength=len(planes))
    area = np.bincount(rings[:, 0], weights=rings[:, 3], minlength=len(planes)).astype(np.int64)
    assert np.array_equal(outer, ops.mask_components(t, connectivity=conn, want_table=False)[1].cpu().numpy())
    assert np.array_equal(area, ops.mask_boxes(t)[1].cpu().numpy())


@pytest.mark.parametrize("conn", CONN)
def test_index_list_chunking_and_empty_batch(ops, conn):
    H, W = 33, 65
    planes = case_planes(H, W)
    n = len(planes)
    index = [3, 0, 0, -1, n, 2, 3, 10, 1]                             # repeats and entries outside [0, n): the empty plane
    picked = np.stack([planes[r] if 0 <= r < n else np.zeros((H, W), bool) for r in index])
    want = np_tables(picked, conn)
    t = dev(ops, planes, torch.uint8)
    idx = torch.tensor(index, dtype=torch.int32, device=ops.device)
    check_tables(ops.mask_outlines(t, index=idx, connectivity=conn), want)
    check_tables(ops.mask_outlines(t, index=idx, connectivity=conn, max_workspace_bytes=1), want)            # one row per chunk: the same tensors
    check_tables(ops.mask_outlines(dev(ops, planes, torch.float32), connectivity=conn, max_workspace_bytes=1), case_tables(H, W, conn))
    got = ops.mask_outlines(t, index=idx, connectivity=conn)
    for kw in ({}, {"max_workspace_bytes": 1}):
        assert np.array_equal(ops.mask_fill_polygons(got[2], got[3], picked.shape, **kw).cpu().numpy(), picked.astype(np.uint8))
    none = ops.mask_outlines(t, index=torch.zeros(0, dtype=torch.int32, device=ops.device), connectivity=conn)
    assert [tuple(v.shape) for v in none] == [(0,), (0,), (0, 4), (0, 2)]
    none = ops.mask_outlines(torch.zeros(0, 5, 7, dtype=torch.uint8, device=ops.device), connectivity=conn)
    assert [tuple(v.shape) for v in none] == [(0,), (0,), (0, 4), (0, 2)]
    blank = ops.mask_outlines(torch.zeros(2, 5, 7, dtype=torch.uint8, device=ops.device), connectivity=conn)
    assert [tuple(v.shape) for v in blank] == [(2,), (2,), (0, 4), (0, 2)] and not blank[0].cpu().numpy().any()
    assert tuple(ops.mask_fill_polygons(blank[2], blank[3], (0, 5, 7)).shape) == (0, 5, 7)
    assert not ops.mask_fill_polygons(blank[2], blank[3], (2, 5, 7)).cpu().numpy().any()


def test_hand_cases_on_the_kernel(ops):
    one = ops.mask_outlines(torch.ones(1, 1, 1, dtype=torch.uint8, device=ops.device))
    assert one[2].cpu().tolist() == [[0, 0, 4, 1]] and one[3].cpu().tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    diag = torch.eye(2, dtype=torch.uint8, device=ops.device)[None]
    assert ops.mask_outlines(diag, connectivity=8)[2].cpu().tolist() == [[0, 0, 8, 2]]
    assert ops.mask_outlines(diag, connectivity=4)[2].cpu().tolist() == [[0, 0, 4, 1], [0, 4, 4, 1]]
    ring = np.ones((1, 5, 5), np.uint8)
    ring[0, 1:4, 1:4] = 0
    ring[0, 2, 2] = 1
    got = ops.mask_outlines(torch.from_numpy(ring).to(ops.device))
    assert got[2].cpu().numpy()[:, 3].tolist() == [25, -9, 1] and got[0].cpu().tolist() == [3] and got[1].cpu().tolist() == [12]


# ---------------------------------------------------------------------------------------------------- the fill rule on general polygons
def general_polygons(H, W):
    star = [(2, 1), (W - 3, H - 2), (1, H // 2), (W - 1, H // 3), (4, H - 1)]                 # a pentagram: crosses itself
    tri = [(1, 1), (W - 1, 3), (5, H - 1)]
    return [
        [[(0, 0), (8, 0), (0, 8)]],                                   # the hypotenuse passes through pixel centres: they stay unset
        [[(0, 0), (8, 8), (0, 8)], [(W, 0), (W - 6, 6), (W, 12)]],    # ... the other way round; an edge along the plane's right border
        [tri],
        [star],
        [tri, tri],                                                   # a ring given twice fills to nothing
        [[(0, 0), (W, 0), (W, H), (0, H)], [(3, 2), (3, H - 2), (W - 2, H - 2), (W - 2, 2)]],      # the whole plane with a hole
        [[(1, 3), (W - 1, 3)], [(2, 2), (2, 2), (9, 2), (9, 11)]],    # degenerate rings: a two-vertex ring, a repeated vertex
        [],
    ]


def test_fill_equals_the_rule_on_general_polygons(ops):
    H, W = 23, 37
    polys = general_polygons(H, W)
    want = np.stack([np_fill(p, H, W) for p in polys]).astype(np.uint8)
    assert want[0, 3, 4] == 0 and want[0, 3, 3] == 1 and want[0].sum() == 28 and not want[4].any() and want[5].sum() == H * W - (H - 4) * (W - 5)
    rings, verts = tables_of(polys)
    r, v = torch.from_numpy(rings).to(ops.device), torch.from_numpy(verts).to(ops.device)
    assert np.array_equal(ops.mask_fill_polygons(r, v, want.shape).cpu().numpy(), want)
    assert np.array_equal(ops.mask_fill_polygons(r, v, want.shape, max_workspace_bytes=1).cpu().numpy(), want)
    order = np.arange(len(rings))[::-1].copy()                        # the ring rows in any order, the planes unsorted: the same planes
    assert np.array_equal(ops.mask_fill_polygons(torch.from_numpy(rings[order]).to(ops.device), v, want.shape).cpu().numpy(), want)
    bad = rings.copy()
    bad[0] = [0, len(verts) - 1, 3, 0]                                # a vertex range that leaves the table, a plane outside the call: passed over
    bad[1] = [99, 0, 3, 0]
    want_bad = want.copy()
    want_bad[0] = 0
    want_bad[1] = np_fill(polys[1][1:], H, W)
    assert np.array_equal(ops.mask_fill_polygons(torch.from_numpy(bad).to(ops.device), v, want.shape).cpu().numpy(), want_bad)
    out = torch.full((len(polys), H, W), 7, dtype=torch.uint8, device=ops.device)
    assert ops.mask_fill_polygons(r, v, want.shape, out=out) is out and np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- errors
def test_error_returns(ops):
    m = torch.ones(2, 8, 9, dtype=torch.uint8, device=ops.device)
    for bad in (5, 0, 6, True, None):
        with pytest.raises(PsalmHipError, match="connectivity"):
            ops.mask_outlines(m, connectivity=bad)
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_outlines(m.to(torch.int32))
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_outlines(m[0])
    with pytest.raises(PsalmHipError, match="index"):
        ops.mask_outlines(m, index=torch.zeros(2, dtype=torch.int64, device=ops.device))
    with pytest.raises(PsalmHipError, match="max_workspace_bytes"):
        ops.mask_outlines(m, max_workspace_bytes=-1)
    got = ops.mask_outlines(m)
    for r, v in ((got[2][:, :3], got[3]), (got[2].to(torch.int64), got[3]), (got[2], got[3].reshape(-1)), (got[2], got[3].to(torch.float32)), (None, got[3])):
        with pytest.raises(PsalmHipError, match="rings|vertices"):
            ops.mask_fill_polygons(r, v, (2, 8, 9))
    for shape in ((8, 9), (2, 8, -9), (2, 8.5, 9), None, (65536, 8, 9)):
        with pytest.raises(PsalmHipError, match="shape|planes"):
            ops.mask_fill_polygons(got[2], got[3], shape)
    with pytest.raises(PsalmHipError, match="out"):
        ops.mask_fill_polygons(got[2], got[3], (2, 8, 9), out=torch.zeros(2, 8, 8, dtype=torch.uint8, device=ops.device))
    if not ops.is_emu:
        with pytest.raises(PsalmHipError, match="GPU tensors"):
            ops.mask_outlines(m.cpu())
    # the library's own error codes
    raw = ops._cdll_raw
    wo, wf = raw.psalm_mask_outlines_workspace, raw.psalm_mask_fill_polygons_workspace
    wo.restype = wf.restype = ctypes.c_long
    assert wo(-1, 8, 8, 4) == -1 and wo(65536, 8, 8, 4) == -1 and wo(1, 32768, 16384, 4) == -1 and wo(1, 8, 8, -1) == -1 and wo(1, 8, 8, 163) == -1
    assert wo(3, 8, 8, 0) == 0 and wo(0, 8, 8, 4) == 0 and wo(1, 8, 8, 162) > 0
    assert wf(-1, 8, 8) == -1 and wf(1, 32768, 16384) == -1 and wf(2, 8, 9) == 2 * 8 * 10 * 4
    counts = ops.empty(3, 2, dtype=torch.int32)
    rings, verts, ws = ops.empty(8, 4, dtype=torch.int32), ops.empty(32, 2, dtype=torch.int32), ops.empty(1 << 16, dtype=torch.uint8)
    p, L, null = ops._p, ctypes.c_long, ctypes.c_void_p(0)
    assert ops.lib.psalm_mask_outline_totals(p(m), 1, 2, 8, 9, null, 2, p(counts), ops._stream()) == 0
    assert counts.cpu().tolist() == [[34, 34], [4, 4], [0, 0]]
    assert ops.lib.psalm_mask_outline_totals(p(m), 1, 2, 8, 9, null, 1, p(counts), ops._stream()) == -1      # without an index list m must equal n

    def call(conn=8, row0=0, rows=2, cap=34, ws_bytes=1 << 16, mm=2):
        return ops.lib.psalm_mask_outlines(p(m), 1, 2, 8, 9, null, mm, row0, rows, conn, cap, p(counts), p(rings), 8, p(verts), 32, p(ws), L(ws_bytes),
                                           ops._stream())

    assert call() == 0 and counts.cpu().tolist()[2] == [1, 1] and rings.cpu().tolist()[:2] == [[0, 0, 4, 72], [1, 4, 4, 72]]
    assert call(conn=6) == -1 and b"connectivity" in ops.lib.psalm_last_error()
    assert call(row0=1, rows=2) == -1 and call(mm=1) == -1 and call(cap=-1) == -1 and call(cap=181) == -1
    assert call(ws_bytes=100) == -1 and b"workspace" in ops.lib.psalm_last_error()
    assert call(cap=0, ws_bytes=0) == 0 and call(rows=0) == 0
    out = ops.empty(2, 8, 9, dtype=torch.uint8)

    def fill(R=2, V=8, rows=2, ws_bytes=1 << 16):
        return ops.lib.psalm_mask_fill_polygons(p(rings), R, p(verts), V, 0, rows, 8, 9, p(out), p(ws), L(ws_bytes), ops._stream())

    assert fill() == 0 and out.cpu().numpy().all()
    assert fill(R=-1) == -1 and fill(ws_bytes=8) == -1 and fill(rows=65536) == -1 and fill(rows=0) == 0
