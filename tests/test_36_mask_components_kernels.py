"""csrc/components.hip -- psalm_mask_components / psalm_mask_clean -- against the numpy oracle of tests/components_util.py.  Integer results:
every comparison is np.array_equal.  Runs on the host emulation of the kernel sources and, marked gpu, on the MI355X."""
import ctypes

import numpy as np
import pytest
import torch

from components_util import np_clean, np_clean_many, np_components, np_set, np_table
from ops_backend import make_ops, ops  # noqa: F401  (fixture)
from psalm_amd.hip_ops import PsalmHipError

# the tile edge of csrc/components.hip (CC_T), restated: a block labels a T x T tile in LDS, tiles meet in the merge launch
T = 32
H0, W0 = 2 * T + 6, 2 * T + 22          # 3 x 3 tiles, ragged on both edges

DTYPES = [torch.float32, torch.uint8, torch.bool]
IDS = ["f32", "u8", "bool"]
CONN = [4, 8]


def dev(ops, a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)
    return t != 0 if dtype == torch.bool else t.to(dtype)


def check_components(ops, masks_np, dtype, conn, index=None, invert=False, max_comp=64, t=None, **kw):
    """labels, count and table of Ops.mask_components == the oracle's on every plane; returns the oracle's counts"""
    masks_np = np.asarray(masks_np)
    n, H, W = masks_np.shape
    flags = np_set(masks_np) if dtype == torch.float32 else masks_np != 0
    t = dev(ops, masks_np, dtype) if t is None else t
    idx = None if index is None else torch.tensor(index, dtype=torch.int32, device=ops.device)
    labels, count, table = ops.mask_components(t, index=idx, connectivity=conn, invert=invert, max_components=max_comp, **kw)
    rows = range(n) if index is None else index
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (len(rows), H, W)
    assert count.dtype == torch.int32 and tuple(count.shape) == (len(rows),)
    assert table.dtype == torch.int32 and tuple(table.shape) == (len(rows), max_comp, 6)
    got_l, got_c, got_t = labels.cpu().numpy(), count.cpu().numpy(), table.cpu().numpy()
    counts = []
    for i, r in enumerate(rows):
        f = flags[r] if 0 <= r < n else np.zeros((H, W), bool)
        want_l, want_c = np_components(~f if invert else f, conn)
        assert got_c[i] == want_c, (i, got_c[i], want_c)
        assert np.array_equal(got_l[i], want_l), (i, np.argwhere(got_l[i] != want_l)[:5])
        assert np.array_equal(got_t[i], np_table(want_l, want_c, max_comp)), i
        counts.append(want_c)
    return counts


def check_clean(ops, masks_np, dtype, conn, min_island, max_hole, index=None, **kw):
    masks_np = np.asarray(masks_np)
    n, H, W = masks_np.shape
    flags = np_set(masks_np) if dtype == torch.float32 else masks_np != 0
    idx = None if index is None else torch.tensor(index, dtype=torch.int32, device=ops.device)
    out, areas, filled, removed = ops.mask_clean(dev(ops, masks_np, dtype), index=idx, connectivity=conn, min_island=min_island, max_hole=max_hole, **kw)
    if index is not None:
        flags = np.stack([flags[r] if 0 <= r < n else np.zeros((H, W), bool) for r in index])
    want = np_clean_many(flags, min_island, max_hole, conn)
    assert out.dtype == torch.uint8 and all(v.dtype == torch.int32 for v in (areas, filled, removed))
    for name, g, w in zip(("out", "areas", "filled", "removed"), (out, areas, filled, removed), want):
        assert np.array_equal(g.cpu().numpy(), w), (name, g.cpu().numpy() if g.dim() == 1 else None, w if w.ndim == 1 else None)
    return want


# ---------------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_equals_scipy_label():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(7)
    for k in range(300):
        H, W = g.integers(1, 41, 2)
        f = g.random((H, W)) < g.choice([0.3, 0.41, 0.59, 0.8])
        for conn in CONN:
            want, n = ndi.label(f, structure=np.ones((3, 3)) if conn == 8 else None)
            got, cnt = np_components(f, conn)
            assert cnt == n and np.array_equal(got, want), (k, conn)


def test_oracle_on_hand_cases():
    f = np.array([[1, 0, 1], [0, 1, 0], [1, 0, 0]], bool)
    assert np_components(f, 8)[1] == 1 and np_components(f, 4)[0].tolist() == [[1, 0, 2], [0, 3, 0], [4, 0, 0]]
    ring = np.ones((5, 5), bool)
    ring[1:4, 1:4] = False
    ring[2, 2] = True
    assert np_clean(ring, 0, 7, 8)[1:] == (17, 0, 0) and np_clean(ring, 0, 8, 8)[1:] == (25, 8, 0)      # the hole holds an island: 8 unset pixels
    assert np_clean(ring, 2, 0, 8)[1:] == (16, 0, 1) and np_clean(ring, 2, 8, 8)[1:] == (25, 8, 0)      # holes first: the island is part of the blob
    assert np_table(*np_components(ring, 8), 4).tolist() == [[0, 0, 5, 5, 16, 1], [2, 2, 3, 3, 1, 0], [0] * 6, [0] * 6]


# ---------------------------------------------------------------------------------------------------- shapes
def corner_planes(H, W):
    m = np.zeros((6, H, W), np.float32)
    m[1] = 1
    m[2, 0, 0] = m[3, 0, W - 1] = m[4, H - 1, 0] = m[5, H - 1, W - 1] = 1
    return m


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_degenerate_planes(ops, dtype, conn):
    """empty, full, one pixel in each corner -- at the tiled shape and at 1 x 1, 1 x W, H x 1"""
    for H, W in ((H0, W0), (1, 1), (1, W0), (H0, 1)):
        counts = check_components(ops, corner_planes(H, W), dtype, conn)
        assert counts == [0, 1, 1, 1, 1, 1]
    checker = np.indices((1, W0)).sum(0)[None] % 2 == 0
    assert check_components(ops, checker.astype(np.float32), dtype, conn) == [W0 // 2]


@pytest.mark.parametrize("conn", CONN)
def test_float_set_semantics(ops, conn):
    """NaN, -0.0 and negatives are not set; tiny positives and +inf are"""
    g = np.random.default_rng(3)
    m = g.choice(np.array([np.nan, -0.0, 0.0, -1.5, -np.inf, 1e-30, 2.0, np.inf], np.float32), size=(2, H0, W0))
    check_components(ops, m, torch.float32, conn, max_comp=512)
    check_clean(ops, m, torch.float32, conn, 3, 2)
    bytes_ = g.choice(np.array([0, 0, 1, 255, 128], np.uint8), size=(1, H0, W0))
    check_components(ops, bytes_, torch.uint8, conn, max_comp=512)


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_checkerboard(ops, dtype, conn):
    """under 4 every set pixel is a component of its own -- HW / 2 of them, far more than max_comp: the table is truncated, the count exact;
    under 8 the board is one component"""
    m = (np.indices((H0, W0)).sum(0) % 2 == 0).astype(np.float32)[None]
    assert check_components(ops, m, dtype, conn, max_comp=100) == [H0 * W0 // 2 if conn == 4 else 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_diagonal_touch_at_a_tile_corner(ops, dtype):
    """two blobs that touch only diagonally, exactly at the corner where four tiles meet: one component under 8, two under 4 -- both ways round"""
    m = np.zeros((2, H0, W0), np.float32)
    m[0, T - 5:T, T - 7:T] = 1                                     # ends at pixel (T - 1, T - 1)
    m[0, T:T + 4, T:T + 9] = 1                                     # starts at pixel (T, T)
    m[1, T - 5:T, 2 * T:2 * T + 6] = 1                             # ends at (T - 1, 2T): the anti-diagonal
    m[1, T:T + 3, 2 * T - 8:2 * T] = 1                             # starts at (T, 2T - 1)
    assert check_components(ops, m, dtype, 8) == [1, 1]
    assert check_components(ops, m, dtype, 4) == [2, 2]


def serpentine(H, W):
    m = np.zeros((H, W), np.float32)
    m[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    m = np.zeros((H, W), np.float32)
    m[:, 0::2] = 1
    m[-1] = 1
    m[-2, 1::2] = 0
    return m


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_serpentine_and_comb(ops, dtype, conn):
    """a one-pixel path through every tile and back (merge chains over many tile edges) and a comb whose teeth join only in the last row: one
    component each, under both connectivities; without its last row the comb is W / 2 teeth"""
    m = np.stack([serpentine(H0, W0), comb(H0, W0), comb(H0, W0)])
    m[2, -1] = 0
    assert check_components(ops, m, dtype, conn) == [1, 1, W0 // 2]


def rings():
    m = np.zeros((H0, W0), np.float32)
    m[10:60, 10:70] = 1                                            # island ...
    m[14:56, 14:66] = 0                                            # ... with a hole ...
    m[20:50, 20:60] = 1                                            # ... that holds an island ...
    m[T - 2:T + 2, T - 1:T + 3] = 0                                # ... with a hole astride a tile corner
    m[0:7, 74:] = 1                                                # a ring cut by the image border: its inside reaches the border,
    m[0:5, 76:] = 0                                                # it is no hole
    return m


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nested_rings(ops, dtype, conn):
    m = rings()[None]
    assert check_components(ops, m, dtype, conn) == [3]
    assert check_components(ops, m, dtype, conn, invert=True) == [4]          # the outside, the cut ring's inside (the ring reaches the border twice), the ring hole, the inner hole
    want = check_clean(ops, m, dtype, conn, 0, 10 ** 6)
    assert want[2].tolist() == [42 * 52 - 30 * 40 + 16]                       # both holes fill, the cut ring's inside does not


@pytest.mark.parametrize("conn,p", [(4, 0.59), (8, 0.41)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_percolation_noise(ops, dtype, conn, p):
    """noise near the percolation threshold of the connectivity: large ragged components across all tiles"""
    m = (np.random.default_rng(11).random((3, H0, W0)) < p).astype(np.float32)
    counts = check_components(ops, m, dtype, conn, max_comp=300)
    assert min(counts) > 20
    check_components(ops, m, dtype, conn, invert=True, max_comp=300)
    check_clean(ops, m, dtype, conn, 9, 4)


@pytest.mark.parametrize("conn", CONN)
def test_storage_offset_index_list_and_chunking(ops, conn):
    g = np.random.default_rng(5)
    m = (g.random((4, H0 - 1, W0 - 2)) < 0.5).astype(np.float32)
    for dtype in DTYPES:                                           # planes behind a one-element storage offset: no alignment beyond the element's own
        flat = dev(ops, np.concatenate([[0], m.ravel()]), dtype)
        view = flat[1:].view(m.shape)
        assert view.storage_offset() == 1 and view.is_contiguous()
        check_components(ops, m, dtype, conn, t=view, max_comp=128)
    index = [3, 0, 0, -1, 4, 2, 3]                                 # repeats and entries outside [0, n): the empty plane
    counts = check_components(ops, m, torch.float32, conn, index=index, max_comp=128)
    assert counts[3] == counts[4] == 0 and counts[0] == counts[6]
    assert check_components(ops, m, torch.uint8, conn, index=index, invert=True, max_comp=128)[3] == 1
    one_plane = 3 * 4 * (H0 - 1) * (W0 - 2)                        # a workspace of one plane's three int32 planes: one row per chunk
    check_components(ops, m, torch.float32, conn, max_comp=128, max_workspace_bytes=one_plane)
    check_components(ops, m, torch.float32, conn, index=index, max_comp=128, max_workspace_bytes=one_plane)
    check_clean(ops, m, torch.uint8, conn, 5, 3, max_workspace_bytes=one_plane)
    check_clean(ops, m, torch.float32, conn, 5, 3, index=index, max_workspace_bytes=0)
    check_clean(ops, m, torch.bool, conn, 5, 3, index=index)


# ---------------------------------------------------------------------------------------------------- cleanup
@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clean_thresholds_sit_exactly_at_the_size(ops, dtype, conn):
    m = np.zeros((H0, W0), np.float32)
    m[3, T - 3:T + 3] = 1                                          # island of 6 astride a vertical tile edge
    m[T - 2:T + 3, 5] = 1                                          # island of 5 astride a horizontal tile edge
    m[20:50, 40:80] = 1                                            # a block of 1200 ...
    m[T - 2:T + 2, 50] = 0                                         # ... with a hole of 4 astride a horizontal edge
    m[40, 2 * T - 2:2 * T + 3] = 0                                 # ... and a hole of 5 astride a vertical edge
    m = m[None]
    for min_island, removed in ((5, 0), (6, 5), (7, 11)):          # an island of min_island pixels stays, one of min_island - 1 goes
        want = check_clean(ops, m, dtype, conn, min_island, 0)
        assert want[3].tolist() == [removed] and want[2].tolist() == [0]
    for max_hole, filled in ((3, 0), (4, 4), (5, 9)):              # a hole of max_hole pixels fills, one of max_hole + 1 stays
        want = check_clean(ops, m, dtype, conn, 0, max_hole)
        assert want[2].tolist() == [filled] and want[3].tolist() == [0]
    want = check_clean(ops, m, dtype, conn, 6, 4)
    assert (want[1].tolist(), want[2].tolist(), want[3].tolist()) == ([1200 - 5 + 6], [4], [5])
    want = check_clean(ops, m, dtype, conn, 0, 0)                  # both zero: binarise only
    assert (want[1].tolist(), want[2].tolist(), want[3].tolist()) == ([1200 - 9 + 11], [0], [0])


@pytest.mark.parametrize("conn", CONN)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clean_rings(ops, dtype, conn):
    """a 3 x 3 ring (8 pixels, hole of 1) is lifted to 9 by its filled hole and survives min_island = 9; a 4 x 4 ring (12 pixels, hole of 4) keeps
    its hole under max_hole = 1 and is removed whole under min_island = 13, nothing left behind"""
    m = np.zeros((2, H0, W0), np.float32)
    m[0, T - 2:T + 1, T - 1:T + 2] = 1
    m[0, T - 1, T] = 0
    m[1, 2 * T - 2:2 * T + 2, T - 2:T + 2] = 1
    m[1, 2 * T - 1:2 * T + 1, T - 1:T + 1] = 0
    want = check_clean(ops, m, dtype, conn, 9, 1)
    assert (want[1].tolist(), want[2].tolist(), want[3].tolist()) == ([9, 12], [1, 0], [0, 0])
    want = check_clean(ops, m, dtype, conn, 13, 1)
    assert (want[1].tolist(), want[2].tolist(), want[3].tolist()) == ([0, 0], [1, 0], [9, 12]) and not want[0].any()
    want = check_clean(ops, m, dtype, conn, 9, 0)                  # islands alone: without the fill the small ring goes too
    assert want[1].tolist() == [0, 12] and want[3].tolist() == [8, 0]
    want = check_clean(ops, m, dtype, conn, 0, 4)                  # holes alone
    assert want[1].tolist() == [9, 16] and want[2].tolist() == [1, 4]


def test_hole_connectivity_is_the_complement(ops):
    """a hole that leaks to the outside through a diagonal gap: under connectivity 8 the holes are judged 4-connected (it is a hole, it fills),
    under 4 they are judged 8-connected (it is part of the outside, it stays)"""
    m = np.zeros((1, H0, W0), np.float32)
    m[0, T - 3:T + 2, T - 3:T + 2] = 1
    m[0, T - 2:T + 1, T - 2:T + 1] = 0                             # a 5 x 5 ring with a 3 x 3 hole at the tile corner ...
    m[0, T - 3, T - 3] = 0                                         # ... whose corner pixel is missing
    assert check_clean(ops, m, torch.uint8, 8, 0, 20)[2].tolist() == [9]
    assert check_clean(ops, m, torch.uint8, 4, 0, 20)[2].tolist() == [0]


# ---------------------------------------------------------------------------------------------------- errors
def test_error_returns(ops):
    m = dev(ops, np.ones((2, 8, 9), np.float32), torch.float32)
    for bad in (5, 0, 6, True, None):
        with pytest.raises(PsalmHipError, match="connectivity"):
            ops.mask_components(m, connectivity=bad)
        with pytest.raises(PsalmHipError, match="connectivity"):
            ops.mask_clean(m, connectivity=bad)
    for kw in ({"min_island": -1}, {"max_hole": -3}):
        with pytest.raises(PsalmHipError, match=">= 0"):
            ops.mask_clean(m, **kw)
    for bad in (0, 65537, -4):
        with pytest.raises(PsalmHipError, match="max_components"):
            ops.mask_components(m, max_components=bad)
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_components(m.to(torch.int32))
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_clean(m[0])
    with pytest.raises(PsalmHipError, match="index"):
        ops.mask_components(m, index=torch.zeros(2, dtype=torch.int64, device=ops.device))
    with pytest.raises(PsalmHipError, match="out"):
        ops.mask_clean(m, out=torch.zeros(2, 8, 8, dtype=torch.uint8, device=ops.device))
    if not ops.is_emu:
        with pytest.raises(PsalmHipError, match="GPU tensors"):
            ops.mask_components(m.cpu())
    # the library's own error codes
    raw = ops._cdll_raw
    for fn in (raw.psalm_mask_components_workspace, raw.psalm_mask_clean_workspace):
        fn.restype = ctypes.c_long
        assert fn(-1, 8, 8) == -1 and fn(65536, 8, 8) == -1 and fn(1, 65536, 32768) == -1 and fn(1, -1, 8) == -1 and fn(0, 8, 8) == 0
    assert raw.psalm_mask_components_workspace(2, 70, 86) == 2 * 4 * (3 * 70 * 86 + (70 * 86 + 1023) // 1024)
    assert raw.psalm_mask_clean_workspace(2, 70, 86) == 2 * 4 * 3 * 70 * 86
    labels, count = ops.empty(2, 8, 9, dtype=torch.int32), ops.empty(2, dtype=torch.int32)
    ws = ops.empty(4096, dtype=torch.uint8)
    p, L, null = ops._p, ctypes.c_long, ctypes.c_void_p(0)

    def comp(conn=8, invert=0, max_comp=4, table=null, ws_bytes=4096, idx=null, mm=2):
        return ops.lib.psalm_mask_components(p(m), 0, 2, 8, 9, idx, mm, conn, invert, p(labels), p(count), table, max_comp, p(ws), L(ws_bytes), ops._stream())

    assert comp() == 0
    assert comp(conn=6) == -1 and b"connectivity" in ops.lib.psalm_last_error()
    assert comp(invert=2) == -1
    assert comp(mm=1) == -1                                        # without an index list m must equal n
    assert comp(ws_bytes=100) == -1 and b"workspace" in ops.lib.psalm_last_error()
    tab = ops.empty(2, 4, 6, dtype=torch.int32)
    assert comp(table=p(tab), max_comp=0) == -1 and comp(table=p(tab), max_comp=65537) == -1 and comp(table=p(tab)) == 0
    out, a3 = ops.empty(2, 8, 9, dtype=torch.uint8), ops.empty(3, 2, dtype=torch.int32)

    def clean(conn=8, mi=1, mh=1, ws_bytes=4096):
        return ops.lib.psalm_mask_clean(p(m), 0, 2, 8, 9, null, 2, conn, mi, mh, p(out), p(a3[0]), p(a3[1]), p(a3[2]), p(ws), L(ws_bytes), ops._stream())

    assert clean() == 0 and clean(conn=7) == -1 and clean(mi=-1) == -1 and clean(mh=-1) == -1 and clean(ws_bytes=8) == -1
    assert clean(mi=0, mh=0, ws_bytes=0) == 0                      # the binarising gather needs no workspace


def test_empty_batch_and_empty_planes(ops):
    labels, count, table = ops.mask_components(torch.zeros(0, 5, 7, dtype=torch.uint8, device=ops.device))
    assert tuple(labels.shape) == (0, 5, 7) and tuple(count.shape) == (0,) and tuple(table.shape) == (0, 256, 6)
    out, areas, filled, removed = ops.mask_clean(torch.zeros(0, 5, 7, dtype=torch.uint8, device=ops.device), min_island=3)
    assert tuple(out.shape) == (0, 5, 7) and tuple(areas.shape) == (0,)


# ---------------------------------------------------------------------------------------------------- all tiles in flight at once
@pytest.mark.gpu
def test_noise_1024_on_the_gpu_twice():
    """(1, 1024, 1024) noise at p = 0.59, 4-connected: 1024 tiles in flight across the XCDs, which the emulation (one block at a time) cannot
    show -- the merge launch's unions race and read stale links.  Two runs give the oracle's result, hence the same bytes."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    o = make_ops("hip")
    f = np.random.default_rng(59).random((1, 1024, 1024)) < 0.59
    t = torch.from_numpy(f).to(o.device)
    want_l, want_c = np_components(f[0], 4)
    want_t = np_table(want_l, want_c, 1024)
    for _ in range(2):
        labels, count, table = o.mask_components(t, connectivity=4, max_components=1024)
        assert int(count.cpu()[0]) == want_c
        assert np.array_equal(labels.cpu().numpy()[0], want_l)
        assert np.array_equal(table.cpu().numpy()[0], want_t)
    want = np_clean_many(f, 30, 6, 4)
    for _ in range(2):
        got = o.mask_clean(t, connectivity=4, min_island=30, max_hole=6)
        for g, w in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), w)
