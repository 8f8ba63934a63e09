"""The video-tracking kernels (csrc/video.hip: psalm_video_pick, psalm_video_fuse, psalm_mask_resize_nearest_pad, psalm_mask_select_points)
against numpy / Pillow / torch restatements of the host formulas they replace.  Everything is integer work (or one correctly rounded division):
every comparison is exact.  Runs on the host emulation and, marked gpu, on the MI355X."""
import numpy as np
import pytest
import torch

from ops_backend import ops  # noqa: F401  (fixture: "emu" on the CPU, "hip" marked gpu)
from psalm_amd.preprocess import apply_segmentation, nearest_pad_tables
from video_util import np_fuse, np_pairs, np_pick


def _dev(ops, a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(ops.device)


# ---------------------------------------------------------------------------------------------------- pick
def _pick(ops, scores):
    q, s = ops.video_pick(_dev(ops, scores))
    return q.cpu().tolist(), s.cpu().numpy()


def test_pick_objects_move_down_their_lists(ops):
    """Q = 16, R = 3, distinct scores, all three objects rank query 5 first: objects 1 and 2 must take their second / third choice"""
    rng = np.random.default_rng(0)
    s = rng.permutation(16 * 3).reshape(16, 3).astype(np.float32) / 100.0
    s[5, :] = [9.0, 8.0, 7.0]
    s[11, :] = [0.005, 7.5, 6.5]                    # second choice of objects 1 and 2: object 1 gets it, object 2 moves to its third
    want_q, want_s = np_pick(s)
    assert want_q[0] == 5 and want_q[1] == 11 and want_q[2] not in (5, 11)
    got_q, got_s = _pick(ops, s)
    assert got_q == want_q and np.array_equal(got_s, np.asarray(want_s, np.float32))


def test_pick_exhausted_objects_repeat_the_previous_pick(ops):
    """Q = 16, R = 12, every object ranks the same ten queries first: objects 0..9 take them in order, objects 10 and 11 find all ten taken and
    repeat object 9's pick and score (the reference loop's leftover variables)"""
    rng = np.random.default_rng(1)
    top = rng.permutation(16)[:10]
    s = np.zeros((16, 12), np.float32)
    for r in range(12):
        s[:, r] = rng.random(16).astype(np.float32) * 0.1
        s[top, r] = 1.0 + np.arange(10, 0, -1, dtype=np.float32) + 0.01 * r       # same order for every object
    want_q, want_s = np_pick(s)
    assert want_q[:10] == [int(t) for t in top] and want_q[10] == want_q[11] == want_q[9]
    got_q, got_s = _pick(ops, s)
    assert got_q == want_q and np.array_equal(got_s, np.asarray(want_s, np.float32))


def test_pick_ties_take_the_lowest_query(ops):
    s = np.zeros((12, 2), np.float32)
    s[[3, 7, 9], 0] = 0.5
    s[[3, 7], 1] = 0.5
    assert _pick(ops, s)[0] == [3, 7] == np_pick(s)[0]


def test_pick_refuses_fewer_than_ten_queries(ops):
    from psalm_amd.hip_ops import PsalmHipError
    with pytest.raises(PsalmHipError):
        ops.video_pick(_dev(ops, np.zeros((9, 2), np.float32)))


# ---------------------------------------------------------------------------------------------------- fuse
def _fuse_check(ops, masks_q, pick, fill):
    """masks_q (Q,H,W) 0/1; every integer output against numpy"""
    picked, fused, inter, union, nonzero, flag = ops.video_fuse(_dev(ops, masks_q.astype(np.float32)), _dev(ops, np.asarray(pick, np.int32)),
                                                                _dev(ops, np.asarray(fill, np.int32)))
    want = [masks_q[q].astype(np.uint8) for q in pick]
    wi, wu, wf = np_pairs(want)
    assert np.array_equal(picked.cpu().numpy(), np.stack(want))
    assert np.array_equal(fused.cpu().numpy(), np_fuse(want, fill))
    assert np.array_equal(inter.cpu().numpy(), wi) and np.array_equal(union.cpu().numpy(), wu)
    assert nonzero.cpu().tolist() == [int(m.sum()) for m in want]
    assert int(flag.cpu()) == int(wf)
    return wf


def test_fuse_32_objects_odd_size(ops):
    """R = 32 (bit 31 of the per-pixel set in use: one pixel lies in all 32 masks), 37 x 53 pixels (no vector width divides it), overlapping masks
    whose paint order shows in the label map, picks in a scrambled order"""
    rng = np.random.default_rng(2)
    m = (rng.random((40, 37, 53)) < 0.15).astype(np.uint8)
    m[:, 17, 29] = 1
    m[:, 36, 52] = 1                               # ... and the last pixel
    pick = rng.permutation(40)[:32]
    fill = rng.integers(0, 256, 32)
    _fuse_check(ops, m, pick, fill)
    assert len(set(np_fuse([m[q] for q in pick], fill).reshape(-1).tolist())) > 8


def test_fuse_many_blocks_and_the_iou_threshold(ops):
    """300 x 301 pixels = 353 blocks of 256 (the cross-block sums).  Objects 0 and 1 overlap in exactly 200 of 500 pixels: IoU == 2/5, NOT above
    0.4 in numpy's float64 -> flag stays 1; objects 2 and 3 are both empty (0 / 0 = nan: not above).  One more shared pixel -> flag 0."""
    H, W = 300, 301
    flat = np.zeros((12, H * W), np.uint8)
    flat[4, 1000:1350] = 1
    flat[9, 1150:1500] = 1
    m = flat.reshape(12, H, W)
    assert _fuse_check(ops, m, [4, 9, 0, 1], [7, 200, 3, 4]) is True
    flat[9, 1149] = 1                                # inter 201, union 500
    assert _fuse_check(ops, m, [4, 9, 0, 1], [7, 200, 3, 4]) is False


def test_fuse_paint_order(ops):
    """two overlapping rectangles: the overlap carries the LATER object's fill number, whichever way round they are picked"""
    m = np.zeros((10, 20, 30), np.uint8)
    m[2, 2:12, 3:20] = 1
    m[6, 8:18, 10:28] = 1
    _fuse_check(ops, m, [2, 6], [5, 9])
    _fuse_check(ops, m, [6, 2], [9, 5])
    _, fused, *_ = ops.video_fuse(_dev(ops, m.astype(np.float32)), _dev(ops, np.asarray([2, 6], np.int32)), _dev(ops, np.asarray([5, 9], np.int32)))
    assert int(fused[9, 15]) == 9 and int(fused[3, 5]) == 5 and int(fused[0, 0]) == 0


# ---------------------------------------------------------------------------------------------------- resize + select
GEOMETRIES = [((37, 53), (45, 64), 64),            # up-scale, non-square, padding below only
              ((96, 96), (96, 96), 96),            # identity, no pad
              ((130, 70), (64, 34), 64)]           # down-scale, padding on the right only


def _masks_for(h, w, nh, nw, rng):
    """R = 3 source masks: a dense one; one whose pixels sit in a few rows separated by runs of empty rows; a single pixel that lands in the LAST
    real row of the output"""
    rows, cols = nearest_pad_tables(h, w, nh, nw, 0, 0)
    a = (rng.random((h, w)) < 0.3).astype(np.uint8)
    b = np.zeros((h, w), np.uint8)
    for y in (rows[1], rows[nh // 2], rows[nh - 2]):
        b[y] = (rng.random(w) < 0.5).astype(np.uint8)
        b[y, cols[0]] = b[y, cols[nw - 1]] = 1
    c = np.zeros((h, w), np.uint8)
    c[rows[nh - 1], cols[nw // 3]] = 1
    return np.stack([a, b, c])


@pytest.mark.parametrize("src,dst,S", GEOMETRIES)
def test_resize_nearest_pad_and_select_points(ops, src, dst, S):
    (h, w), (nh, nw) = src, dst
    tr = {"resize": (h, w, nh, nw), "pad": (S - nh, S - nw)}
    rng = np.random.default_rng(h * 1000 + w)
    masks = _masks_for(h, w, nh, nw, rng)
    want = np.stack([apply_segmentation(m, tr) for m in masks])               # Pillow NEAREST + zero pad
    assert want.shape == (3, S, S) and want[2].sum() == 1 and want[2, nh - 1].sum() == 1
    rows, cols = nearest_pad_tables(h, w, nh, nw, S - nh, S - nw)
    total = torch.zeros(3, dtype=torch.int32).to(ops.device)
    out, row_cnt = ops.mask_resize_nearest_pad(_dev(ops, masks), _dev(ops, rows), _dev(ops, cols), total=total)
    assert out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(row_cnt.cpu().numpy(), want.astype(bool).sum(2))
    assert total.cpu().tolist() == want.astype(bool).sum((1, 2)).tolist()
    # ranks: 0, m - 1, first / last pixel of rows, among them the row behind a run of empty rows (mask 1), the one pixel of mask 2
    n = 8
    idx, pts_want = [], []
    wh = torch.tensor([S, S])[None]
    for r in range(3):
        nz = torch.from_numpy(want[r]).nonzero()
        m = nz.shape[0]
        ys = nz[:, 0].numpy()
        starts = np.flatnonzero(np.r_[True, ys[1:] != ys[:-1]])               # rank of every occupied row's first pixel
        ends = np.r_[starts[1:] - 1, m - 1]
        k = [0, m - 1, int(starts[len(starts) // 2]), int(ends[len(starts) // 2]), int(starts[-1]), int(ends[-1]), int(ends[0]), int(rng.integers(0, m))]
        idx.append(k)
        pts_want.append((nz / wh)[torch.tensor(k)].float())                  # model.region_points' expression
    pts = ops.mask_select_points(out, row_cnt, _dev(ops, np.asarray(idx, np.int32)))
    assert pts.shape == (3, n, 2) and pts.dtype == torch.float32
    assert torch.equal(pts.cpu(), torch.stack(pts_want))                      # bit for bit


def test_select_points_every_rank_of_a_mask(ops):
    """all m ranks of one mask at S = 45 x 64 (divisors that are no powers of two: the quotients need the correctly rounded division)"""
    rng = np.random.default_rng(5)
    m = (rng.random((1, 45, 64)) < 0.2).astype(np.uint8)
    m[0, 10:20] = 0
    rows, cols = nearest_pad_tables(45, 64, 45, 64, 0, 0)
    out, row_cnt = ops.mask_resize_nearest_pad(_dev(ops, m), _dev(ops, rows), _dev(ops, cols))
    nz = torch.from_numpy(m[0]).nonzero()
    k = torch.arange(nz.shape[0], dtype=torch.int32)[None]
    pts = ops.mask_select_points(out, row_cnt, _dev(ops, k))
    assert torch.equal(pts.cpu()[0], (nz / torch.tensor([45, 64])[None]).float())
