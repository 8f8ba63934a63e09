"""Helpers of the connected-component tests (tests/test_36_mask_components_kernels.py, test_37_segment_everything_clean_emu.py,
test_38_segment_everything_clean_gpu.py): a numpy / Python oracle of csrc/components.hip without a scipy requirement -- a run-based two-pass
union-find -- that restates the canonical numbering, the component table and the two cleanup steps.  Everything is integer-exact: every
comparison is for equality."""
import numpy as np


def np_set(masks):
    """array -> bool: float32 is set when > 0 (NaN, -0.0, negatives are not), everything else when != 0"""
    masks = np.asarray(masks)
    if masks.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return masks > 0
    return masks != 0


def np_components(flags, connectivity=8):
    """bool (H, W) -> (labels (H, W) int32, count).  The rows' runs of set pixels are the union-find's elements, numbered in row-major order;
    runs of neighbouring rows are united when they overlap (8: when they overlap or touch diagonally); the root of a set is its smallest run,
    i.e. the run that holds the component's lowest row-major pixel; label = 1 + the rank of the root among the roots."""
    assert connectivity in (4, 8)
    flags = np.asarray(flags, bool)
    H, W = flags.shape
    labels = np.zeros(H * W + 1, np.int64)
    if H == 0 or W == 0 or not flags.any():
        return labels[:-1].reshape(H, W).astype(np.int32), 0
    pad = np.zeros((H, W + 2), np.int8)
    pad[:, 1:-1] = flags
    d = np.diff(pad, axis=1)
    ry, rs = np.nonzero(d == 1)                                   # row, first column of every run, row-major
    re = np.nonzero(d == -1)[1]                                   # one past its last column
    c = 1 if connectivity == 8 else 0
    K = W + 2
    # for run a of row y, the runs b of row y + 1 with b.start < a.end + c and b.end > a.start - c: a contiguous range of the sorted run list
    lo = np.searchsorted(ry * K + re, (ry + 1) * K + rs - c, side="right")
    hi = np.searchsorted(ry * K + rs, (ry + 1) * K + re + c, side="left")
    cnt = np.maximum(hi - lo, 0)
    ia = np.repeat(np.arange(len(ry)), cnt)
    jb = np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    parent = list(range(len(ry)))
    for a, b in zip(ia.tolist(), jb.tolist()):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a < b:
            parent[b] = a
        elif b < a:
            parent[a] = b
    parent = np.asarray(parent)
    while True:                                                   # second pass: every run to its root
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            break
        parent = nxt
    is_root = parent == np.arange(len(parent))
    rank = np.cumsum(is_root)                                     # 1-based number of a root
    lab = rank[parent]
    np.add.at(labels, ry * W + rs, lab)                           # paint the runs: +label at the start, -label one past the end, prefix sum
    np.add.at(labels, ry * W + re, -lab)
    return np.cumsum(labels)[:-1].reshape(H, W).astype(np.int32), int(is_root.sum())


def np_table(labels, count, max_comp):
    """labels (H, W) -> (max_comp, 6) int32 of [x0, y0, x1, y1, area, border] for the components 1 .. min(count, max_comp), zeros below"""
    H, W = labels.shape
    t = np.zeros((max_comp, 6), np.int32)
    ys, xs = np.nonzero((labels >= 1) & (labels <= max_comp))
    if len(ys) == 0:
        return t
    k = labels[ys, xs] - 1
    n = min(count, max_comp)
    x0, y0 = np.full(n, W), np.full(n, H)
    x1, y1, border = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.minimum.at(x0, k, xs)
    np.minimum.at(y0, k, ys)
    np.maximum.at(x1, k, xs + 1)
    np.maximum.at(y1, k, ys + 1)
    np.maximum.at(border, k, ((xs == 0) | (ys == 0) | (xs == W - 1) | (ys == H - 1)).astype(np.int64))
    t[:n] = np.stack([x0, y0, x1, y1, np.bincount(k, minlength=n), border], 1)
    return t


def np_clean(flags, min_island=0, max_hole=0, connectivity=8):
    """bool (H, W) -> (out bool (H, W), area, filled, removed): first the components of the UNSET pixels under the complementary connectivity
    that hold no border pixel and have at most max_hole pixels become set; then the components of the set pixels of that result under
    `connectivity` with fewer than min_island pixels are cleared.  A parameter of 0 skips its step."""
    out = np.array(flags, bool)
    H, W = out.shape
    filled = removed = 0
    if max_hole > 0:
        lab, cnt = np_components(~out, 4 if connectivity == 8 else 8)
        t = np_table(lab, cnt, max(cnt, 1))
        fill = np.zeros(cnt + 1, bool)
        fill[1:] = (t[:cnt, 5] == 0) & (t[:cnt, 4] <= max_hole)
        hit = fill[lab]
        filled = int(hit.sum())
        out |= hit
    if min_island > 0:
        lab, cnt = np_components(out, connectivity)
        area = np.bincount(lab.ravel(), minlength=cnt + 1)
        drop = np.zeros(cnt + 1, bool)
        drop[1:] = area[1:] < min_island
        hit = drop[lab]
        removed = int(hit.sum())
        out &= ~hit
    return out, int(out.sum()), filled, removed


def np_clean_many(flags, min_island=0, max_hole=0, connectivity=8):
    """bool (n, H, W) -> (out (n, H, W) uint8, areas (n), filled (n), removed (n) int32)"""
    res = [np_clean(f, min_island, max_hole, connectivity) for f in flags]
    out = np.stack([r[0] for r in res]).astype(np.uint8) if len(res) else np.zeros(np.shape(flags), np.uint8)
    return (out,) + tuple(np.array([r[i] for r in res], np.int32) for i in (1, 2, 3))
