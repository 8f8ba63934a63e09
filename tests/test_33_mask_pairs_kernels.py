"""csrc/maskpairs.hip -- psalm_mask_pack_bits / _unpack_bits / _pair_counts / _nms / _paint_bits -- against the numpy oracle of
tests/everything_util.py.  Integer results: every comparison is np.array_equal.  Runs on the host emulation of the kernel sources and, marked gpu,
on the MI355X."""
import numpy as np
import pytest
import torch

from everything_util import bits_np, discs, np_nms, np_pack, np_paint, np_pair_counts, np_set
from ops_backend import ops  # noqa: F401  (fixture)
from psalm_amd.hip_ops import PsalmHipError

# the constants of csrc/maskpairs.hip, restated: the pair tile's edge (MP_TILE), the words per LDS step (MP_KC), the least number of words per
# K split (MP_KS; with one tile of pairs and nw <= 65536 the split IS this many words) and the words of a plane per pack block (MP_PACK_WORDS)
MP_TILE, MP_KC, MP_KS, MP_PACK_WORDS = 64, 32, 64, 256


def dev(ops, a, dtype):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)
    return t != 0 if dtype == torch.bool else t.to(dtype)


def check_pack(ops, masks_np, dtype, index=None):
    """pack == the oracle's words (so the tail of the last word is zero) and areas; unpack(pack(x)) == x set"""
    n, HW = masks_np.shape[0], int(np.prod(masks_np.shape[1:]))
    flags = np_set(masks_np if dtype == torch.float32 else masks_np != 0).reshape(n, HW)
    t = dev(ops, masks_np, dtype)
    idx = None if index is None else torch.tensor(index, dtype=torch.int32, device=ops.device)
    bits, areas = ops.mask_pack_bits(t, index=idx)
    if index is not None:
        flags = np.stack([flags[i] if 0 <= i < n else np.zeros(HW, bool) for i in index])
    nw = (HW + 63) // 64
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (len(flags), nw) and areas.dtype == torch.int32
    assert ops.mask_bits_words(HW) == nw
    got = bits_np(bits)
    assert np.array_equal(got, np_pack(flags))
    if HW % 64:
        assert np.array_equal(got[:, -1] >> np.uint64(HW % 64), np.zeros(len(flags), np.uint64))       # on the raw words: the tail is zero
    assert np.array_equal(areas.cpu().numpy(), flags.sum(1).astype(np.int32))
    back = ops.mask_unpack_bits(bits, tuple(masks_np.shape[1:]))
    assert back.dtype == torch.uint8 and np.array_equal(back.cpu().numpy(), flags.reshape((len(flags),) + masks_np.shape[1:]).astype(np.uint8))
    return bits, areas


DTYPES = [torch.float32, torch.uint8, torch.bool]
IDS = ["f32", "u8", "bool"]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_70x150(ops, dtype):
    """(6, 70, 150): empty, full, the four corner pixels, two pixels astride a 64-pixel word boundary, blobs; HW = 10500 is no multiple of 64"""
    m = np.zeros((6, 70, 150), np.float32)
    m[1] = 1
    m[2, 0, 0] = m[2, 0, 149] = m[2, 69, 0] = m[2, 69, 149] = 1
    m[3].reshape(-1)[63] = m[3].reshape(-1)[64] = 1
    m[4].reshape(-1)[10499] = 3
    m[5] = discs(1, 70, 150, 1)[0]
    bits, areas = check_pack(ops, m, dtype)
    assert areas.tolist()[:5] == [0, 10500, 4, 2, 1]
    w = bits_np(bits)
    assert w[3, 0] == np.uint64(1) << np.uint64(63) and w[3, 1] == 1 and w[4, -1] == np.uint64(1) << np.uint64(10499 % 64)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_misaligned_planes(ops, dtype):
    """(5, 33, 67) behind a storage offset of one element: every plane starts off a 16-byte boundary"""
    m = discs(5, 33, 67, 2, rmin=3).astype(np.float32) * (1 if dtype == torch.bool else 2)
    m[3] = 0
    m[3, 32, 66] = 1
    store = torch.float32 if dtype == torch.float32 else torch.uint8
    flat = torch.zeros(5 * 33 * 67 + 1, dtype=store, device=ops.device)
    flat[1:] = torch.from_numpy(m.reshape(-1)).to(ops.device).to(store)
    shifted = flat[1:].view(5, 33, 67)
    shifted = shifted.view(torch.bool) if dtype == torch.bool else shifted
    bits, areas = ops.mask_pack_bits(shifted)
    flags = (m != 0).reshape(5, -1)
    assert np.array_equal(bits_np(bits), np_pack(flags)) and np.array_equal(areas.cpu().numpy(), flags.sum(1).astype(np.int32))
    out = torch.full((5 * 33 * 67 + 2,), 9, dtype=torch.uint8, device=ops.device)               # the unpack's output misaligned as well
    ops.mask_unpack_bits(bits, (33, 67), out=out[1:-1].view(5, 33, 67))
    assert out[0] == 9 and out[-1] == 9 and np.array_equal(out[1:-1].cpu().numpy(), flags.reshape(-1).astype(np.uint8))
    check_pack(ops, m, dtype)                                                                    # (and from an aligned base)


def test_pack_f32_specials(ops):
    """NaN, -0.0, -1 and a denormal: only the denormal and the positives are set"""
    m = np.zeros((2, 9, 21), np.float32)
    m[0, 1, 2], m[0, 2, 19], m[0, 7, 0], m[0, 4, 11], m[0, 8, 20], m[0, 3, 3] = -1.0, -0.0, np.nan, 1e-45, 0.5, np.inf
    m[1] = np.nan
    m[1, 8, 20] = 1e-30
    assert m[0, 4, 11] > 0
    bits, areas = check_pack(ops, m, torch.float32)
    assert areas.tolist() == [3, 1]
    assert sorted(np.flatnonzero(ops.mask_unpack_bits(bits, 9 * 21).cpu().numpy()[0]).tolist()) == [3 * 21 + 3, 4 * 21 + 11, 8 * 21 + 20]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pack_index_list_and_unpack_rows(ops, dtype):
    """[2, 0, 2, -1, 3] over 3 planes: rows 2, 0, 2, empty, empty; outputs into views of a caller's block; unpack by rows, a negative row = zeros"""
    m = discs(3, 40, 90, 3)
    bits, areas = check_pack(ops, m, dtype, index=[2, 0, 2, -1, 3])
    assert areas.tolist()[3:] == [0, 0] and not bits_np(bits)[3:].any()
    nw = bits.shape[1]
    block = torch.full((7, nw), -1, dtype=torch.int64, device=ops.device)
    ar = torch.full((7,), -1, dtype=torch.int32, device=ops.device)
    ops.mask_pack_bits(dev(ops, m, dtype), index=torch.tensor([1, 7], dtype=torch.int32, device=ops.device), out_bits=block[2:4], out_areas=ar[2:4])
    assert np.array_equal(bits_np(block[2:3]), np_pack(m[1:2].reshape(1, -1) != 0)) and not bits_np(block[3:4]).any()
    assert (block[:2] == -1).all() and (block[4:] == -1).all() and ar.tolist() == [-1, -1, int(m[1].sum()), 0, -1, -1, -1]
    rows = torch.tensor([1, -1, 0, 1], dtype=torch.int32, device=ops.device)
    back = ops.mask_unpack_bits(bits, (40, 90), rows=rows).cpu().numpy()
    assert np.array_equal(back, np.stack([m[0], np.zeros_like(m[0]), m[2], m[0]]))
    b2, a2 = ops.mask_pack_bits(dev(ops, m, dtype), want_areas=False)
    assert a2 is None and np.array_equal(bits_np(b2), np_pack(m.reshape(3, -1) != 0))
    b0, a0 = ops.mask_pack_bits(torch.zeros(0, 4, 4, dtype=torch.uint8, device=ops.device))
    assert tuple(b0.shape) == (0, 1) and tuple(a0.shape) == (0,)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 64 * MP_PACK_WORDS - 1, 64 * MP_PACK_WORDS + 65])
def test_pack_small_and_block_edges(ops, dtype, HW):
    """HW = 1, 63, 64, 65 and one below / beyond the words of one pack block; the first and the last pixel set, and all of them"""
    m = np.zeros((3, HW), np.uint8)
    m[0, 0] = m[0, -1] = 1
    m[1] = 1
    m[2] = np.random.default_rng(HW).integers(0, 2, HW)
    check_pack(ops, m, dtype)


def pair_case(ops, ma, mb, HW, seed, self_case=False):
    g = np.random.default_rng(seed)
    a = g.random((ma, HW)) < 0.4
    b = a if self_case else g.random((mb, HW)) < 0.6
    ba, aa = ops.mask_pack_bits(dev(ops, a, torch.uint8))
    bb = ba if self_case else ops.mask_pack_bits(dev(ops, b, torch.uint8))[0]
    inter = ops.mask_pair_counts(ba, None if self_case else bb)
    want = np_pair_counts(a, b)
    assert inter.dtype == torch.int32 and np.array_equal(inter.cpu().numpy(), want)
    return inter, aa, ba, bb, want


def test_pair_counts_rectangular(ops):
    """5 x 70 (ma != mb, mb beyond one tile) and the same pair swapped"""
    pair_case(ops, 5, 70, 1000, 1)
    pair_case(ops, 70, 5, 1000, 2)


@pytest.mark.parametrize("ma,mb", [(MP_TILE - 1, MP_TILE), (MP_TILE, MP_TILE + 1), (MP_TILE + 1, MP_TILE - 1), (1, 1)])
def test_pair_counts_tile_edges(ops, ma, mb):
    """ma and mb one below, at and one above the pair tile's edge"""
    pair_case(ops, ma, mb, 64 * 3 + 5, 10 + ma)


@pytest.mark.parametrize("nw", [1, MP_KC - 1, MP_KC, MP_KC + 1, MP_KS - 1, MP_KS, MP_KS + 1, 3 * MP_KS + 7])
def test_pair_counts_k_edges(ops, nw):
    """nw = 1 and one below, at and one above the LDS step and the K split (HW ends inside the last word)"""
    pair_case(ops, 6, 9, 64 * nw - 3, 20 + nw)


def test_pair_counts_self_and_twice(ops):
    """a against itself: symmetric, the diagonal == the areas; a second call into the same buffer gives the same numbers (the call zeroes what
    it accumulates into), also from a buffer full of rubbish"""
    inter, areas, ba, _, want = pair_case(ops, 37, 37, 64 * 70 + 9, 5, self_case=True)
    got = inter.cpu().numpy()
    assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), areas.cpu().numpy())
    again = ops.mask_pair_counts(ba, out=inter)
    assert again.data_ptr() == inter.data_ptr() and np.array_equal(again.cpu().numpy(), want)
    inter.fill_(12345)
    assert np.array_equal(ops.mask_pair_counts(ba, ba, out=inter).cpu().numpy(), want)


def test_pair_counts_1024(ops):
    """ma = mb = 1024, the limit, at HW = 192"""
    inter, areas, *_ = pair_case(ops, 1024, 1024, 192, 6, self_case=True)
    assert np.array_equal(np.diag(inter.cpu().numpy()), areas.cpu().numpy())


def run_nms(ops, inter, areas, scores, num, den, min_area=1, min_score=None):
    inter, areas = np.asarray(inter, np.int32), np.asarray(areas, np.int32)
    scores = np.asarray(scores, np.float32)
    t = [torch.from_numpy(x).to(ops.device) for x in (inter, areas, scores)]
    kept, keep, owner = [x.cpu().numpy() for x in ops.mask_nms(*t, num, den, min_area=min_area, min_score=min_score)]
    wk, wkeep, wowner = np_nms(inter, areas, scores, num, den, min_area, min_score)
    assert kept.dtype == np.int32 and kept.shape == (len(areas) + 1,)
    assert np.array_equal(kept, wk), (kept, wk)
    assert np.array_equal(keep, wkeep) and np.array_equal(owner, wowner)
    return kept.tolist(), keep.tolist(), owner.tolist()


def sym(m, areas, pairs):
    inter = np.zeros((m, m), np.int32)
    inter[np.arange(m), np.arange(m)] = areas
    for (i, j), v in pairs.items():
        inter[i, j] = inter[j, i] = v
    return inter


def test_nms_chain(ops):
    """A > B > C by score, A suppresses B, B would suppress C, A does not: C is KEPT (a suppressed candidate suppresses nothing)"""
    areas = [100, 100, 100]
    inter = sym(3, areas, {(0, 1): 90, (1, 2): 90, (0, 2): 10})
    kept, keep, owner = run_nms(ops, inter, areas, [0.9, 0.8, 0.7], 1, 2)
    assert kept == [2, 0, 2, -1] and keep == [1, 0, 1] and owner == [0, 0, 2]


def test_nms_threshold_is_strict_and_exact(ops):
    """inter 7, union 10, threshold 7/10: IoU == threshold, not suppressed; inter 8, union 11: suppressed; a zero union suppresses nothing"""
    kept, keep, owner = run_nms(ops, sym(2, [9, 8], {(0, 1): 7}), [9, 8], [2.0, 1.0], 7, 10)
    assert keep == [1, 1] and owner == [0, 1] and kept == [2, 0, 1]
    kept, keep, owner = run_nms(ops, sym(2, [10, 9], {(0, 1): 8}), [10, 9], [2.0, 1.0], 7, 10)
    assert keep == [1, 0] and owner == [0, 0] and kept == [1, 0, -1]
    kept, keep, owner = run_nms(ops, np.zeros((2, 2), np.int32), [0, 0], [2.0, 1.0], 1, 4096, min_area=0)
    assert keep == [1, 1]
    # products beyond 32 bits: areas near 2^31, threshold 4095/4096
    big = 2 ** 31 - 1
    kept, keep, owner = run_nms(ops, sym(2, [big, big], {(0, 1): big}), [big, big], [1.0, 2.0], 4095, 4096)
    assert keep == [0, 1] and owner == [1, 1]
    kept, keep, owner = run_nms(ops, sym(2, [big, big], {(0, 1): big - 2 ** 20}), [big, big], [1.0, 2.0], 4095, 4096)
    assert keep == [1, 1]


def test_nms_ties_and_duplicates(ops):
    """equal scores go to the lowest index first; exact duplicates: the first stands for all"""
    areas = [50, 50, 50, 20]
    inter = sym(4, areas, {(0, 1): 50, (0, 2): 50, (1, 2): 50})
    kept, keep, owner = run_nms(ops, inter, areas, [0.5, 0.5, 0.5, 0.5], 7, 10)
    assert kept == [2, 0, 3, -1, -1] and keep == [1, 0, 0, 1] and owner == [0, 0, 0, 3]
    kept, keep, owner = run_nms(ops, inter, areas, [0.5, 0.6, 0.6, 0.6], 7, 10)
    assert kept == [2, 1, 3, -1, -1] and owner == [1, 1, 1, 3]
    # the rule reads inter[candidate][kept]: an asymmetric table shows which entry is used
    inter = np.array([[10, 0], [10, 10]], np.int32)
    kept, keep, owner = run_nms(ops, inter, [10, 10], [2.0, 1.0], 1, 2)
    assert keep == [1, 0]
    kept, keep, owner = run_nms(ops, inter.T.copy(), [10, 10], [2.0, 1.0], 1, 2)
    assert keep == [1, 1]


def test_nms_filters(ops):
    """min_area and min_score: a filtered candidate (the best score) would otherwise have suppressed a kept one"""
    areas = [4, 100, 100, 100]
    inter = sym(4, areas, {(0, 1): 4, (1, 2): 95})
    kept, keep, owner = run_nms(ops, inter, areas, [0.9, 0.8, 0.7, 0.1], 1, 50, min_area=5)
    assert keep == [-1, 1, 0, 1] and owner == [-1, 1, 1, 3]
    kept, keep, owner = run_nms(ops, inter, areas, [0.9, 0.8, 0.7, 0.1], 1, 50, min_area=4)
    assert keep == [1, 0, 1, 1] and owner == [0, 0, 2, 3]                       # unfiltered, 0 suppresses 1 (IoU 4 / 100 > 1 / 50), so 2 survives
    kept, keep, owner = run_nms(ops, inter, areas, [0.9, 0.8, 0.7, 0.1], 1, 50, min_area=5, min_score=0.7)
    assert keep == [-1, 1, 0, -1] and kept == [1, 1, -1, -1, -1]
    kept, keep, owner = run_nms(ops, inter, areas, [0.9, 0.8, 0.7, 0.1], 1, 50, min_score=0.75, min_area=5)
    assert keep == [-1, 1, -1, -1] and owner == [-1, 1, -1, -1]


def test_nms_one_and_none(ops):
    """m = 1; every candidate filtered: K = 0"""
    assert run_nms(ops, [[5]], [5], [0.3], 7, 10) == ([1, 0], [1], [0])
    assert run_nms(ops, [[5]], [5], [0.3], 7, 10, min_area=6) == ([0, -1], [-1], [-1])
    kept, keep, owner = run_nms(ops, sym(3, [1, 2, 3], {}), [1, 2, 3], [0.1, 0.2, 0.3], 1, 1, min_score=0.5)
    assert kept == [0, -1, -1, -1] and keep == [-1] * 3 and owner == [-1] * 3


@pytest.mark.parametrize("thr", [(1, 2), (7, 10), (1, 1)], ids=["1/2", "7/10", "1/1"])
def test_nms_1024_random(ops, thr):
    """m = 1024 overlapping discs on a 48 x 64 plane with many equal scores, against the oracle"""
    m = discs(1024, 48, 64, 7, rmin=3, rmax=12).reshape(1024, -1) != 0
    g = np.random.default_rng(8)
    scores = (g.integers(0, 200, 1024) / 200).astype(np.float32)
    areas = m.sum(1).astype(np.int32)
    kept, keep, owner = run_nms(ops, np_pair_counts(m, m), areas, scores, *thr, min_area=30, min_score=0.05)
    assert thr == (1, 1) or (1 < kept[0] < 1024 and 0 in keep and -1 in keep)


def test_paint(ops):
    """three overlapping discs: a contested pixel takes the lowest k; K = 0: all zeros; the pixels beyond HW are never written"""
    H, W = 37, 53                                               # HW = 1961: the last word holds 41 pixels
    yy, xx = np.mgrid[:H, :W]
    m = np.stack([(yy - cy) ** 2 + (xx - cx) ** 2 <= 144 for cy, cx in ((15, 20), (20, 30), (25, 22))])
    flags = m.reshape(3, -1)
    bits, _ = ops.mask_pack_bits(dev(ops, m, torch.uint8))
    guarded = torch.full((H * W + 64,), -7, dtype=torch.int32, device=ops.device)
    for kept in ([3, 2, 0, 1], [2, 1, 2, -1], [1, 0, -1, -1], [0, -1, -1, -1]):
        k = torch.tensor(kept, dtype=torch.int32, device=ops.device)
        guarded.fill_(-7)
        lab = ops.mask_paint_bits(bits, k, (H, W), out=guarded[:H * W].view(H, W))
        assert lab.data_ptr() == guarded.data_ptr()
        assert np.array_equal(lab.cpu().numpy().reshape(-1), np_paint(flags, kept))
        assert (guarded[H * W:] == -7).all()
    lab = ops.mask_paint_bits(bits, torch.tensor([3, 2, 0, 1], dtype=torch.int32, device=ops.device), (H, W)).cpu().numpy()
    assert lab[20, 25] == 1 and m[:, 20, 25].all()              # all three discs hold (20, 25): the first of the kept list (disc 2) wins
    assert set(np.unique(lab).tolist()) == {0, 1, 2, 3}
    assert not ops.mask_paint_bits(bits, torch.tensor([0, 2, 0, 1], dtype=torch.int32, device=ops.device), H * W).any()


def test_pipeline_on_blobs(ops):
    """pack -> pairs -> NMS -> paint -> unpack of the survivors, several pack blocks per plane, against the oracle end to end"""
    H, W = 130, 140                                             # nw = 285: two pack blocks
    m = discs(40, H, W, 11, rmin=8, rmax=30)
    m[7] = m[3]
    flags = m.reshape(40, -1) != 0
    scores = np.random.default_rng(12).random(40).astype(np.float32)
    bits, areas = ops.mask_pack_bits(dev(ops, m, torch.float32))
    inter = ops.mask_pair_counts(bits)
    kept, keep, owner = ops.mask_nms(inter, areas, torch.from_numpy(scores).to(ops.device), 3, 10)
    wk, wkeep, wowner = np_nms(np_pair_counts(flags, flags), flags.sum(1), scores, 3, 10)
    assert np.array_equal(kept.cpu().numpy(), wk) and np.array_equal(keep.cpu().numpy(), wkeep) and np.array_equal(owner.cpu().numpy(), wowner)
    assert 1 < wk[0] < 40 and wkeep[3] + wkeep[7] <= 1
    assert np.array_equal(ops.mask_paint_bits(bits, kept, (H, W)).cpu().numpy().reshape(-1), np_paint(flags, wk))
    K = int(wk[0])
    assert np.array_equal(ops.mask_unpack_bits(bits, (H, W), rows=kept[1:1 + K]).cpu().numpy(), m[wk[1:1 + K]])


def test_errors(ops):
    d = ops.device
    f = torch.zeros(2, 8, 8, device=d)
    with pytest.raises(PsalmHipError, match="float32 / uint8 / bool"):
        ops.mask_pack_bits(f.to(torch.int32))
    with pytest.raises(PsalmHipError, match="contiguous"):
        ops.mask_pack_bits(f.permute(0, 2, 1))
    with pytest.raises(PsalmHipError, match="index"):
        ops.mask_pack_bits(f, index=torch.zeros(2, dtype=torch.int64, device=d))
    with pytest.raises(PsalmHipError, match="out_bits"):
        ops.mask_pack_bits(f, out_bits=torch.zeros(2, 2, dtype=torch.int64, device=d))
    bits, areas = ops.mask_pack_bits(f)
    with pytest.raises(PsalmHipError, match="int64"):
        ops.mask_pair_counts(bits.to(torch.int32))
    with pytest.raises(PsalmHipError, match="contiguous int64"):
        ops.mask_pair_counts(torch.zeros(2, 4, dtype=torch.int64, device=d)[:, ::2])
    with pytest.raises(PsalmHipError, match="words"):
        ops.mask_pair_counts(bits, torch.zeros(2, 2, dtype=torch.int64, device=d))
    with pytest.raises(PsalmHipError, match="1025 x 2"):
        ops.mask_pair_counts(torch.zeros(1025, 1, dtype=torch.int64, device=d), bits)
    with pytest.raises(PsalmHipError, match="words"):
        ops.mask_unpack_bits(bits, (8, 9))
    with pytest.raises(PsalmHipError, match="rows"):
        ops.mask_unpack_bits(bits, (8, 8), rows=torch.zeros(1, dtype=torch.int64, device=d))
    sc = torch.zeros(2, device=d)
    inter = ops.mask_pair_counts(bits)
    for num, den in ((7, 0), (0, 10), (11, 10), (1, 4097), (-1, 2)):
        with pytest.raises(PsalmHipError, match="threshold"):
            ops.mask_nms(inter, areas, sc, num, den)
    with pytest.raises(PsalmHipError, match="1025 candidates"):
        ops.mask_nms(torch.zeros(1025, 1025, dtype=torch.int32, device=d), torch.zeros(1025, dtype=torch.int32, device=d), torch.zeros(1025, device=d), 7, 10)
    with pytest.raises(PsalmHipError, match="inter"):
        ops.mask_nms(inter.float(), areas, sc, 7, 10)
    with pytest.raises(PsalmHipError, match="areas"):
        ops.mask_nms(inter, areas.to(torch.int64), sc, 7, 10)
    with pytest.raises(PsalmHipError, match="scores"):
        ops.mask_nms(inter, areas, torch.zeros(4, device=d)[::2], 7, 10)
    with pytest.raises(PsalmHipError, match="inter"):
        ops.mask_nms(torch.zeros(2, 3, dtype=torch.int32, device=d), areas, sc, 7, 10)
    kept = ops.mask_nms(inter, areas, sc, 7, 10, min_area=0)[0]
    with pytest.raises(PsalmHipError, match="kept"):
        ops.mask_paint_bits(bits, kept[:2], (8, 8))
    with pytest.raises(PsalmHipError, match="words"):
        ops.mask_paint_bits(bits, kept, (9, 8))
    with pytest.raises(PsalmHipError, match="out"):
        ops.mask_paint_bits(bits, kept, (8, 8), out=torch.zeros(8, 8, device=d))
    with pytest.raises(PsalmHipError, match="pixels per plane"):
        ops.mask_bits_words(0)
    with pytest.raises(PsalmHipError, match="pixels per plane"):
        ops.mask_bits_words(2 ** 31)
    assert ops.mask_bits_words(2 ** 31 - 1) == 2 ** 25
    # the library's own checks, past the binding: m = 1025 and thr_den = 0
    lib, p = ops.lib, ops._p
    assert lib.psalm_mask_nms(p(inter), p(areas), p(sc), 1025, 7, 10, 1, ops_float(0), p(kept), p(areas), p(areas), ops._stream()) == -1
    assert b"1 <= m <= 1024" in lib.psalm_last_error()
    assert lib.psalm_mask_nms(p(inter), p(areas), p(sc), 2, 7, 0, 1, ops_float(0), p(kept), p(areas), p(areas), ops._stream()) == -1
    assert b"thr_den" in lib.psalm_last_error()
    assert lib.psalm_mask_pair_counts(p(bits), 1025, p(bits), 2, 1, p(inter), ops._stream()) == -1


def ops_float(v):
    from ctypes import c_float
    return c_float(v)
