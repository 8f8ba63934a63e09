"""psalm_label_pair_counts / psalm_pq_accumulate (csrc/panopticq.hip) against the numpy oracles of tests/panoptic_quality_util.py, on the host
emulation of the kernels and (marked gpu) on the MI355X.  Every comparison is equality: the overlap tables as integers, tp / fp / fn and the
notes as integers, the IoU sums bit for bit."""
import numpy as np
import pytest
import torch

import panoptic_quality_util as U
from ops_backend import ops  # noqa: F401  (fixture)
from psalm_amd import evalout as E
from psalm_amd.hip_ops import PsalmHipError

SHAPES = [(1, 1), (1, 67), (67, 1), (33, 65), (130, 70)]
SIZES = (0, 1, 3)
# the listed ids come from POOL (G = 3 lists all of it, so with fewer the others are unlisted); VALUES are what the maps hold: VOID, the pool,
# unlisted values and -- int32 maps only -- negatives
POOL = {False: [1, 2 ** 24 - 1, 2 ** 31 - 1], True: [1, 255 * 256 + 7, 2 ** 24 - 1]}
VALUES = {False: [0, 1, 2 ** 24 - 1, 2 ** 31 - 1, -5, 12345, 77, -2 ** 31], True: [0, 1, 255 * 256 + 7, 2 ** 24 - 1, 65536, 12345, 77, 256]}


def maps_of(kind, shape, rgb_g, rgb_p, seed=0):
    Hh, Ww = shape
    i = np.arange(Hh * Ww)
    vg, vp = np.array(VALUES[rgb_g], np.int64), np.array(VALUES[rgb_p], np.int64)
    if kind == "constant":
        a, b = np.full(i.shape, 1), np.full(i.shape, 2)
    elif kind == "checker2":                                     # two pairs: (listed, listed) and (VOID, unlisted)
        a, b = np.where(i % 2, 1, 0), np.where(i % 2, 3, 5)
    elif kind == "checker64":                                    # 64 distinct pairs: every lane of a wavefront holds another key
        a, b = i % 64 // 8, i % 8
    else:
        rng = np.random.default_rng(seed)
        a = rng.permutation(8)[U.voronoi(rng, Hh, Ww, 8)].reshape(-1)
        b = rng.permutation(8)[U.voronoi(rng, Hh, Ww, 8)].reshape(-1)
    return vg[a].reshape(Hh, Ww), vp[b].reshape(Hh, Ww)


def dev_map(ops, m, rgb):
    return torch.from_numpy(U.np_id2rgb(m) if rgb else m.astype(np.int32)).to(ops.device)


def dev_ids(ops, ids):
    return torch.tensor(list(ids), dtype=torch.int32).to(ops.device)


def check_counts(ops, gt, gt_ids, pred, pred_ids, rgb_g=False, rgb_p=False):
    got = ops.label_pair_counts(dev_map(ops, gt, rgb_g), dev_ids(ops, gt_ids), dev_map(ops, pred, rgb_p), dev_ids(ops, pred_ids))
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(gt_ids) + 2, len(pred_ids) + 2)
    got = got.cpu().numpy()
    want = U.np_pair_counts(gt, gt_ids, pred, pred_ids)
    assert int(want.sum()) == gt.size
    assert np.array_equal(got, want), (got, want)
    return got


@pytest.mark.parametrize("rgb", [(False, False), (True, False), (False, True), (True, True)], ids=["i32_i32", "rgb_i32", "i32_rgb", "rgb_rgb"])
@pytest.mark.parametrize("kind", ["constant", "checker2", "checker64", "voronoi"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pair_counts(ops, shape, kind, rgb):
    rgb_g, rgb_p = rgb
    gt, pred = maps_of(kind, shape, rgb_g, rgb_p, seed=shape[0])
    seen = 0
    for G in SIZES:
        for P in SIZES:
            got = check_counts(ops, gt, POOL[rgb_g][:G], pred, POOL[rgb_p][3 - P:], rgb_g, rgb_p)
            seen += int(got[1:G + 1, 1:P + 1].sum())
    if kind in ("checker64", "voronoi") and shape[0] * shape[1] >= 64:
        assert seen > 0                                          # (the listed x listed block is exercised)


def test_pair_counts_overwrites_its_output(ops):
    gt, pred = maps_of("voronoi", (33, 65), False, False)
    out = torch.full((5, 5), 77, dtype=torch.int32).to(ops.device)
    got = ops.label_pair_counts(dev_map(ops, gt, False), dev_ids(ops, POOL[False]), dev_map(ops, pred, False), dev_ids(ops, POOL[False]), out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), U.np_pair_counts(gt, POOL[False], pred, POOL[False]))


def test_every_pair_once(ops):
    """255 x 255, gt = 1 + row, pred = 1 + column: 65 025 distinct pairs of count 1 -- more than a block's (key, count) table holds: the adds
    that find it full go to global memory"""
    r, c = np.mgrid[:255, :255]
    ids = list(range(1, 256))
    got = check_counts(ops, 1 + r, ids, 1 + c, ids)
    assert (got[1:-1, 1:-1] == 1).all()


def test_dense_table_beyond_64_kb(ops):
    """G = P = 150: the dense table (92 KB) is the largest kind of LDS block the kernel asks for"""
    rng = np.random.default_rng(3)
    gt, pred = 1 + 2 * U.voronoi(rng, 33, 65, 160), 1 + 3 * U.voronoi(rng, 33, 65, 160)
    check_counts(ops, gt, [1 + 2 * k for k in range(150)], pred, [1 + 3 * k for k in range(150)])


@pytest.mark.parametrize("P", [2, 1023])
def test_limits(ops, P):
    """a (3, 1100) strip with G = 1023 listed ids: every table entry is searched for, the values beyond it are unlisted"""
    gt = np.stack([1 + 3 * np.arange(1100), 3 * np.arange(1100), np.full(1100, 1 + 3 * 1022)])
    pred = np.stack([2 * np.arange(1100), np.full(1100, 2), 5 + 2 * np.arange(1100)])
    got = check_counts(ops, gt, [1 + 3 * k for k in range(1023)], pred, [2 + 2 * k for k in range(P)])
    assert got[-1].sum() > 0 and got[:, -1].sum() > 0


def test_rejections(ops):
    m = torch.zeros(3, 4, dtype=torch.int32).to(ops.device)
    ok = dev_ids(ops, [1, 2])
    with pytest.raises(PsalmHipError, match="1024 ids"):
        ops.label_pair_counts(m, dev_ids(ops, range(1, 1025)), m, ok)
    for bad in ([2, 1], [1, 1], [0, 1], [-3, 4]):
        with pytest.raises(PsalmHipError, match="ascending"):
            ops.label_pair_counts(m, ok, m, dev_ids(ops, bad))
    with pytest.raises(PsalmHipError, match="id map"):
        ops.label_pair_counts(m.float(), ok, m, ok)
    with pytest.raises(PsalmHipError, match="against"):
        ops.label_pair_counts(m, ok, torch.zeros(4, 3, dtype=torch.int32).to(ops.device), ok)
    # the C entry itself
    big = dev_ids(ops, range(1, 1025))
    out = torch.zeros(1026, 4, dtype=torch.int32).to(ops.device)
    rc = ops.lib.psalm_label_pair_counts(ops._p(m), 0, ops._p(big), 1024, ops._p(m), 0, ops._p(ok), 2, 3, 4, ops._p(out), ops._stream())
    assert rc == -1 and b"1023" in ops.lib.psalm_last_error()
    rc = ops.lib.psalm_pq_accumulate(ops._p(out), 1024, 2, ops._p(big), ops._p(big), ops._p(ok), ops._p(ok), 3, ops._p(out), ops._p(out), ops._p(out),
                                     ops._stream())
    assert rc == -1
    # the evaluator-level wrapper sorts, and refuses what cannot be sorted into a table
    for bad in ([3, 3], [0, 2], [-1], [2 ** 31], [1.5]):
        with pytest.raises(ValueError):
            E.label_pair_counts(m, bad, m, [1], ops=ops)


def test_evalout_wrapper_sorts_and_reports_the_order(ops):
    gt, pred = maps_of("voronoi", (33, 65), False, True, seed=5)
    gids, pids = [2 ** 31 - 1, 1, 2 ** 24 - 1], [2 ** 24 - 1, 1]
    for dev in (False, True):
        g, p = torch.from_numpy(gt.astype(np.int32)), torch.from_numpy(U.np_id2rgb(pred))
        counts, go, po = E.label_pair_counts(g.to(ops.device) if dev else g.numpy(), gids, p.to(ops.device) if dev else p, pids, ops=ops)
        assert [gids[k] for k in go] == sorted(gids) and [pids[k] for k in po] == sorted(pids)
        assert np.array_equal(counts.cpu().numpy(), U.np_pair_counts(gt, sorted(gids), pred, sorted(pids)))


# ---------------------------------------------------------------------------------------------------------------- psalm_pq_accumulate
class Accumulators:
    def __init__(self, ops, categories):
        self.ops, self.categories = ops, categories
        C = len(categories)
        self.stat = torch.zeros(C, 3, dtype=torch.int64).to(ops.device)
        self.iou = torch.zeros(C, dtype=torch.float64).to(ops.device)
        self.notes = torch.zeros(4, dtype=torch.int64).to(ops.device)

    def update(self, sc, table_from):
        ops = self.ops
        t = U.kernel_tables(sc, self.categories)
        if table_from == "oracle":
            counts = torch.from_numpy(U.np_pair_counts(sc["gt"], t["gt_ids"], sc["pred"], t["pred_ids"])).to(ops.device)
        else:
            counts = ops.label_pair_counts(dev_map(ops, sc["gt"], False), dev_ids(ops, t["gt_ids"]), dev_map(ops, sc["pred"], False),
                                           dev_ids(ops, t["pred_ids"]))
        d = {k: torch.from_numpy(v).to(ops.device) for k, v in t.items()}
        assert ops.pq_accumulate(counts, d["gt_cat"], d["gt_crowd"], d["pred_cat"], d["pred_crowd_slot"], self.stat, self.iou, self.notes) is None

    def check(self, scenes):
        stat, notes = U.oracle_of(scenes, self.categories)
        s, i, n = U.stat_arrays(stat, notes, self.categories)
        assert np.array_equal(self.stat.cpu().numpy(), s), (self.stat.cpu().numpy(), s)
        assert np.array_equal(self.notes.cpu().numpy(), n), (self.notes.cpu().numpy(), n)
        assert np.array_equal(self.iou.cpu().numpy().view(np.int64), i.view(np.int64)), (self.iou.cpu().numpy(), i)
        return stat, notes


def test_oracle_on_the_hand_case():
    U.check_oracle_on_hand_case()


@pytest.mark.parametrize("table_from", ["oracle", "kernel"])
def test_accumulate_hand_case(ops, table_from):
    acc = Accumulators(ops, U.HAND_CATEGORIES)
    acc.update(U.hand_case(), table_from)
    stat, _ = acc.check([U.hand_case()])
    assert stat == U.HAND_STAT


EDGE_WANT = {"iou_half": {7: (0, 1, 1), 8: (0, 0, 0)}, "fp_half": {7: (0, 1, 0), 8: (0, 0, 1)}, "fp_forgiven": {7: (0, 0, 0), 8: (0, 0, 1)},
             "gt_no_pixel": {7: (1, 0, 0), 8: (0, 0, 1)}, "pred_no_pixel": {7: (1, 0, 0), 8: (0, 0, 0)}, "two_crowds": {7: (0, 1, 0), 8: (0, 0, 0)},
             "two_crowds_other_order": {7: (0, 1, 0), 8: (0, 0, 0)}, "unlisted": {7: (1, 0, 0), 8: (0, 0, 0)}}


@pytest.mark.parametrize("table_from", ["oracle", "kernel"])
@pytest.mark.parametrize("name", sorted(EDGE_WANT))
def test_accumulate_edge_cases(ops, name, table_from):
    sc, cats = U.edge_cases()[name]
    acc = Accumulators(ops, cats)
    acc.update(sc, table_from)
    stat, notes = acc.check([sc])
    assert {c: (v["tp"], v["fp"], v["fn"]) for c, v in stat.items()} == EDGE_WANT[name]
    if name == "pred_no_pixel":
        assert notes["empty_pred_segments"] == 2
    if name == "unlisted":
        assert (notes["unlisted_gt_pixels"], notes["unlisted_pred_pixels"]) == (2, 1)
    if name.startswith("two_crowds"):                            # which prediction is forgiven depends on the JSON order alone
        t = U.kernel_tables(sc, cats)
        assert t["pred_crowd_slot"].tolist() == ([1, 1] if name == "two_crowds" else [2, 2])


@pytest.mark.parametrize("table_from", ["oracle", "kernel"])
def test_accumulate_random_scenes(ops, table_from):
    """200 random small scenes, accumulated three consecutive updates at a time and compared after each"""
    scenes = U.random_scenes(200, seed=46)
    seen = {"tp": 0, "fp": 0, "fn": 0}
    for k in range(0, len(scenes), 3):
        acc = Accumulators(ops, U.RANDOM_CATEGORIES)
        for j in range(k, min(k + 3, len(scenes))):
            acc.update(scenes[j], table_from)
            stat, _ = acc.check(scenes[k:j + 1])
        for key in seen:
            seen[key] += sum(v[key] for v in stat.values())
    assert all(v >= 50 for v in seen.values()), seen               # the scenes exercise every outcome


def test_accumulate_rejections(ops):
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt).to(ops.device)
    counts, g, p = z(4, 3), z(2), z(1)
    stat, iou, notes = z(3, 3, dt=torch.int64), z(3, dt=torch.float64), z(4, dt=torch.int64)
    ops.pq_accumulate(counts, g, g, p, p, stat, iou, notes)
    with pytest.raises(PsalmHipError):
        ops.pq_accumulate(counts, p, g, p, p, stat, iou, notes)
    with pytest.raises(PsalmHipError):
        ops.pq_accumulate(counts, g, g, p, p, stat.int(), iou, notes)
    with pytest.raises(PsalmHipError):
        ops.pq_accumulate(counts, g, g, p, p, stat, iou.float(), notes)
    with pytest.raises(PsalmHipError):
        ops.pq_accumulate(counts.long(), g, g, p, p, stat, iou, notes)
