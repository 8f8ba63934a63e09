"""PSALM.segment_everything -- a grid of clicks per session, duplicates removed on the device -- on the tiny region model (96 x 96 canvas, 60 x 80
original), kernels in the host emulation.  The yardstick is the numpy oracle of tests/everything_util.py applied to what
`segment(regions=<the same clicks>, pick=True)` returns on the same session under the same sampler: every comparison is for equality.  Also
evalout.mask_pair_counts / mask_nms on crafted blobs through the public API."""
import numpy as np
import pytest
import torch

from everything_util import (crafted_picks_case, discs, equality_case, errors_case, np_nms, np_pair_counts, same_click_twice_case,
                             unchanged_case)
from ops_backend import make_ops
from psalm_amd import evalout as E
from psalm_amd.hip_ops import PsalmHipError


@pytest.mark.parametrize("counts", [(12,), (5, 7)], ids=["one_prompt", "two_prompts_5_7"])
def test_equals_the_oracle_on_segments_picks(counts):
    equality_case("emu", counts)


def test_equals_the_oracle_f16x3_and_filters():
    """the model's other precision; a threshold given as a fraction, an area and a score filter"""
    equality_case("emu", (5, 7), precision="f16x3", iou_thr=(1, 2), min_area=2, min_score=0.0)


def test_the_same_click_twice_is_a_duplicate():
    same_click_twice_case("emu")


def test_all_clicks_kept_without_an_area_filter():
    """the tiny model's masks are empty and its scores equal: with min_area=0 nothing is filtered and nothing overlaps, so all 12 clicks are
    kept in index order and the survivors' masks, boxes and areas come back through the unpack"""
    out, want = equality_case("emu", (5, 7), min_area=0)
    assert out["regions"].tolist() == list(range(12)) and tuple(out["masks"].shape) == (12, 60, 80)


@pytest.mark.parametrize("kw", [{}, {"thr": (1, 10), "min_area": 1200}, {"thr": (1, 2), "min_score": 0.9}], ids=["3/10", "1/10_area1200", "1/2_score"])
def test_device_step_on_crafted_picks(kw):
    """The tiny synthetic model cannot show a non-degenerate case -- every mask it predicts is empty and every score zero, at any threshold --
    so the case in which the oracle keeps >= 2 and suppresses >= 1 candidate runs the device step on crafted picks (two prompts, 5 + 7 regions)"""
    crafted_picks_case("emu", **kw)


def test_errors():
    errors_case("emu")


def test_segment_is_unchanged():
    unchanged_case("emu")


# ---------------------------------------------------------------------------------------------------- evalout on crafted blobs
def test_evalout_mask_pair_counts():
    """prediction x ground truth, rectangular, the three dtypes, host tensors moved to the binding's device; a against itself"""
    o = make_ops("emu")
    pred, gt = discs(7, 50, 70, 21) * 3, discs(4, 50, 70, 22)
    want = np_pair_counts(pred.reshape(7, -1) != 0, gt.reshape(4, -1) != 0)
    for a, b in ((torch.from_numpy(pred), torch.from_numpy(gt)), (torch.from_numpy(pred).float(), torch.from_numpy(gt != 0))):
        inter, aa, ab = E.mask_pair_counts(a, b, ops=o)
        assert inter.dtype == torch.int32 and aa.dtype == torch.int32 and inter.device.type == o.device.type
        assert np.array_equal(inter.cpu().numpy(), want)
        assert np.array_equal(aa.cpu().numpy(), (pred != 0).reshape(7, -1).sum(1)) and np.array_equal(ab.cpu().numpy(), gt.reshape(4, -1).sum(1))
    inter, aa, ab = E.mask_pair_counts(torch.from_numpy(gt), ops=o)
    assert ab is aa and np.array_equal(inter.cpu().numpy(), np_pair_counts(gt.reshape(4, -1) != 0, gt.reshape(4, -1) != 0))
    iou = inter.cpu().numpy() / (aa.cpu().numpy()[:, None] + ab.cpu().numpy()[None] - inter.cpu().numpy())
    assert np.array_equal(np.diag(iou), np.ones(4))
    with pytest.raises(PsalmHipError, match="mask_pair_counts"):
        E.mask_pair_counts(torch.from_numpy(pred).double(), ops=o)
    with pytest.raises(PsalmHipError, match="mask_pair_counts"):
        E.mask_pair_counts(torch.from_numpy(pred)[0], ops=o)
    with pytest.raises(PsalmHipError, match="against masks of"):
        E.mask_pair_counts(torch.from_numpy(pred), torch.from_numpy(gt)[:, :, :64], ops=o)
    with pytest.raises(PsalmHipError, match="1025 masks"):
        E.mask_pair_counts(torch.zeros(1025, 2, 2, dtype=torch.uint8), ops=o)


def test_evalout_mask_nms():
    """crafted blobs: the oracle keeps several and suppresses several; 0.7 is the rational 7/10 and the rule is strict"""
    o = make_ops("emu")
    m = discs(30, 64, 80, 23, rmin=8, rmax=20)
    m[11] = m[4]
    flags = m.reshape(30, -1) != 0
    scores = np.random.default_rng(24).random(30).astype(np.float32)
    for thr, frac in ((0.7, (7, 10)), (0.25, (1, 4)), ((2, 5), (2, 5)), (1 / 3, (1, 3))):
        assert E.iou_fraction(thr) == frac
        out = E.mask_nms(torch.from_numpy(m), torch.from_numpy(scores), iou_thr=thr, min_area=250, min_score=0.1, ops=o)
        kept, keep, owner = np_nms(np_pair_counts(flags, flags), flags.sum(1), scores, *frac, min_area=250, min_score=0.1)
        assert out["kept"].dtype == torch.int64 and out["kept"].tolist() == kept[1:1 + kept[0]].tolist()
        assert np.array_equal(out["keep"].cpu().numpy(), keep) and np.array_equal(out["owner"].cpu().numpy(), owner)
        assert np.array_equal(out["areas"].cpu().numpy(), flags.sum(1)) and np.array_equal(out["inter"].cpu().numpy(), np_pair_counts(flags, flags))
        assert (keep == 1).sum() >= 2 and (keep == 0).sum() >= 1 and (keep == -1).sum() >= 1
    # IoU exactly 7/10: inter 7, union 10 -- kept under 0.7, suppressed under anything below
    a = np.zeros((2, 1, 16), np.uint8)
    a[0, 0, :9] = 1
    a[1, 0, 2:10] = 1
    sc = torch.tensor([0.9, 0.8])
    assert E.mask_nms(torch.from_numpy(a), sc, iou_thr=0.7, ops=o)["keep"].tolist() == [1, 1]
    assert E.mask_nms(torch.from_numpy(a), sc, iou_thr=0.6999, ops=o)["keep"].tolist() == [1, 0]
    assert E.mask_nms(torch.from_numpy(a), sc, ops=o)["kept"].tolist() == [0, 1]
    assert E.mask_nms(torch.from_numpy(a), sc, min_score=0.95, ops=o)["kept"].tolist() == []
    for bad in (0.0, 1.0001, (3, 2), (1, 4097), "x"):
        with pytest.raises((ValueError, TypeError)):
            E.mask_nms(torch.from_numpy(a), sc, iou_thr=bad, ops=o)
    with pytest.raises(PsalmHipError, match="scores"):
        E.mask_nms(torch.from_numpy(a), sc[:1], ops=o)
