"""PSALM.segment_everything on the MI355X: the cases of tests/test_34_segment_everything_emu.py on the real kernels.  The oracle runs on this
call's own picks (what `segment` returns on the GPU), not on the emulator's masks."""
import numpy as np
import pytest
import torch

from everything_util import crafted_picks_case, discs, equality_case, errors_case, np_nms, np_pair_counts, same_click_twice_case, unchanged_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("counts", [(12,), (5, 7)], ids=["one_prompt", "two_prompts_5_7"])
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_equals_the_oracle_on_segments_picks(precision, counts):
    equality_case("hip", counts, precision=precision)


def test_equals_the_oracle_under_filters():
    equality_case("hip", (5, 7), iou_thr=(1, 50), min_area=2, min_score=0.0)


def test_all_clicks_kept_without_an_area_filter():
    """min_area=0: no click is filtered for an empty mask, so the survivors' masks, boxes and areas come back through the unpack"""
    equality_case("hip", (5, 7), min_area=0)


@pytest.mark.parametrize("kw", [{}, {"thr": (1, 10), "min_area": 1200}, {"thr": (1, 2), "min_score": 0.9}], ids=["3/10", "1/10_area1200", "1/2_score"])
def test_device_step_on_crafted_picks(kw):
    crafted_picks_case("hip", **kw)


def test_the_same_click_twice_is_a_duplicate():
    same_click_twice_case("hip")


def test_errors():
    errors_case("hip")


def test_segment_is_unchanged():
    unchanged_case("hip")


def test_evalout_on_blobs():
    """evalout.mask_pair_counts (prediction x ground truth) and evalout.mask_nms at a size with several pack blocks and K splits"""
    from psalm_amd import evalout as E
    pred, gt = discs(70, 300, 333, 31, rmin=20, rmax=90), discs(9, 300, 333, 32, rmin=20, rmax=90)
    fp, fg = pred.reshape(70, -1) != 0, gt.reshape(9, -1) != 0
    inter, aa, ab = E.mask_pair_counts(torch.from_numpy(pred).float(), torch.from_numpy(gt))
    assert np.array_equal(inter.cpu().numpy(), np_pair_counts(fp, fg))
    assert np.array_equal(aa.cpu().numpy(), fp.sum(1)) and np.array_equal(ab.cpu().numpy(), fg.sum(1))
    scores = np.random.default_rng(33).random(70).astype(np.float32)
    out = E.mask_nms(torch.from_numpy(pred), torch.from_numpy(scores), iou_thr=0.3)
    kept, keep, owner = np_nms(np_pair_counts(fp, fp), fp.sum(1), scores, 3, 10)
    assert out["kept"].tolist() == kept[1:1 + kept[0]].tolist() and 1 < kept[0] < 70
    assert np.array_equal(out["keep"].cpu().numpy(), keep) and np.array_equal(out["owner"].cpu().numpy(), owner)
