"""PSALM.segment_everything(min_island=, max_hole=, connectivity=) -- every click's picked mask cleaned on the device before the duplicates are
removed -- on the tiny region model of tests/test_34_segment_everything_emu.py, kernels in the host emulation.  The yardstick is the numpy
pipeline of tests/everything_clean_util.py on `segment`'s picks; every comparison is for equality.  The tiny random-weight model's masks are
empty at any size, so the case in which a click's mask changes feeds `_everything_dedup` prompts whose `pred_masks` carry planted specks and
pin-holes (planting WAS needed); the public call is checked on the model's own picks as well.  Also evalout.mask_components / clean_masks."""
import numpy as np
import pytest
import torch

from components_util import np_clean_many, np_components, np_table
from everything_clean_util import defaults_case, errors_case, model_path_case, planted_case
from everything_util import discs
from ops_backend import make_ops
from psalm_amd import evalout as E
from psalm_amd.hip_ops import PsalmHipError


def test_defaults_are_the_call_without_the_arguments():
    defaults_case("emu")


@pytest.mark.parametrize("kw", [{}, {"connectivity": 4}, {"min_island": 0, "max_hole": 3}, {"min_island": 3, "max_hole": 0},
                                {"thr": (1, 10), "min_area": 1200, "min_island": 30, "max_hole": 1}],
                         ids=["4_2_conn8", "4_2_conn4", "holes_only", "islands_only", "area1200"])
def test_cleaning_on_planted_picks(kw):
    planted_case("emu", **kw)


def test_public_call_on_the_models_own_picks():
    model_path_case("emu")


def test_errors():
    errors_case("emu")


def test_evalout_components_and_clean():
    """the public functions take host tensors of the three dtypes and return device tensors equal to the oracle"""
    o = make_ops("emu")
    m = discs(5, 70, 90, 3, rmin=5, rmax=20)
    m[:, 3, 4] = 1
    m[:, 40, 41] = 0
    for t in (torch.from_numpy(m), torch.from_numpy(m).float(), torch.from_numpy(m) != 0):
        for conn in (4, 8):
            got = E.mask_components(t, connectivity=conn, max_components=8, ops=o)
            assert set(got) == {"labels", "count", "table"}
            for i in range(5):
                lab, cnt = np_components(m[i] != 0, conn)
                assert np.array_equal(got["labels"][i].numpy(), lab) and int(got["count"][i]) == cnt
                assert np.array_equal(got["table"][i].numpy(), np_table(lab, cnt, 8))
            got = E.clean_masks(t, min_island=2, max_hole=1, connectivity=conn, ops=o)
            assert set(got) == {"masks", "areas", "removed", "filled"}
            want = np_clean_many(m != 0, 2, 1, conn)
            for k, w in zip(("masks", "areas", "filled", "removed"), want):
                assert np.array_equal(got[k].numpy(), w), k
    with pytest.raises(PsalmHipError):
        E.mask_components(torch.zeros(3, 4), ops=o)
    with pytest.raises(PsalmHipError):
        E.clean_masks(torch.zeros(1, 3, 4, dtype=torch.int64), ops=o)
    with pytest.raises(PsalmHipError):
        E.clean_masks(torch.zeros(1, 3, 4), min_island=-1, ops=o)
    with pytest.raises(PsalmHipError):
        E.mask_components(torch.zeros(1, 3, 4), connectivity=6, ops=o)
