"""PSALM.segment_everything(min_island=, max_hole=, connectivity=) on the MI355X: the cases of tests/test_37_segment_everything_clean_emu.py on the
real kernels.  The oracle runs on this call's own picks (what `segment` returns on the GPU); the case in which a click's mask changes uses
planted specks and pin-holes, as there (the tiny model's masks are empty)."""
import numpy as np
import pytest
import torch

from components_util import np_clean_many, np_components, np_table
from everything_clean_util import defaults_case, errors_case, model_path_case, planted_case
from everything_util import discs

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_defaults_are_the_call_without_the_arguments():
    defaults_case("hip")


@pytest.mark.parametrize("kw", [{}, {"connectivity": 4}, {"min_island": 0, "max_hole": 3}, {"min_island": 3, "max_hole": 0},
                                {"thr": (1, 10), "min_area": 1200, "min_island": 30, "max_hole": 1}],
                         ids=["4_2_conn8", "4_2_conn4", "holes_only", "islands_only", "area1200"])
def test_cleaning_on_planted_picks(kw):
    planted_case("hip", **kw)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_public_call_on_the_models_own_picks(precision):
    model_path_case("hip", precision)


def test_errors():
    errors_case("hip")


def test_evalout_on_blobs_with_forced_chunks():
    """evalout.mask_components / clean_masks on host tensors at a size with many tiles; Ops-level chunking down to one plane gives the same bytes"""
    from psalm_amd import evalout as E
    from psalm_amd.hip_ops import get_ops
    m = discs(6, 300, 333, 31, rmin=20, rmax=90)
    g = np.random.default_rng(2)
    m ^= (g.random(m.shape) < 0.02).astype(np.uint8)
    got = E.mask_components(torch.from_numpy(m), connectivity=8, max_components=64)
    want = [np_components(p != 0, 8) for p in m]
    assert got["labels"].device.type == "cuda" and got["count"].cpu().tolist() == [c for _, c in want]
    assert np.array_equal(got["labels"].cpu().numpy(), np.stack([l for l, _ in want]))
    assert np.array_equal(got["table"].cpu().numpy(), np.stack([np_table(l, c, 64) for l, c in want]))
    o = get_ops()
    chunked = o.mask_components(torch.from_numpy(m).cuda(), connectivity=8, max_components=64, max_workspace_bytes=1)
    for a, b in zip(chunked, (got["labels"], got["count"], got["table"])):
        assert torch.equal(a, b)
    got = E.clean_masks(torch.from_numpy(m).float(), min_island=12, max_hole=5, connectivity=4)
    for k, w in zip(("masks", "areas", "filled", "removed"), np_clean_many(m != 0, 12, 5, 4)):
        assert np.array_equal(got[k].cpu().numpy(), w), k
