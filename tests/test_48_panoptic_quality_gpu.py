"""evalout.PanopticQuality on the MI355X: the cases of tests/test_47_panoptic_quality_emu.py (tests/panoptic_quality_util.py) on the real
kernels, plus one 256 x 256 scene."""
import pytest
import torch

import panoptic_quality_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_hand_case():
    U.hand_meter_case("hip")


def test_random_scenes_and_two_images():
    U.random_meter_case("hip")


def test_scene_of_256_x_256():
    from ops_backend import make_ops
    scenes = U.random_scenes(1, seed=50, H=256, W=256, n_gt=40, n_pred=100)
    U.meter_case(make_ops("hip"), scenes, U.RANDOM_CATEGORIES)


def test_prediction_equal_to_ground_truth():
    U.identity_case("hip")


def test_strict_and_refused_updates():
    U.strict_case("hip")


def test_category_ids():
    U.category_ids_case("hip")


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_real_panoptic_result(precision):
    U.real_result_case("hip", precision)


def test_all_reduce():
    U.all_reduce_case("hip")
