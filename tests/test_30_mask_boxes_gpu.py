"""`PSALM.mask_boxes` on the MI355X: the cases of tests/test_29_mask_boxes_model_emu.py (tests/mask_boxes_util.py) on the real library -- crafted
predictor outputs through the post-processing of all five tasks (the native call where the mode has one, and the op-level sequence), the region
pick, the tracker's bookkeeping, and one end-to-end call per session path."""
import pytest
import torch

import mask_boxes_util as U

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


@pytest.mark.parametrize("native", [True, False], ids=["native", "ops"])
@pytest.mark.parametrize("task", U.TASKS)
def test_boxes_of_every_task(task, native):
    U.task_case("hip", "f16x3", task, native=native)


def test_boxes_fp32_panoptic():
    U.task_case("hip", "fp32", "panoptic")


def test_boxes_panoptic_native_call():
    """72 queries: the panoptic task runs as ONE native call, whose `counts` block carries the segment table behind its own words"""
    out = U.task_case("hip", "f16x3", "panoptic", queries=72)
    assert "psalm_postprocess_panoptic" in out["_calls"]


def test_picked_boxes():
    U.pick_case("hip", "f16x3")


def test_tracker_boxes():
    U.observe_case("hip", "f16x3")


def test_end_to_end_plumbing():
    U.e2e_case("hip", "f16x3")
