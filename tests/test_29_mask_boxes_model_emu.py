"""`PSALM.mask_boxes` on the host emulation of the kernels (CPU): crafted predictor outputs through the post-processing of all five tasks, the
region pick and the tracker's bookkeeping -- boxes, areas and panoptic segment records against numpy on the returned masks; the default (switch
off) unchanged.  Cases in tests/mask_boxes_util.py; the same cases run on the MI355X in tests/test_30_mask_boxes_gpu.py."""
import pytest

import mask_boxes_util as U


@pytest.mark.parametrize("native", [True, False], ids=["native", "ops"])
@pytest.mark.parametrize("task", U.TASKS)
def test_boxes_of_every_task(task, native):
    U.task_case("emu", "fp32", task, native=native)


def test_boxes_f16x3_panoptic():
    U.task_case("emu", "f16x3", "panoptic")


def test_boxes_panoptic_native_call():
    """72 queries: the panoptic task runs as ONE native call, whose `counts` block carries the segment table behind its own words"""
    out = U.task_case("emu", "f16x3", "panoptic", queries=72)
    assert "psalm_postprocess_panoptic" in out["_calls"]


def test_picked_boxes():
    U.pick_case("emu")


def test_tracker_boxes():
    U.observe_case("emu")


def test_switch_is_off_by_default_and_a_from_pretrained_keyword():
    import inspect
    from psalm_amd.model import PSALM
    assert U.model_for("emu", "fp32", "region").mask_boxes is False
    assert inspect.signature(PSALM.from_pretrained).parameters["mask_boxes"].default is False


def test_end_to_end_plumbing():
    U.e2e_case("emu")
