"""VideoTracker.start / track / adopt (psalm_amd/video.py: a track that begins with clicks, boxes, scribbles or masks instead of a dataset record) on
the tiny region model, kernels in the host emulation.  The yardstick is the existing public `VideoTracker.step` fed with the prompt prepared on the
host (tests/click_track_util.py); both sides run the same kernels on the same inputs, so every comparison is bit for bit."""
import pytest

from click_track_util import adopt_case, clip_case, errors_case, launches_check, memory_case, start_case, unchanged_case

_CALLS = {}


@pytest.mark.parametrize("precision,R,orig,fill", [("f16x3", 3, (80, 60), [5, 9, 200]), ("fp32", 1, (60, 80), None),
                                                   ("fp32", 3, (60, 80), None), ("fp32", 1, (80, 60), [255])])
def test_start_equals_step_prompted_from_the_frame_itself(precision, R, orig, fill):
    """Case 1: one click / box + scribble + device bool mask, both precisions, both original sizes"""
    start_case("emu", precision, R, orig, fill)


def test_three_frame_clip_equals_the_step_tracker(record_property):
    """Case 2 (f16x3: its launch records serve the launch-count test below)"""
    taken = clip_case("emu", "f16x3", calls=_CALLS)
    record_property("branches (used_memory, memory_updated) per frame", str(taken))
    print("branches (used_memory, memory_updated) per frame:", taken)


def test_start_and_origin_track_run_one_vision_pass():
    """Case 5, from the records of the clip above"""
    if not _CALLS:
        clip_case("emu", "f16x3", calls=_CALLS)
    launches_check(_CALLS)


def test_track_from_memory_equals_the_memory_step():
    """Case 3 (fp32 here: a third of the emulator's time per frame; tests/test_27_click_track_gpu.py runs it in f16x3)"""
    memory_case("emu", "fp32")


def test_track_after_adopt_equals_step_with_the_session_as_prompt():
    adopt_case("emu", "fp32")


def test_step_is_unchanged_after_start_track_reset():
    unchanged_case("emu", "fp32")


def test_errors_leave_the_tracker_as_it_was():
    errors_case("emu")
