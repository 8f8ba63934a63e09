"""VideoTracker.start / track / adopt on the MI355X: cases 1 (three prompts), 2, 3 and 5 of tests/test_26_click_track_emu.py (same helpers, same
bit-for-bit bars) on the real library at size 96."""
import pytest

from click_track_util import clip_case, launches_check, memory_case, start_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision,orig", [("f16x3", (80, 60)), ("fp32", (60, 80))])
def test_start_equals_step_prompted_from_the_frame_itself_gpu(precision, orig):
    start_case("hip", precision, 3, orig, [5, 9, 200])


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_three_frame_clip_equals_the_step_tracker_gpu(precision, record_property):
    calls = {}
    taken = clip_case("hip", precision, calls=calls)
    record_property("branches (used_memory, memory_updated) per frame", str(taken))
    print("branches (used_memory, memory_updated) per frame:", taken)
    if precision == "f16x3":
        launches_check(calls)


def test_track_from_memory_equals_the_memory_step_gpu():
    memory_case("hip", "f16x3")
