"""VideoTracker on the MI355X: items 1 and 2 of tests/test_14_video_tracker_emu.py (same helpers, same bit-for-bit bars) on the real library at
size 96 -- the memory path against eval_video on the memory frame in both precisions, and the three-frame clip against the host loop in f16x3."""
import pytest

from test_14_video_tracker_emu import clip_case, memory_path_case, model_for

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_memory_path_equals_eval_video_on_the_memory_frame_gpu(precision):
    calls = {}
    memory_path_case(model_for("hip", precision), calls=calls)
    if precision == "f16x3":
        assert calls["step"].count("psalm_swin_forward") == 1 and calls["eval_video"].count("psalm_swin_forward") == 2


def test_three_frame_clip_equals_the_host_loop_gpu(record_property):
    taken = clip_case(model_for("hip", "f16x3"))
    record_property("branches (used_memory, memory_updated) per frame", str(taken))
    print("branches (used_memory, memory_updated) per frame:", taken)
