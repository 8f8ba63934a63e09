"""evalout.PanopticQuality -- PQ / SQ / RQ on the device -- on the host emulation of the kernels (CPU), against the literal numpy restatement of
panopticapi's pq_compute_single_core / pq_average in tests/panoptic_quality_util.py: integers exact, floats ==.  The same cases run on the
MI355X in tests/test_48_panoptic_quality_gpu.py."""
import panoptic_quality_util as U


def test_oracle_on_the_hand_case():
    U.check_oracle_on_hand_case()


def test_hand_case():
    U.hand_meter_case("emu")


def test_random_scenes_and_two_images():
    U.random_meter_case("emu")


def test_prediction_equal_to_ground_truth():
    U.identity_case("emu")


def test_strict_and_refused_updates():
    U.strict_case("emu")


def test_category_ids():
    U.category_ids_case("emu")


def test_real_panoptic_result():
    U.real_result_case("emu", "fp32")


def test_all_reduce():
    U.all_reduce_case("emu")
