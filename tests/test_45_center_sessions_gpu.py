"""Centres through the model's public calls on the MI355X: the cases of tests/test_44_center_sessions_emu.py on the real kernels (the oracle
runs on this call's own masks)."""
import pytest
import torch

from distance_util import click_round_trip_case, everything_centers_case, public_centers_case

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("extra", [{}, {"outlines": True}, {"min_island": 5, "max_hole": 4}, {"outlines": True, "min_island": 5, "max_hole": 4}],
                         ids=["plain", "outlines", "clean", "outlines-clean"])
def test_everything_centers_on_planted_picks(extra):
    everything_centers_case("hip", **extra)


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_public_calls_gain_only_the_center_keys(precision):
    public_centers_case("hip", precision)


def test_centers_are_click_prompts():
    click_round_trip_case("hip")
