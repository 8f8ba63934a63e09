"""Centres through the model's public calls -- PSALM.segment_everything(centers=True), segment / segment_many(centers=True), the centres fed back
as {"points": ...} region prompts -- on the tiny region model, kernels in the host emulation.  The yardsticks are evalout.mask_centers on the
call's own masks and the numpy oracle of tests/distance_util.py; every comparison is for equality.  The tiny random-weight model's masks are
empty at any size, so the case with real shapes feeds the device step the planted picks of tests/everything_clean_util.py."""
import pytest

from distance_util import click_round_trip_case, everything_centers_case, public_centers_case


@pytest.mark.parametrize("extra", [{}, {"outlines": True}, {"min_island": 5, "max_hole": 4}, {"outlines": True, "min_island": 5, "max_hole": 4}],
                         ids=["plain", "outlines", "clean", "outlines-clean"])
def test_everything_centers_on_planted_picks(extra):
    everything_centers_case("emu", **extra)


def test_public_calls_gain_only_the_center_keys():
    public_centers_case("emu")


def test_centers_are_click_prompts():
    click_round_trip_case("emu")
