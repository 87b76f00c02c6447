"""The device build of the tile test (rt_debug_tile_test_batch: tile_dirs_f with v_rcp_f32 +
tile_misses_box_f, the one definition tile_cull_kernel and tile_cut_kernel call), one lane per
item, on the sets of tests/tile_cases.py: no item "missed" where some ray of the tile passes
ref_aabb, every item the doubled-margin float64 model culls culled, neither with a tolerance.
The host build runs the same sets in tests/test_tile_tests_host.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import tile_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tc.TILE_CASES)
def test_device_build_both_sides(name):
    got = tc.check_set(tc.device_fn, name)
    host = tc.run_groups(tc.host_fn, tc.tile_case(name))
    print(f"{name}: device and host builds differ on {int((got != host).sum())} of {got.size} items")


def test_short_batches():
    tc.check_short_batches(tc.device_fn)
