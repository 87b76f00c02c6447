"""The host build of the tile test (rt_debug_tile_test_host: tile_dirs_f + tile_misses_box_f, the
one definition tile_cull_kernel and tile_cut_kernel call) on the sets of tests/tile_cases.py.

Sound side, no tolerance: no item is "missed" where some ray of the tile (rt.camera_rays under a
jitter table spanning the one-pixel pad) passes box_cases.ref_aabb.  Tight side, no tolerance:
every item the doubled-margin float64 model culls is culled.  The device build runs the same sets
in tests/test_gpu_tile_tests.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import tile_cases as tc
from raytracinginonesemester_amd import _lib

RT_ERR_ARG = -1


@pytest.mark.parametrize("name", tc.TILE_CASES)
def test_sets_meet_their_conditions(name):
    """The references alone: in every band, on both sides, items where some ray passes and items
    where all rays miss both occur; the model culls some of the 1e-3 and 1e-2 outer bands."""
    groups = tc.tile_case(name)
    band, side = tc.gather(groups, "band"), tc.gather(groups, "side")
    any_pass, model = tc.gather(groups, "any_pass"), tc.gather(groups, "model_cull")
    assert not (any_pass & model).any()  # the model is itself sound on these sets
    for b in range(len(tc.BANDS)):
        for s in (1, -1):
            sel = (band == b) & (side == s)
            assert any_pass[sel].any() and (~any_pass[sel]).any(), (name, tc.BANDS[b], s)
    for b in (4, 5):
        sel = (band == b) & (side == 1)
        assert model[sel].any(), (name, tc.BANDS[b])
    widths = {g["cam"].pixel_width for g in groups}
    assert widths == {w for w, _ in tc.IMAGES}
    assert any(g["rect"][1] >= 3836 for g in groups) and any(1916 <= g["rect"][1] <= 1919 for g in groups)
    assert any(g["rect"][0] == 0 for g in groups)


@pytest.mark.parametrize("name", tc.TILE_CASES)
def test_host_build_both_sides(name, capsys):
    tc.check_set(tc.host_fn, name)


def test_short_batches():
    tc.check_short_batches(tc.host_fn)


def test_refuses_bad_arguments():
    import ctypes as C

    L = _lib.lib()
    g = tc.tile_case("axis")[0]
    out = np.zeros(4, np.int32)
    cam, t, b, o = C.byref(g["cam"].c), g["tiles"].ctypes.data, g["boxes"].ctypes.data, out.ctypes.data
    assert L.rt_debug_tile_test_host(cam, t, b, 0, None) == 0
    for args in ((None, t, b, 1, o), (cam, None, b, 1, o), (cam, t, None, 1, o), (cam, t, b, 1, None), (cam, t, b, -1, o)):
        assert L.rt_debug_tile_test_host(*args) == RT_ERR_ARG
        assert L.rt_debug_tile_test_batch(0, *args) == RT_ERR_ARG
