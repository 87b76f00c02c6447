"""The host build of the wave-family entry test (rt_debug_family_test_host: family_axis +
family_entry_passes, what family_dirs and frustum_loop call, the wave reductions as plain loops)
on the sets of tests/family_cases.py.

Sound side, no tolerance: an entry passes wherever some live lane's own box_cases.ref_aabb passes
with that lane's bestT.  Tight side, no tolerance: every entry the float64 model with the 2^-18
widening rejects is rejected, and the loop form (out_loose) is the model's.  The device build runs
the same sets in tests/test_gpu_family_test.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import family_cases as fc
from raytracinginonesemester_amd import _lib

RT_ERR_ARG = -1
from tile_cases import BANDS


@pytest.mark.parametrize("name", fc.FAMILY_CASES)
def test_sets_meet_their_conditions(name):
    """The references alone: in every band, on both sides, entries some lane passes and entries
    all lanes miss both occur; the model rejects some of the 1e-3 and 1e-2 outer bands; both loop
    forms occur; one, half and all lanes live."""
    c = fc.family_case(name)
    assert not (c["any_pass"] & ~c["model_pass"]).any()  # the model is itself sound on these sets
    for b in range(len(BANDS)):
        for s in (1, -1):
            sel = (c["band"] == b) & (c["side"] == s)
            assert c["any_pass"][sel].any() and (~c["any_pass"][sel]).any(), (name, BANDS[b], s)
    for b in (4, 5):
        sel = (c["band"] == b) & (c["side"] == 1)
        assert (~c["model_pass"][sel]).any(), (name, BANDS[b])
    assert c["model_loose"].any() and (~c["model_loose"]).any()
    assert {1, 32, 64} <= set((c["active"] != 0).sum(axis=1).tolist())


@pytest.mark.parametrize("name", fc.FAMILY_CASES)
def test_host_build_both_sides(name):
    fc.check_set(fc.host_fn, name)


@pytest.mark.parametrize("name", ["camera_axis", "free"])
def test_inactive_lanes_change_no_answer(name):
    fc.check_inactive_lanes(fc.host_fn, name)


def test_short_batches():
    fc.check_short_batches(fc.host_fn)


def test_no_bound_axis_and_parallel_lanes_occur():
    c = fc.family_case("free")
    assert (c["bmax"] >= 1e30).any()
    live = c["active"] != 0
    assert ((np.abs(c["rays"][..., 3:]) < 1e-8).any(axis=2) & live).any()
    cross = [(np.where(live, c["rays"][..., 3 + a], np.inf).min(axis=1) < 0) &
             (np.where(live, c["rays"][..., 3 + a], -np.inf).max(axis=1) > 0) for a in range(3)]
    n = np.sum(cross, axis=0)
    assert (n == 2).any() and (n == 3).any()


def test_refuses_bad_arguments():
    L = _lib.lib()
    c = fc.family_case("free")
    out, lo = np.zeros(32, np.int32), np.zeros(1, np.int32)
    good = [c["rays"].ctypes.data, None, c["best_t"].ctypes.data, c["bmax"].ctypes.data, c["boxes"].ctypes.data, 1,
            out.ctypes.data, lo.ctypes.data]
    assert L.rt_debug_family_test_host(*good[:5], 0, None, None) == 0
    for k in (0, 2, 3, 4, 6, 7):
        bad = list(good)
        bad[k] = None
        assert L.rt_debug_family_test_host(*bad) == RT_ERR_ARG
        assert L.rt_debug_family_test_batch(0, *bad) == RT_ERR_ARG
    bad = list(good)
    bad[5] = -1
    assert L.rt_debug_family_test_host(*bad) == RT_ERR_ARG
