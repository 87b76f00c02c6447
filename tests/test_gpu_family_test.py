"""The device build of the wave-family entry test (rt_debug_family_test_batch: family_dirs with
its wave reductions and v_rcp_f32, then family_entry_passes in the loop form the wave takes, what
frustum_loop calls), one wave per item, on the sets of tests/family_cases.py: an entry passes
wherever some live lane's own ref_aabb passes with its bestT, every entry the float64 model with
the 2^-18 widening rejects is rejected, the loop form is the model's; no tolerance.  The host
build runs the same sets in tests/test_family_test_host.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import family_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fc.FAMILY_CASES)
def test_device_build_both_sides(name):
    out, _ = fc.check_set(fc.device_fn, name)
    c = fc.family_case(name)
    host, _ = fc.host_fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"])
    print(f"{name}: device and host builds differ on {int((out != host).sum())} of {out.size} entries")


@pytest.mark.parametrize("name", ["camera_axis", "free"])
def test_inactive_lanes_change_no_answer(name):
    fc.check_inactive_lanes(fc.device_fn, name)


def test_short_batches():
    fc.check_short_batches(fc.device_fn)
