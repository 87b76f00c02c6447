"""The device build of the box tests (rt_box_test_batch: make_ray with v_rcp_f32 reciprocals,
box_ends / box_ends_pk, box_classify, box_hit and the three box_hit_mask forms the traversals
instantiate) against ref_aabb, numpy's float64 restatement of the reference's intersectAABB
(G/include/bvh.h:81-129), item for item and with no tolerance, on the sets of tests/box_cases.py:
random and extreme magnitudes, rays aimed at corners, edges and faces with tmax on the aimed
parameter and its float neighbours, tmax bands across the pre-classification's margin, the same
under scene-like bounds, degenerate boxes and directions.  The host build runs the same sets in
tests/test_box_filter.py.

So that the test cannot pass by sending everything to the double path: without a parallel axis
the random sets are ambiguous on at most 0.1 % of the items (the host build, whose reciprocal is
exact: none), every class occurs on the bands set, and a sure class never contradicts ref_aabb.
"""
from __future__ import annotations

import numpy as np
import pytest

import box_cases as bc
from raytracinginonesemester_amd import _lib

pytestmark = pytest.mark.gpu

MASK_COLS = (2, 3, 4)  # box_hit_mask<false,false>, <true,false>, <true,true>


def _run(case, bmax=None, active=None, n=None):
    n = case["ref"].size if n is None else n
    out = np.full((n, 5), -1, np.int32)
    bm = None if bmax is None else np.ascontiguousarray(bmax, np.float32)
    act = None if active is None else np.ascontiguousarray(active, np.uint8)
    _lib.check(_lib.lib().rt_box_test_batch(
        0, case["rays"].ctypes.data, case["boxes"].ctypes.data, case["tmm"].ctypes.data,
        None if bm is None else bm.ctypes.data, None if act is None else act.ctypes.data, n, out.ctypes.data))
    return out


def _check(case, out, what):
    ref = case["ref"][:out.shape[0]].astype(np.int32)
    for col in (0,) + MASK_COLS:
        bad = np.flatnonzero(out[:, col] != ref)
        assert bad.size == 0, (f"{what}: column {col} differs from ref_aabb on {bad.size} of {ref.size} items "
                               f"(device {out[bad[:5], col]}, class {out[bad[:5], 1]})\n" + bc.hex_triples(case, bad))
    cls = out[:, 1]
    assert np.isin(cls, (0, 1, 2)).all()
    bad = np.flatnonzero((cls != 2) & (cls != ref))
    assert bad.size == 0, f"{what}: {bad.size} sure classes contradict ref_aabb\n" + bc.hex_triples(case, bad)
    return {k: float((cls == v).mean()) for k, v in (("miss", 0), ("hit", 1), ("ambiguous", 2))}


@pytest.mark.parametrize("name", bc.BOX_CASES)
def test_sets_match_the_numpy_reference(name):
    c = bc.box_case(name)
    out = _run(c)
    share = _check(c, out, name)
    print(f"{name}: n {c['ref'].size}, hit share {c['ref'].mean():.3f}, device classes {share}")
    if name in bc.RANDOM_CASES:
        sel = bc.no_parallel_axis(c)
        amb = float((out[sel, 1] == 2).mean())
        print(f"{name}: ambiguous share without a parallel axis {amb:.6f} of {int(sel.sum())}")
        assert amb <= 1e-3
    if name == "bands":
        assert all(v > 0 for v in share.values()), share


@pytest.mark.parametrize("factor", bc.BOUND_FACTORS)
@pytest.mark.parametrize("name", bc.BOUND_CASES)
def test_scene_like_bounds(name, factor):
    """bmax a multiple of the box's own, as a scene's bound exceeds a node's: a wider margin E,
    more ambiguous items, the same answers."""
    c = bc.box_case(name)
    share = _check(c, _run(c, bmax=bc.own_bmax(c["boxes"]) * np.float32(factor)), f"{name} x{factor:g}")
    print(f"{name} bmax x{factor:g}: device classes {share}")
    if name == "bands":
        assert all(v > 0 for v in share.values()), share


N_MIXED = 200_003  # not a multiple of 64: the last wave is partial


@pytest.mark.parametrize("pattern", ["all", "half", "waves_off", "one_lane", "nonzero_bytes"])
def test_active_patterns(pattern):
    """The wave forms answer for the lanes of `active` (and i < n) only, inactive lanes read 0,
    and what the other lanes do changes no active lane's answer; the scalar forms ignore it."""
    c = bc.mixed_case(N_MIXED)
    act = bc.active_patterns(N_MIXED)[pattern]
    out = _run(c, active=act)
    ref = c["ref"].astype(np.int32)
    on = np.ones(N_MIXED, bool) if act is None else act != 0
    for col in MASK_COLS:
        bad = np.flatnonzero(out[:, col] != np.where(on, ref, 0))
        assert bad.size == 0, (f"{pattern}: column {col} wrong on {bad.size} items ({int(on[bad].sum())} of them "
                               f"active)\n" + bc.hex_triples(c, bad))
    assert np.array_equal(out[:, 0], ref)
    bad = np.flatnonzero((out[:, 1] != 2) & (out[:, 1] != ref))
    assert bad.size == 0


def test_short_batches():
    """n below a wave, one past a wave and one past a block: nothing is written past n."""
    c = bc.mixed_case(N_MIXED)
    for n in (1, 63, 65, 257):
        out = _run(c, n=n)
        assert np.array_equal(out[:, 0], c["ref"][:n].astype(np.int32)), n
        for col in MASK_COLS:
            assert np.array_equal(out[:, col], out[:, 0]), (n, col)
