"""The rebuild's host side (rt_build_bvh_triangles, rt_debug_box_weight_host, the refusals of
rt_scene_rebuild*), on the CPU.

rt_build_bvh_triangles is rt_build_bvh over the flattened vertices, places internal nodes first and
leaves last, and its trees pack to 4-ary records without the deep kernels for every scene and pose
the GPU tests rebuild.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import rebuild_cases as rbc
import refit_cases as rc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

NONE = 0xFFFFFFFF
CASES = [(s, k) for s in rbc.DEVICE_SCENES + ("p1",) for k in rbc.poses_of(s) + (() if s in rbc.SHIPPED else ("wobble_b",))]
IDS = [f"{s}-{k}" for s, k in CASES]


@pytest.mark.parametrize("name,kind", CASES, ids=IDS)
def test_build_bvh_triangles_is_build_bvh_over_the_flattened_vertices(name, kind):
    tris = rbc.pose(name, kind)
    P = tris.shape[0]
    nodes, aabbs = rbc.tree(name, kind)
    pos = np.ascontiguousarray(tris[:, :9]).reshape(-1, 3)
    n2, a2 = rt.build_bvh(pos, np.arange(3 * P, dtype=np.uint32).reshape(P, 3))
    assert nodes.tobytes() == n2.tobytes() and aabbs.tobytes() == a2.tobytes()
    # internal nodes first, leaves last, every triangle once
    assert (nodes[:P - 1, 3] == NONE).all() and (nodes[P - 1:, 3] != NONE).all()
    assert np.array_equal(np.sort(nodes[P - 1:, 3]), np.arange(P, dtype=np.uint32))
    assert (nodes[:P - 1, 1:3] < 2 * P - 1).all()


@pytest.mark.parametrize("name,kind", [c for c in CASES if c[0] != "p1"], ids=[i for i in IDS if not i.startswith("p1")])
def test_rebuilt_trees_take_the_wide_records_and_are_not_deep(name, kind):
    info, _ = rbc.expected(name, kind)
    f = dict(zip(rc.INFO, (int(x) for x in info[:12])))
    assert f["wide"] == 1 and f["deep"] == 0, f
    assert f["f_log2"] == 5
    assert f["binary_stack"] <= 64 and f["wide_stack"] <= 64


def test_cornell_wobble_arity_falls_back_with_the_stack_cap():
    """What the GPU test's caps rely on: f_log2 5, 4, 3, 2 at caps 128, 60, 40, 25."""
    want = {128: (5, 68), 60: (4, 47), 40: (3, 29), 25: (2, None)}
    try:
        for cap, (log2, bound) in want.items():
            rt.set_tuning("frustum_stack_cap", cap)
            info, _ = rbc.expected("cornell", "wobble")
            assert int(info[8]) == log2, (cap, int(info[8]), int(info[9]))
            if bound is not None:
                assert int(info[9]) == bound
    finally:
        rt.reset_tuning()


def _weights(boxes, leaves, rule):
    boxes = np.ascontiguousarray(boxes, np.float32)
    leaves = np.ascontiguousarray(leaves, np.uint32)
    out = np.zeros(leaves.size, np.float64)
    L.check(L.lib().rt_debug_box_weight_host(L.ptr(boxes), L.ptr(leaves), rule, leaves.size, L.ptr(out)))
    return out


def test_box_weight_host_is_numpy_float64():
    rng = np.random.default_rng(5)
    lo = rng.uniform(-3, 3, (4000, 3)).astype(np.float32)
    ext = rng.uniform(-0.5, 4, (4000, 3)).astype(np.float32)  # some extents negative: they count 0
    boxes = np.hstack([lo, lo + ext]).astype(np.float32)
    boxes[:8, 3:] = boxes[:8, :3]      # zero extent
    boxes[8:16, 3:] = np.float32(1e30)  # the area overflows no double, the product with sqrt may not either
    boxes[16, 3] = np.inf
    boxes[17, 0] = np.nan
    leaves = rng.integers(1, 1 << 30, 4000).astype(np.uint32)
    d = np.maximum(0.0, boxes[:, 3:].astype(np.float64) - boxes[:, :3].astype(np.float64))
    d = np.where(np.isnan(d), 0.0, d)  # std::max(0.0, NaN) is 0.0
    area = d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0]
    for rule, w in ((1, area), (2, area * np.sqrt(leaves.astype(np.float64)))):
        w = np.where(np.isfinite(w), w, 1e300)
        got = _weights(boxes, leaves, rule)
        assert got.tobytes() == w.tobytes(), np.flatnonzero(got != w)[:8]
    assert _weights(boxes[16:17], leaves[16:17], 1)[0] == 1e300


def test_refusals():
    lib = L.lib()
    tris = np.zeros((2, 18), np.float32)
    nodes, aabbs = np.zeros((3, 4), np.uint32), np.zeros((3, 6), np.float32)
    assert lib.rt_build_bvh_triangles(2, None, L.ptr(nodes), L.ptr(aabbs)) == -1
    assert lib.rt_build_bvh_triangles(2, L.ptr(tris), None, L.ptr(aabbs)) == -1
    assert lib.rt_build_bvh_triangles(2, L.ptr(tris), L.ptr(nodes), None) == -1
    assert lib.rt_build_bvh_triangles(0, L.ptr(tris), L.ptr(nodes), L.ptr(aabbs)) == -1
    with pytest.raises(L.RTError):
        rt.build_bvh_triangles(np.zeros((0, 18), np.float32))
    assert lib.rt_scene_rebuild(None, L.ptr(tris), None, None, None) == -1
    assert lib.rt_scene_rebuild_device(None, L.ptr(tris), None, None, None, None) == -1
    assert lib.rt_scene_rebuild_path(None) == L.RT_REBUILD_NONE
    out = np.zeros(1, np.float64)
    assert lib.rt_debug_box_weight_host(None, None, 1, 1, L.ptr(out)) == -1
    assert lib.rt_debug_box_weight_host(None, None, 1, 0, None) == 0
