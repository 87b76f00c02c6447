"""The host side of the refit (rt_scene_refit): no GPU.

rt_refit_aabbs_host against boxes computed here in numpy (refit_cases.numpy_refit_aabbs) and
against rt_build_bvh; rt_debug_scene_refit_pack — pack_scene, then rt::refit_packed, the host
restatement of the device refit — against rt_debug_scene_pack where a plain pack must give the
same bytes, and against the numpy boxes' root elsewhere.  Every comparison is of bit patterns and
digests.

The chain scenes' shipped aabbs hold z = -0 where aabb_of_triangle gives a max corner of +0
(tests/golden/chain_bvh.py: -0.01 * 0), equal as numbers, not as bits; a refit writes
aabb_of_triangle's boxes, so for those scenes the identity refit is compared with the plain pack
of (nodes, numpy boxes, tris) after checking that the numpy boxes equal the shipped ones as
numbers.  For every other scene the shipped aabbs are the numpy boxes bit for bit.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

from conftest import REPO, host_scene

import refit_cases as rc
from raytracinginonesemester_amd import _lib
import raytracinginonesemester_amd as rt

NONE = rc.NONE
NEW_NAMES = ["rt_scene_create_refittable", "rt_scene_refit_device", "rt_scene_refit", "rt_refit_aabbs_host",
             "rt_triangles_from_mesh_device", "rt_debug_scene_digest", "rt_debug_scene_refit_pack",
             "rt_debug_scene_refit_chain"]
CASES = [(s, d) for s in rc.SCENES for d in rc.DEFORMATIONS]


def test_new_names_are_declared_and_bound():
    hdr = (REPO / "include" / "rt_mi355x.h").read_text()
    added = hdr[hdr.index("#define RT_ABI_VERSION"):hdr.index("enum {")]
    for name in NEW_NAMES:
        assert re.search(rf"\b{name}\b", added), name  # the "added since" list of RT_ABI_VERSION
        assert re.search(rf"\b{name}\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib(), name), name
    assert _lib.lib().rt_abi_version() == 3
    assert "#define RT_ABI_VERSION 3 " in hdr


@pytest.mark.parametrize("scene", ["sphere_single", "frog", "cornell"])
def test_refit_aabbs_of_the_build_are_the_builds(scene):
    """On rt_build_bvh's tree and the triangles it was built from, the refit boxes are the build's."""
    hs = host_scene(scene + ".json")
    nodes, aabbs = rt.build_bvh(hs.positions, hs.indices)
    got = rt.refit_aabbs(nodes, hs.triangles)
    assert got.tobytes() == aabbs.tobytes()
    assert got.tobytes() == np.ascontiguousarray(hs.aabbs, np.float32).tobytes()


@pytest.mark.parametrize("scene,kind", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_refit_aabbs_are_the_numpy_boxes(scene, kind):
    a = rc.scene(scene)
    got = rt.refit_aabbs(a["nodes"], rc.deformed(scene, kind))
    assert got.tobytes() == rc.expected_aabbs(scene, kind).tobytes()


@pytest.mark.parametrize("scene", rc.SCENES)
def test_identity_refit_is_the_plain_pack(scene):
    a = rc.scene(scene)
    boxes = rc.expected_aabbs(scene, "identity")
    assert np.array_equal(boxes, a["aabbs"])  # as numbers
    if not scene.startswith("chain"):
        assert boxes.tobytes() == a["aabbs"].tobytes()  # (the chains: -0 vs +0, see the module docstring)
    want = rc.pack(a["P"], a["nodes"], boxes, a["tris"])
    got = rc.refit_pack(scene, a["tris"])
    assert rc.same(got, want), (got, want)


@pytest.mark.parametrize("scene", rc.SCENES)
def test_times_two_refit_is_the_pack_of_the_doubled_scene(scene):
    """Doubling is exact: every greedy weight scales by 4, every choice stays."""
    a = rc.scene(scene)
    new = rc.deformed(scene, "times2")
    boxes = rc.expected_aabbs(scene, "identity") * np.float32(2)
    assert boxes.tobytes() == rc.expected_aabbs(scene, "times2").tobytes()
    assert rc.same(rc.refit_pack(scene, new), rc.pack(a["P"], a["nodes"], boxes, new))


@pytest.mark.parametrize("scene,kind", CASES, ids=[f"{s}-{d}" for s, d in CASES])
def test_refit_keeps_the_topology_and_bounds_the_new_geometry(scene, kind):
    a = rc.scene(scene)
    info0, dig0 = rc.pack(a["P"], a["nodes"], a["aabbs"], a["tris"])
    info, dig = rc.refit_pack(scene, rc.deformed(scene, kind))
    assert info[rc.TOPOLOGY].tolist() == info0[rc.TOPOLOGY].tolist()
    assert dig[0::2].tolist() == dig0[0::2].tolist()  # every array keeps its length
    root = rc.expected_aabbs(scene, kind)[0]
    assert [int(x) & 0xFFFFFFFF for x in info[rc.ROOT_BOX]] == rc.bits(root)
    assert [int(x) & 0xFFFFFFFF for x in info[rc.BMAX]] == rc.bmax_bits(root)


@pytest.mark.parametrize("scene", rc.SCENES)
def test_refit_there_and_back(scene):
    """A, then B, then A again: A's digests (nothing of B, or of the order of refits, stays)."""
    a = rc.scene(scene)
    A, B = rc.deformed(scene, "wobble"), rc.deformed(scene, "wobble_b")
    want = rc.refit_pack(scene, A)
    assert not rc.same(want, rc.refit_pack(scene, B))
    info, dig = np.zeros(21, np.int64), np.zeros(22, np.uint64)
    poses = (C.c_void_p * 3)(A.ctypes.data, B.ctypes.data, A.ctypes.data)
    _lib.check(_lib.lib().rt_debug_scene_refit_chain(int(a["P"]), a["nodes"].ctypes.data, a["aabbs"].ctypes.data,
                                                     a["tris"].ctypes.data, 3, poses, info.ctypes.data, dig.ctypes.data))
    assert rc.same((info, dig), want)


def _small_tree():
    """P = 4, a full tree: (nodes, tris)."""
    leaf = lambda parent, obj: (parent, NONE, NONE, obj)  # noqa: E731
    nodes = np.array([(NONE, 1, 2, NONE), (0, 3, 4, NONE), (0, 5, 6, NONE), leaf(1, 0), leaf(1, 1), leaf(2, 2), leaf(2, 3)],
                     np.uint32)
    return nodes, rc._hand_tris(4)


@pytest.mark.parametrize("what", ["leaf_names_no_triangle", "missing_child", "unreachable_node"])
def test_improper_trees_are_refused(what):
    nodes, tris = _small_tree()
    if what == "leaf_names_no_triangle":
        nodes[4, 3] = 9
    elif what == "missing_child":
        nodes[1, 2] = NONE  # (leaf 4 is then unreachable too)
    else:  # node 2's right child is leaf 5 again: leaf 6 is reached from nowhere
        nodes[2, 2] = 5
    boxes = np.zeros((7, 6), np.float32)
    boxes[:, 3:] = 8
    info, dig = np.zeros(21, np.int64), np.zeros(22, np.uint64)
    lib = _lib.lib()
    assert lib.rt_debug_scene_pack(4, nodes.ctypes.data, boxes.ctypes.data, tris.ctypes.data, info.ctypes.data,
                                   dig.ctypes.data) == 0  # a plain scene takes the tree
    assert lib.rt_debug_scene_refit_pack(4, nodes.ctypes.data, boxes.ctypes.data, tris.ctypes.data, tris.ctypes.data,
                                         info.ctypes.data, dig.ctypes.data) == -7  # RT_ERR_UNSUPPORTED
    out = np.zeros((7, 6), np.float32)
    assert lib.rt_refit_aabbs_host(4, nodes.ctypes.data, tris.ctypes.data, out.ctypes.data) == -7
    # rt_scene_create_refittable packs before it looks for a device: refused here too, nothing created
    h = C.c_void_p()
    assert lib.rt_scene_create_refittable(0, 4, nodes.ctypes.data, boxes.ctypes.data, tris.ctypes.data, None, None, 0,
                                          None, 0, C.byref(h)) == -7
    assert not h


def test_quantised_records_are_refused(tune):
    a = rc.scene("frog")
    tune(quant_records=1)
    info, dig = np.zeros(21, np.int64), np.zeros(22, np.uint64)
    assert _lib.lib().rt_debug_scene_refit_pack(int(a["P"]), a["nodes"].ctypes.data, a["aabbs"].ctypes.data,
                                                a["tris"].ctypes.data, a["tris"].ctypes.data, info.ctypes.data,
                                                dig.ctypes.data) == -7


def test_a_vertex_that_is_not_finite_is_refused():
    a = rc.scene("cornell")
    for bad in (np.nan, np.inf):
        t = a["tris"].copy()
        t[a["P"] // 2, 4] = bad
        info, dig = np.zeros(21, np.int64), np.zeros(22, np.uint64)
        assert _lib.lib().rt_debug_scene_refit_pack(int(a["P"]), a["nodes"].ctypes.data, a["aabbs"].ctypes.data,
                                                    a["tris"].ctypes.data, t.ctypes.data, info.ctypes.data,
                                                    dig.ctypes.data) == -1
