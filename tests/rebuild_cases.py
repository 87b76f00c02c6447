"""Scenes, poses and expectations of the rebuild tests (rt_scene_rebuild): a helper
module, no tests here.

A rebuild's expectation is the host's own: rt_build_bvh_triangles over the pose, then
rt_debug_scene_pack of (that tree, the pose) — what rt_scene_create_refittable would hold.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import refit_cases as rc
import tie_scenes as ts

F32 = np.float32
SEED = 20241020
SHIPPED = ("sphere_single", "cornell", "frog")
POSES = ("identity", "wobble", "flat", "shift4096")
SOUP_SIZES = (2, 3, 33, 64, 65, 1025, 5000)
SOUPS = tuple(f"soup{p}" for p in SOUP_SIZES)
# every scene the device path must take (p1 takes the host path)
DEVICE_SCENES = SHIPPED + ("ties", "same500") + SOUPS
ARRAYS = ("inode", "wnode", "fnode", "qent", "qhdr", "ibox", "leaf", "tnorm", "cut", "cut2", "tri")


def _borrowed_tables(P):
    import chain_bvh

    d = chain_bvh.chain_scene(8)
    return {"triobj": np.zeros(P, np.int32), "mats": d["mats"].view(F32).reshape(-1, 13), "lights": d["lights"],
            "light": np.array((3.0, 3.0, 5.0), np.float64)}


def _soup(P):
    rng = np.random.default_rng(SEED + P)
    c = rng.uniform(-1, 1, (P, 1, 3))
    v = c + rng.normal(scale=0.15, size=(P, 3, 3))
    n = rng.normal(size=(P, 3, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    return np.ascontiguousarray(np.hstack([v.reshape(P, 9), n.reshape(P, 9)]), F32)


@lru_cache(maxsize=None)
def scene(name: str) -> dict:
    """ray_batches.scene_arrays' keys; nodes / aabbs: the tree the scene is created with (the shipped
    one, or the host LBVH of the triangles)."""
    import raytracinginonesemester_amd as rt

    if name in SHIPPED or name == "p1":
        return rc.scene(name)
    if name == "ties":
        a = dict(ts.scene("small"))
    else:
        if name == "same500":
            one = np.array([0, 0, 0, 1, 0, 0.25, 0, 1, 0.5, 0, 0, 1, 0, 0, 1, 0, 0, 1], F32)
            tris = np.ascontiguousarray(np.tile(one, (500, 1)))
        else:
            tris = _soup(int(name[4:]))
        nodes, aabbs = rt.build_bvh_triangles(tris)
        a = {"P": tris.shape[0], "nodes": nodes, "aabbs": aabbs, "tris": tris, **_borrowed_tables(tris.shape[0])}
    a["nodes"] = np.ascontiguousarray(a["nodes"], np.uint32).reshape(-1, 4)
    a["aabbs"] = np.ascontiguousarray(a["aabbs"], F32)
    a["tris"] = np.ascontiguousarray(a["tris"], F32)
    for v in a.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return a


def poses_of(name: str):
    return POSES if name in SHIPPED else ("identity",)


@lru_cache(maxsize=None)
def pose(name: str, kind: str) -> np.ndarray:
    """The scene's triangles in that pose (refit_cases' deformations for the shipped scenes; the
    others have `identity` and a second pose `wobble_b`, their y moved by their z)."""
    if name in SHIPPED:
        return rc.deformed(name, kind)
    t = scene(name)["tris"].copy()
    if kind == "wobble_b":
        v = np.ascontiguousarray(t[:, :9]).reshape(-1, 3)
        v[:, 1] += F32(0.07) * np.cos(F32(5) * v[:, 2]).astype(F32)
        t[:, :9] = v.reshape(-1, 9)
    elif kind != "identity":
        raise KeyError(kind)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def tree(name: str, kind: str):
    """rt_build_bvh_triangles of the pose: (nodes, aabbs), read-only."""
    import raytracinginonesemester_amd as rt

    nodes, aabbs = rt.build_bvh_triangles(pose(name, kind))
    nodes.setflags(write=False)
    aabbs.setflags(write=False)
    return nodes, aabbs


def expected(name: str, kind: str):
    """rt_debug_scene_pack of (tree, pose) under the knobs in force: (info, digests)."""
    nodes, aabbs = tree(name, kind)
    return rc.pack(scene(name)["P"], nodes, aabbs, pose(name, kind))


def refit_expected(name: str, kind: str, kind_b: str):
    """rt_debug_scene_refit_pack: the scene packed from (tree, pose), refitted to pose_b."""
    from raytracinginonesemester_amd import _lib

    nodes, aabbs = tree(name, kind)
    a, b = pose(name, kind), pose(name, kind_b)
    return rc._words(_lib.lib().rt_debug_scene_refit_pack, int(scene(name)["P"]), nodes.ctypes.data, aabbs.ctypes.data,
                     a.ctypes.data, b.ctypes.data)


def differences(got, want) -> list:
    """The names of what differs between two (info, digests): info words by name, arrays by name."""
    names = rc.INFO + [f"root_box[{i}]" for i in range(6)] + [f"bmax[{i}]" for i in range(3)]
    out = [names[i] for i in range(21) if int(got[0][i]) != int(want[0][i])]
    for i, a in enumerate(ARRAYS):
        if int(got[1][2 * i]) != int(want[1][2 * i]):
            out.append(f"{a} (bytes {int(got[1][2 * i])} vs {int(want[1][2 * i])})")
        elif int(got[1][2 * i + 1]) != int(want[1][2 * i + 1]):
            out.append(a)
    return out


def oracle_arrays(name: str, kind: str) -> dict:
    a = scene(name)
    nodes, aabbs = tree(name, kind)
    return {"P": a["P"], "nodes": nodes, "aabbs": aabbs, "tris": pose(name, kind), "triobj": a["triobj"], "mats": a["mats"],
            "lights": a["lights"]}
