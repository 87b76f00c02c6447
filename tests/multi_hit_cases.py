"""Scenes, rays, bounds and a model of the multi-hit query (rt_trace_multi_hits):
a helper module, no tests here.

The model does not call the code under test.  It walks the tree breadth-first in numpy, carrying
only the (ray, node) pairs that survive: each pair's box goes through rt_box_test_host's out_exact
(the reference's double slab test) at [1e-4, tmax]; the surviving leaves' (ray, triangle) pairs go
through rt_hit_record_host (intersectTriangle at [1e-4, FLT_MAX]) and are kept when t <= tmax; the
list is sorted by (t, triangle).  For trees tall enough to fill the reference's 512-entry stack it
replays SearchBVH's pushes and pops per ray on the recorded box answers, and a ray whose replay
sets the overflow flag takes the brute-force set instead: every triangle of the scene that
rt_hit_record_host accepts with t <= tmax.
"""
from __future__ import annotations

import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

import ray_batches as rb
import refit_cases as rc
import tie_scenes as ts

HERE = Path(__file__).resolve().parent
if str(HERE / "golden") not in sys.path:
    sys.path.insert(0, str(HERE / "golden"))

NONE = 0xFFFFFFFF
F32 = np.float32
TMIN = F32(1e-4)
FLT_MAX = np.finfo(np.float32).max
STACK = 512  # SearchBVH's STACK_CAPACITY (G/include/query.h:245)
KS = (0, 1, 2, 4, 5, 8, 32)
LATTICE = ("small", "scaled")
CHAINS = ("chain24", "chain300", "chain600")
SCENES = ("sphere_single", "frog", "cornell") + CHAINS + LATTICE
BOUNDS = ("none", "around")  # max_t = None, or per ray around the model's own hit distances


@lru_cache(maxsize=None)
def arrays(name: str) -> dict:
    """ray_batches.scene_arrays' keys: P, nodes (2P-1, 4) uint32, aabbs, tris, ... (read-only)."""
    a = dict(ts.scene(name)) if name in LATTICE else dict(rb.scene_arrays(name))
    a["nodes"] = np.ascontiguousarray(a["nodes"]).view(np.uint32).reshape(-1, 4)
    a["aabbs"] = np.ascontiguousarray(a["aabbs"], F32).reshape(-1, 6)
    a["tris"] = np.ascontiguousarray(a["tris"], F32).reshape(-1, 18)
    return a


def closest(name: str) -> dict:
    """The scene's 4096-ray batch with the oracle's SearchBVH answers (rays, idx, t)."""
    return ts.batch(name) if name in LATTICE else rb.batch(name)


def axis_ray() -> np.ndarray:
    """From chain_bvh.CAMERA's position towards the origin: through every level of a chain scene."""
    import chain_bvh

    pos = np.array(chain_bvh.CAMERA[0], np.float64)
    return np.concatenate([pos, -pos]).astype(F32)


@lru_cache(maxsize=None)
def rays(name: str) -> np.ndarray:
    """The batch's rays; for the chain scenes one more, the axis ray, at the end."""
    r = closest(name)["rays"]
    if name in CHAINS:
        r = np.vstack([r, axis_ray()[None, :]])
    r = np.ascontiguousarray(r, F32)
    r.setflags(write=False)
    return r


def device_scene(name: str, device: int = 0, refittable: bool = False):
    import raytracinginonesemester_amd as rt

    a = arrays(name)
    return rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], device,
                          refittable=refittable)


# ---- the model ---------------------------------------------------------------------------------
def _boxes_pass(r, boxes, tmax):
    """out_exact of rt_box_test_host for (ray, box, [1e-4, tmax]) triples."""
    from raytracinginonesemester_amd import _lib as L

    n = r.shape[0]
    r, boxes = np.ascontiguousarray(r, F32), np.ascontiguousarray(boxes, F32)
    tm = np.empty((n, 2), F32)
    tm[:, 0], tm[:, 1] = TMIN, tmax
    fast, exact, cls = (np.zeros(n, np.int32) for _ in range(3))
    if n:
        L.check(L.lib().rt_box_test_host(r.ctypes.data, boxes.ctypes.data, tm.ctypes.data, n, fast.ctypes.data,
                                         exact.ctypes.data, cls.ctypes.data))
    return exact != 0


def _accepted(r, tris, tmax):
    """(hit, t, u, v) of rt_hit_record_host for (ray, triangle) pairs, a hit kept when t <= tmax."""
    import raytracinginonesemester_amd as rt

    n = r.shape[0]
    hit, t, u, v = np.zeros(n, bool), np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    for s in range(0, n, 1 << 18):
        e = min(n, s + (1 << 18))
        rec = rt.hit_record_host(r[s:e], tris[s:e])
        hit[s:e] = (rec["tri"] >= 0) & (rec["t"] <= tmax[s:e])
        t[s:e], u[s:e], v[s:e] = rec["t"], rec["u"], rec["v"]
    return hit, t, u, v


def _replay_overflow(nodes, passed_pairs, n):
    """SearchBVH's stack, replayed for n rays at once on the recorded box answers (passed_pairs:
    (ray, node) of every pair whose box passed): per ray whether a push met a full stack, and the
    (n, nodes) table of the nodes that replay opened (those whose pushes were dropped are not)."""
    nn = nodes.shape[0]
    ok = np.zeros((n, nn), bool)
    ok[passed_pairs[0], passed_pairs[1]] = True
    seen = np.zeros((n, nn), bool)
    left, right, obj = (nodes[:, k].astype(np.int64) for k in (1, 2, 3))
    stack = np.zeros((n, STACK), np.int64)
    sp = np.ones(n, np.int64)  # the root is pushed unconditionally
    overflow = np.zeros(n, bool)
    rows = np.arange(n)
    while (sp > 0).any():
        live = sp > 0
        sp = np.where(live, sp - 1, sp)
        node = stack[rows, sp]
        passed = live & ok[rows, node]
        seen[rows[passed], node[passed]] = True
        opened = passed & (obj[node] == NONE)
        for child in (left, right):
            c = child[node]
            push = opened & (c != NONE)
            push &= ok[rows, np.where(push, c, 0)]
            full = push & (sp >= STACK)
            overflow |= full
            push &= ~full
            stack[rows[push], sp[push]] = c[push]
            sp = sp + push
    return overflow, seen


def model_lists(name_or_arrays, r, max_t=None) -> dict:
    """The model's answers for rays r (n, 6) and bounds max_t (n,) or None: count (n,), the flat
    hit list sorted by (ray, t, tri) as ray, tri, t, u, v, start (n + 1 offsets into it), overflow
    (n,) and dfs_count (n,), the count without the overflow rule: the hits at the leaves the replayed
    DFS reached, its dropped pushes left out."""
    a = arrays(name_or_arrays) if isinstance(name_or_arrays, str) else name_or_arrays
    nodes, aabbs, tris, P = a["nodes"], a["aabbs"], a["tris"], int(a["P"])
    r = np.ascontiguousarray(r, F32)
    n = r.shape[0]
    tmax = np.full(n, FLT_MAX, F32) if max_t is None else np.ascontiguousarray(max_t, F32)
    ray, node = np.arange(n), np.zeros(n, np.int64)
    leaf_ray, leaf_tri, leaf_node, passed = [], [], [], []
    while ray.size:
        ok = _boxes_pass(r[ray], aabbs[node], tmax[ray])
        ray, node = ray[ok], node[ok]
        passed.append((ray, node))
        is_leaf = nodes[node, 3] != NONE
        names = is_leaf & (nodes[node, 3] < P)  # a leaf that names no triangle contributes nothing
        leaf_ray.append(ray[names])
        leaf_tri.append(nodes[node[names], 3].astype(np.int64))
        leaf_node.append(node[names])
        ray, node = ray[~is_leaf], node[~is_leaf]
        kids = np.stack([nodes[node, 1], nodes[node, 2]], axis=1).astype(np.int64)
        ray = np.repeat(ray, 2)
        node = kids.reshape(-1)
        keep = node != NONE
        ray, node = ray[keep], node[keep]
    hr_, ht_ = np.concatenate(leaf_ray), np.concatenate(leaf_tri)
    hit, t, u, v = _accepted(r[hr_], tris[ht_], tmax[hr_])
    hn_ = np.concatenate(leaf_node)[hit]
    hr_, ht_, t, u, v = hr_[hit], ht_[hit], t[hit], u[hit], v[hit]
    dfs_count = np.bincount(hr_, minlength=n).astype(np.int32)
    overflow = np.zeros(n, bool)
    if int(rc.heights(nodes)[0]) + 1 > STACK:  # a DFS stack holds at most height + 1 entries
        pr = np.concatenate([p[0] for p in passed])
        pn = np.concatenate([p[1] for p in passed])
        overflow, seen = _replay_overflow(nodes, (pr, pn), n)
        dfs_count = np.bincount(hr_[seen[hr_, hn_]], minlength=n).astype(np.int32)
        assert (seen[hr_, hn_] | overflow[hr_]).all()  # without overflow the DFS opens every passing leaf
    if overflow.any():
        who = np.flatnonzero(overflow)
        br, bt = np.repeat(who, P), np.tile(np.arange(P, dtype=np.int64), who.size)
        bh, t2, u2, v2 = _accepted(r[br], tris[bt], tmax[br])
        keep = ~overflow[hr_]
        hr_ = np.concatenate([hr_[keep], br[bh]])
        ht_ = np.concatenate([ht_[keep], bt[bh]])
        t, u, v = (np.concatenate([x[keep], y[bh]]) for x, y in ((t, t2), (u, u2), (v, v2)))
    order = np.lexsort((ht_, t.view(np.uint32), hr_))  # t >= 1e-4: the bits order as the floats
    hr_, ht_, t, u, v = hr_[order], ht_[order], t[order], u[order], v[order]
    count = np.bincount(hr_, minlength=n).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    return {"count": count, "ray": hr_, "tri": ht_.astype(np.int32), "t": t, "u": u, "v": v, "start": start,
            "overflow": overflow, "dfs_count": dfs_count}


def take(m: dict, k: int):
    """(count, tri, t, u, v) as the query returns them for a list length k: (n, k) arrays, the
    slots past count holding -1, -1.0, 0, 0."""
    n = m["count"].size
    tri = np.full((n, k), -1, np.int32)
    t = np.full((n, k), -1.0, F32)
    u, v = np.zeros((n, k), F32), np.zeros((n, k), F32)
    rank = np.arange(m["ray"].size) - m["start"][m["ray"]]
    sel = rank < k
    rr, kk = m["ray"][sel], rank[sel]
    tri[rr, kk], t[rr, kk], u[rr, kk], v[rr, kk] = m["tri"][sel], m["t"][sel], m["u"][sel], m["v"][sel]
    return m["count"].copy(), tri, t, u, v


def bounds_around(m: dict, seed: int = 7) -> np.ndarray:
    """A max_t per ray drawn around the unbounded model m's hit distances, by ray index mod 4:
    exactly the t of one of the ray's hits, one ulp below it, below 1e-4 (5e-5), and inf.  (A ray
    without hits takes 1.0 for the t.)"""
    n = m["count"].size
    rng = np.random.default_rng(seed)
    pick = m["start"][:-1] + (rng.integers(0, 1 << 30, n) % np.maximum(m["count"], 1))
    t = np.where(m["count"] > 0, m["t"][np.minimum(pick, max(m["t"].size - 1, 0))] if m["t"].size else F32(1), F32(1)).astype(F32)
    kind = np.arange(n) % 4
    out = np.select([kind == 0, kind == 1, kind == 2], [t, np.nextafter(t, F32(0)), np.full(n, 5e-5, F32)],
                    np.full(n, np.inf, F32)).astype(F32)
    return out


@lru_cache(maxsize=None)
def model(name: str, bound: str = "none") -> dict:
    """model_lists for the scene's rays (shared, read-only), with max_t (None for "none")."""
    if bound == "none":
        m = model_lists(name, rays(name))
        m["max_t"] = None
    else:
        mt = bounds_around(model(name, "none"))
        m = model_lists(name, rays(name), mt)
        m["max_t"] = mt
    for x in m.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return m


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing_rays(got, want):
    """Indices of the rays where any of (count, tri, t, u, v) differs in any byte."""
    bad = got[0] != want[0]
    for g, w in zip(got[1:], want[1:]):
        if g.shape[1]:
            bad |= (np.ascontiguousarray(g).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32)).any(axis=1)
    return np.flatnonzero(bad)
