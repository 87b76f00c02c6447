"""The closest-point query without a GPU (rt_closest_points_host):

* the host build equals the numpy model of tests/closest_point_cases.py byte for byte on every
  scene, point class and bound mode;
* the lemma the kernel's pruning rests on, tested directly: the float distance to a leaf's box and
  to every ancestor's box is <= the leaf's float D for every (point, leaf) pair, and the
  confinement is what makes it so (the unconfined point does leave its box);
* the inputs themselves: ties on the lattice, every region on frog, the pruning floor on frog;
* sqrt(d2) against a float64 restatement;
* the argument rules and the miss record.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import closest_point_cases as cp
import refit_cases as rc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

F32 = np.float32


@pytest.fixture(scope="module")
def host():
    """rt.closest_points_host on the scene's 4096 points per (scene, bound), computed once."""
    memo = {}

    def get(name, bound="none"):
        if (name, bound) not in memo:
            a = cp.arrays(name)
            memo[name, bound] = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], cp.points(name),
                                                       cp.max_d2(name, bound), evals=True)
        return memo[name, bound]

    return get


# ---- 1. the host build is the model -------------------------------------------------------------
@pytest.mark.parametrize("bound", cp.BOUNDS)
@pytest.mark.parametrize("name", cp.SCENES)
def test_host_build_equals_the_model(name, bound, host):
    m = cp.model(name, bound)
    got = host(name, bound)
    sub = tuple(g[m["idx"]] for g in got[:6])
    bad = cp.differing_points(sub, cp.as_tuple(m))
    assert bad.size == 0, (name, bound, bad[:4], [g[bad[:4]] for g in sub], [w[bad[:4]] for w in cp.as_tuple(m)])
    assert all(cp.same_bytes(g, w) for g, w in zip(sub, cp.as_tuple(m)))
    assert m["idx"].size == cp.MODEL_POINTS.get(name, cp.N_POINTS)
    # evals of the host build: the number of leaves, for every point
    assert (got[6] == cp.leaves(cp.arrays(name))["tri"].size).all()
    hit = m["tri"] >= 0
    print(f"{name} {bound}: {int(hit.sum())} of {hit.size} with a surface in bound, regions "
          f"{np.bincount(m['region'][hit], minlength=7).tolist()}, {int((m['ties'] >= 2).sum())} ties")


def test_bounds_are_around_the_distances():
    """max_d2 exactly the model's d2 keeps the winner, one ulp below loses it (nothing else is as
    near), 0 keeps only a point on a surface, inf is no bound."""
    for name in ("frog", "cornell", "small", cp.MOVED):
        free, m = cp.model(name, "none"), cp.model(name, "around")
        kind = np.arange(free["tri"].size) % 4
        assert (free["tri"] >= 0).all()
        for k in (0, 3):
            assert all(cp.same_bytes(x[kind == k], y[kind == k]) for x, y in zip(cp.as_tuple(m), cp.as_tuple(free)))
        assert (m["tri"][kind == 1] == -1).all() and (m["d2"][kind == 1] == -1.0).all()
        zero = kind == 2
        assert ((m["tri"][zero] >= 0) == (free["d2"][zero] == 0)).all()
        assert (m["region"][m["tri"] < 0] == -1).all() and not m["p"][m["tri"] < 0].any()


# ---- 2. the lemma -------------------------------------------------------------------------------
def ancestors_lb(a, q):
    """Per (point, node): the largest lb(q, box) over the node and all its ancestors, (n, 2P-1)."""
    nodes, aabbs = a["nodes"], a["aabbs"]
    lb = cp.box_lb(q[:, None, :], aabbs[None, :, 0:3], aabbs[None, :, 3:6])
    parent = np.full(nodes.shape[0], -1, np.int64)
    internal = np.flatnonzero(nodes[:, 3] == cp.NONE)
    for k in (1, 2):
        c = nodes[internal, k].astype(np.int64)
        parent[c[c != cp.NONE]] = internal[c != cp.NONE]
    depth = int(rc.heights(nodes)[0]) + 1
    up = lb.copy()
    anc = parent.copy()
    for _ in range(depth):  # fold in one more ancestor per round
        has = anc >= 0
        if not has.any():
            break
        up[:, has] = np.maximum(up[:, has], lb[:, anc[has]])
        anc[has] = parent[anc[has]]
    return up


@pytest.mark.parametrize("name", cp.SCENES)
def test_box_distance_is_a_lower_bound_of_the_confined_distance(name):
    a = cp.arrays(name)
    m = cp.model(name)
    sl = cp.class_slices(m["idx"].size)["c"]
    q = np.ascontiguousarray(cp.points(name)[m["idx"][sl]])
    Lf = cp.leaves(a)
    assert np.isfinite(a["aabbs"]).all()
    below = outside = pairs = 0
    loose_below = 0
    step = max(1, 1_000_000 // Lf["tri"].size)
    for s in range(0, q.shape[0], step):
        D, _, _, _, _ = cp.pairs(q[s:s + step], Lf)
        up = ancestors_lb(a, q[s:s + step])[:, Lf["node"]]
        below += int((up > D).sum())
        D0, _, _, _, p0 = cp.pairs(q[s:s + step], Lf, confined=False)
        outside += int(((p0 < Lf["lo"][None]) | (p0 > Lf["hi"][None])).any(axis=2).sum())
        loose_below += int((up > D0).sum())
        pairs += D.size
    print(f"{name}: {pairs} pairs, lb > D for {below}; unconfined: {outside} leave their box, lb > D for {loose_below}")
    assert below == 0
    _OUTSIDE[name] = outside


_OUTSIDE: dict = {}


def test_the_unconfined_point_does_leave_its_box():
    """(After the lemma's cases, whose counts it sums.)"""
    for name in cp.SCENES:
        if name not in _OUTSIDE:
            test_box_distance_is_a_lower_bound_of_the_confined_distance(name)
    assert sum(_OUTSIDE.values()) >= 100, _OUTSIDE
    assert _OUTSIDE["frog"] >= 100, _OUTSIDE


# ---- 3. the inputs ------------------------------------------------------------------------------
def test_lattice_points_hold_ties_and_the_lowest_index_wins():
    a = cp.arrays("small")
    m = cp.model("small")
    assert m["idx"].size == cp.N_POINTS
    assert (m["ties"] >= 2).sum() * 4 >= cp.N_POINTS, int((m["ties"] >= 2).sum())
    # the winner is the lowest index at the winning D: recount from the pairs
    Lf = cp.leaves(a)
    who = np.flatnonzero(m["ties"] >= 2)[:512]
    D = cp.pairs(np.ascontiguousarray(cp.points("small")[who]), Lf)[0]
    at = D == m["d2"][who][:, None]
    assert np.array_equal(at.sum(axis=1), m["ties"][who])
    assert np.array_equal(np.where(at, Lf["tri"][None, :], cp.INT_MAX).min(axis=1), m["tri"][who])
    assert (np.where(at, Lf["tri"][None, :], -1).max(axis=1) > m["tri"][who]).all()


def test_every_region_wins_on_frog():
    """The model's 1024 points and the rest of class c, which the model answers here."""
    m = cp.model("frog")
    c = cp.class_slices()["c"]
    rest = np.setdiff1d(np.arange(c.start, c.stop), m["idx"])
    more = cp.model_answers(cp.arrays("frog"), cp.points("frog")[rest])
    count = np.bincount(np.concatenate([m["region"], more["region"]]), minlength=7)
    print("frog: winners by region", dict(zip(cp.REGIONS, count.tolist())))
    assert count.size == 7 and (count >= 64).all(), count


def test_frog_floor_of_the_pruning_condition():
    """The least a correct walk evaluates, the leaves whose own box is no further than the answer,
    is far below P/20 on classes a and b: tests/test_gpu_closest_points.py may ask the kernel's mean
    evals to stay below P/20."""
    m = cp.model("frog")
    sl = cp.class_slices(m["idx"].size)
    floor = np.concatenate([m["floor"][sl["a"]], m["floor"][sl["b"]]])
    P = int(cp.arrays("frog")["P"])
    print(f"frog classes a, b: mean floor {floor.mean():.2f}, largest {floor.max()}, P/20 = {P / 20:.0f}")
    assert floor.min() >= 1 and floor.mean() < P / 20


# ---- 4. against float64 -------------------------------------------------------------------------
# The largest |sqrt(d2) - d64| / max(d64, 1e-3 extent) measured over every scene's sub-sample, d64
# the distance to the nearest triangle in float64 (no confinement): 1.5e-4, on cornell_moved, whose
# coordinates near 2^23 carry half a unit of rounding each; 1.5e-5 (sphere_single) to 9.4e-5 (the
# chains) on the scenes at their own size.  The largest gaps belong to points on or within 1e-6
# extents of a surface, where D is the square of a difference of rounded coordinates and the root
# magnifies its error; the bound is the measured value times 4, for other seeds.
GAP_MEASURED = 1.5e-4


def distance64(a, q):
    """Distance to the nearest leaf triangle in float64 (the same regions, no confinement)."""
    Lf = cp.leaves(a)
    L64 = {k: (v.astype(np.float64) if v.dtype == F32 else v) for k, v in Lf.items()}
    A, E1, E2 = (L64[k][None] for k in ("a", "e1", "e2"))
    Q = q.astype(np.float64)[:, None, :]
    dot = cp.dot
    with np.errstate(all="ignore"):
        ap = Q - A
        d1, d2 = dot(E1, ap), dot(E2, ap)
        bp = ap - E1
        d3, d4 = dot(E1, bp), dot(E2, bp)
        cq = ap - E2
        d5, d6 = dot(E1, cq), dot(E2, cq)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        den = 1.0 / (va + vb + vc)
        wbc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v = np.select(conds, [0.0, 1.0, d1 / (d1 - d3), 0.0, 0.0, 1.0 - wbc], vb * den)
        w = np.select(conds, [0.0, 0.0, 0.0, 1.0, d2 / (d2 - d6), wbc], vc * den)
        d = Q - (A + E1 * v[..., None] + E2 * w[..., None])
        return np.sqrt(np.nanmin(dot(d, d), axis=1))


@pytest.mark.parametrize("name", cp.SCENES)
def test_distance_against_float64(name):
    a = cp.arrays(name)
    m = cp.model(name)
    who = np.arange(0, m["idx"].size, 8)  # every eighth point of the model's: all four classes
    q = cp.points(name)[m["idx"][who]]
    d64 = distance64(a, q)
    extent = float((a["aabbs"][0, 3:6].astype(np.float64) - a["aabbs"][0, 0:3]).max())
    gap = np.abs(np.sqrt(m["d2"][who].astype(np.float64)) - d64) / np.maximum(d64, 1e-3 * extent)
    print(f"{name}: largest relative gap {gap.max():.3g} over {who.size} points")
    assert gap.max() <= 4 * GAP_MEASURED


# ---- 5. arguments and the miss record -----------------------------------------------------------
# A scene handle that is never read: every check below answers before the scene is touched.
_FAKE_SCENE = C.create_string_buffer(64)
_PTS = np.zeros((4, 3), F32)
_BUF = np.zeros(4 * 32 + 64, np.uint8)
_EV = np.zeros(4, np.uint32)
_ALIGNED = _BUF.ctypes.data + (-_BUF.ctypes.data) % 16
_S, _Q, _E = C.addressof(_FAKE_SCENE), _PTS.ctypes.data, _EV.ctypes.data
BIN = L.RT_FLAG_BINARY

# (scene, points, max_d2, n, flags, hits, evals) -> code
ARG_CASES = {
    "null scene": ((None, _Q, None, 4, 0, _ALIGNED, _E), -1),
    "null points": ((_S, None, None, 4, 0, _ALIGNED, _E), -1),
    "null hits": ((_S, _Q, None, 4, 0, None, _E), -1),
    "unknown flag": ((_S, _Q, None, 4, L.RT_FLAG_NO_CULL, _ALIGNED, _E), -1),
    "unknown flag beside BINARY": ((_S, _Q, None, 4, BIN | 8, _ALIGNED, _E), -1),
    "misaligned points": ((_S, _Q + 2, None, 4, 0, _ALIGNED, _E), -1),
    "misaligned max_d2": ((_S, _Q, _Q + 1, 4, 0, _ALIGNED, _E), -1),
    "misaligned evals": ((_S, _Q, None, 4, 0, _ALIGNED, _E + 2), -1),
    "n = 2^31": ((_S, _Q, None, 1 << 31, 0, _ALIGNED, None), -7),
}


@pytest.mark.parametrize("entry", ["rt_closest_points", "rt_closest_points_device"])
@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_argument_errors_need_no_device(entry, case):
    args, code = ARG_CASES[case]
    rc_ = getattr(L.lib(), entry)(*args, None)  # kernel_ms / hip_stream
    assert rc_ == code, (case, rc_, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _BUF.any() and not _EV.any()  # nothing was written


def test_no_points_no_launch_and_misaligned_records():
    lib = L.lib()
    for entry in (lib.rt_closest_points, lib.rt_closest_points_device):
        assert entry(_S, _Q, None, 0, 0, _ALIGNED, _E, None) == 0  # no points: no launch, no device
        assert entry(_S, _Q, None, 0, BIN, _ALIGNED, None, None) == 0
    for off in (4, 8, 12):
        assert lib.rt_closest_points_device(_S, _Q, None, 4, 0, _ALIGNED + off, _E, None) == -1
        assert b"aligned" in lib.rt_last_error()
    assert lib.rt_closest_points_variant(None) == rt.RT_RAYS_VARIANT_NONE
    assert rt.POINT_HIT_DTYPE.itemsize == 32
    assert [rt.POINT_HIT_DTYPE.fields[f][1] for f in ("tri", "d2", "p", "v", "w", "region")] == [0, 4, 8, 20, 24, 28]
    assert not _BUF.any() and not _EV.any()


def test_host_build_arguments():
    lib = L.lib()
    a = cp.arrays("sphere_single")
    nd, bx, tr = (a[k].ctypes.data for k in ("nodes", "aabbs", "tris"))
    P = int(a["P"])
    ok = (P, nd, bx, tr, _Q, None, 4)
    assert lib.rt_closest_points_host(*ok, _ALIGNED, _E) == 0
    assert lib.rt_closest_points_host(*ok, _ALIGNED + 4, None) == 0  # host records need no alignment
    assert lib.rt_closest_points_host(P, nd, bx, tr, None, None, 0, None, None) == 0
    for args in ((*ok, None, _E), (0, nd, bx, tr, _Q, None, 4, _ALIGNED, _E), (P, None, bx, tr, _Q, None, 4, _ALIGNED, _E),
                 (P, nd, None, tr, _Q, None, 4, _ALIGNED, _E), (P, nd, bx, None, _Q, None, 4, _ALIGNED, _E),
                 (P, nd, bx, tr, None, None, 4, _ALIGNED, _E)):
        assert lib.rt_closest_points_host(*args) == -1, args
        assert lib.rt_last_error()
    assert lib.rt_closest_points_host(P, nd, bx, tr, _Q, None, 1 << 31, _ALIGNED, _E) == -7
    with pytest.raises(ValueError):
        rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((2, 4), F32))
    with pytest.raises(ValueError):
        rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((2, 3), F32), max_d2=np.zeros(3, F32))
    with pytest.raises(ValueError):
        rt.closest_points_host(a["nodes"][:-1], a["aabbs"], a["tris"], np.zeros((2, 3), F32))
    tri, d2, p, v, w, region = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((0, 3), F32))
    assert tri.shape == d2.shape == v.shape == w.shape == region.shape == (0,) and p.shape == (0, 3)


MISS = np.zeros(1, rt.POINT_HIT_DTYPE)
MISS["tri"], MISS["d2"], MISS["region"] = -1, -1.0, -1


def test_the_miss_record():
    """A bound of 0 away from every surface, a NaN bound and a negative one: {-1, -1.0f, 0..., -1}
    over a pre-filled buffer, every byte."""
    a = cp.arrays("cornell")
    q = np.ascontiguousarray(cp.points("cornell")[cp.class_slices()["d"]][:96])  # far points
    n = q.shape[0]
    md = np.zeros(n, F32)
    md[1::3] = np.nan
    md[2::3] = -1.0
    buf = np.full(n * 32 + 32, 0xA5, np.uint8)
    rc_ = L.lib().rt_closest_points_host(int(a["P"]), a["nodes"].ctypes.data, a["aabbs"].ctypes.data, a["tris"].ctypes.data,
                                         q.ctypes.data, md.ctypes.data, n, buf.ctypes.data, None)
    assert rc_ == 0
    assert buf[:n * 32].tobytes() == MISS.tobytes() * n
    assert (buf[n * 32:] == 0xA5).all()
    # a leaf that names no triangle contributes nothing: a scene of one such leaf has no surface
    nodes = np.array([[cp.NONE, cp.NONE, cp.NONE, 7]], np.uint32)
    got = rt.closest_points_host(nodes, a["aabbs"][:1], a["tris"][:1], q, evals=True)
    assert (got[0] == -1).all() and (got[5] == -1).all() and (got[6] == 0).all()


def test_unspecified_inputs_terminate_and_fill_every_output():
    """NaN and infinite points: the call returns and writes every record (values unspecified
    beyond: a winner has a region, a point without one has the miss record)."""
    a = cp.arrays("cornell")
    q = cp.points("cornell")[:64].copy()
    q[0::4, 0] = np.nan
    q[1::4, 1] = np.inf
    q[2::4] = -np.inf
    tri, d2, p, v, w, region = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], q)
    won = tri >= 0
    assert ((region >= 0) == won).all() and (region <= 6).all()
    assert (d2[~won] == -1.0).all() and not p[~won].any()
    assert not won[0::4].any()  # a NaN coordinate: every D is NaN, and a NaN D never wins
