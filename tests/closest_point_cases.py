"""Scenes, query points, bounds and a model of the closest-point query (rt_closest_points, DESIGN.md
§4.28): a helper module, no tests here.

The model calls none of the code under test.  It restates the definition of include/rt_mi355x.h in
numpy float32 (IEEE, no contraction) over all (point, leaf) pairs, in chunks of points: the seven
regions in their order, p = (a + e1*v) + e2*w, the confinement to the leaf's box, D = len2(q - p),
and the winner by (D, triangle index) among the leaves with D <= the bound.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import multi_hit_cases as mh

F32 = np.float32
NONE = 0xFFFFFFFF
INT_MAX = np.iinfo(np.int32).max
N_POINTS = 4096
SEED = 20
MOVED = "cornell_moved"  # cornell times 2^12, plus 4096 on every axis; the tree rebuilt
SCENES = mh.SCENES + (MOVED,)
BOUNDS = ("none", "around")
CLASSES = "abcd"  # uniform | on triangles | at vertices and edges | far
REGIONS = ("A", "B", "C", "AB", "AC", "BC", "face")
MODEL_POINTS = {"frog": 1024}  # the model's share of the batch (a prefix of every class); all elsewhere


@lru_cache(maxsize=None)
def arrays(name: str) -> dict:
    """multi_hit_cases.arrays' keys: P, nodes (2P-1, 4) uint32, aabbs (2P-1, 6), tris (P, 18), ..."""
    if name != MOVED:
        return mh.arrays(name)
    import raytracinginonesemester_amd as rt

    a = dict(mh.arrays("cornell"))
    tris = a["tris"].copy()
    tris[:, :9] = tris[:, :9] * F32(4096.0) + F32(4096.0)
    nodes, aabbs = rt.build_bvh_triangles(tris)
    a["tris"] = tris
    a["nodes"] = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)
    a["aabbs"] = np.ascontiguousarray(aabbs, F32).reshape(-1, 6)
    lights = a["lights"].copy()
    lights["position"] = lights["position"] * F32(4096.0) + F32(4096.0)
    a["lights"] = lights
    for x in a.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a


def device_scene(name: str, device: int = 0, refittable: bool = False):
    import raytracinginonesemester_amd as rt

    a = arrays(name)
    return rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], device,
                          refittable=refittable)


def leaves(a: dict) -> dict:
    """The scene's surfaces: nodes j in [P-1, 2P-1) naming a triangle i < P; node, tri (int32), a,
    e1, e2 (L, 3) as the library stores them, lo, hi (L, 3) of aabbs[j]."""
    P = int(a["P"])
    j = np.arange(P - 1, 2 * P - 1)
    obj = a["nodes"][j, 3].astype(np.int64)
    j, obj = j[obj < P], obj[obj < P]
    T = a["tris"][obj]
    v0 = np.ascontiguousarray(T[:, 0:3], F32)
    return {"node": j, "tri": obj.astype(np.int32), "a": v0, "e1": T[:, 3:6] - v0, "e2": T[:, 6:9] - v0,
            "lo": np.ascontiguousarray(a["aabbs"][j, 0:3]), "hi": np.ascontiguousarray(a["aabbs"][j, 3:6])}


def class_slices(n: int = N_POINTS) -> dict:
    q = n // 4
    return {c: slice(i * q, (i + 1) * q) for i, c in enumerate(CLASSES)}


# ---- the query points --------------------------------------------------------------------------
def make_points(a: dict, n: int = N_POINTS, seed: int = SEED) -> np.ndarray:
    """n points in four equal classes (class_slices), float32:
    a  uniform in the root box inflated 1.5 times about its centre;
    b  on a random triangle, moved along its normal by {0, 1e-6, 1e-3, 0.1} x the scene's extent;
    c  aimed at vertices and edges: a, a + e1 * (1 - k 2^-24) and a + e2 * (1 - k 2^-24) for k in
       0..3, random points of the three edges; as they are, moved in the plane by a few 2^-20 of the
       edges, or moved off the plane by 2^-20 or 1e-3 of the extent;
    d  far: 30 extents from the centre in a random direction."""
    rng = np.random.default_rng(seed)
    L = leaves(a)
    lo, hi = a["aabbs"][0, 0:3].astype(np.float64), a["aabbs"][0, 3:6].astype(np.float64)
    centre, extent = (lo + hi) / 2, float((hi - lo).max())
    q = n // 4
    pa = centre + (rng.random((q, 3)) - 0.5) * 1.5 * (hi - lo)
    # b: a random point of a random leaf's triangle
    t = rng.integers(0, L["tri"].size, q)
    A, E1, E2 = (L[k][t].astype(np.float64) for k in ("a", "e1", "e2"))
    nrm = np.cross(E1, E2)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1), 1e-300)[:, None]
    u, v = rng.random(q), rng.random(q)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    off = np.array([0.0, 1e-6, 1e-3, 0.1])[np.arange(q) % 4] * extent * rng.choice([-1.0, 1.0], q)
    pb = A + E1 * u[:, None] + E2 * v[:, None] + nrm * off[:, None]
    # c: float32 throughout, so that the targets are the float32 points the kernel computes
    t = rng.integers(0, L["tri"].size, q)
    A, E1, E2 = (L[k][t] for k in ("a", "e1", "e2"))
    i = np.arange(q)
    kind, k = i % 6, (i // 6) % 4
    near1 = (F32(1) - k.astype(F32) * F32(2.0 ** -24)).astype(F32)
    s = rng.random(q).astype(F32)
    f1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0, near1, 0, s, 0], s).astype(F32)
    f2 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [0, 0, near1, 0, s], F32(1) - s).astype(F32)
    pc = ((A + E1 * f1[:, None]) + E2 * f2[:, None]).astype(F32)
    move = (i // 24) % 3
    r1, r2 = ((rng.integers(-4, 5, q)).astype(F32) * F32(2.0 ** -20) for _ in range(2))
    inplane = (E1 * r1[:, None] + E2 * r2[:, None]).astype(F32)
    n32 = np.cross(E1.astype(np.float64), E2.astype(np.float64))
    n32 /= np.maximum(np.linalg.norm(n32, axis=1), 1e-300)[:, None]
    lift = np.where(i % 2 == 0, 2.0 ** -20, 1e-3) * extent * rng.choice([-1.0, 1.0], q)
    offplane = (n32 * lift[:, None]).astype(F32)
    pc = np.where((move == 1)[:, None], pc + inplane, np.where((move == 2)[:, None], pc + offplane, pc)).astype(F32)
    d = rng.normal(size=(q, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pd = centre + d * 30.0 * extent
    out = np.ascontiguousarray(np.vstack([pa.astype(F32), pb.astype(F32), pc, pd.astype(F32)]), F32)
    assert out.shape == (n, 3) and np.isfinite(out).all()
    return out


@lru_cache(maxsize=None)
def points(name: str) -> np.ndarray:
    p = make_points(arrays(name))
    p.setflags(write=False)
    return p


def model_subset(name: str) -> np.ndarray:
    """Indices of the points the model answers: all, or the first quarter of every class."""
    m = MODEL_POINTS.get(name, N_POINTS)
    per = m // 4
    return np.concatenate([np.arange(s.start, s.start + per) for s in class_slices().values()])


# ---- the model ---------------------------------------------------------------------------------
def dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def confine(p, lo, hi):
    return np.where(p < lo, lo, np.where(p > hi, hi, p))


def box_lb(q, lo, hi):
    """lb(q, B) for q (n, 1, 3) against boxes (m, 3): (n, m) float32."""
    d = q - confine(q, lo, hi)
    return dot(d, d)


def pairs(q, L, confined: bool = True):
    """The definition for every (point, leaf) pair: D, v, w (n, L) float32, region (n, L) int8 and
    p (n, L, 3); confined=False leaves p as computed (the lemma's counter-example)."""
    assert q.dtype == F32
    Q = q[:, None, :]
    a, e1, e2 = L["a"][None], L["e1"][None], L["e2"][None]
    zero, one = F32(0), F32(1)
    with np.errstate(all="ignore"):
        ap = Q - a
        d1, d2 = dot(e1, ap), dot(e2, ap)
        bp = ap - e1
        d3, d4 = dot(e1, bp), dot(e2, bp)
        cp = ap - e2
        d5, d6 = dot(e1, cp), dot(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        region = np.select(conds, [0, 1, 3, 2, 4, 5], 6).astype(np.int8)
        den = one / ((va + vb) + vc)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        v = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                      [zero, one, d1 / (d1 - d3), zero, zero, one - w_bc], vb * den).astype(F32)
        w = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                      [zero, zero, zero, one, d2 / (d2 - d6), w_bc], vc * den).astype(F32)
        p = (a + e1 * v[..., None]) + e2 * w[..., None]
        if confined:
            p = confine(p, L["lo"][None], L["hi"][None])
        d = Q - p
        D = dot(d, d)
    assert D.dtype == F32 and p.dtype == F32
    return D, v, w, region, p


def model_answers(a: dict, q: np.ndarray, max_d2=None) -> dict:
    """The model's answers for points q (n, 3): tri, d2, p, v, w, region as the query returns them,
    and per point ties (leaves at the winning D, within the bound) and floor (leaves whose own box
    has lb <= the final best D: the least a correct walk evaluates)."""
    q = np.ascontiguousarray(q, F32)
    n = q.shape[0]
    L = leaves(a)
    nl = L["tri"].size
    bound = np.full(n, np.inf, F32) if max_d2 is None else np.ascontiguousarray(max_d2, F32)
    out = {"tri": np.full(n, -1, np.int32), "d2": np.full(n, -1.0, F32), "p": np.zeros((n, 3), F32), "v": np.zeros(n, F32),
           "w": np.zeros(n, F32), "region": np.full(n, -1, np.int32), "ties": np.zeros(n, np.int64),
           "floor": np.zeros(n, np.int64)}
    step = max(1, 1_500_000 // max(nl, 1))
    for s in range(0, n, step):
        e = min(n, s + step)
        D, v, w, region, p = pairs(q[s:e], L)
        with np.errstate(all="ignore"):
            ok = D <= bound[s:e, None]
            best = np.where(ok, D, np.inf).min(axis=1) if nl else np.full(e - s, np.inf, F32)
            at = ok & (D == best[:, None])
            tri = np.where(at, L["tri"][None, :], INT_MAX).min(axis=1) if nl else np.full(e - s, INT_MAX)
            col = (at & (L["tri"][None, :] == tri[:, None])).argmax(axis=1) if nl else np.zeros(e - s, np.int64)
            won = at.any(axis=1) if nl else np.zeros(e - s, bool)
            final = np.where(won, best, bound[s:e])
            lb = box_lb(q[s:e, None, :], L["lo"][None], L["hi"][None])
            out["floor"][s:e] = (lb <= final[:, None]).sum(axis=1)
        r = np.arange(e - s)
        out["ties"][s:e] = at.sum(axis=1)
        for k, x in (("tri", tri), ("d2", best), ("v", v[r, col]), ("w", w[r, col]), ("region", region[r, col])):
            out[k][s:e] = np.where(won, x, out[k][s:e])
        out["p"][s:e] = np.where(won[:, None], p[r, col], out["p"][s:e])
    return out


def bounds_around(m: dict) -> np.ndarray:
    """A max_d2 per point around the unbounded model's d2, by index mod 4: exactly d2, one ulp below
    it, 0, and inf.  (The unbounded model has a winner wherever the scene has a leaf.)"""
    d2 = np.where(m["tri"] >= 0, m["d2"], F32(1)).astype(F32)
    kind = np.arange(d2.size) % 4
    return np.select([kind == 0, kind == 1, kind == 2], [d2, np.nextafter(d2, F32(-np.inf)), np.zeros_like(d2)],
                     np.full(d2.size, np.inf, F32)).astype(F32)


@lru_cache(maxsize=None)
def model(name: str, bound: str = "none") -> dict:
    """model_answers on the scene's model_subset (shared, read-only), with idx, the subset, and
    max_d2: per point of the subset, or None for "none"."""
    idx = model_subset(name)
    q = points(name)[idx]
    if bound == "none":
        m = model_answers(arrays(name), q)
        m["max_d2"] = None
    else:
        md = bounds_around(model(name, "none"))
        m = model_answers(arrays(name), q, md)
        m["max_d2"] = md
    m["idx"] = idx
    for x in m.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return m


@lru_cache(maxsize=None)
def max_d2(name: str, bound: str):
    """The bounds of the whole 4096-point batch: None, or around the model's d2 where the model
    answered and around a scene-sized guess (the root box's squared diagonal / 16) elsewhere."""
    if bound == "none":
        return None
    m = model(name, "none")
    a = arrays(name)
    diag = (a["aabbs"][0, 3:6].astype(np.float64) - a["aabbs"][0, 0:3]) ** 2
    d2 = np.full(N_POINTS, F32(diag.sum() / 16), F32)
    d2[m["idx"]] = np.where(m["tri"] >= 0, m["d2"], F32(1))
    out = bounds_around({"tri": np.zeros(N_POINTS, np.int32), "d2": d2})
    # (a class's quarter starts at a multiple of 4: the subset's kinds are the batch's)
    assert np.array_equal(out[m["idx"]].view(np.uint32), model(name, "around")["max_d2"].view(np.uint32))
    out.setflags(write=False)
    return out


FIELDS = ("tri", "d2", "p", "v", "w", "region")


def as_tuple(m: dict):
    return tuple(m[k] for k in FIELDS)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing_points(got, want):
    """Indices of the points where any of (tri, d2, p, v, w, region) differs in any byte."""
    bad = np.zeros(np.asarray(got[0]).shape[0], bool)
    for g, w in zip(got, want):
        g4 = np.ascontiguousarray(g).view(np.uint32).reshape(bad.size, -1)
        w4 = np.ascontiguousarray(w).view(np.uint32).reshape(bad.size, -1)
        bad |= (g4 != w4).any(axis=1)
    return np.flatnonzero(bad)
