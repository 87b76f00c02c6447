"""Cases for the box tests (rt_box_test_host, rt_box_test_batch) with their float64 numpy
reference (TEST DATA GENERATOR, a helper module: no tests here).

ref_aabb restates the reference's intersectAABB (G/include/bvh.h:81-129) on its own: per axis
inv = 1.0 / double(dir), tNear / tFar = (double(bound) - double(orig)) * inv, the reference's
compares in the reference's order (so NaN and inf fall where they fall there), the parallel-axis
compare `fabsf(dir) < 1e-8f` in float32.

box_case(name) gives a named set {rays (n,6), boxes (n,6), tmm (n,2), ref (n,) bool}, shuffled so
that a wave of 64 consecutive items mixes classes, computed once and read-only.  tmin is the
traversals' 1e-4f everywhere (the wave forms of the box test have no other).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

F32 = np.float32
TMIN = F32(1e-4)  # query.h:233
FLT_MAX = F32(3.4028235e38)
EPS_PAR = F32(1e-8)  # bvh.h:84


# ---- the reference ----------------------------------------------------------------------
def ref_aabb(rays, boxes, tminmax):
    """intersectAABB (bvh.h:81-129) for n (ray, box, [tmin, tmax]) triples, as a bool array."""
    rays, boxes, tminmax = (np.asarray(a, F32) for a in (rays, boxes, tminmax))
    t0 = tminmax[:, 0].astype(np.float64)
    t1 = tminmax[:, 1].astype(np.float64)
    ok = np.ones(rays.shape[0], bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            o, d, mn, mx = rays[:, a], rays[:, 3 + a], boxes[:, a], boxes[:, 3 + a]
            par = np.abs(d) < EPS_PAR  # float32 compare
            inside = ~((o < mn) | (o > mx))
            inv = 1.0 / d.astype(np.float64)
            tn = (mn.astype(np.float64) - o.astype(np.float64)) * inv
            tf = (mx.astype(np.float64) - o.astype(np.float64)) * inv
            sw = tn > tf
            tn, tf = np.where(sw, tf, tn), np.where(sw, tn, tf)
            t0 = np.where(~par & (tn > t0), tn, t0)
            t1 = np.where(~par & (tf < t1), tf, t1)
            ok &= np.where(par, inside, ~(t0 > t1))
    return ok


def own_bmax(boxes):
    """Per item and axis the bound rt_box_test_host derives: max(|min|, |max|), inf on every axis
    of an inverted or NaN box."""
    boxes = np.asarray(boxes, F32)
    bm = np.fmax(np.abs(boxes[:, :3]), np.abs(boxes[:, 3:]))
    with np.errstate(invalid="ignore"):
        bad = ~(boxes[:, :3] <= boxes[:, 3:]).all(axis=1)
    bm[bad] = np.inf
    return np.ascontiguousarray(bm, F32)


def hex_triples(case, idx, limit=5):
    """The first `limit` items of idx as hex floats: ray, box, [tmin, tmax]."""
    out = []
    for i in np.asarray(idx)[:limit]:
        out.append("item %d: ray %s box %s tmm %s" % (
            i, [float(v).hex() for v in case["rays"][i]], [float(v).hex() for v in case["boxes"][i]],
            [float(v).hex() for v in case["tmm"][i]]))
    return "\n".join(out)


# ---- box test sets ----------------------------------------------------------------------
def _boxes(rng, n, scale):
    c = rng.normal(size=(n, 3)) * scale
    h = np.abs(rng.normal(size=(n, 3))) * scale * rng.choice([1.0, 1e-3, 0.0], size=(n, 1), p=[0.8, 0.15, 0.05])
    return np.concatenate([c - h, c + h], axis=1).astype(F32)


def _tmm(tmax):
    tmax = np.asarray(tmax, F32)
    return np.stack([np.full(tmax.shape[0], TMIN, F32), tmax], axis=1)


def _random(rng, n, scale):
    """test_box_filter.test_random_rays_and_boxes' construction (3 % parallel components)."""
    boxes = _boxes(rng, n, scale)
    o = (rng.normal(size=(n, 3)) * scale * 3).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    par = rng.random((n, 3)) < 0.03
    d[par] = rng.choice([0.0, 5e-9, -5e-9, 2e-8], size=par.sum())
    tmax = rng.choice([3.4028235e38, scale, scale * 10], size=n)
    return np.concatenate([o, d], axis=1), boxes, _tmm(tmax)


def _extreme(rng, n):
    """test_extreme_magnitudes' and test_near_parallel_and_overflow_scales' constructions."""
    parts = []
    for scale in (1e-30, 1e-20, 1e20, 1e35):
        boxes = _boxes(rng, n, scale)
        o = (rng.normal(size=(n, 3)) * scale * 2).astype(F32)
        d = rng.normal(size=(n, 3)).astype(F32)
        parts.append((np.concatenate([o, d], axis=1), boxes, _tmm(np.full(n, FLT_MAX))))
    for scale in (1.0, 1e30, 1e37, 1.5e38):
        with np.errstate(over="ignore", invalid="ignore"):
            boxes = _boxes(rng, n, scale)
            o = (rng.normal(size=(n, 3)) * scale * 1.5).astype(F32)
            boxes = np.where(np.isfinite(boxes), boxes, 0).astype(F32)
            o = np.where(np.isfinite(o), o, 0).astype(F32)
        d = rng.normal(size=(n, 3)).astype(F32)
        d[np.arange(n), rng.integers(0, 3, size=n)] = rng.choice([1.01e-8, -1.01e-8, 1e-7, 3e-6, -1e-5], size=n)
        parts.append((np.concatenate([o, d], axis=1), boxes, _tmm(rng.choice([3.4028235e38, 1.0, 1e30], size=n))))
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


def _aim(rng, n, scale, faces_only=False):
    """test_box_filter.test_adversarial_boundaries' construction at a scale, with edges: rays
    aimed at a box corner (all three coordinates on a bound), at a point of an edge (two) or of a
    face (one), a third each, and the reference's parameter t_aim of the aimed point."""
    boxes = _boxes(rng, n, scale)
    mn, mx = boxes[:, :3], boxes[:, 3:]
    target = np.where(rng.integers(0, 2, size=(n, 3)) == 0, mn, mx)
    free = np.ones(n, np.int64) * 2 if faces_only else rng.integers(0, 3, size=n)  # interior coordinates
    inner = rng.random((n, 3)).argsort(axis=1) < free[:, None]
    interior = mn + (mx - mn) * rng.random((n, 3))
    tgt = np.where(inner, interior, target).astype(F32)
    o = (tgt + rng.normal(size=(n, 3)) * 2 * scale).astype(F32)
    d = (tgt - o).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_aim = ((tgt - o).astype(np.float64) * (1.0 / d.astype(np.float64))).max(axis=1).astype(F32)
    t_aim = np.where(np.isfinite(t_aim), t_aim, scale).astype(F32)
    return np.concatenate([o, d], axis=1), boxes, t_aim


def _aimed(rng, n, scale):
    """tmax at the aimed parameter, its two float neighbours, and FLT_MAX."""
    rays, boxes, t_aim = _aim(rng, n, scale)
    tms = (t_aim, np.nextafter(t_aim, F32(np.inf)), np.nextafter(t_aim, F32(0)), np.full(n, FLT_MAX))
    return np.tile(rays, (4, 1)), np.tile(boxes, (4, 1)), _tmm(np.concatenate(tms))


BAND_K = (0.3, 1.0, 3.0, 10.0, 30.0)


def _bands(rng, n, scale=1.0):
    """Aimed at a face, tmax = t_aim (1 + k 1e-6), k in +-BAND_K: across the width of the float
    pre-classification's margin (kBoxRel = 1e-6), where it turns from sure to ambiguous to sure."""
    rays, boxes, t_aim = _aim(rng, n, scale, faces_only=True)
    ks = [s * k for k in BAND_K for s in (1.0, -1.0)]
    tms = [(t_aim.astype(np.float64) * (1.0 + k * 1e-6)).astype(F32) for k in ks]
    return np.tile(rays, (len(ks), 1)), np.tile(boxes, (len(ks), 1)), _tmm(np.concatenate(tms))


def _degenerate(rng, n):
    """Zero-extent boxes on 1, 2 and 3 axes with the origin on their plane, inverted boxes, NaN
    boxes, direction components of +-0, +-5e-9, +-1.01e-8 and the threshold 1e-8f with its
    neighbour below, tmax below tmin."""
    boxes = _boxes(rng, n, 1.0)
    o = (rng.normal(size=(n, 3)) * 2).astype(F32)
    kind = rng.integers(0, 5, size=n)  # 0 flat, 1 inverted, 2 NaN, 3-4 ordinary
    flat = (rng.random((n, 3)).argsort(axis=1) < rng.integers(1, 4, size=(n, 1))) & (kind == 0)[:, None]
    boxes[:, 3:][flat] = boxes[:, :3][flat]
    o[flat] = boxes[:, :3][flat]
    inv = np.flatnonzero(kind == 1)
    a = rng.integers(0, 3, size=inv.size)
    boxes[inv, a], boxes[inv, 3 + a] = boxes[inv, 3 + a].copy(), boxes[inv, a].copy()
    nan = np.flatnonzero(kind == 2)
    boxes[nan, rng.integers(0, 6, size=nan.size)] = np.nan
    d = rng.normal(size=(n, 3)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    small = rng.random((n, 3)) < 0.3
    e8 = float(EPS_PAR)
    below = float(np.nextafter(EPS_PAR, F32(0)))
    d[small] = rng.choice([0.0, -0.0, 5e-9, -5e-9, 1.01e-8, -1.01e-8, e8, -e8, below, -below], size=small.sum())
    tmax = rng.choice([3.4028235e38, 1.0, 10.0, 5e-5, 0.0, -1.0], size=n, p=[0.3, 0.25, 0.25, 0.1, 0.05, 0.05])
    return np.concatenate([o, d], axis=1), boxes, _tmm(tmax)


_BUILDERS = {
    "random_1e-3": lambda r: _random(r, 100000, 1e-3),
    "random_1": lambda r: _random(r, 100000, 1.0),
    "random_1e3": lambda r: _random(r, 100000, 1e3),
    "extreme": lambda r: _extreme(r, 12000),
    "aimed_1": lambda r: _aimed(r, 20000, 1.0),
    "aimed_2^-10": lambda r: _aimed(r, 20000, 2.0 ** -10),
    "aimed_2^12": lambda r: _aimed(r, 20000, 2.0 ** 12),
    "bands": lambda r: _bands(r, 12000),
    "degenerate": lambda r: _degenerate(r, 80000),
}
BOX_CASES = tuple(_BUILDERS)
RANDOM_CASES = ("random_1e-3", "random_1", "random_1e3")
# the sets that run again under scene-like bounds (bmax a multiple of the box's own)
BOUND_CASES = ("aimed_1", "aimed_2^-10", "aimed_2^12", "bands")
BOUND_FACTORS = (1.0, 16.0, 1024.0)


@lru_cache(maxsize=None)
def box_case(name: str) -> dict:
    rng = np.random.default_rng([11, BOX_CASES.index(name)])
    rays, boxes, tmm = _BUILDERS[name](rng)
    p = rng.permutation(rays.shape[0])
    case = {"rays": np.ascontiguousarray(rays[p], F32), "boxes": np.ascontiguousarray(boxes[p], F32),
            "tmm": np.ascontiguousarray(tmm[p], F32)}
    case["ref"] = ref_aabb(case["rays"], case["boxes"], case["tmm"])
    for v in case.values():
        v.setflags(write=False)
    return case


def no_parallel_axis(case):
    """Items whose ray has no parallel axis (the float pre-classification handles only those)."""
    return (np.abs(case["rays"][:, 3:]) >= EPS_PAR).all(axis=1)


@lru_cache(maxsize=None)
def mixed_case(n: int) -> dict:
    """n items dealt from every set, for the `active` patterns (n need not fill its last wave)."""
    rng = np.random.default_rng(12)
    cs = [box_case(k) for k in BOX_CASES]
    per = -(-n // len(cs))
    pick = [rng.choice(c["ref"].size, size=per, replace=False) for c in cs]
    p = rng.permutation(per * len(cs))[:n]
    case = {k: np.ascontiguousarray(np.concatenate([c[k][i] for c, i in zip(cs, pick)])[p]) for k in ("rays", "boxes", "tmm", "ref")}
    for v in case.values():
        v.setflags(write=False)
    return case


def active_patterns(n: int) -> dict:
    """Named `active` arrays over n items (None: all)."""
    rng = np.random.default_rng(13)
    wave = np.arange(n) // 64
    one = np.zeros(n, np.uint8)
    nw = int(wave[-1]) + 1
    lane = rng.integers(0, 64, size=nw)
    idx = np.minimum(np.arange(nw) * 64 + lane, n - 1)
    one[idx] = 1
    return {
        "all": None,
        "half": (rng.random(n) < 0.5).astype(np.uint8),
        "waves_off": (rng.random(nw) < 0.5)[wave].astype(np.uint8),
        "one_lane": one,
        "nonzero_bytes": rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n),
    }
