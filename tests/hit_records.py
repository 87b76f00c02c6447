"""Hit records for the rt_trace_hits tests, a helper module: no tests here (TEST DATA GENERATOR).

``ref_records`` restates the record intersectTriangle returns for a triangle the ray is known to
hit (G/include/query.h:80-128) in float32 numpy, for the triangle indices the oracle's SearchBVH
gives (ray_batches.oracle_trace): no fused multiply-add, ``dot`` as ``(x*x + y*y) + z*z``,
``normalize = v / sqrtf(dot)`` (vec3.h:51-53).  Whenever it is used it asserts that its ``t`` is
the oracle's ``t`` in every bit.  tests/test_hit_records_host.py pins it against the reference's
own records (tests/golden/hit_records/, recorded by tests/native/ref_hit_records.cpp).

The scenes are ray_batches.SCENES and one tests/shade_fuzz.py case whose per-triangle object ids
leave the material table (FUZZ_CASE), each with ray_batches' 4096-ray batch.
"""
from __future__ import annotations

import gzip
import hashlib
import json
from functools import lru_cache
from pathlib import Path

import numpy as np

import ray_batches as rb

F = np.float32
GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "hit_records"
FUZZ_CASE = "s_l1_d1"  # sphere.json's arrays, a 7-entry table, a random id per triangle (a tenth outside it)
# make_rays seed of the fuzz case's batch: the first of 1234 (ray_batches.SEED), 1, 2, ... that
# gives at least 16 hits with material == -1 (tests/test_hit_records_host.py asserts it)
FUZZ_RAY_SEED = rb.SEED
NAMES = rb.SCENES + (FUZZ_CASE,)
PER_CLASS = 64  # the fixture's rays: the first 64 of each of make_rays' four classes
FIXTURE_FILES = {"rays.f32": F, "hit.u8": np.uint8, "tri.i32": np.int32, "t.f32": F, "p.f32": F, "normal.f32": F,
                 "front.u8": np.uint8}

HIT_DTYPE = np.dtype([("tri", "<i4"), ("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3),
                      ("geom_normal", "<f4", 3), ("front_face", "<i4"), ("object_id", "<i4"), ("material", "<i4")])


@lru_cache(maxsize=None)
def scene(name: str) -> dict:
    """ray_batches.scene_arrays' keys for a ray_batches scene or the fuzz case (mats None: no table)."""
    if name != FUZZ_CASE:
        return rb.scene_arrays(name)
    import shade_fuzz as sf
    import shade_rays_cases as sc

    c = sf.case(name)
    a = sc.scene_of_case(c)
    a["light"] = np.array(c["lights"]["position"][0], np.float64)
    return a


def make_batch(name: str, seed: int) -> dict:
    a = scene(name)
    rays = rb.make_rays(a["aabbs"], a["tris"], a["light"], rb.N_RAYS, seed)
    idx, t = rb.oracle_trace(a["P"], a["nodes"], a["aabbs"], a["tris"], rays)
    return {"rays": rays, "idx": idx, "t": t}


@lru_cache(maxsize=None)
def batch(name: str) -> dict:
    """rays (4096, 6), and the oracle's idx and t (shared, read-only)."""
    if name != FUZZ_CASE:
        return rb.batch(name)
    b = make_batch(name, FUZZ_RAY_SEED)
    for v in b.values():
        v.setflags(write=False)
    return b


def device_scene(name: str, device: int = 0):
    import raytracinginonesemester_amd as rt

    a = scene(name)
    return rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], device)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def _normalize(v):
    return v / np.sqrt(_dot(v, v))[:, None]


def records_and_classes(scene_, rays, idx, t=None):
    """ref_records' array and, per ray, the branches its record took: ``hit``, ``back`` (front_face
    false), ``degenerate`` (length_squared(shadingN) < 1e-12: the geometric normal is taken) and
    ``flipped`` (the normalised shading normal was negated into geomN's hemisphere)."""
    rays = np.ascontiguousarray(rays, F)
    idx = np.ascontiguousarray(idx, np.int32)
    n = rays.shape[0]
    if t is None:
        oi, t = rb.oracle_trace(scene_["P"], scene_["nodes"], scene_["aabbs"], scene_["tris"], rays)
        assert np.array_equal(oi, idx), "idx is not the oracle's"
    t = np.ascontiguousarray(t, F)
    rec = np.zeros(n, HIT_DTYPE)
    rec["tri"] = -1
    rec["t"] = F(-1.0)
    hit = idx >= 0
    cls = {k: np.zeros(n, bool) for k in ("back", "degenerate", "flipped")}
    cls["hit"] = hit
    if not hit.any():
        return rec, cls
    k = np.flatnonzero(hit)
    tri = idx[k]
    T = np.ascontiguousarray(scene_["tris"], F)[tri]
    o, d = rays[k, :3], rays[k, 3:]
    v0, v1, v2, n0, n1, n2 = (T[:, 3 * j:3 * j + 3] for j in range(6))
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        pvec = _cross(d, e2)
        det = _dot(e1, pvec)
        inv = F(1.0) / det
        tvec = o - v0
        u = _dot(tvec, pvec) * inv
        qvec = _cross(tvec, e1)
        v = _dot(d, qvec) * inv
        tt = _dot(e2, qvec) * inv
        p = o + d * tt[:, None]
        g = _normalize(_cross(e1, e2))
        front = _dot(d, g) < F(0.0)
        g = np.where(front[:, None], g, -g)
        w = F(1.0) - u - v
        s = (n0 * w[:, None] + n1 * u[:, None]) + n2 * v[:, None]
        deg = _dot(s, s) < F(1e-12)
        sn = _normalize(s)
        flip = ~deg & (_dot(sn, g) < F(0.0))
        sn = np.where(flip[:, None], -sn, sn)
        sn = np.where(deg[:, None], g, sn)
    for a in (e1, pvec, det, u, v, tt, p, g, s, sn):
        assert a.dtype == F
    assert np.array_equal(tt.view(np.uint32), t[k].view(np.uint32)), "the restated t is not the oracle's t"
    rec["tri"][k] = tri
    rec["t"][k], rec["u"][k], rec["v"][k] = tt, u, v
    rec["p"][k], rec["normal"][k], rec["geom_normal"][k] = p, sn, g
    rec["front_face"][k] = front
    triobj, mats = scene_.get("triobj"), scene_.get("mats")
    oid = np.full(k.size, -1, np.int32) if triobj is None else np.ascontiguousarray(triobj, np.int32)[tri]
    nm = 0 if mats is None else len(mats)
    rec["object_id"][k] = oid
    rec["material"][k] = np.where((oid >= 0) & (oid < nm), oid, -1) if triobj is not None and mats is not None else -1
    cls["back"][k] = ~front
    cls["degenerate"][k] = deg
    cls["flipped"][k] = flip
    return rec, cls


def ref_records(scene_, rays, idx, t=None):
    """The (n,) HIT_DTYPE records rt_trace_hits must return for ``rays`` whose closest-hit triangles
    are ``idx`` (the oracle's; -1: a miss record).  ``t``: the oracle's t if the caller has it,
    else orc_search_bvh runs here; the restated t must equal it in every bit."""
    return records_and_classes(scene_, rays, idx, t)[0]


@lru_cache(maxsize=None)
def reference(name: str):
    """(records, classes) of the scene's batch (computed once, shared, read-only)."""
    b = batch(name)
    rec, cls = records_and_classes(scene(name), b["rays"], b["idx"], b["t"])
    rec.setflags(write=False)
    return rec, cls


# ---- the fixture recorded from the reference --------------------------------------------------
def fixture_pick():
    """Indices into a 4096-ray batch: the first PER_CLASS rays of each class."""
    return np.concatenate([np.arange(s.start, s.start + PER_CLASS) for s in rb.class_slices().values()])


def fixture(name: str) -> dict:
    """The reference's records of the scene's 256 fixture rays, sha256-checked against meta.json."""
    meta = json.loads((GOLDEN_DIR / "meta.json").read_text())
    out = {}
    for f, dt in FIXTURE_FILES.items():
        raw = gzip.open(GOLDEN_DIR / name / (f + ".gz")).read()
        assert hashlib.sha256(raw).hexdigest() == meta["sha256"][name][f], (name, f)
        out[f.split(".")[0]] = np.frombuffer(raw, dt)
    n = 4 * PER_CLASS
    out["rays"] = out["rays"].reshape(n, 6)
    out["p"], out["normal"] = out["p"].reshape(n, 3), out["normal"].reshape(n, 3)
    return out


# ---- camera-ray shapes (rt_camera_rays_host / _device) ------------------------------------------
# name -> camera (a tests/shade_fuzz.py case's, or "c3_small": frog.json's at 192x108), spp, row0,
# rows (None: to the last row).  48 and 32 are no multiples of the 64 lanes of a wave.
CAMERA_SHAPES = {
    "c3_small 192x108x16": ("c3_small", 16, 0, None),
    "chain300 48x32x4": ("c_l3_d1", 4, 0, None),  # chain_bvh.CAMERA: the chain fixtures' camera and shape
    "rows 5..11": ("c_l3_d1", 4, 5, 7),
    "spp 1": ("c3_small", 1, 0, None),
    "spp 5, last row": ("c_l3_d2", 5, 23, 1),
}


def shape_camera(case: str):
    import raytracinginonesemester_amd as rt
    import shade_fuzz as sf
    from conftest import host_scene

    if case in sf.CASES:
        c = sf.case(case)
        pos, look, up, f, s = c["camera"]
        return rt.Camera(pos, look, up, f, s, c["W"], c["H"])
    return host_scene("frog.json").camera(192, 108)
