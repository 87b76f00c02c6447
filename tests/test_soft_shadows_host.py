"""Soft shadows from spherical area lights on the CPU (rt_light_samples_host, rt_path_step_vis_host,
the loader's light shapes), against tests/soft_shadow_cases.py's numpy model and
the oracle: no device.

* rt_light_samples_host is the model byte for byte: rays, bounds, offsets and the rng afterwards;
* rt_path_step_vis_host with 1 - occluded is rt_path_step_host byte for byte, and between 0 and 1
  it interpolates ShadeDirect's value;
* the all-point staged soft path is the oracle's TraceRayIterative;
* the sample points lie on the light's disk, across the axis to the shaded point;
* the penumbra scene has a penumbra (a condition of the tests that use it);
* the loader reads, defaults and rejects the two keys; the argument rules of the new entry points.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

import path_cases as pc
import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc
import soft_shadow_cases as ss
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

F, U = np.float32, np.uint32


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("soft_shadows")


def sweep_kinds(name):
    return ss.SHAPE_SETS + (tuple(f"s{s}" for s in ss.SWEEP) if name in ("penumbra", "s_l1_d4m") else ())


@pytest.mark.parametrize("name", ss.SCENES)
def test_light_samples_host_is_the_model(name, scene_dir):
    e = ss.entries(name, scene_dir)
    nl = e["lights"].size
    for kind in sweep_kinds(name):
        mv = ss.model(name, kind)
        rng = np.array(e["seeds"], U)
        rays, bounds, off = rt.light_samples_host(e["rec"], e["lights"], ss.shapes(kind, nl), rng)
        assert np.array_equal(off, mv["offsets"]), (name, kind)
        assert rays.tobytes() == mv["rays"].tobytes() and bounds.tobytes() == mv["bounds"].tobytes(), (name, kind)
        assert np.array_equal(rng, mv["rng"]), (name, kind)
        if kind != "point":
            assert (rng != e["seeds"]).any()
        else:
            assert np.array_equal(rng, e["seeds"])  # a point light draws nothing


def test_light_samples_host_with_ids_none_rows_and_misses(scene_dir):
    e = ss.entries("s_l3_d1", scene_dir)
    m, nl = e["rec"].shape[0], e["lights"].size
    shp = ss.shapes("mixed", nl)
    perm = np.random.default_rng(5).permutation(m).astype(U)
    ids = perm.copy()
    ids[::7] = L.RT_PATH_NONE
    seeds = np.array(e["seeds"], U)
    want = ss.model_visibility(e["scene"], e["rec"], e["lights"], shp, seeds, ids)
    rng = seeds.copy()
    rays, bounds, off = rt.light_samples_host(e["rec"], e["lights"], shp, rng, ids)
    assert np.array_equal(off, want["offsets"]) and rays.tobytes() == want["rays"].tobytes()
    assert bounds.tobytes() == want["bounds"].tobytes() and np.array_equal(rng, want["rng"])
    per_entry = np.diff(off.astype(np.int64)).reshape(m, nl).sum(axis=1)
    silent = (ids == L.RT_PATH_NONE) | (e["rec"]["tri"] < 0)
    assert silent.any() and (e["rec"]["tri"] < 0).any() and not per_entry[silent].any() and per_entry[~silent].any()
    untouched = np.setdiff1d(np.arange(m), ids[~silent])
    assert np.array_equal(rng[untouched], seeds[untouched])
    assert (want["vis"][silent] == 0).all()


@pytest.mark.parametrize("name", pc.FIXTURE_CASES)
def test_path_step_vis_host_with_whole_visibilities_is_path_step_host(name, scene_dir):
    e = ss.entries(name, scene_dir)
    a, rec, lights = e["scene"], e["rec"], e["lights"]
    m = rec.shape[0]
    occ = pc.shadow_answers(a, rec, lights)
    assert occ.any() and not occ.all()
    table = None if a["mats"] is None else np.ascontiguousarray(a["mats"], F).reshape(-1, 13)
    for last in (False, True):
        out = []
        for fn, arg in ((rt.path_step_host, occ), (rt.path_step_vis_host, (1 - occ).astype(F))):
            rad, thr, rng = np.zeros((m, 3), F), np.ones((m, 3), F), np.array(e["seeds"], U)
            nxt, alive, direct = fn(e["rays"], rec, rad, thr, rng, arg, lights, table, miss_color=sc.MISS, last=last)
            out.append((nxt, alive, direct, rad, thr, rng))
        for x, y in zip(*out):
            assert x.tobytes() == y.tobytes(), (name, last)


def test_path_step_vis_host_scales_a_light_by_its_visibility(scene_dir):
    """One light: direct(v) = direct(0) + v * (direct(1) - direct(0)) up to float32 rounding.  The
    light's term t enters as scale(t, NdotL * v) against scale(t, NdotL) * v here: two roundings of
    relative 2^-24 each on the term, one more on the sum, so 4 * 2^-24 of the largest magnitude
    bounds the difference."""
    e = ss.entries("s_l1_d4m", scene_dir)
    a, rec, lights = e["scene"], e["rec"], e["lights"]
    m = rec.shape[0]
    table = None if a["mats"] is None else np.ascontiguousarray(a["mats"], F).reshape(-1, 13)

    def direct(v):
        rad, thr, rng = np.zeros((m, 3), F), np.ones((m, 3), F), np.array(e["seeds"], U)
        return rt.path_step_vis_host(e["rays"], rec, rad, thr, rng, np.full((m, 1), v, F), lights, table, last=True)[2].astype(np.float64)

    d0, d1 = direct(0.0), direct(1.0)
    assert (d1 != d0).any()
    for v in (0.25, 0.5, 47.0 / 64.0):
        dv = direct(v)
        bound = 4 * 2.0 ** -24 * np.maximum(np.abs(d1), np.abs(d0)) + 1e-30
        assert (np.abs(dv - (d0 + np.float64(F(v)) * (d1 - d0))) <= bound).all(), v
    assert np.array_equal(direct(-1.0), d0) and np.array_equal(direct(float("nan")), d0)  # !(v > 0): skipped


@pytest.mark.parametrize("depth", sc.DEPTHS)
def test_the_all_point_staged_soft_path_is_the_reference(depth):
    name = "cornell"
    a, b = rb.scene_arrays(name), sc.caller_batch(name)
    shp = ss.shapes("point", len(a["lights"]))
    got = ss.cpu_staged_soft_path(a, b["rays"], b["seeds"], depth, True, sc.MISS, shp)
    want = sc.reference(name, depth, True)[0]
    assert np.array_equal(got.view(U), want.view(U))


def test_soft_shapes_change_the_staged_path(scene_dir):
    e = ss.entries("penumbra", scene_dir)
    n = 256
    rays, seeds = e["rays"][:n], e["seeds"][:n]
    hard = ss.cpu_staged_soft_path(e["scene"], rays, seeds, 2, True, sc.MISS, ss.shapes("point", 1))
    soft = ss.cpu_staged_soft_path(e["scene"], rays, seeds, 2, True, sc.MISS, ss.shapes("s8", 1))
    assert (hard != soft).any()


@pytest.mark.parametrize("name", ("penumbra", "s_l8_d4", "cornell"))
def test_sample_points_lie_on_the_disk(name, scene_dir):
    """In float64: every sample point within radius * (1 + 1e-5) of the light, its offset
    perpendicular to the disk's axis within 1e-5 of the radius."""
    e = ss.entries(name, scene_dir)
    for kind in ("soft", "mixed"):
        shp = ss.shapes(kind, e["lights"].size)
        mv = ss.model(name, kind)
        nl = e["lights"].size
        counts = np.diff(mv["offsets"].astype(np.int64))
        light_of = np.repeat(np.tile(np.arange(nl), e["rec"].shape[0]), counts)
        soft = shp["radius"][light_of] > 0
        assert soft.any()
        pts, W = mv["points"][soft].astype(np.float64), mv["W"][soft].astype(np.float64)
        radius = shp["radius"][light_of][soft].astype(np.float64)
        off = pts - e["lights"]["position"][light_of][soft].astype(np.float64)
        assert (np.linalg.norm(off, axis=1) <= radius * (1 + 1e-5)).all()
        assert (np.abs((off * W).sum(axis=1)) <= 1e-5 * radius).all()


def test_the_penumbra_scene_has_a_penumbra(scene_dir):
    """At S = 64 at least 5 % of the entries facing the light are partly lit (sphere_area.json's
    own radius, 0.15)."""
    e = ss.entries("penumbra", scene_dir)
    v = ss.model("penumbra", "s64")["vis"][:, 0]
    rec = e["rec"]
    hit = rec["tri"] >= 0
    Lv = pc._unit((e["lights"]["position"][0][None, :] - rec["p"][hit]).astype(F))
    facing = pc._dot(pc._unit(np.ascontiguousarray(rec["normal"][hit], F)), Lv) > 0
    part = (v[hit][facing] > 0) & (v[hit][facing] < 1)
    assert facing.sum() >= 256 and part.mean() >= 0.05, (int(facing.sum()), float(part.mean()))
    assert float(ss.shapes("s64", 1)["radius"][0]) == F(ss.PENUMBRA_RADIUS)


# ---- the loader ------------------------------------------------------------------------------------
def _load(scene_dir, light_key, light, name):
    doc = json.loads(ss.penumbra_json(scene_dir).read_text())
    del doc["light"]
    doc[light_key] = light
    path = scene_dir / name
    path.write_text(json.dumps(doc))
    return rt.HostScene.load_json(path, ss.REPO)


def test_the_loader_reads_and_defaults_the_light_shapes(scene_dir):
    hs = ss.penumbra(scene_dir)["hs"]
    assert hs.light_shapes.dtype == rt.LIGHT_SHAPE_DTYPE and hs.light_shapes.tolist() == [(F(0.15), 8)]
    base = {"position": [0, 0, 1], "color": [1, 1, 1], "intensity": 2}
    many = _load(scene_dir, "lights", [dict(base, radius=0.5), dict(base, shadow_samples=16.9), base,
                                       dict(base, radius=-2, shadow_samples=-3)], "many.json")
    assert many.light_shapes.tolist() == [(0.5, 1), (0.0, 16), (0.0, 1), (-2.0, -3)]
    assert many.lights["intensity"].tolist() == [2, 2, 2, 2]
    for scene in ("frog.json", "sphere.json"):
        shp = host_scene(scene).light_shapes
        assert shp.shape == host_scene(scene).lights.shape and (shp["radius"] == 0).all() and (shp["shadow_samples"] == 1).all()
    objs = rt.HostScene.load_objs([ss.REPO / "assets" / "meshes" / "sphere.obj"])  # the fallback light
    assert objs.light_shapes.tolist() == [(0.0, 1)]


@pytest.mark.parametrize("key, value", [("radius", "0.15"), ("radius", [0.15]), ("radius", None), ("shadow_samples", "8"),
                                        ("shadow_samples", True), ("shadow_samples", {})])
def test_the_loader_rejects_light_shapes_of_another_type(scene_dir, key, value):
    light = dict(ss.PENUMBRA_LIGHT)
    light[key] = value
    for light_key, arg in (("light", light), ("lights", [light])):
        with pytest.raises(rt.RTError) as err:
            _load(scene_dir, light_key, arg, "bad.json")
        assert err.value.code == -3 and key in str(err.value)


# ---- argument rules (no device is touched: every check runs before any HIP call) ------------------
def test_argument_rules_of_the_device_entry_points():
    lib = L.lib()
    fake = C.c_void_p(16 * 4096)  # never dereferenced: the checks fail first
    vis_dev = lib.rt_light_visibility_device
    assert vis_dev(None, 1, fake, None, fake, fake, 0, 0, fake, None) == -1  # null scene
    assert lib.rt_light_visibility_variant(None) == L.RT_RAYS_VARIANT_NONE
    assert lib.rt_scene_num_lights(None) == 0
    o = L.PathOpts(1, L.Vec3(0, 0, 0), 0)
    st = L.PathStateT(fake, fake, fake)
    step = lib.rt_path_step_vis_device
    assert step(None, 1, fake, fake, None, None, fake, C.byref(o), C.byref(st), fake, fake, None, None) == -1
    assert "null scene" in lib.rt_last_error().decode()


def test_argument_rules_of_the_host_builds(scene_dir):
    e = ss.entries("s_l3_d1", scene_dir)
    k = np.flatnonzero(e["rec"]["tri"] >= 0)[:8]
    rec, lights = np.ascontiguousarray(e["rec"][k]), e["lights"]
    shp = ss.shapes("soft", lights.size)
    rng = np.array(e["seeds"][k], U)
    for s, code in ((256, None), (257, -7), (1 << 20, -7)):
        big = shp.copy()
        big["shadow_samples"][1] = s
        if code is None:
            rt.light_samples_host(rec, lights, big, rng.copy())
        else:
            before = rng.copy()
            with pytest.raises(rt.RTError) as err:
                rt.light_samples_host(rec, lights, big, rng)
            assert err.value.code == code and np.array_equal(rng, before)
    point_big = ss.shapes("point", lights.size)
    point_big["shadow_samples"][0] = 257  # the rule does not read the radius
    with pytest.raises(rt.RTError):
        rt.light_samples_host(rec, lights, point_big, rng)
    with pytest.raises(ValueError):
        rt.light_samples_host(rec, lights, shp[:1], rng)
    with pytest.raises(ValueError):
        rt.light_samples_host(rec, lights, shp, rng[:4])
    lib = L.lib()
    off = np.zeros(8 * lights.size + 1, np.uint64)
    rays, bounds = np.zeros((4, 6), F), np.zeros(4, F)
    args = (8, L.ptr(np.ascontiguousarray(rec)), None, L.ptr(lights), L.ptr(shp), lights.size, L.ptr(rng))
    before = rng.copy()
    assert lib.rt_light_samples_host(*args, 4, L.ptr(rays), L.ptr(bounds), L.ptr(off)) == -1  # too little room
    assert np.array_equal(rng, before) and not rays.any() and int(off[-1]) > 4
    assert lib.rt_light_samples_host(*args, 4, L.ptr(rays), None, L.ptr(off)) == -1
    assert lib.rt_light_samples_host(*args, 0, None, None, None) == -1
    m = 8
    rad, thr = np.zeros((m, 3), F), np.ones((m, 3), F)
    with pytest.raises(ValueError):
        rt.path_step_vis_host(e["rays"][k], rec, rad, thr, rng, np.ones((m, lights.size + 1), F), lights)
    o = L.PathOpts(1, L.Vec3(0, 0, 0), 0)
    st = L.PathStateT(L.ptr(rad), L.ptr(thr), L.ptr(rng))
    r, h = np.ascontiguousarray(e["rays"][k]), np.ascontiguousarray(rec)
    nxt, alive = np.zeros((m, 6), F), np.zeros(m, np.uint8)
    call = lambda vis, opt=o, n=nxt: lib.rt_path_step_vis_host(m, L.ptr(r), L.ptr(h), None, None, None, 0, L.ptr(lights),  # noqa: E731
                                                              lights.size, vis, C.byref(opt), C.byref(st), L.ptr(n) if n is not None else None,
                                                              L.ptr(alive), None)
    assert call(None) == -1  # lights without visibilities
    assert call(L.ptr(np.ones((m, lights.size), F)), n=None) == -1  # no next rays without RT_PATH_LAST
    assert call(L.ptr(np.ones((m, lights.size), F)), opt=L.PathOpts(1, L.Vec3(0, 0, 0), 64)) == -1  # unknown flag
    assert call(L.ptr(np.ones((m, lights.size), F))) == 0


def test_the_shape_sets_cover_the_issue(scene_dir):
    seen_s, seen_r = set(), set()
    for name in ss.SCENES:
        nl = ss.entries(name, scene_dir)["lights"].size
        for kind in sweep_kinds(name):
            shp = ss.shapes(kind, nl)
            soft = shp["radius"] > 0
            seen_s |= set(shp["shadow_samples"][soft].tolist())
            seen_r |= {repr(float(r)) for r in shp["radius"]}
    assert set(ss.SWEEP) <= seen_s and {repr(float(F(r))) for r in ss.RADII} <= seen_r
    assert sorted(ss.entries(n, scene_dir)["lights"].size for n in pc.FIXTURE_CASES) == [1, 3, 8]
    a = rb.scene_arrays("chain600")
    assert sc.rule_variant(a)[0] == L.RT_RAYS_VARIANT_DEEP
    e = ss.entries("cornell", scene_dir)  # radius 2.0 encloses some hit points
    d = np.linalg.norm(e["rec"]["p"][e["rec"]["tri"] >= 0] - e["lights"]["position"][0][None, :], axis=1)
    assert (d < 2.0).any()
