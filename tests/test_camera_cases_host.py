"""Degenerate, extreme and non-finite cameras (tests/camera_cases.py) on the CPU.

- The cases contain what they are for (check_expect: all hit, all hit with NaN t, 10-90 % fallback
  rays, some fallback ray; every class has a hit on cornell or sphere_single).
- The oracle at these cameras is the reference: tests/golden/cameras holds the reference's own
  Camera, render() and SearchBVH output for every constructor-parameter case on above_origin
  (gen_golden.py gen_cameras); orc_camera_init and orc_render_g must give those bits.  t is
  compared by bits; where the reference's is NaN the other side must be NaN, sign and payload
  free (camera_cases.same_bits), here and in every camera test.
- rt_camera_init gives orc_camera_init's basis; rt.camera_rays (host build) gives a numpy
  restatement of get_ray: the 1e-12 rule, the overflow to zero directions, the NaN spread.
- rt_debug_camera_class (what render_frame asks before it culls or picks a wave kernel): a camera
  it calls proven has no fallback, zero or NaN ray; one it does not send to the lane kernel has no
  zero or NaN ray; the suite's ordinary cameras are all proven.
- The tile test on the camera sets of tile_cases.py: nothing culled where a ray passes.
"""
from __future__ import annotations

import gzip
import hashlib
import json

import numpy as np
import pytest

import camera_cases as cc
import tile_cases as tc
from conftest import GOLDEN, hexv
from oracle import pyoracle as orc

import raytracinginonesemester_amd as rt

F32 = np.float32
BASIS = ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v")


@pytest.mark.parametrize("cls", cc.CLASSES)
def test_cases_contain_what_they_are_for(cls):
    names = cc.names_of(cls)
    assert len(names) >= 3 and {"above_origin"} < {cc.TABLE[n][1] for n in names}
    other_hits = 0
    for n in names:
        c = cc.case(n)
        cc.check_expect(c)
        assert c["W"] <= 96 and c["H"] <= 64 and c["spp"] <= 4
        if c["scene"] in ("cornell", "sphere_single"):
            other_hits += int((c["hits"] >= 0).sum())
    assert other_hits > 0, cls
    if cls in ("fallback", "nonfinite"):
        assert all(cc.TABLE[n][8] is not None for n in names if cc.TABLE[n][1] == "above_origin" and "inf_" not in n)


def test_threshold_and_fallback_lengths():
    """|D| itself, in float64 from the basis: below 1e-12 everywhere (fallback), on both sides of
    it (threshold)."""
    for n in cc.names_of("fallback") + cc.names_of("threshold"):
        c = cc.case(n)
        b = {k: v.astype(np.float64) for k, v in c["cam"].basis().items()}
        xs, ys = np.meshgrid(np.arange(c["W"]), np.arange(c["H"]))
        D = (b["pixel00_loc"] - b["center"])[None, None] + xs[..., None] * b["pixel_delta_u"] + ys[..., None] * b["pixel_delta_v"]
        ln = np.linalg.norm(D, axis=-1)
        if c["cls"] == "fallback":
            assert ln.max() < 1e-12, n
        else:
            assert ln.min() < 0.6e-12 and ln.max() > 2e-12, (n, ln.min(), ln.max())


@pytest.mark.parametrize("name", cc.CTOR_NAMES)
def test_camera_init_matches_oracle(name):
    spec = cc.TABLE[name][2][1]
    for (W, H) in ((cc.TABLE[name][3], cc.TABLE[name][4]), (16, 8), (1, 1)):
        for hw1 in (False, True):
            got = rt.Camera(*spec, W, H, hw1=hw1).basis()
            o = orc.camera(*spec, W, H, hw1=hw1)
            for k, ok in zip(BASIS, (o.center, o.pixel00, o.du, o.dv)):
                want = np.array([ok.x, ok.y, ok.z], F32)
                assert cc.same_bits(got[k], want), (name, W, H, hw1, k, got[k], want)


@pytest.mark.parametrize("name", cc.NAMES)
def test_camera_rays_host_matches_get_ray(name):
    c = cc.case(name)
    rays, _seeds = rt.camera_rays(c["cam"], spp=c["spp"], jitter=c["table"])
    rays = rays.reshape(c["H"], c["W"], c["spp"], 6)
    ctr = c["cam"].basis()["center"]
    assert cc.same_bits(rays[..., :3], np.broadcast_to(ctr, rays[..., :3].shape))
    assert cc.same_bits(rays[..., 3:], c["rays"]), (name, cc.count_diff(rays[..., 3:], c["rays"]))
    if name.startswith("pl_") or c["cls"] == "threshold":  # a second table: the samples move across the rule
        tab = rt.jittered_samples(4)
        r2, _ = rt.camera_rays(c["cam"], spp=4, jitter=tab)
        assert cc.same_bits(r2[:, 3:].reshape(c["H"], c["W"], 4, 3), cc.ref_rays(c["cam"].basis(), c["W"], c["H"], tab))


def test_ray_kinds_occur():
    """The restated get_ray produces each kind somewhere: fallback, zero and NaN directions, rays
    NaN on one axis only, and frames that mix fallback or zero directions with ordinary ones."""
    kinds = {"fallback": 0, "zero": 0, "nan3": 0, "nan1": 0, "mixed_fb": 0, "mixed_zero": 0}
    for n in cc.NAMES:
        r = cc.case(n)["rays"].reshape(-1, 3)
        fb, zero = cc.is_fallback(r), (r == 0).all(axis=1)
        nn = np.isnan(r).sum(axis=1)
        kinds["fallback"] += int(fb.any())
        kinds["zero"] += int(zero.any())
        kinds["nan3"] += int((nn == 3).any())
        kinds["nan1"] += int((nn == 1).any())
        kinds["mixed_fb"] += int(fb.any() and not fb.all())
        kinds["mixed_zero"] += int(zero.any() and not zero.all())
    print(kinds)
    assert all(v > 0 for v in kinds.values()), kinds


# ---- the reference's own frames ------------------------------------------------------------------
def _fixtures():
    d = GOLDEN / "cameras"
    meta = json.loads((d / "meta.json").read_text())
    W, H, spp = meta["width"], meta["height"], meta["spp"]
    n = len(meta["cases"])
    fb = np.frombuffer(gzip.open(d / "fb.f32.gz").read(), F32).reshape(n, H, W, 3)
    hi = np.frombuffer(gzip.open(d / "hits.i32.gz").read(), np.int32).reshape(n, H, W, spp)
    ht = np.frombuffer(gzip.open(d / "hitt.f32.gz").read(), F32).reshape(n, H, W, spp)
    return meta, fb, hi, ht


def test_fixtures_cover_the_constructor_cases():
    meta, fb, hi, ht = _fixtures()
    s = cc.scene("above_origin")
    for k, sha in meta["sha256"].items():
        assert hashlib.sha256(s[k].tobytes()).hexdigest() == sha, f"{k} differs from the fixtures' input"
    want = [(n, d) for n in cc.CTOR_NAMES if cc.TABLE[n][1] == "above_origin" for d in (1, 2)]
    assert [(c["name"], c["depth"]) for c in meta["cases"]] == want
    for c in meta["cases"]:
        spec = cc.TABLE[c["name"]][2][1]
        flat = [*spec[0], *spec[1], *spec[2], spec[3], spec[4]]
        assert [float(v).hex() for v in flat] == c["camera"], c["name"]
    # the reference's frames hold the classes' content too
    by = {(c["name"], c["depth"]): i for i, c in enumerate(meta["cases"])}
    assert (hi[by[("fb_negz", 1)]] >= 0).all() and (hi[by[("co_neg_focal", 1)]] >= 0).any()
    i = by[("nf_pos_x_nan", 1)]
    assert (hi[i] >= 0).all() and np.isnan(ht[i]).all() and np.isfinite(fb[i]).all()
    assert (hi[by[("ov_sensor_1e25", 1)]] < 0).all()


def test_oracle_matches_reference_at_these_cameras():
    meta, fb, hi, ht = _fixtures()
    W, H, spp = meta["width"], meta["height"], meta["spp"]
    s = cc.scene("above_origin")
    bad = []
    for i, c in enumerate(meta["cases"]):
        spec = cc.TABLE[c["name"]][2][1]
        ocam = orc.camera(*spec, W, H)
        for k, v in zip(BASIS, (ocam.center, ocam.pixel00, ocam.du, ocam.dv)):
            if not cc.same_bits(np.array([v.x, v.y, v.z], F32), hexv(c[k])):
                bad.append((c["name"], c["depth"], k))
        rgb, h, t = orc.render_g(s["P"], ocam, s["nodes"], s["aabbs"], s["tris"], s["objids"], s["mats"], s["lights"],
                                 spp=spp, max_depth=c["depth"], aov=True)
        # (the reference's driver writes t = -1 for a miss, as the oracle does)
        for what, a, b in (("hits", h, hi[i]), ("t", t, ht[i]), ("frame", rgb, fb[i])):
            if not cc.same_bits(a, b):
                bad.append((c["name"], c["depth"], what, cc.count_diff(a, b)))
    assert not bad, bad


# ---- the camera's class ----------------------------------------------------------------------------
def _ray_facts(dirs):
    r = np.asarray(dirs).reshape(-1, 3)
    return bool(cc.is_fallback(r).any()), bool((r == 0).all(axis=1).any()), bool(np.isnan(r).any())


def test_class_of_every_case():
    for n in cc.NAMES:
        c = cc.case(n)
        k = c["cam"].frame_class()
        fb, zero, nan = _ray_facts(c["rays"])
        # directions that only equal (0, 0, 1) (a camera looking along +z with dv = 0) are no fallback
        b = {q: v.astype(np.float64) for q, v in c["cam"].basis().items()}
        if c["cls"] in ("fallback", "threshold", "plane"):
            assert k == 1, (n, k)
        if c["cls"] == "nonfinite":
            assert k == 2, (n, k)
        if zero or nan:
            assert k == 2, (n, k, zero, nan)
        if k == 0:
            D0 = b["pixel00_loc"] - b["center"]
            assert np.isfinite(D0).all() and not nan and not zero
    assert cc.case("ov_pos_1e20")["cam"].frame_class() >= 1


def test_class_is_sound_on_random_extreme_cameras():
    """Random bases over the whole float range, with pads from 1 to 40: class 0 has no fallback,
    zero or NaN ray under a table that reaches the pad's corners; class <= 1 no zero or NaN ray."""
    rng = np.random.default_rng(77)
    seen = {0: 0, 1: 0, 2: 0}
    near = 0
    for i in range(3000):
        W, H = int(rng.integers(1, 48)), int(rng.integers(1, 32))
        kind = i % 6
        e = rng.choice([-44.0, -38.0, -20.0, -13.0, -12.0, -11.0, -6.0, 0.0, 6.0, 17.0, 18.0, 19.0, 20.0, 30.0, 38.0])
        mag = 10.0 ** (e + rng.uniform(-1, 1))
        ctr = rng.normal(size=3) * rng.choice([0.0, 1e-20, 1.0, 4096.0, 1e20, 3e38])
        fwd = rng.normal(size=3)
        fwd /= np.linalg.norm(fwd)
        u = np.cross(fwd, rng.normal(size=3))
        u /= np.linalg.norm(u)
        v = np.cross(fwd, u)
        spread = mag * rng.choice([1e-3, 0.03, 1.0, 30.0])
        du, dv = u * spread, v * spread
        if kind == 1:
            du = rng.normal(size=3) * spread  # any parallelogram
        elif kind == 2:
            dv = du * rng.uniform(-2, 2)  # collapsed
        elif kind == 3:
            du = du * 0
        p00 = ctr + fwd * mag - du * (W - 1) / 2 * rng.choice([0, 1]) - dv * (H - 1) / 2 * rng.choice([0, 1])
        with np.errstate(all="ignore"):
            cam = rt.Camera.from_basis(*(np.asarray(x, np.float64).astype(F32) for x in (ctr, p00, du, dv)), W, H)
        pad = float(rng.choice([1.0, 1.0, 2.5, 40.0]))
        tab = np.array([(pad, pad), (-pad, pad), (pad, -pad), (-pad, -pad), (0, 0), (0.3, -0.7)], F32)
        k = cam.frame_class(pad)
        seen[k] += 1
        fb, zero, nan = _ray_facts(cc.ref_rays(cam.basis(), W, H, tab))
        # (a direction that merely equals (0, 0, 1) is told from the fallback by the length)
        if fb:
            b = {q: x.astype(np.float64) for q, x in cam.basis().items()}
            fb = bool(np.linalg.norm(b["pixel00_loc"] - b["center"]) < 1e-9 or spread * 50 > mag)
        if k == 0:
            assert not (fb or zero or nan), (i, cam.basis(), W, H, pad, fb, zero, nan)
        if k <= 1:
            assert not (zero or nan), (i, cam.basis(), W, H, pad, zero, nan)
        near += int(k == 0 and (mag < 1e-10 or mag > 1e17))
    print(seen, "proven within 100x of an end:", near)
    assert min(seen.values()) > 100 and near > 0


def test_ordinary_cameras_are_proven():
    """Every camera of the tile sets (four kinds x scales 2^-10 .. 2^12 x a shift by 4096 x three
    focal lengths x images up to 3840 x 2160) and the shipped scenes' own keep the cull."""
    from conftest import host_scene

    n = 0
    for name in tc.TILE_CASES:
        for g in tc.tile_case(name):
            assert g["cam"].frame_class() == 0, (name, g["cam"].basis())
            n += 1
    for s in ("frog.json", "cornell.json", "sphere_single.json", "heightfield_c5.json", "sphere.json"):
        hs = host_scene(s)
        for wh in ((None, None), (96, 64), (3840, 2160)):
            assert hs.camera(*wh).frame_class() == 0 and hs.camera(*wh).frame_class(1.5) == 0, (s, wh)
    for sc in cc.ORDINARY:
        assert cc.ordinary_camera(sc, 40, 24).frame_class() == 0
    print(n, "tile-set cameras")


def test_class_refuses_null():
    import ctypes as C

    from raytracinginonesemester_amd import _lib

    out = C.c_int32(7)
    cam = cc.ordinary_camera("above_origin", 8, 8)
    assert _lib.lib().rt_debug_camera_class(None, 1.0, C.byref(out)) == -1
    assert _lib.lib().rt_debug_camera_class(C.byref(cam.c), 1.0, None) == -1
    assert cam.frame_class(float("nan")) == 0 and cam.frame_class(float("inf")) == 2


# ---- the tile test behind the class ------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.CAMERA_TILE_CASES)
def test_tile_test_is_sound_at_these_cameras(name):
    """Before camera_class (render_frame's check of the camera) the tile test
    culled, although a ray of the tile passes the box: on "fallback" 739 of 1760 items (fb_negz,
    fb_posx, fb_diag, fb_negz_d2, fb_negz_37x23_1spp, fb_raw_subnormal: every ray is (0, 0, 1) and
    hits what is over the origin), on "threshold" 64 of 660 (th_negz, th_negz_c1e-20), on
    "nonfinite" 370 of 4840 (the cases with a NaN word on one axis: the other two axes culled).  On
    "overflow" it culled 186 items, none of them with a passing ray."""
    got = tc.check_camera_set(tc.host_fn, name)
    assert not got.any()  # none of these cameras is proven: nothing is culled at all


# ---- the wave family at what such frames bring to a wave -------------------------------------------
@pytest.mark.parametrize("name", __import__("family_cases").DEGENERATE_CASES)
def test_family_test_is_sound_with_degenerate_lanes(name):
    import family_cases as fc

    fc.check_degenerate(fc.host_fn, name)


# ---- HW1: the binned path's rectangles at these cameras ----------------------------------------------
def test_hw1_leg_has_every_class_and_some_hits():
    assert {cc.TABLE[n][0] for n in cc.HW1_NAMES} == set(cc.HW1_CLASSES) and len(cc.HW1_NAMES) >= 16
    hits = {cls: 0 for cls in cc.HW1_CLASSES}
    nan_frames = 0
    for n in cc.HW1_NAMES:
        rgb, hi, _t = cc.hw1_case(n)["ref"]
        hits[cc.TABLE[n][0]] += int((hi >= 0).sum())
        nan_frames += int(np.isnan(rgb).any())
    print(hits, "frames with NaN pixels:", nan_frames)
    assert hits["fallback"] > 0 and hits["collapsed"] > 0


@pytest.mark.parametrize("name", cc.HW1_NAMES)
def test_hw1_accepted_samples_lie_in_the_tile_range(name):
    """hw1_rect (rt_hw1_rects_host) is conservative at these cameras too: every sample at which the
    oracle accepts a triangle lies in the tiles the triangle is listed in."""
    import hw1_cases as hc
    from test_hw1_rects_host import missed

    c = cc.hw1_case(name)
    acc = hc.accepted(c)
    rects, tiles = rt.hw1_rects_host(c["positions"], c["indices"], c["camera"])
    assert (rects[:, 0] >= -2).all() and (rects[:, 1] >= -2).all() and (rects[:, 2] <= cc.HW1_W + 1).all() and \
        (rects[:, 3] <= cc.HW1_H + 1).all()
    listed = tiles[:, 1] >= tiles[:, 0]
    assert (tiles[listed, 0] >= 0).all() and (tiles[listed, 2] >= 0).all()
    assert (tiles[:, 1] < -(-cc.HW1_W // hc.TW)).all() and (tiles[:, 3] < -(-cc.HW1_H // hc.TH)).all()
    bad = missed(c, acc, tiles)
    print(f"{name}: {int(acc.sum())} accepted samples, listed tiles {hc.range_area(tiles)}")
    assert not bad, f"{name}: accepted samples outside their triangle's tile range: {bad[:4]}"
