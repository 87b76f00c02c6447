"""Frames over degenerate, extreme and non-finite cameras (tests/camera_cases.py) through every
frame path: hits, t and the float frame must be the oracle's bit for bit (t by bits; NaN where
the oracle's is NaN), the P6 bytes those of the oracle's frame, for every case through

- rt_render with the default kernel and the cull on, RT_FLAG_NO_CULL, RT_FLAG_BINARY,
  RT_KERNEL_LANE, RT_KERNEL_WAVE and RT_KERNEL_WAVE_PIXELS, a 3 spp frame (a pixel per lane), the
  forced cut (cull_coverage 1.0) and two band shards;
- rt_render_device_pair with an ordinary camera as the partner, in both orders (the partner's
  frame must be its frame alone), and one frame through rt_renderer;
- camera_rays(device=0) and camera_rays_pixels against the host build, and render_rays (camera
  rays -> shade_rays -> film) against the same oracle frame;
- the device build of the tile test and of the wave-family test on the camera sets.

After every degenerate frame an ordinary camera's frame is unchanged, and ds.faults() stays 0.
What the frame does for each class is render_frame's camera_class: only a
camera whose |D| range is proven is culled or cut, a camera with a non-finite word or a length
that may overflow takes the lane kernel.  The HW1 leg runs the constructor cameras through the
binned and brute-force paths against orc.render_hw1.

Before that check, on an MI355X, the frames of fb_negz, fb_posx, fb_diag, fb_negz_d2,
fb_negz_37x23_1spp, fb_raw_subnormal (6 of the 8 fallback cases) and of th_negz, th_negz_c1e-20 (2
of the 3 threshold cases) differed from the oracle through every path that culls (the default
frame, RT_FLAG_BINARY, each RT_KERNEL_*, the forced cut): whole tiles of the miss colour where
every ray hits, 2560 to 3840 of 3840 samples.  With RT_FLAG_NO_CULL they were exact, and so were
the plane and collapsed cases everywhere.  The overflow and non-finite cases were not run on the
unchecked build (their rays are zero or NaN in the wave kernels); with the check every case passes.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import camera_cases as cc
from conftest import oracle_camera
from oracle import pyoracle as orc

import raytracinginonesemester_amd as rt

pytestmark = pytest.mark.gpu

NO_CULL, BINARY = rt._lib.RT_FLAG_NO_CULL, rt._lib.RT_FLAG_BINARY
SCENES = ("above_origin", "deep_chain", "cornell", "sphere_single")
# name -> ds.render keywords
RENDER_PATHS = {
    "default": {},
    "no_cull": {"flags": NO_CULL},
    "binary": {"flags": BINARY},
    "lane": {"kernel": rt.RT_KERNEL_LANE},
    "wave": {"kernel": rt.RT_KERNEL_WAVE},
    "wave_pixels": {"kernel": rt._lib.RT_KERNEL_WAVE_PIXELS},
}


@lru_cache(maxsize=None)
def _ds(scene: str):
    return cc.device_scene(scene)


@lru_cache(maxsize=None)
def _oracle(scene: str, spec, W: int, H: int, spp: int, table_key, depth: int):
    """The oracle's (frame, hits, t) for a camera that is not a case's own (3 spp frames, the
    ordinary partner)."""
    s = cc.scene(scene)
    cam = cc.make_camera(spec, W, H)
    tab = rt.jittered_samples(spp) if table_key is None else np.frombuffer(table_key, np.float32).reshape(-1, 2)
    out = orc.render_g(s["P"], oracle_camera(cam), s["nodes"], s["aabbs"], s["tris"], s["objids"], s["mats"], s["lights"],
                       spp=spp, max_depth=depth, miss=s["miss"], jitter_tab=tab, aov=True)
    for a in out:
        a.setflags(write=False)
    return out


def _key(c):
    return None if c["jitter"] is None else c["jitter"].tobytes()


def _ordinary(c):
    """The ordinary camera of the case's scene at the case's frame shape, and its oracle frame."""
    spec = ("ctor", cc.ORDINARY[c["scene"]])
    return cc.make_camera(spec, c["W"], c["H"]), _oracle(c["scene"], spec, c["W"], c["H"], c["spp"], _key(c), c["depth"])


def _diff(got, want):
    """Names of the outputs that differ, with the counts."""
    names = ("frame", "hits", "t")
    return [(n, cc.count_diff(g, w)) for n, g, w in zip(names, got, want) if not cc.same_bits(g, w)]


def _p6_of(frame) -> bytes:
    return orc.ppm_quantize(frame).astype(np.uint8).tobytes()


def _kw(c):
    return dict(spp=c["spp"], max_depth=c["depth"], miss_color=c["miss"], jitter=c["jitter"])


@pytest.mark.parametrize("path", list(RENDER_PATHS) + ["forced_cut"])
def test_every_case_renders_the_oracles_frame(path, tune):
    if path == "forced_cut":
        tune(cull_coverage=1.0)
    kw = RENDER_PATHS.get(path, {})
    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        ds = _ds(c["scene"])
        d = _diff(ds.render(c["cam"], aov=True, **_kw(c), **kw), (c["frame"], c["hits"], c["t"]))
        if d:
            bad.append((name, d))
        # an ordinary frame after it is unchanged
        ocam, want = _ordinary(c)
        d = _diff(ds.render(ocam, aov=True, **_kw(c), **kw), want)
        if d:
            bad.append((name, "the ordinary frame after it", d))
    print(f"{path}: {len(bad)} of {2 * len(cc.NAMES)} frames differ: {[b[0] for b in bad]}")
    assert not bad, bad[:8]
    for s in SCENES:
        assert _ds(s).faults() == 0, s


def test_three_samples_a_pixel_per_lane():
    """3 spp is no power of two: the kernels that give a lane a pixel and loop over its samples."""
    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        if c["spp"] != 4:
            continue
        tab = None if c["jitter"] is None else np.ascontiguousarray(c["jitter"][:3])
        want = _oracle(c["scene"], c["spec"], c["W"], c["H"], 3, None if tab is None else tab.tobytes(), c["depth"])
        for kw in ({}, {"flags": NO_CULL}):
            got = _ds(c["scene"]).render(c["cam"], spp=3, max_depth=c["depth"], miss_color=c["miss"], jitter=tab, aov=True, **kw)
            d = _diff(got, want)
            if d:
                bad.append((name, kw, d))
    print(f"3 spp: {len(bad)} frames differ: {[b[:2] for b in bad]}")
    assert not bad, bad[:8]
    for s in SCENES:
        assert _ds(s).faults() == 0, s


def test_two_band_shards():
    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        H = c["H"]
        out = [np.zeros_like(a) for a in (c["frame"], c["hits"], c["t"])]
        for b in range(2):
            rows = [y for y in range(H) if (y // 8) % 2 == b]
            if not rows:  # an 8-row frame has one band
                continue
            strip = _ds(c["scene"]).render(c["cam"], aov=True, band_rows=8, band_index=b, band_count=2, **_kw(c))
            assert strip[0].shape[0] == len(rows)
            for o, s in zip(out, strip):
                o[rows] = s
        d = _diff(out, (c["frame"], c["hits"], c["t"]))
        if d:
            bad.append((name, d))
    print(f"band shards: {len(bad)} frames differ: {[b[0] for b in bad]}")
    assert not bad, bad[:8]


def test_pairs_with_an_ordinary_partner():
    """rt_render_device_pair, the degenerate camera first and second: both frames and their P6
    bytes; the partner's frame is its frame alone.  With and without RT_FLAG_NO_CULL (without the
    cull the two frames' parameters differ in nothing but the camera)."""
    import torch

    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        W, H = c["W"], c["H"]
        ds = _ds(c["scene"])
        ocam, owant = _ordinary(c)
        want = {"case": (c["frame"], _p6_of(c["frame"])), "partner": (owant[0], _p6_of(owant[0]))}
        cams = {"case": c["cam"], "partner": ocam}
        for flags in (0, NO_CULL):
            o, _keep = rt.DeviceScene.make_opts(spp=c["spp"], max_depth=c["depth"], miss_color=c["miss"], jitter=c["jitter"],
                                                flags=flags)
            for order in (("case", "partner"), ("partner", "case")):
                rgb = [torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda") for _ in order]
                p6 = [torch.full((H, W, 3), 99, dtype=torch.uint8, device="cuda") for _ in order]
                ds.render_device_pair(cams[order[0]], cams[order[1]], o, rgb[0].data_ptr(), p6[0].data_ptr(),
                                      rgb[1].data_ptr(), p6[1].data_ptr())
                torch.cuda.synchronize()
                for k, who in enumerate(order):
                    if not cc.same_bits(rgb[k].cpu().numpy(), want[who][0]):
                        bad.append((name, flags, order, who, "frame", cc.count_diff(rgb[k].cpu().numpy(), want[who][0])))
                    if p6[k].cpu().numpy().tobytes() != want[who][1]:
                        bad.append((name, flags, order, who, "p6"))
    print(f"pairs: {len(bad)} outputs differ: {sorted({b[0] for b in bad})}")
    assert not bad, bad[:8]
    for s in SCENES:
        assert _ds(s).faults() == 0, s


@pytest.mark.parametrize("scene", SCENES)
def test_one_frame_through_the_renderer(scene):
    s = cc.scene(scene)
    bad = []
    r = rt.Renderer(s["P"], s["nodes"], s["aabbs"], s["tris"], s["objids"], s["mats"], s["lights"], devices=(0,),
                    deliver=rt.RT_DELIVER_F32)
    try:
        for name in cc.names_of(scene_name=scene):
            c = cc.case(name)
            W, H = c["W"], c["H"]
            o, _keep = rt.DeviceScene.make_opts(spp=c["spp"], max_depth=c["depth"], miss_color=c["miss"], jitter=c["jitter"])
            ocam, owant = _ordinary(c)
            for who, cam, want in (("case", c["cam"], c["frame"]), ("ordinary after it", ocam, owant[0])):
                addr, n = r.wait(r.submit(cam, o))
                assert n == W * H * 12
                got = np.ctypeslib.as_array((C.c_float * (n // 4)).from_address(addr)).reshape(H, W, 3).copy()
                if not cc.same_bits(got, want):
                    bad.append((name, who, cc.count_diff(got, want)))
    finally:
        r.close()
    print(f"renderer {scene}: {len(bad)} frames differ: {bad[:10]}")
    assert not bad, bad[:8]


def test_camera_rays_on_the_device():
    """camera_rays(device=0) and camera_rays_pixels (host and device) give the host build's rays,
    which test_camera_cases_host holds to get_ray."""
    import torch

    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        W, H, spp = c["W"], c["H"], c["spp"]
        table = np.array(c["table"])  # (writable: torch wraps it)
        host, hseeds = rt.camera_rays(c["cam"], spp=spp, jitter=table)
        dev, dseeds = rt.camera_rays(c["cam"], spp=spp, jitter=table, device=0)
        if not cc.same_bits(dev.cpu().numpy(), host) or not np.array_equal(dseeds.cpu().numpy().view(np.uint32), hseeds):
            bad.append((name, "camera_rays", cc.count_diff(dev.cpu().numpy(), host)))
        # every other pixel, backwards, from the second sample on
        px = np.arange(W * H - 1, -1, -2).astype(np.uint32)
        counts = np.ones(W * H, np.uint32)
        n = spp - 1
        if n < 1:
            continue
        hp, hs = rt.camera_rays_pixels(c["cam"], px, counts, n, table)
        want = host.reshape(H * W, spp, 6)[px.astype(np.int64), 1:].reshape(-1, 6)
        if not cc.same_bits(hp, want):
            bad.append((name, "camera_rays_pixels host", cc.count_diff(hp, want)))
        dp, dsd = rt.camera_rays_pixels(c["cam"], px, counts, n, table, device=0)
        torch.cuda.synchronize()
        if not cc.same_bits(dp.cpu().numpy(), hp) or not np.array_equal(dsd.cpu().numpy().view(np.uint32), hs):
            bad.append((name, "camera_rays_pixels device", cc.count_diff(dp.cpu().numpy(), hp)))
    print(f"camera rays: {len(bad)} differ: {bad[:10]}")
    assert not bad, bad[:8]


def test_the_query_path_renders_the_same_frames():
    """render_rays: camera rays -> shade_rays -> film, no tile test and no wave family anywhere."""
    bad = []
    for name in cc.NAMES:
        c = cc.case(name)
        tab = None if c["jitter"] is None else np.array(c["jitter"])  # (writable: torch wraps it)
        out = _ds(c["scene"]).render_rays(c["cam"], c["spp"], max_depth=c["depth"], miss_color=c["miss"], jitter=tab)
        out = out[0] if isinstance(out, tuple) else out
        got = out.cpu().numpy().reshape(c["frame"].shape)
        if not cc.same_bits(got, c["frame"]):
            bad.append((name, cc.count_diff(got, c["frame"])))
    print(f"render_rays: {len(bad)} of {len(cc.NAMES)} frames differ: {bad[:12]}")
    assert not bad, bad[:8]
    for s in SCENES:
        assert _ds(s).faults() == 0, s


# ---- the group-wide tests' device builds on the camera sets --------------------------------------
@pytest.mark.parametrize("name", __import__("tile_cases").CAMERA_TILE_CASES)
def test_device_tile_test_is_sound_at_these_cameras(name):
    import tile_cases as tc

    got = tc.check_camera_set(tc.device_fn, name)
    assert not got.any()


@pytest.mark.parametrize("name", __import__("family_cases").DEGENERATE_CASES)
def test_device_family_test_is_sound_with_degenerate_lanes(name):
    import family_cases as fc

    out, loose = fc.check_degenerate(fc.device_fn, name)
    hout, hloose = fc.check_degenerate(fc.host_fn, name)
    assert np.array_equal(loose, hloose)
    print(f"{name}: device and host builds differ on {int((out != hout).sum())} of {out.size} entries")


# ---- HW1 ----------------------------------------------------------------------------------------
def test_hw1_binned_and_brute_force():
    """The constructor cameras of four classes (hw1=True) over a 120-triangle soup at 40 x 24, 4
    spp: the binned path, the brute-force path and orc.render_hw1 agree on frame, winner and t.
    (HW1's Ray has no 1e-12 fallback: a zero D is a NaN direction, a NaN pixel.)"""
    import hw1_cases as hc

    bad = []
    for name in cc.HW1_NAMES:
        c = cc.hw1_case(name)
        got = {}
        for brute in (False, True):
            got[brute] = rt.render_hw1(c["positions"], c["normals"], c["indices"], c["camera"], *hc.LIGHT, spp=c["spp"],
                                       jitter=c["jitter"], aov=True, brute=brute)
            d = _diff(got[brute], c["ref"])
            if d:
                bad.append((name, "brute" if brute else "binned", d))
        d = _diff(got[False], got[True])
        if d:
            bad.append((name, "binned vs brute", d))
    print(f"hw1: {len(bad)} differ of {3 * len(cc.HW1_NAMES)}: {bad[:12]}")
    assert not bad, bad[:8]
    # an ordinary frame after them
    c = hc.case(cc.HW1_SOUP, cc.HW1_W, cc.HW1_H)
    got = rt.render_hw1(c["positions"], c["normals"], c["indices"], c["camera"], *hc.LIGHT, spp=c["spp"], jitter=c["jitter"],
                        aov=True)
    assert not _diff(got, hc.reference(c))
