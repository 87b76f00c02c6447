"""The frame's pre-passes (rt_prepass.hpp: tile_cull_kernel, tile_cut_kernel and the pair forms)
at the shapes where the cut pass's group-wide form can go wrong: list lengths around a group
boundary, partial tiles, every tile order, band shards, every cut size, full heavy lists, pairs.

Bar: every frame is the oracle's bit for bit (rgb, hit index, hit t; the P6 bytes where a P6
pointer is given), whatever the passes culled, and on the full c3 frame the passes still leave
the render kernel exactly the camera rays they left before (culling power).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

from conftest import host_scene, oracle_camera

import raytracinginonesemester_amd as rt
from oracle import pyoracle as orc
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

ORDERS = [rt.RT_TILES_ROWS, rt.RT_TILES_LINEAR, rt.RT_TILES_XCD_CHUNK]


def _cam(hs, kind, w, h):
    """away: nothing of the scene in view; corner: one corner of the root box at the image's
    edge; frog: the scene's own camera; inside: from the root box's centre (the root test never
    culls: every tile reaches the cut pass); far: the scene small in the view."""
    base = hs.camera(w, h)
    pos, look = np.array(base.pos, np.float64), np.array(base.look_at, np.float64)
    lo, hi = hs.aabbs[0, :3].astype(np.float64), hs.aabbs[0, 3:].astype(np.float64)
    if kind == "away":
        look = pos + (pos - look)
    elif kind == "corner":
        # aim beside the corner so that it lands near the image's border
        d = hi - pos
        side = np.cross(d, np.array(base.up, np.float64))
        look = hi + 0.42 * side / np.linalg.norm(side) * np.linalg.norm(d) * (24.0 / base.focal_length_mm) * w / h
    elif kind == "inside":
        pos = (lo + hi) / 2
        look = pos + (look - np.array(base.pos, np.float64))
    elif kind == "far":
        pos = look + 6.0 * (pos - look)
    elif kind == "moved":
        pos = pos + np.array([0.004, 0.0, 0.003])
    return rt.Camera(tuple(pos), tuple(look), base.up, base.focal_length_mm, base.sensor_height_mm, w, h)


@lru_cache(maxsize=None)
def _ref(scene, kind, w, h, spp):
    """The oracle's frame (computed once per case, shared, never written to)."""
    hs = host_scene(scene)
    out = orc.render_g(hs.num_triangles, oracle_camera(_cam(hs, kind, w, h)), hs.nodes, hs.aabbs, hs.triangles,
                       hs.tri_object_ids, hs.materials, hs.lights, spp=spp, max_depth=1, aov=True)
    for a in out:
        a.setflags(write=False)
    return out


def _same(got, ref, what, rows=None):
    for name, x, y in zip(("rgb", "hit index", "hit t"), got, ref):
        y = np.asarray(y) if rows is None else np.asarray(y)[rows]
        x = np.asarray(x)
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: {name} differs from the oracle"


@lru_cache(maxsize=None)
def _scene(scene):
    return rt.DeviceScene.from_host(host_scene(scene), device=0)


def _p6(ds, cam, o, w, h):
    """The frame through rt_render_device_p6: float framebuffer and P6 bytes, device buffers."""
    rgb = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    p6 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    ds.render_device(cam, o, rgb.data_ptr(), p6_dev_ptr=p6.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), p6.cpu().numpy().tobytes()


@pytest.mark.parametrize("w,h", [(4, 4), (28, 4), (32, 4), (36, 4), (64, 4), (68, 4), (36, 36)])
def test_every_tile_survives_the_root_test(w, h, tune):
    """16 spp: 4x4 tiles.  From inside the root box no tile fails the root test, so with the cut
    forced on one list (RT_TILES_LINEAR) holds all w/4 * h/4 tiles: 1, 7, 8, 9, 16 and 17 slots
    (a group is 8), and 81 over eight lists."""
    tune(cull_coverage=1.0)
    hs = host_scene("frog.json")
    ds = _scene("frog.json")
    cam = _cam(hs, "inside", w, h)
    order = rt.RT_TILES_LINEAR if h == 4 else rt.RT_TILES_ROWS
    got = ds.render(cam, spp=16, max_depth=1, aov=True, tile_order=order)
    assert ds.live_tiles() == ((w // 4) * (h // 4), (w // 4) * (h // 4))
    _same(got, _ref("frog.json", "inside", w, h, 16), (w, h))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("kind", ["away", "corner", "frog", "far"])
def test_cameras_and_tile_orders(kind, order, tune):
    """No root survivor (away), a few (corner), the frog near and far; one list and eight; the
    float frame, the AOVs and the P6 bytes."""
    tune(cull_coverage=1.0)
    hs = host_scene("frog.json")
    ds = _scene("frog.json")
    w, h = 96, 64
    cam = _cam(hs, kind, w, h)
    ref = _ref("frog.json", kind, w, h, 16)
    got = ds.render(cam, spp=16, max_depth=1, aov=True, tile_order=order)
    live, total = ds.live_tiles()
    assert total == 24 * 16
    if kind == "away":
        assert live == 0 and not (ref[1] >= 0).any()
    elif kind == "corner":
        assert 0 < live < total // 4, live
    else:
        assert live > 0 and (ref[1] >= 0).any()
    _same(got, ref, (kind, order))
    o, _j = rt.DeviceScene.make_opts(spp=16, max_depth=1, tile_order=order)
    rgb, p6 = _p6(ds, cam, o, w, h)
    assert np.array_equal(rgb.view(np.uint32), np.asarray(ref[0]).view(np.uint32))
    assert p6 == rt.encode_p6(np.asarray(ref[0]))[-w * h * 3:]


@pytest.mark.parametrize("order", [rt.RT_TILES_ROWS, rt.RT_TILES_LINEAR])
@pytest.mark.parametrize("spp", [1, 3, 16])
@pytest.mark.parametrize("w,h", [(37, 23), (65, 3), (1, 1)])
def test_partial_tiles(w, h, spp, order, tune):
    tune(cull_coverage=1.0)
    hs = host_scene("frog.json")
    ds = _scene("frog.json")
    for kind in ("frog", "far"):
        cam = _cam(hs, kind, w, h)
        got = ds.render(cam, spp=spp, max_depth=1, aov=True, tile_order=order)
        _same(got, _ref("frog.json", kind, w, h, spp), (kind, w, h, spp))
        o, _j = rt.DeviceScene.make_opts(spp=spp, max_depth=1, tile_order=order)
        rgb, p6 = _p6(ds, cam, o, w, h)
        assert p6 == rt.encode_p6(np.asarray(_ref("frog.json", kind, w, h, spp)[0]))[-w * h * 3:]


@pytest.mark.parametrize("band_count,band_index", [(3, 0), (3, 2), (8, 0), (8, 5)])
def test_band_shards(band_count, band_index, tune):
    """Band shards (global_row): the shard's rows of the oracle's whole frame."""
    tune(cull_coverage=1.0)
    hs = host_scene("frog.json")
    ds = _scene("frog.json")
    w, h = 96, 64
    rows = np.concatenate([np.arange(8 * b, 8 * b + 8) for b in range(band_index, h // 8, band_count)])
    for kind in ("frog", "far"):
        ref = _ref("frog.json", kind, w, h, 16)
        got = ds.render(_cam(hs, kind, w, h), spp=16, max_depth=1, aov=True, band_rows=8, band_index=band_index,
                        band_count=band_count)
        assert got[0].shape[0] == len(rows) == L.lib().rt_shard_rows(h, 8, band_index, band_count)
        _same(got, ref, (kind, band_count, band_index), rows)


@pytest.mark.parametrize("boxes", [1, 8, 64])
@pytest.mark.parametrize("sub", [0, 2, 16, 64])
@pytest.mark.parametrize("scene", ["frog.json", "cornell.json"])
def test_cut_sizes(scene, sub, boxes, tune):
    """Fewer cut boxes than lanes, no second level, and second levels of 32, 4 and 1 pairs per
    pass (more pairs than one pass holds)."""
    tune(cull_coverage=1.0, cut_sub=sub, cull_boxes=boxes)
    hs = host_scene(scene)
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        w, h = 80, 48
        for kind in ("frog", "far", "inside"):
            got = ds.render(_cam(hs, kind, w, h), spp=16, max_depth=1, aov=True)
            _same(got, _ref(scene, kind, w, h, 16), (scene, sub, boxes, kind))
    finally:
        ds.close()


@pytest.mark.parametrize("env", [{"heavy_cap": 8}, {"heavy_frac": 1e-6}, {"heavy_cap": 8, "heavy_frac": 1e-6}])
def test_heavy_lists_and_spill(env, tune):
    """Three frames in a row: the second and third sort their tiles by the costs of the one
    before (heavy lists of 8 entries spill into the survivor lists; a tiny threshold makes every
    tile heavy)."""
    tune(cull_coverage=1.0, **env)
    hs = host_scene("frog.json")
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        w, h = 320, 180
        cam = _cam(hs, "frog", w, h)
        ref = _ref("frog.json", "frog", w, h, 16)
        heavy = []
        for _ in range(3):
            got = ds.render(cam, spp=16, max_depth=1, aov=True)
            heavy.append(ds.heavy_tiles())
            _same(got, ref, (env, len(heavy)))
        assert heavy[0] == 0 and heavy[1] > 0 and heavy[2] > 0, heavy
        if "heavy_cap" in env:
            assert max(heavy) <= 8 * 3 * 8, heavy
    finally:
        ds.close()


@pytest.mark.parametrize("a,b", [("frog", "moved"), ("far", "far"), ("corner", "away")])
def test_pairs(a, b, tune):
    """Two frames' pre-passes in one cull and one cut launch (render_device_pair)."""
    tune(cull_coverage=1.0)
    hs = host_scene("frog.json")
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        w, h = 96, 64
        o, _j = rt.DeviceScene.make_opts(spp=16, max_depth=1)
        bufs = [(torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"),
                 torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")) for _ in range(4)]
        for i in range(2):  # two pairs back to back: the second's pre-passes overlap the first
            (ra, pa), (rb, pb) = bufs[2 * i], bufs[2 * i + 1]
            ds.render_device_pair(_cam(hs, a, w, h), _cam(hs, b, w, h), o, ra.data_ptr(), pa.data_ptr(),
                                  rb.data_ptr(), pb.data_ptr())
        torch.cuda.synchronize()
        for i, kind in enumerate((a, b, a, b)):
            ref = np.asarray(_ref("frog.json", kind, w, h, 16)[0])
            rgb, p6 = bufs[i]
            assert np.array_equal(rgb.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (i, kind)
            assert p6.cpu().numpy().tobytes() == rt.encode_p6(ref)[-w * h * 3:], (i, kind)
    finally:
        ds.close()


# camera rays of the full c3 frame that the pre-passes leave to the render kernel: the value
# before the cut pass took its group-wide form (BENCH_r06.json, rays_per_frame.camera_traced)
C3_CAMERA_TRACED = 1_639_424


def test_culling_power_c3():
    """An exact pass that culled less would pass every parity check: the full c3 frame
    (1920x1080x16) must leave the render kernel the same camera rays as before."""
    hs = host_scene("frog.json")
    ds = _scene("frog.json")
    rays = ds.count_rays(hs.camera(1920, 1080), spp=16, max_depth=1)
    assert rays["camera"] == 1920 * 1080 * 16
    assert rays["camera_traced"] == C3_CAMERA_TRACED
