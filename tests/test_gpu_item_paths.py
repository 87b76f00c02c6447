"""The render kernel's per-item paths: a depth-1 wave none of whose lanes hit
takes the host's all-miss pixel, a hitting wave sums with one lane per (pixel, channel), and the
tile's column and row come from a multiply and a shift.

Bar: every frame (rgb, hit index, hit t, P6 bytes) is the oracle's bit for bit, equals the same
call with RT_FLAG_NO_CULL (where the quarters that miss the root box reach the render kernel) and
equals render_rays' frame (the query path: no tiles, no items).  The cases are the smallest that
reach each path; test_cases_hold_both_kinds_of_quarter proves on the CPU, from the oracle alone,
that the frames hold a tile with hits one of whose quarters (a wave's item) misses entirely, and a
quarter with hits and misses both.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from conftest import host_scene, oracle_camera

import raytracinginonesemester_amd as rt
from oracle import pyoracle as orc

gpu = pytest.mark.gpu

NO_CULL = rt._lib.RT_FLAG_NO_CULL
SCENES = ("frog.json", "sphere_single.json")
SIZES = ((37, 23), (96, 64))
SPPS = (4, 16)
OUTSIDE = (1.5, -0.2, 0.3)  # a miss colour outside [0, 1]: clamped per sample


def _miss(scene: str):
    return tuple(float(x) for x in host_scene(scene).settings["miss_color"])


@lru_cache(maxsize=None)
def oracle_frame(scene: str, size: tuple, spp: int, miss: tuple, lights: bool = True, move: tuple = (0.0, 0.0, 0.0)):
    """(rgb, hit index, hit t, P6 samples) of the reference at depth 1, the scene's camera moved
    by ``move``."""
    hs = host_scene(scene)
    cam = _moved(hs.camera(*size), move) if any(move) else hs.camera(*size)
    li = hs.lights if lights else np.zeros(0, rt.LIGHT_DTYPE)
    rgb, hi, ht = orc.render_g(hs.num_triangles, oracle_camera(cam), hs.nodes, hs.aabbs, hs.triangles,
                               hs.tri_object_ids, hs.materials, li, spp=spp, max_depth=1, miss=miss, aov=True)
    out = (rgb, hi, ht, orc.ppm_quantize(rgb).astype(np.uint8))
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _device_scene(scene: str, lights: bool = True):
    hs = host_scene(scene)
    if lights:
        return rt.DeviceScene.from_host(hs, device=0)
    return rt.DeviceScene(hs.num_triangles, hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids, hs.materials, None)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(np.asarray(y).reshape(np.asarray(x).shape))) for x, y in zip(a, b))


def _quarters(hit_px: np.ndarray, spp: int):
    """Per tile of the samples kernel (256 / spp pixels, square at these spp) and quarter (a
    wave's item: a half-side square, the Z order's top two bits): the number of pixels inside
    the frame and of those with a hit; shape (tiles_y, tiles_x, 2, 2)."""
    side = {4: 8, 16: 4}[spp]
    H, W = hit_px.shape
    ty, tx = -(-H // side), -(-W // side)
    pad = np.zeros((ty * side, tx * side), bool)
    inside = pad.copy()
    pad[:H, :W] = hit_px
    inside[:H, :W] = True
    h = side // 2

    def fold(a):
        return a.reshape(ty, 2, h, tx, 2, h).sum(axis=(2, 5)).transpose(0, 2, 1, 3)

    return fold(inside), fold(pad)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", SCENES)
def test_cases_hold_both_kinds_of_quarter(scene, size, spp):
    """The oracle alone (no GPU): the frame has a tile with a hit (so no culling pass can drop
    it) one of whose quarters has pixels and no hit in any sample, a quarter in which some samples
    hit and some miss, and at 37 x 23, no multiple of either tile, an all-miss quarter with lanes
    outside the frame."""
    hi = oracle_frame(scene, size, spp, _miss(scene))[1]
    any_hit, all_hit = (hi >= 0).any(axis=2), (hi >= 0).all(axis=2)
    n_in, n_hit = _quarters(any_hit, spp)
    _, n_full = _quarters(all_hit, spp)
    tile_live = n_hit.sum(axis=(2, 3)) > 0
    miss_q = (n_in > 0) & (n_hit == 0) & tile_live[:, :, None, None]
    mixed_q = (n_hit > 0) & (n_full < n_in)
    full = (256 // spp) // 4
    # at the frame's ragged edge (the render kernel sees these tiles with RT_FLAG_NO_CULL)
    ragged_miss_q = (n_in > 0) & (n_in < full) & (n_hit == 0)
    print(f"{scene} {size} spp {spp}: {int(miss_q.sum())} all-miss quarters in tiles with hits, "
          f"{int(ragged_miss_q.sum())} ragged all-miss quarters, {int(mixed_q.sum())} mixed quarters")
    assert miss_q.any() and mixed_q.any()
    if size == (37, 23):
        assert ragged_miss_q.any()


def _device_frames(ds, cam, spp, miss, flags, rgb, p6, aov):
    """One render_device call writing the chosen outputs; returns them as numpy (None if off)."""
    import torch

    H, W = cam.pixel_height, cam.pixel_width
    o, _j = rt.DeviceScene.make_opts(spp=spp, max_depth=1, miss_color=miss, flags=flags)
    t_rgb = torch.full((H, W, 3), -7.0, dtype=torch.float32, device="cuda") if rgb else None
    t_p6 = torch.full((H, W, 3), 77, dtype=torch.uint8, device="cuda") if p6 else None
    t_hi = torch.full((H, W, spp), -9, dtype=torch.int32, device="cuda") if aov else None
    t_ht = torch.full((H, W, spp), -9.0, dtype=torch.float32, device="cuda") if aov else None
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    ds.render_device(cam, o, ptr(t_rgb), ptr(t_hi), ptr(t_ht), p6_dev_ptr=ptr(t_p6))
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (t_rgb, t_hi, t_ht, t_p6)]


@gpu
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", SCENES)
def test_frames_three_ways(scene, size, spp):
    """rt_render with and without the cull, render_rays, and rt_render_device writing rgb only,
    P6 only and both, with and without the AOVs: all the oracle's frame, for the scene's miss
    colour and one outside [0, 1]."""
    ds = _device_scene(scene)
    cam = host_scene(scene).camera(*size)
    for miss in (_miss(scene), OUTSIDE):
        ref = oracle_frame(scene, size, spp, miss)
        for flags in (0, NO_CULL):
            got = ds.render(cam, spp=spp, max_depth=1, miss_color=miss, aov=True, flags=flags)
            assert _same(got, ref[:3]), (miss, flags, "rt_render")
            for rgb, p6, aov in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                out = _device_frames(ds, cam, spp, miss, flags, rgb, p6, aov)
                for k, (a, b) in enumerate(zip(out, ref)):
                    assert a is None or np.array_equal(_bits(a), _bits(b)), (miss, flags, (rgb, p6, aov), k)
        q_rgb, q_p6 = ds.render_rays(cam, spp, max_depth=1, miss_color=miss, p6=True)
        assert _same((q_rgb.cpu().numpy(), q_p6.cpu().numpy()), (ref[0], ref[3])), (miss, "render_rays")
    assert ds.faults() == 0


@gpu
@pytest.mark.parametrize("case", ["spp64", "spp256", "spp3", "no_lights", "cornell"])
def test_paths_left_as_they_were(case):
    """Items the change leaves alone: one pixel per wave (64 spp), block-wide pixels (256 spp), the
    pixel loop (3 spp), a scene without lights and cornell's light loop; each against the oracle
    and RT_FLAG_NO_CULL, with a miss colour outside [0, 1] too."""
    scene, spp, lights, size = {"spp64": ("frog.json", 64, True, (37, 23)), "spp256": ("frog.json", 256, True, (37, 23)),
                                "spp3": ("frog.json", 3, True, (37, 23)), "no_lights": ("frog.json", 16, False, (37, 23)),
                                "cornell": ("cornell.json", 16, True, (37, 23))}[case]
    hs = host_scene(scene)
    if case == "cornell":
        assert hs.lights.shape[0] > 1
    ds = _device_scene(scene, lights)
    cam = hs.camera(*size)
    for miss in (_miss(scene), OUTSIDE):
        ref = oracle_frame(scene, size, spp, miss, lights)
        assert (ref[1] >= 0).any() and (case == "cornell" or (ref[1] < 0).any())  # the box fills cornell's view
        for flags in (0, NO_CULL):
            got = ds.render(cam, spp=spp, max_depth=1, miss_color=miss, aov=True, flags=flags)
            assert _same(got, ref[:3]), (case, miss, flags)
            out = _device_frames(ds, cam, spp, miss, flags, 1, 1, 0)
            assert _same((out[0], out[3]), (ref[0], ref[3])), (case, miss, flags, "device")
    assert ds.faults() == 0


def _moved(cam, d):
    return rt.Camera(tuple(np.add(cam.pos, d)), cam.look_at, cam.up, cam.focal_length_mm, cam.sensor_height_mm,
                     cam.pixel_width, cam.pixel_height)


HEAVY_MOVE, PAIR_MOVE = (0.05, 0.0, 0.02), (0.004, 0.0, 0.003)


@gpu
@pytest.mark.parametrize("knobs", [dict(), dict(heavy_cap=1), dict(heavy_frac=1e-6), dict(heavy_cap=1, heavy_frac=1e-6)],
                         ids=["default", "cap1", "all_heavy", "cap1_all_heavy"])
def test_heavy_lists(knobs, tune):
    """Consecutive frames with the cut pass on, so the render waves' costs feed the next frame's
    heavy lists: lists of one entry that overflow, every tile heavy, and the camera moved between
    frames.  Each frame is the oracle's for its camera, and its own no-cull frame."""
    scene, size, spp = "frog.json", (96, 64), 16
    hs = host_scene(scene)
    ds = rt.DeviceScene.from_host(hs, device=0)  # its own: the costs are the scene's state
    try:
        miss = _miss(scene)
        base, far = hs.camera(*size), _moved(hs.camera(*size), HEAVY_MOVE)
        cams = [base, base, base, far, far, base]
        want = {id(base): oracle_frame(scene, size, spp, miss)[:3],
                id(far): oracle_frame(scene, size, spp, miss, True, HEAVY_MOVE)[:3]}
        assert not np.array_equal(want[id(base)][1], want[id(far)][1])
        for c in (base, far):
            assert _same(ds.render(c, spp=spp, max_depth=1, miss_color=miss, aov=True, flags=NO_CULL), want[id(c)])
        tune(cull_coverage=1.0, **knobs)
        heavy = []
        for k, c in enumerate(cams):
            got = ds.render(c, spp=spp, max_depth=1, miss_color=miss, aov=True)
            heavy.append(ds.heavy_tiles())
            assert _same(got, want[id(c)]), (knobs, k)
            out = _device_frames(ds, c, spp, miss, 0, 1, 1, 0)
            assert np.array_equal(_bits(out[0]), _bits(want[id(c)][0])), (knobs, k, "device")
        # the pair kernel's lists (both frames' heavy classes interleaved, then their survivors)
        import torch

        o, _keep = rt.DeviceScene.make_opts(spp=spp, max_depth=1, miss_color=miss)
        bufs = [torch.zeros((size[1], size[0], 3), dtype=torch.float32, device="cuda") for _ in range(2)]
        ds.render_device_pair(cams[0], cams[3], o, bufs[0].data_ptr(), None, bufs[1].data_ptr(), None)
        torch.cuda.synchronize()
        heavy.append(ds.heavy_tiles())
        for b, c in zip(bufs, (cams[0], cams[3])):
            assert np.array_equal(_bits(b.cpu().numpy()), _bits(want[id(c)][0])), (knobs, "pair")
        print(f"{knobs}: kernel {ds.kernel_name()}, heavy tiles per frame {heavy}")
        if "heavy_frac" in knobs:  # every traced tile's cost is over the threshold
            assert max(heavy[1:]) > 0, heavy
        assert ds.faults() == 0
    finally:
        ds.close()


@gpu
def test_pair_renderer_and_band_shards(tune):
    """The same frames through render_device_pair (two cameras), Renderer.submit three deep and a
    3-way band shard on half waves."""
    import torch

    scene, size, spp = "frog.json", (96, 64), 16
    W, H = size
    hs = host_scene(scene)
    miss = _miss(scene)
    base = hs.camera(W, H)
    cams = [base, _moved(base, PAIR_MOVE)]
    ds = _device_scene(scene)
    # what every path below must give: the oracle's frame of each camera; the no-cull frame and
    # the query path's frame are checked against it first
    refs = [oracle_frame(scene, size, spp, miss), oracle_frame(scene, size, spp, miss, True, PAIR_MOVE)]
    want, want_p6 = [r[0] for r in refs], [r[3] for r in refs]
    assert not np.array_equal(_bits(want[0]), _bits(want[1]))
    for c, r in zip(cams, refs):
        assert _same(ds.render(c, spp=spp, max_depth=1, miss_color=miss, aov=True, flags=NO_CULL), r[:3])
        q_rgb, q_p6 = ds.render_rays(c, spp, max_depth=1, miss_color=miss, p6=True)
        assert _same((q_rgb.cpu().numpy(), q_p6.cpu().numpy()), (r[0], r[3]))
    # a pair: both orders, floats and P6
    o, _keep = rt.DeviceScene.make_opts(spp=spp, max_depth=1, miss_color=miss)
    for a, b in ((0, 1), (1, 0), (0, 0)):
        rgb = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in range(2)]
        p6 = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
        ds.render_device_pair(cams[a], cams[b], o, rgb[0].data_ptr(), p6[0].data_ptr(), rgb[1].data_ptr(), p6[1].data_ptr())
        torch.cuda.synchronize()
        assert ds.kernel_name().startswith("render_pair_kernel<49, true, true, 7, 0>"), ds.kernel_name()
        for k, c in enumerate((a, b)):
            assert np.array_equal(_bits(rgb[k].cpu().numpy()), _bits(want[c])), ("pair", a, b, k)
            assert np.array_equal(p6[k].cpu().numpy(), want_p6[c]), ("pair P6", a, b, k)
    # the frame renderer, three frames in flight
    r = rt.Renderer.from_host(hs, devices=(0,), deliver=rt.RT_DELIVER_P6, depth=3)
    try:
        order = [0, 1, 1, 0, 0, 1, 0]
        pend = []
        for k in order:
            if len(pend) == 3:
                c, t = pend.pop(0)
                addr, n = r.wait(t)
                assert bytes((C.c_uint8 * n).from_address(addr)) == want_p6[c].tobytes(), ("renderer", c)
            pend.append((k, r.submit(cams[k], o)))
        for c, t in pend:
            addr, n = r.wait(t)
            assert bytes((C.c_uint8 * n).from_address(addr)) == want_p6[c].tobytes(), ("renderer", c)
    finally:
        r.close()
    # band shards, half waves (as the shards of a wide split take them)
    tune(half_waves=1)
    out = np.zeros_like(want[0])
    for b in range(3):
        strip = ds.render(cams[0], spp=spp, max_depth=1, miss_color=miss, band_rows=8, band_index=b, band_count=3)
        assert ds.kernel_name() == "render_tiles_kernel<49, true, true, 7, 1>", ds.kernel_name()
        out[[y for y in range(H) if (y // 8) % 3 == b]] = strip
    assert np.array_equal(_bits(out), _bits(want[0]))
    assert ds.faults() == 0


@gpu
@pytest.mark.parametrize("flags", [0, NO_CULL])
def test_queue_extremes(flags):
    """A camera looking away (every queue empty under the cull; every wave all-miss without it)
    and a frame of two tiles (fewer items than the grid's static first items)."""
    scene, spp = "frog.json", 16
    hs = host_scene(scene)
    ds = _device_scene(scene)
    miss = _miss(scene)
    base = hs.camera(37, 23)
    away = rt.Camera(base.pos, tuple(2.0 * np.asarray(base.pos) - np.asarray(base.look_at)), base.up,
                     base.focal_length_mm, base.sensor_height_mm, 37, 23)
    for cam, hits in ((away, False), (hs.camera(5, 3), True)):
        ref = orc.render_g(hs.num_triangles, oracle_camera(cam), hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids,
                           hs.materials, hs.lights, spp=spp, max_depth=1, miss=miss, aov=True)
        assert (ref[1] >= 0).any() == hits
        got = ds.render(cam, spp=spp, max_depth=1, miss_color=miss, aov=True, flags=flags)
        assert _same(got, ref), (hits, flags)
        out = _device_frames(ds, cam, spp, miss, flags, 1, 1, 1)
        assert _same(out, (*ref, orc.ppm_quantize(ref[0]).astype(np.uint8))), (hits, flags, "device")
    assert ds.faults() == 0
