"""Frames with a caller's jitter table (rt_render_opts.jitter) through the G path: any table must
render exactly.  The tile cull pads a tile by one pixel, which covers tables with every entry
finite and |entry| <= 1; a frame with any other table runs without the cull (render_frame).

Every frame (rgb, hit index, hit t) must equal the oracle's orc.render_g(..., jitter_tab=table)
bit for bit and the same call with RT_FLAG_NO_CULL, for the default table passed explicitly, the
[0, 1) table, the four corners (+-1, +-1), +-2.5, a constant (6, -6), one entry at 40 px, one NaN
entry and one inf entry; with the cut pass at its default and forced (cull_coverage 1.0) and every
RT_KERNEL_*; through render_device_pair, Renderer.submit and a 3-way band shard; and against
render_rays, the on-device route that never culls.

Before this guard the frames of the +-2.5, (6, -6) and 40 px tables had silhouette tiles written
with the miss colour (see test_shifted_tables_move_geometry_into_empty_tiles: the CPU check that
those tables do move geometry into tiles the default table leaves empty).
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

from conftest import host_scene, oracle_camera
from oracle import pyoracle as orc

import raytracinginonesemester_amd as rt

gpu = pytest.mark.gpu

SCENES = ("frog.json", "cornell.json", "sphere_single.json")
SIZES = ((96, 64), (37, 23))
SPPS = (4, 16)
KERNELS = (rt.RT_KERNEL_AUTO, rt.RT_KERNEL_WAVE, rt.RT_KERNEL_LANE, rt._lib.RT_KERNEL_WAVE_PIXELS)
NO_CULL = rt._lib.RT_FLAG_NO_CULL
TABLES = ("default", "unit01", "corners", "pm2.5", "const6", "one40", "nan", "inf")
SHIFTED = ("pm2.5", "const6", "one40")  # beyond the one-pixel pad


@lru_cache(maxsize=None)
def table(name: str, spp: int) -> np.ndarray:
    rng = np.random.default_rng([51, TABLES.index(name), spp])
    t = rt.jittered_samples(spp).copy()
    if name == "unit01":
        t = rt.jittered_samples(spp, 42, centered=False).copy()
    elif name == "corners":
        t = np.array([(1, 1), (1, -1), (-1, 1), (-1, -1)] * (spp // 4), np.float32)
    elif name == "pm2.5":
        t = rng.choice(np.array([-2.5, 2.5], np.float32), size=(spp, 2))
    elif name == "const6":
        t = np.tile(np.array([6.0, -6.0], np.float32), (spp, 1))
    elif name == "one40":
        t[1] = (40.0, 0.25)
    elif name == "nan":
        t[2] = (np.nan, 0.0)
    elif name == "inf":
        t[0] = (np.inf, 0.125)
    t = np.ascontiguousarray(t, np.float32)
    t.setflags(write=False)
    return t


@lru_cache(maxsize=None)
def oracle_frame(scene: str, size: tuple, spp: int, name: str):
    hs = host_scene(scene)
    cam = hs.camera(*size)
    out = orc.render_g(hs.num_triangles, oracle_camera(cam), hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids,
                       hs.materials, hs.lights, spp=spp, max_depth=1, jitter_tab=table(name, spp), aov=True)
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _device_scene(scene: str):
    return rt.DeviceScene.from_host(host_scene(scene), device=0)


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32)) for x, y in zip(a, b))


def _diff(a, b):
    return [int((np.asarray(x).view(np.uint32) != np.asarray(y).view(np.uint32)).sum()) for x, y in zip(a, b)]


@pytest.mark.parametrize("name", SHIFTED)
def test_shifted_tables_move_geometry_into_empty_tiles(name):
    """The references alone (no GPU): on frog at 96 x 64, for both sample counts, some pixel tile of
    the render kernels' shape (8 x 8 at 4 spp, 4 x 4 at 16) has no hit under the default table and
    a hit under the shifted one: a frame culled with the default pad there and traced with the
    caller's table differs, so the frame tests below can tell.  The other cases' counts are
    printed (a 40 px shift leaves a 37 px image; sphere_single's disc moved by (6, -6) covers no
    new 8 x 8 tile)."""
    total = 0
    for scene in ("frog.json", "sphere_single.json"):
        for size in SIZES:
            for spp in SPPS:
                tw = 8 if spp == 4 else 4
                base = oracle_frame(scene, size, spp, "default")[1]
                moved = oracle_frame(scene, size, spp, name)[1]
                H, W = base.shape[:2]
                found = 0
                for y in range(0, H, tw):
                    for x in range(0, W, tw):
                        if (base[y:y + tw, x:x + tw] < 0).all() and (moved[y:y + tw, x:x + tw] >= 0).any():
                            found += 1
                print(f"{name} {scene} {size} spp {spp}: {found} tiles")
                total += found
                if size == SIZES[0] and scene == "frog.json":
                    assert found > 0, (scene, size, spp)
    print(f"{name}: {total} such tiles over all cases")


@gpu
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", SCENES)
def test_any_table_renders_exactly(scene, size, spp, kernel, tune):
    ds = _device_scene(scene)
    cam = host_scene(scene).camera(*size)
    bad = []
    for cov in (None, 1.0):
        if cov is not None:
            tune(cull_coverage=cov)
        for name in TABLES:
            ref = oracle_frame(scene, size, spp, name)
            a = ds.render(cam, spp=spp, max_depth=1, aov=True, jitter=table(name, spp), kernel=kernel)
            b = ds.render(cam, spp=spp, max_depth=1, aov=True, jitter=table(name, spp), kernel=kernel, flags=NO_CULL)
            if not (_same(a, ref) and _same(a, b)):
                bad.append((name, kernel, cov, "vs oracle", _diff(a, ref), "vs no cull", _diff(a, b)))
    print(f"{scene} {size} spp {spp} kernel {kernel}: {len(bad)} of {2 * len(TABLES)} frames differ; "
          f"(table, kernel, cull_coverage): {[b[:3] for b in bad]}")
    assert not bad, bad[:6]
    assert ds.faults() == 0


@gpu
@pytest.mark.parametrize("name", ["pm2.5", "one40"])
def test_pair_renderer_and_band_shards(name):
    """The same frames through render_device_pair, Renderer.submit and a 3-way band shard."""
    import torch

    scene, size, spp = "frog.json", (96, 64), 16
    W, H = size
    hs = host_scene(scene)
    cams = [hs.camera(W, H), rt.Camera((0.3, -2.4, 0.9), (0.0, 0.0, 0.2), (0, 0, 1), 35.0, 24.0, W, H)]
    ds = _device_scene(scene)
    jit = table(name, spp)
    want = [ds.render(c, spp=spp, max_depth=1, jitter=jit, flags=NO_CULL) for c in cams]
    ref = oracle_frame(scene, size, spp, name)[0]
    assert np.array_equal(want[0].view(np.uint32), ref.view(np.uint32))
    # a pair
    o, _keep = rt.DeviceScene.make_opts(spp=spp, max_depth=1, jitter=jit)
    bufs = [torch.zeros((H, W, 3), dtype=torch.float32, device="cuda") for _ in cams]
    ds.render_device_pair(cams[0], cams[1], o, bufs[0].data_ptr(), None, bufs[1].data_ptr(), None)
    torch.cuda.synchronize()
    for k in range(2):
        assert np.array_equal(bufs[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), ("pair", k)
    # band shards
    out = np.zeros_like(want[0])
    for b in range(3):
        strip = ds.render(cams[0], spp=spp, max_depth=1, jitter=jit, band_rows=8, band_index=b, band_count=3)
        out[[y for y in range(H) if (y // 8) % 3 == b]] = strip
    assert np.array_equal(out.view(np.uint32), want[0].view(np.uint32))
    # the frame renderer
    r = rt.Renderer.from_host(hs, devices=(0,), deliver=rt.RT_DELIVER_F32)
    try:
        for k, c in enumerate(cams):
            addr, n = r.wait(r.submit(c, o))
            assert n == W * H * 12
            got = np.ctypeslib.as_array((C.c_uint32 * (n // 4)).from_address(addr)).reshape(H, W, 3)
            assert np.array_equal(got, want[k].view(np.uint32)), ("renderer", k)
    finally:
        r.close()


@gpu
def test_against_the_query_path():
    """render_rays (camera_rays -> shade_rays -> film: no tile culling anywhere) with the same
    table gives render()'s frame."""
    scene, size, spp = "frog.json", (96, 64), 4
    ds = _device_scene(scene)
    cam = host_scene(scene).camera(*size)
    for name in ("pm2.5", "const6"):
        jit = table(name, spp)
        a = ds.render(cam, spp=spp, max_depth=1, jitter=jit)
        b = ds.render_rays(cam, spp, max_depth=1, jitter=jit)
        b = b[0] if isinstance(b, tuple) else b
        assert np.array_equal(a.view(np.uint32), b.cpu().numpy().reshape(a.shape).view(np.uint32)), name
