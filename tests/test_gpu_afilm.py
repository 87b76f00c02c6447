"""Adaptive sampling on the GPU (rt_camera_rays_pixels_device, rt_afilm_*, DeviceScene.render_adaptive;
DESIGN.md §4.22), bit for bit (no tolerance):

* pixel-list camera rays made on the device against the host build;
* afilm_add_* / afilm_resolve_* against the host build (rt_afilm_host, pinned on the CPU by
  tests/test_afilm_host.py): dense, shuffled and sparse lists, aligned and unaligned radiance,
  successive adds, guard bytes around every output;
* the selection against the host build: indices, order and count, around the block and scan-tile
  sizes of the compaction, nothing and everything selected;
* whole adaptive frames: at depth 1 against the oracle's per-sample radiance run through the host
  build, with bounces against DeviceScene.render at each pixel's own count;
* an adaptive pass on a second stream beside a Renderer's frames.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest
import torch

import afilm_cases as ac
import film_cases as fc
from conftest import REPO, host_scene
from film_cases import bits
from test_gpu_film import Guarded, p6_body, upload

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

F = np.float32
DEV = torch.device("cuda", 0)
W, H = ac.W_SMALL, ac.H_SMALL


def dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).to(DEV)


def scan_tile():
    """PATH_TILE of the compaction kernels (rt_scan.hpp): BLOCK * PATH_ROUNDS."""
    src = (REPO / "raytracinginonesemester_amd" / "csrc" / "rt_scan.hpp").read_text()
    rounds = int(re.search(r"constexpr int PATH_ROUNDS = (\d+);", src).group(1))
    block = int(re.search(r"constexpr int BLOCK = (\d+);", (REPO / "raytracinginonesemester_amd" / "csrc" / "rt_frame.hip").read_text()).group(1))
    assert "PATH_TILE = BLOCK * PATH_ROUNDS" in src
    return block * rounds


# ---- rays ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, W * H])
def test_pixel_rays_device_equals_host(m, ns):
    cam = host_scene("frog.json").camera(W, H)
    rng = np.random.default_rng(100 + m)
    counts = np.array(ac.COUNTS, np.uint32)[rng.integers(0, len(ac.COUNTS), W * H)]
    pixels = rng.permutation(W * H)[:m].astype(np.uint32)
    if m >= 63:
        pixels[m // 2] = ac.PIXEL_NONE
    table = rt.jittered_samples(max(ac.COUNTS) + ns)
    want_r, want_s = rt.camera_rays_pixels(cam, pixels, counts, ns, table)
    rays, seeds = rt.camera_rays_pixels(cam, dev_words(pixels), dev_words(counts), ns, table, device=0)
    assert rays.shape == (m * ns, 6) and seeds.shape == (m * ns,) and seeds.dtype == torch.int32
    assert rays.cpu().numpy().tobytes() == want_r.tobytes()
    assert seeds.cpu().numpy().view(np.uint32).tobytes() == want_s.tobytes()
    # the raw entry into guarded buffers, the jitter table resident on the device
    jd = torch.from_numpy(np.ascontiguousarray(table)).to(DEV)
    px, ct = dev_words(pixels), dev_words(counts)
    g_r, g_s = Guarded(want_r.nbytes, 0), Guarded(want_s.nbytes, 0)
    assert L.lib().rt_camera_rays_pixels_device(C.byref(cam.c), px.data_ptr(), m, ct.data_ptr(), ns, jd.data_ptr(),
                                                table.shape[0], g_r.ptr, g_s.ptr, 0, None) == 0, L.lib().rt_last_error()
    torch.cuda.synchronize(DEV)
    assert g_r.read(np.uint8).tobytes() == want_r.tobytes() and g_s.read(np.uint8).tobytes() == want_s.tobytes()
    if m == W * H:  # the NULL forms: every pixel in order, no samples yet
        r0, s0 = rt.camera_rays_pixels(cam, None, None, ns, table, device=0)
        w0, ws0 = rt.camera_rays(cam, ns, table[:ns])
        assert r0.cpu().numpy().tobytes() == w0.tobytes() and s0.cpu().numpy().view(np.uint32).tobytes() == ws0.tobytes()


# ---- add and resolve -------------------------------------------------------------------------------
def raw_add(film, pixels, m, ptr, n):
    return L.lib().rt_afilm_add_device(film._h, None if pixels is None else pixels.data_ptr(), m, ptr, n, None)


def resolve_check(film, want_rgb, want_counts, off_rgb, off_p6):
    """rt_afilm_resolve_device into guarded outputs at the given misalignments: all three outputs,
    then each alone; then a band."""
    Wd, Hd = film.width, film.height
    for row0, rows in ((0, Hd), (1, Hd - 2)):
        n = rows * Wd * 3
        w_rgb, w_cnt = want_rgb[row0:row0 + rows], want_counts.reshape(Hd, Wd)[row0:row0 + rows].reshape(-1)
        w_p6 = p6_body(w_rgb)
        for use in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
            g_rgb, g_p6, g_cnt = Guarded(4 * n, off_rgb), Guarded(n, off_p6), Guarded(4 * rows * Wd, 0)
            rc = L.lib().rt_afilm_resolve_device(film._h, row0, rows, g_rgb.ptr if use[0] else None,
                                                 g_p6.ptr if use[1] else None, g_cnt.ptr if use[2] else None, None)
            assert rc == 0, L.lib().rt_last_error()
            torch.cuda.synchronize(DEV)
            if use[0]:
                got = g_rgb.read(np.uint32)
                assert np.array_equal(got, bits(w_rgb).reshape(-1)), int((got != bits(w_rgb).reshape(-1)).sum())
            else:
                assert g_rgb.untouched()
            if use[1]:
                assert np.array_equal(g_p6.read(np.uint8), w_p6)
            else:
                assert g_p6.untouched()
            if use[2]:
                assert np.array_equal(g_cnt.read(np.uint32), w_cnt)
            else:
                assert g_cnt.untouched()


@pytest.mark.parametrize("rad_off", [0, 1], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("n", fc.NS_GPU)
@pytest.mark.parametrize("shape", [(W, H), (64, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_add_and_resolve_equal_the_host_build(shape, n, rad_off):
    Wd, Hd = shape
    with rt.AdaptiveFilm(Wd, Hd) as film:
        for kind in ("dense", "perm", "sparse"):
            film.clear()
            state = None
            # two successive adds with different lists: the case's own, then a sparse one with
            # entries outside the image
            for k, nn, seed in ((kind, n, 21), ("none", 3, 22)):
                px = ac.pixel_list(k, Wd, Hd, seed)
                m = Wd * Hd if px is None else px.size
                rad = ac.list_radiance(m, nn, seed)
                state = rt.afilm_host(Wd, Hd, state, rad, px, nn)["state"]
                keep, ptr = upload(rad, rad_off)
                assert ptr % 16 == 4 * rad_off
                pd = None if px is None else dev_words(px)
                assert raw_add(film, pd, m, ptr, nn) == 0, L.lib().rt_last_error()
                torch.cuda.synchronize(DEV)
                del keep
            want = rt.afilm_host(Wd, Hd, state, resolve=True)
            assert len(set(state[1].tolist())) >= 2
            assert np.array_equal(film.counts.cpu().numpy().view(np.uint32), state[1])
            for off_rgb, off_p6 in ((0, 0), (4, 1)):
                resolve_check(film, want["rgb"], state[1], off_rgb, off_p6)


def test_api_add_resolve_and_counts():
    """AdaptiveFilm on tensors: shapes, dtypes, defaults, the counts view, argument checks that need a film."""
    n = 5
    px = ac.pixel_list("sparse", W, H, 31)
    rad = ac.list_radiance(px.size, n, 31)
    want = rt.afilm_host(W, H, None, rad, px, n, resolve=True)
    lib = L.lib()
    with rt.AdaptiveFilm(W, H) as film:
        view = film.counts
        assert view.shape == (W * H,) and view.dtype == torch.int32 and view.data_ptr() == film._counts_ptr()
        assert not view.any()
        film.add(torch.from_numpy(rad).to(DEV), dev_words(px))
        assert np.array_equal(view.cpu().numpy().view(np.uint32), want["state"][1])  # the memory itself
        rgb, cnt, b = film.resolve(p6=True, counts=True)
        assert rgb.shape == (H, W, 3) and cnt.shape == (H, W) and cnt.dtype == torch.int32 and b.dtype == torch.uint8
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(want["rgb"]))
        assert np.array_equal(b.cpu().numpy(), want["bytes"])
        assert np.array_equal(cnt.cpu().numpy().reshape(-1).view(np.uint32), want["state"][1])
        band = film.resolve(row0=2, rows=3)
        assert np.array_equal(bits(band.cpu().numpy()), bits(want["rgb"][2:5]))
        with pytest.raises(ValueError):
            film.add(torch.zeros(7, dtype=torch.float32, device=DEV), dev_words(px))
        with pytest.raises(ValueError):
            film.add(torch.from_numpy(rad), dev_words(px))  # a host tensor
        keep, ptr = upload(rad)
        out = Guarded(4 * W * H * 3, 0)
        pd = dev_words(px)
        o = L.AFilmSelectOpts(2, 16, 2, 0.1, 1e-3)
        sel = torch.zeros(W * H + 1, dtype=torch.int32, device=DEV)
        cases = [
            raw_add(film, pd, px.size, None, n),                     # null radiance
            raw_add(film, pd, px.size, ptr, 0),                      # nsamples < 1
            raw_add(film, None, px.size, ptr, n),                    # a null list with m != W * H
            lib.rt_afilm_resolve_device(film._h, 0, H, None, None, None, None),   # every output null
            lib.rt_afilm_resolve_device(film._h, -1, 1, out.ptr, None, None, None),
            lib.rt_afilm_resolve_device(film._h, 3, H, out.ptr, None, None, None),
            lib.rt_afilm_select_device(film._h, None, sel.data_ptr(), sel.data_ptr() + 4 * W * H, out.ptr, None),
            lib.rt_afilm_select_device(film._h, C.byref(o), None, sel.data_ptr(), out.ptr, None),
            lib.rt_afilm_select_device(film._h, C.byref(o), sel.data_ptr(), None, out.ptr, None),
            lib.rt_afilm_select_device(film._h, C.byref(o), sel.data_ptr(), sel.data_ptr() + 4 * W * H, None, None),
            lib.rt_afilm_select_device(film._h, C.byref(o), sel.data_ptr(), sel.data_ptr() + 4 * W * H, out.ptr + 1, None),
            lib.rt_afilm_select_device(film._h, C.byref(L.AFilmSelectOpts(1, 16, 2, 0.1, 1e-3)), sel.data_ptr(),
                                       sel.data_ptr() + 4 * W * H, out.ptr, None),
        ]
        assert cases == [-1] * len(cases), cases
        assert raw_add(film, pd, 1 << 30, ptr, 2) == -7
        assert raw_add(film, pd, 0, ptr, 2) == 0 and lib.rt_afilm_resolve_device(film._h, 2, 0, out.ptr, None, None, None) == 0
        torch.cuda.synchronize(DEV)
        assert out.untouched() and not sel.any()
        assert np.array_equal(film.counts.cpu().numpy().view(np.uint32), want["state"][1])  # a refused call adds nothing
        film.clear()
        assert not film.counts.any() and not film.resolve().any()
        del keep
    with pytest.raises(rt.RTError):
        film.resolve()  # closed
    h = C.c_void_p()
    assert lib.rt_afilm_create(99, W, H, C.byref(h)) == -1 and not h  # no such device


# ---- select ----------------------------------------------------------------------------------------
TILE = 2048
SELECT_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (W, H), (TILE, 1), (TILE + 1, 1)]
SELECT_OPTS = [(2, 16, 2, 0.05, 1e-3), (4, 64, 4, 0.2, 0.25), (2, 64, 1, 0.0, 1e-3), (2, 3, 2, 0.05, 1e-3)]


def fill(film, Wd, Hd, seed):
    """Uneven counts from a dense add and two sparse ones, on the device and through the host build.
    Every fourth pixel gets one value of its own for all its samples: never noisy."""
    state = None
    npix = Wd * Hd
    rng = np.random.default_rng(seed)
    base = rng.random(npix, dtype=F)
    for j, n in enumerate((2, 3, 5)):
        px = np.arange(npix, dtype=np.uint32) if j == 0 else np.sort(rng.permutation(npix)[:max(npix // (j + 1), 1)]).astype(np.uint32)
        rad = ac.list_radiance(px.size, n, seed + j)
        flat = px % 4 == 0
        rad[flat] = base[px[flat], None, None]
        state = rt.afilm_host(Wd, Hd, state, rad, px, n)["state"]
        film.add(torch.from_numpy(rad).to(DEV), None if j == 0 else dev_words(px), n)
    return state


@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_device_equals_host(shape):
    assert scan_tile() == TILE
    Wd, Hd = shape
    with rt.AdaptiveFilm(Wd, Hd) as film:
        state = fill(film, Wd, Hd, 40)
        sizes = []
        for opts in SELECT_OPTS:
            want = rt.afilm_host(Wd, Hd, state, select=opts)["selected"]
            px, n = film.select(*opts)
            assert isinstance(n, int) and n == want.size and px.shape == (n,) and px.dtype == torch.int32, (opts, n, want.size)
            assert np.array_equal(px.cpu().numpy().view(np.uint32), want), opts
            sizes.append(n)
        assert sizes[3] == 0                      # nothing selected: every count + 2 is past max 3
        if Wd * Hd > 1:
            assert 0 < sizes[0] < Wd * Hd         # (the equal-sample entries are not noisy)
        film.clear()
        px, n = film.select(2, 16, 2, 0.05)       # everything selected: no samples yet
        assert n == Wd * Hd and np.array_equal(px.cpu().numpy(), np.arange(Wd * Hd, dtype=np.int32))
        # the raw entry: guard bytes around the list and the count
        g_px, g_n = Guarded(4 * Wd * Hd, 0), Guarded(4, 0)
        scratch = torch.empty(L.lib().rt_afilm_select_scratch_bytes(film._h) + 4, dtype=torch.uint8, device=DEV)
        o = L.AFilmSelectOpts(2, 16, 2, 0.05, 1e-3)
        assert L.lib().rt_afilm_select_device(film._h, C.byref(o), g_px.ptr, g_n.ptr, scratch.data_ptr(), None) == 0
        torch.cuda.synchronize(DEV)
        assert g_n.read(np.uint32)[0] == Wd * Hd and np.array_equal(g_px.read(np.uint32), np.arange(Wd * Hd, dtype=np.uint32))


def test_select_past_one_scan_tile_of_tiles():
    """2048 * 2048 + 1 pixels: the first size whose tile counts need a second scan level, which moves
    the flag bytes in the scratch."""
    Wd, Hd = TILE * TILE + 1, 1
    rng = np.random.default_rng(50)
    rad = rng.random((Wd * Hd, 2, 3), dtype=F)
    rad[::3, 1] = rad[::3, 0]  # a third: equal samples
    state = rt.afilm_host(Wd, Hd, None, rad, None, 2)["state"]
    with rt.AdaptiveFilm(Wd, Hd) as film:
        film.add(torch.from_numpy(rad).to(DEV), None, 2)
        want = rt.afilm_host(Wd, Hd, state, select=(2, 16, 2, 0.3))["selected"]
        px, n = film.select(2, 16, 2, 0.3)
        assert 0 < n < Wd * Hd and n == want.size
        assert torch.equal(px, torch.from_numpy(want.view(np.int32)).to(DEV))


# ---- whole frames ----------------------------------------------------------------------------------
def device_scene(name):
    hs = host_scene(name + ".json")
    return hs, rt.DeviceScene.from_host(hs, device=0)


# tol = 0.1 was chosen on the CPU with afilm_cases.oracle_adaptive alone (the reference's per-sample
# radiance through the host build), among 0.02, 0.05, 0.1, 0.2, as the value at which both scenes'
# count maps spread most evenly.  At 64x48, min 2 / max 16 / step 2 the oracle model gives
#   sphere_single  {2: 2935, 4: 18, 6: 9, 8: 14, 10: 26, 12: 11, 14: 3, 16: 56}
#   frog           {2: 2958, 4: 6, 6: 3, 8: 2, 10: 2, 12: 3, 14: 2, 16: 96}
DEPTH1_TOL = 0.1
DEPTH1_HIST = {"sphere_single": {2: 2935, 4: 18, 6: 9, 8: 14, 10: 26, 12: 11, 14: 3, 16: 56},
               "frog": {2: 2958, 4: 6, 6: 3, 8: 2, 10: 2, 12: 3, 14: 2, 16: 96}}


@pytest.mark.parametrize("name", ["sphere_single", "frog"])
def test_adaptive_frame_at_depth_1_equals_the_oracle_model(name):
    hs, ds = device_scene(name)
    try:
        cam = hs.camera(64, 48)
        miss = hs.settings["miss_color"]
        want_rgb, want_cnt, want_p6 = ac.oracle_adaptive(hs, cam, 2, 16, 2, DEPTH1_TOL, miss=miss)
        v, c = np.unique(want_cnt, return_counts=True)
        hist = dict(zip(v.tolist(), c.tolist()))
        print(name, "oracle count histogram", hist)
        assert hist == DEPTH1_HIST[name]          # the reference alone meets the condition:
        assert len(hist) >= 3 and 2 in hist and 16 in hist
        rgb, cnt, b = ds.render_adaptive(cam, 2, 16, 2, DEPTH1_TOL, max_depth=1, miss_color=miss, p6=True)
        assert rgb.shape == (48, 64, 3) and cnt.shape == (48, 64) and cnt.dtype == torch.int32
        got_cnt = cnt.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_cnt, want_cnt), int((got_cnt != want_cnt).sum())
        bad = (bits(rgb.cpu().numpy()) != bits(want_rgb)).any(axis=2)
        assert not bad.any(), int(bad.sum())
        assert np.array_equal(b.cpu().numpy(), want_p6)
    finally:
        ds.close()


# With bounces no CPU model of the per-sample radiance exists (the oracle renders whole pixels), so
# this tolerance was chosen from a GPU run of render_adaptive itself: cornell 48x32, depth 3,
# min 2 / max 8 / step 2 gave the count histograms
#   tol 0.02 {2: 148, 4: 1, 8: 1387}            tol 0.05 {2: 252, 4: 9, 6: 1, 8: 1274}
#   tol 0.1  {2: 388, 4: 39, 6: 26, 8: 1083}    tol 0.2  {2: 666, 4: 210, 6: 304, 8: 356}
#   tol 0.3  {2: 913, 4: 469, 6: 152, 8: 2}
# and 0.2 spreads the pixels most evenly.  The check itself is against render() per count.
BOUNCE_TOL = 0.2


def test_adaptive_frame_with_bounces_equals_render_at_each_pixels_count():
    hs, ds = device_scene("cornell")
    try:
        cam = hs.camera(48, 32)
        miss = hs.settings["miss_color"]
        rgb, cnt = ds.render_adaptive(cam, 2, 8, 2, BOUNCE_TOL, max_depth=3, miss_color=miss)
        rgb, cnt = rgb.cpu().numpy(), cnt.cpu().numpy()
        v, c = np.unique(cnt, return_counts=True)
        print("cornell count histogram", dict(zip(v.tolist(), c.tolist())))
        assert len(v) >= 3 and 2 in v and 8 in v and set(v.tolist()) <= {2, 4, 6, 8}
        frames = {}
        for k in v.tolist():
            frames[k] = ds.render(cam, spp=k, max_depth=3, miss_color=miss)
            at = cnt == k
            bad = (bits(rgb)[at] != bits(frames[k])[at]).any(axis=1)
            assert not bad.any(), (k, int(bad.sum()), int(at.sum()))
        # tol = 0: every pixel goes to max_spp, the frame is render's and render_rays'
        full, cnt0, b0 = ds.render_adaptive(cam, 2, 8, 2, 0.0, max_depth=3, miss_color=miss, p6=True)
        assert (cnt0 == 8).all()
        assert np.array_equal(bits(full.cpu().numpy()), bits(frames[8]))
        via_rays, b1 = ds.render_rays(cam, 8, 3, True, miss, p6=True)
        assert torch.equal(full.view(torch.int32), via_rays.view(torch.int32)) and torch.equal(b0, b1)
        # the scene's own materials through the hooks: the same frame
        table = torch.from_numpy(np.ascontiguousarray(hs.materials, F).reshape(-1, 13)).to(DEV)
        seen = []

        def own_materials(hits, rays, ids, depth):
            mi = rt.hit_fields(hits)["material"].long()
            return table[mi.clamp(0, table.shape[0] - 1)]

        def same_rays(rays, seeds, pixels, counts, n):
            assert rays.shape == (pixels.shape[0] * n, 6) and seeds.shape == (rays.shape[0],) and counts.shape == (48 * 32,)
            seen.append((int(pixels.shape[0]), n))
            return rays

        hooked, cnt1 = ds.render_adaptive(cam, 2, 8, 2, BOUNCE_TOL, max_depth=3, miss_color=miss, material_fn=own_materials,
                                          ray_fn=same_rays)
        assert np.array_equal(cnt1.cpu().numpy(), cnt) and np.array_equal(bits(hooked.cpu().numpy()), bits(rgb))
        assert seen[0] == (48 * 32, 2) and all(n == 2 for _, n in seen) and len(seen) >= 3
        assert [m for m, _ in seen[1:]] == [int((cnt >= k).sum()) for k in (4, 6, 8)][:len(seen) - 1]
    finally:
        ds.close()


# ---- beside frames ---------------------------------------------------------------------------------
def test_adaptive_pass_beside_a_renderers_frames():
    """Three frames in flight on a Renderer while an adaptive frame of the same scene is made on a
    stream of its own on the same device: the frames are the frame rendered alone, the adaptive
    frame the one made alone."""
    hs = host_scene("cornell.json")
    cam = hs.camera(64, 48)
    miss = hs.settings["miss_color"]
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=miss)
    rr = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    try:
        kept = rr.render(cam, spp=4, max_depth=1, miss_color=miss).tobytes()
        ds = rr.scene(0)
        alone_rgb, alone_cnt = ds.render_adaptive(cam, 2, 8, 2, BOUNCE_TOL, max_depth=3, miss_color=miss)
        side = torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        tickets = [rr.submit(cam, o) for _ in range(3)]
        with torch.cuda.stream(side):  # the adaptive calls' default stream is torch's current one
            rgb, cnt = ds.render_adaptive(cam, 2, 8, 2, BOUNCE_TOL, max_depth=3, miss_color=miss)
        for k in tickets:
            addr, nb = rr.wait(k)
            assert bytes((C.c_uint8 * nb).from_address(addr)) == kept, k
        assert ds.faults() == 0
        side.synchronize()
        assert torch.equal(cnt, alone_cnt) and torch.equal(rgb.view(torch.int32), alone_rgb.view(torch.int32))
        assert len(torch.unique(cnt)) >= 2
    finally:
        rr.close()
