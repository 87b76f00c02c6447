"""Adaptive sampling (rt_camera_rays_pixels_*, rt_afilm_*), the part that needs no
device: the prefix property of the jitter table, pixel-list camera rays against the sample passes
of the whole frame, the host build of the adaptive film (rt_afilm_host: the functions the kernels
run) against afilm_cases.Model's numpy restatement and against rt_film_pixels_host, the selection
rule and its properties, and every argument check that answers without a device.  All comparisons
are on bit patterns."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import afilm_cases as ac
import film_cases as fc
from conftest import GOLDEN, host_scene
from film_cases import bits

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

F = np.float32
W, H = ac.W_SMALL, ac.H_SMALL
NAMES = ("rt_camera_rays_pixels_host", "rt_camera_rays_pixels_device", "rt_afilm_create", "rt_afilm_destroy",
         "rt_afilm_clear_device", "rt_afilm_counts_device", "rt_afilm_add_device", "rt_afilm_resolve_device",
         "rt_afilm_select_scratch_bytes", "rt_afilm_select_device", "rt_afilm_host")


def test_entry_points_exist():
    lib = L.lib()
    hdr = (GOLDEN.parents[1] / "include" / "rt_mi355x.h").read_text()
    added = hdr[hdr.index("#define RT_ABI_VERSION"):hdr.index("enum {")]
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES and name in added, name
    assert "RT_PIXEL_NONE" in added and "#define RT_PIXEL_NONE 0xFFFFFFFFu" in hdr
    assert callable(rt.AdaptiveFilm) and callable(rt.camera_rays_pixels) and callable(rt.DeviceScene.render_adaptive)
    assert lib.rt_abi_version() == 3
    assert C.sizeof(L.AFilmSelectOpts) == 32


# ---- the prefix property ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 16])
def test_jitter_table_is_a_prefix_of_the_longer_table(k):
    assert rt.jittered_samples(k).tobytes() == rt.jittered_samples(64)[:k].tobytes()


# ---- rays ------------------------------------------------------------------------------------------
def ray_case(seed=3):
    cam = host_scene("frog.json").camera(W, H)
    rng = np.random.default_rng(seed)
    counts = np.array(ac.COUNTS, np.uint32)[rng.integers(0, len(ac.COUNTS), W * H)]
    assert set(counts.tolist()) == set(ac.COUNTS)
    return cam, rng.permutation(W * H).astype(np.uint32), counts


@pytest.mark.parametrize("ns", [1, 3])
def test_pixel_rays_equal_the_pass_rays_of_the_same_pixel(ns):
    cam, pixels, counts = ray_case()
    table = rt.jittered_samples(max(ac.COUNTS) + ns)
    rays, seeds = rt.camera_rays_pixels(cam, pixels, counts, ns, table)
    assert rays.shape == (W * H * ns, 6) and seeds.shape == (W * H * ns,) and seeds.dtype == np.uint32
    rays, seeds = rays.reshape(W * H, ns, 6), seeds.reshape(W * H, ns)
    for c in ac.COUNTS:
        want_r, want_s = rt.camera_rays(cam, ns, table[c:c + ns], sample0=c)
        want_r, want_s = want_r.reshape(W * H, ns, 6), want_s.reshape(W * H, ns)
        k = np.flatnonzero(counts[pixels] == c)
        assert k.size > 0
        assert np.array_equal(bits(rays[k]), bits(want_r[pixels[k]]))
        assert np.array_equal(seeds[k], want_s[pixels[k]])
    # the NULL forms: every pixel in order, no samples yet, the default table
    r0, s0 = rt.camera_rays_pixels(cam, None, None, ns, ns)
    w0, ws0 = rt.camera_rays(cam, ns)
    assert r0.tobytes() == w0.tobytes() and s0.tobytes() == ws0.tobytes()


def test_pixel_rays_outside_the_image_and_past_the_table():
    cam, pixels, counts = ray_case()
    table = rt.jittered_samples(16)
    px = np.array([5, ac.PIXEL_NONE, W * H, W * H - 1], np.uint32)
    rays, seeds = rt.camera_rays_pixels(cam, px, counts, 2, table)
    rays = rays.reshape(4, 2, 6)
    center = np.asarray(cam.basis()["center"], F)
    for k in (1, 2):  # the documented null ray
        assert np.array_equal(bits(rays[k, :, :3]), bits(np.tile(center, (2, 1))))
        assert not bits(rays[k, :, 3:]).any() and not seeds.reshape(4, 2)[k].any()
    assert bits(rays[0, :, 3:]).any() and bits(rays[3, :, 3:]).any()
    # a sample past the table reads the last entry: memory-safe (the result is unspecified)
    far = np.full(W * H, 1000, np.uint32)
    rays, _ = rt.camera_rays_pixels(cam, px[:1], far, 1, table)
    want, _ = rt.camera_rays_pixels(cam, px[:1], np.full(W * H, 15, np.uint32), 1, table)
    assert rays.tobytes() == want.tobytes()


# ---- add and resolve -------------------------------------------------------------------------------
def run_adds(Wd, Hd, adds=ac.ADDS):
    """The same adds through the model and the host build; yields after each."""
    model, state = ac.Model(Wd, Hd), None
    for kind, n, seed in adds:
        px = ac.pixel_list(kind, Wd, Hd, seed)
        rad = ac.list_radiance(Wd * Hd if px is None else px.size, n, seed)
        model.add(px, rad)
        out = rt.afilm_host(Wd, Hd, state, rad, px, n, resolve=True)
        state = out["state"]
        yield model, out


def test_host_add_and_resolve_equal_the_restatement():
    assert sorted({n for _, n, _ in ac.ADDS}) == [1, 2, 3, 5, 16, 17]
    model = None
    for model, out in run_adds(W, H):
        want = model.state()
        for got, w in zip(out["state"], want):
            assert got.tobytes() == w.tobytes()
        assert np.array_equal(bits(out["rgb"]), bits(model.rgb()))
        want_p6 = np.frombuffer(rt.encode_p6(model.rgb())[len(rt.p6_header(W, H)):], np.uint8)
        assert np.array_equal(out["bytes"].reshape(-1), want_p6)
    assert len(set(model.count.tolist())) >= 4  # uneven counts


def test_a_pixel_without_samples_resolves_to_zero():
    px = np.array([3, 7], np.uint32)
    out = rt.afilm_host(W, H, None, ac.list_radiance(2, 2, 1) + F(0.5), px, 2, resolve=True)
    rgb = out["rgb"].reshape(-1, 3)
    rest = np.setdiff1d(np.arange(W * H), px)
    assert not bits(rgb[rest]).any() and not out["bytes"].reshape(-1, 3)[rest].any()
    assert (rgb[px] > 0).all() and out["state"][1].sum() == 4


@pytest.mark.parametrize("n", [1, 5, 16])
def test_dense_equal_counts_are_the_films_pixels(n):
    r = fc.radiance(W, H, n)
    want_sum, want = rt.film_pixels_host(r, W, H, n)
    out = rt.afilm_host(W, H, None, r, None, n, resolve=True)
    assert out["state"][0].tobytes() == want_sum.tobytes()
    assert np.array_equal(bits(out["rgb"]), bits(want))
    assert (out["state"][1] == n).all()


# ---- select ----------------------------------------------------------------------------------------
OPTS = [(2, 16, 2, 0.05, 1e-3), (4, 20, 4, 0.2, 0.25), (2, 8, 1, 0.0, 1e-3), (3, 12, 5, 1.0, 1e-3), (2, 30, 2, 0.02, 0.5)]


@pytest.mark.parametrize("opts", OPTS)
def test_host_select_equals_the_restatement(opts):
    npix = W * H
    count, m1, m2, const = ac.random_accumulators(npix, seed=7)
    state = (np.zeros(npix * 3, F), count.copy(), np.ascontiguousarray(np.stack([m1, m2], axis=1)).reshape(-1))
    got = rt.afilm_host(W, H, state, select=opts)["selected"]
    want = ac.selected(count, m1, m2, *opts)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    mn, mx, step, tol, floor = opts
    sel = np.zeros(npix, bool)
    sel[got] = True
    c = count.astype(np.int64)
    assert (np.diff(got.astype(np.int64)) > 0).all()            # strictly increasing
    assert not sel[c + step > mx].any()                          # never beyond max_samples
    assert sel[(c < mn) & (c + step <= mx)].all()                # always below min_samples
    if tol > 0:
        assert not sel[const & (c >= mn)].any()                  # equal samples are never noisy
    assert 0 < got.size < npix or tol == 0.0


def test_equal_samples_are_never_noisy_and_noise_is():
    """A pixel fed the same sample n times has var 0 up to the float moments' rounding, which the
    max(0, .) and the tolerance absorb; a pixel fed 0 and 1 alternately is noisy at a tolerance its
    standard error exceeds."""
    px = np.array([0, 1], np.uint32)
    state = None
    for n in (2, 3, 5):
        rad = np.zeros((2, n, 3), F)
        rad[0] = F(0.37)
        rad[1, ::2] = F(1.0)
        state = rt.afilm_host(W, H, state, rad, px, n)["state"]
        got = rt.afilm_host(W, H, state, select=(2, 64, 1, 0.05))["selected"]
        assert 0 not in got and 1 in got
        assert np.array_equal(np.sort(got), got) and got.size == W * H - 1  # (the rest has no samples)


# ---- arguments -------------------------------------------------------------------------------------
def test_argument_checks_answer_without_a_device():
    lib = L.lib()
    cam = host_scene("frog.json").camera(W, H)
    cc = C.byref(cam.c)
    px = np.arange(4, dtype=np.uint32)
    rays = np.zeros((W * H * 2, 6), F)
    jit = rt.jittered_samples(4)
    host = lib.rt_camera_rays_pixels_host
    dev = lib.rt_camera_rays_pixels_device
    p = L.ptr
    bad = [
        host(None, p(px), 4, None, 1, p(jit), 4, p(rays), None),       # null camera
        host(cc, p(px), 4, None, 1, p(jit), 4, None, None),            # null rays
        host(cc, p(px), 4, None, 0, p(jit), 4, p(rays), None),         # nsamples < 1
        host(cc, p(px), 4, None, 1, p(jit), 0, p(rays), None),         # table_spp < 1
        host(cc, None, 4, None, 1, p(jit), 4, p(rays), None),          # a null list with m != W * H
        dev(None, p(px), 4, None, 1, p(jit), 4, p(rays), None, 0, None),
        dev(cc, p(px), 4, None, 1, p(jit), 4, None, None, 0, None),
        dev(cc, p(px), 4, None, 1, None, 4, p(rays), None, 0, None),   # null jitter on the device
        dev(cc, p(px), 4, None, 0, p(jit), 4, p(rays), None, 0, None),
        dev(cc, p(px), 4, None, 1, p(jit), -1, p(rays), None, 0, None),
    ]
    assert bad == [-1] * len(bad), bad
    assert host(cc, p(px), 1 << 30, None, 2, p(jit), 4, p(rays), None) == -7      # m * nsamples > 2^31-1
    assert dev(cc, p(px), 1 << 30, None, 2, p(jit), 4, p(rays), None, 0, None) == -7
    assert host(cc, p(px), 0, None, 2, p(jit), 4, p(rays), None) == 0             # m == 0: nothing to do
    assert dev(cc, p(px), 0, None, 2, p(jit), 4, p(rays), None, 0, None) == 0
    assert host(cc, None, W * H, None, 2, None, 4, p(rays), None) == 0            # the NULL forms

    h = C.c_void_p()
    assert lib.rt_afilm_create(0, 0, 4, C.byref(h)) == -1 and lib.rt_afilm_create(0, 4, -1, C.byref(h)) == -1
    assert lib.rt_afilm_create(0, 4, 4, None) == -1
    assert lib.rt_afilm_create(0, 1 << 16, 1 << 16, C.byref(h)) == -7 and not h
    o = L.AFilmSelectOpts(2, 16, 2, 0.1, 1e-3)
    nul = [
        lib.rt_afilm_clear_device(None, None),
        lib.rt_afilm_add_device(None, None, 0, p(rays), 1, None),
        lib.rt_afilm_resolve_device(None, 0, 1, p(rays), None, None, None),
        lib.rt_afilm_select_device(None, C.byref(o), p(px), p(px), p(px), None),
    ]
    assert nul == [-1] * len(nul), nul
    assert lib.rt_afilm_counts_device(None) is None and lib.rt_afilm_select_scratch_bytes(None) == 0
    lib.rt_afilm_destroy(None)

    s, c, m = np.zeros(W * H * 3, F), np.zeros(W * H, np.uint32), np.zeros(W * H * 2, F)
    rad = np.zeros(W * H * 3 * 2, F)
    sel, n = np.zeros(W * H, np.uint32), C.c_uint32()
    ah = lib.rt_afilm_host

    def select_rc(*fields):
        return ah(W, H, p(s), p(c), p(m), None, 0, None, 1, None, None, C.byref(L.AFilmSelectOpts(*fields)), p(sel), C.byref(n))

    bad = [
        ah(0, H, p(s), p(c), p(m), None, 0, None, 1, None, None, None, None, None),
        ah(W, H, None, p(c), p(m), None, 0, None, 1, None, None, None, None, None),
        ah(W, H, p(s), None, p(m), None, 0, None, 1, None, None, None, None, None),
        ah(W, H, p(s), p(c), None, None, 0, None, 1, None, None, None, None, None),
        ah(W, H, p(s), p(c), p(m), p(px), 4, p(rad), 0, None, None, None, None, None),   # nsamples < 1
        ah(W, H, p(s), p(c), p(m), None, 4, p(rad), 1, None, None, None, None, None),    # null list, m != W * H
        select_rc(1, 16, 2, 0.1, 1e-3),      # min_samples < 2
        select_rc(2, 16, 0, 0.1, 1e-3),      # step < 1
        select_rc(2, 16, 2, -0.1, 1e-3),     # tol < 0
        select_rc(2, 16, 2, float("nan"), 1e-3),
        select_rc(2, 16, 2, 0.1, 0.0),       # floor <= 0
        select_rc(2, 16, 2, 0.1, float("nan")),
        ah(W, H, p(s), p(c), p(m), None, 0, None, 1, None, None, C.byref(o), None, C.byref(n)),  # null pixels_out
        ah(W, H, p(s), p(c), p(m), None, 0, None, 1, None, None, C.byref(o), p(sel), None),
    ]
    assert bad == [-1] * len(bad), bad
    assert ah(W, H, p(s), p(c), p(m), p(px), 1 << 30, p(rad), 2, None, None, None, None, None) == -7
    assert ah(1 << 16, 1 << 16, p(s), p(c), p(m), None, 0, None, 1, None, None, None, None, None) == -7
    assert not c.any() and not s.any()       # a refused call adds nothing
    assert select_rc(2, 16, 2, 0.0, 1e-3) == 0 and n.value == W * H   # no samples: everything selected
    assert select_rc(2, 1, 2, 0.0, 1e-3) == 0 and n.value == 0        # max_samples below the step: nothing
    for name in ("min_spp", "step"):
        with pytest.raises(ValueError):
            rt.DeviceScene.render_adaptive(None, cam, **{"min_spp": 2, "max_spp": 8, "step_spp": 2, "tol": 0.1,
                                                         **({"min_spp": 1} if name == "min_spp" else {"step_spp": 0})})
