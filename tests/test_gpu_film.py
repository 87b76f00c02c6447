"""The film on the GPU (rt_film_*, rt_camera_rays_pass_device, DeviceScene.render_rays; DESIGN.md
§4.20), bit for bit (no tolerance):

* film_add_* / film_resolve_* against the host build (rt_film_pixels_host, pinned on the CPU by
  tests/test_film_host.py): whole images and a band, aligned and unaligned radiance and outputs,
  guard bytes around every output, rows outside the band unchanged;
* sample passes against the one-shot result, resolve between passes, clear and re-add;
* row counts, and every argument check that needs a film;
* camera-ray passes made on the device against the host build;
* frames through render_rays, in passes and bands, against the reference's golden frames and P6
  image and against DeviceScene.render;
* a film on a second stream beside a Renderer's frames.
"""
from __future__ import annotations

import ctypes as C
import gzip

import numpy as np
import pytest
import torch

import film_cases as fc
from conftest import GOLDEN, golden_array, golden_meta, hexv, host_scene
from film_cases import bits

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

F = np.float32
DEV = torch.device("cuda", 0)
PAD = 32  # guard bytes on each side of an output


def p6_body(rgb):
    """write_p6's bytes of (rows, W, 3) float pixels, header dropped."""
    rows, W = rgb.shape[0], rgb.shape[1]
    return np.frombuffer(rt.encode_p6(rgb)[len(rt.p6_header(W, rows)):], np.uint8)


def upload(r, offset_floats=0):
    """(tensor kept alive, device address) of a float array placed offset_floats floats into an
    allocation: 0 keeps the allocator's alignment, 1 leaves the address 4 bytes off it."""
    flat = np.ascontiguousarray(r, F).reshape(-1)
    t = torch.zeros(flat.size + 8, dtype=torch.float32, device=DEV)
    t[offset_floats:offset_floats + flat.size] = torch.from_numpy(flat.copy()).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * offset_floats


class Guarded:
    """nbytes of output behind and before PAD bytes of 0xFF, `off` bytes past a 16-byte boundary."""

    def __init__(self, nbytes, off):
        self.t = torch.full((2 * PAD + nbytes + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        assert self.t.data_ptr() % 16 == 0
        self.start, self.n = PAD + off, nbytes
        self.ptr = self.t.data_ptr() + self.start

    def read(self, dtype):
        h = self.t.cpu().numpy()
        assert (h[:self.start] == 0xFF).all() and (h[self.start + self.n:] == 0xFF).all(), "guard bytes were written"
        return h[self.start:self.start + self.n].copy().view(dtype)

    def untouched(self):
        return bool((self.t == 0xFF).all().item())


def raw_add(film, ptr, row0, rows, n):
    return L.lib().rt_film_add_device(film._h, ptr, row0, rows, n, None)


def resolve_check(film, row0, rows, want_rgb, off_rgb, off_p6):
    """rt_film_resolve_device into guarded outputs at the given misalignments: both outputs, then
    each alone."""
    W = film.width
    n = rows * W * 3
    want_p6 = p6_body(want_rgb)
    for use_rgb, use_p6 in ((True, True), (True, False), (False, True)):
        g_rgb, g_p6 = Guarded(4 * n, off_rgb), Guarded(n, off_p6)
        rc = L.lib().rt_film_resolve_device(film._h, row0, rows, g_rgb.ptr if use_rgb else None,
                                            g_p6.ptr if use_p6 else None, None)
        assert rc == 0, L.lib().rt_last_error()
        torch.cuda.synchronize(DEV)
        if use_rgb:
            got = g_rgb.read(np.uint32)
            assert np.array_equal(got, bits(want_rgb).reshape(-1)), int((got != bits(want_rgb).reshape(-1)).sum())
        else:
            assert g_rgb.untouched()
        if use_p6:
            assert np.array_equal(g_p6.read(np.uint8), want_p6)
        else:
            assert g_p6.untouched()


SHAPES = [(fc.W_SMALL, fc.H_SMALL), (256, 9)]  # (256: every block's span is whole 16-byte vectors)
BAND = (3, 2)


@pytest.mark.parametrize("rad_off", [0, 1], ids=["aligned", "plus4bytes"])
@pytest.mark.parametrize("n", fc.NS_GPU)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_add_and_resolve_equal_the_host_build(shape, n, rad_off):
    W, H = shape
    r = fc.radiance(W, H, n)
    want_sum, want = rt.film_pixels_host(r, W, H, n)
    with rt.Film(W, H) as film:
        # the whole image
        keep, ptr = upload(r, rad_off)
        assert ptr % 16 == 4 * rad_off
        assert raw_add(film, ptr, 0, H, n) == 0, L.lib().rt_last_error()
        assert [film.row_samples(y) for y in range(H)] == [n] * H
        for off_rgb, off_p6 in ((0, 0), (4, 1)):  # aligned, then one element off
            resolve_check(film, 0, H, want, off_rgb, off_p6)
        # a band over a film that already holds one sample per pixel
        film.clear()
        base = fc.radiance(W, H, 1, seed=2)
        keep0, ptr0 = upload(base)
        assert raw_add(film, ptr0, 0, H, 1) == 0
        row0, rows = BAND
        keep1, ptr1 = upload(r[row0:row0 + rows], rad_off)
        assert raw_add(film, ptr1, row0, rows, n) == 0
        assert [film.row_samples(y) for y in range(H)] == [1 + n if row0 <= y < row0 + rows else 1 for y in range(H)]
        sums = np.ascontiguousarray(base[:, :, 0, :]).copy()  # (0 + x: the sums of one sample are the samples)
        band_sum, band = rt.film_pixels_host(r[row0:row0 + rows], W, rows, n, np.ascontiguousarray(sums[row0:row0 + rows]),
                                             count_after=1 + n)
        for off_rgb, off_p6 in ((0, 0), (4, 1)):
            resolve_check(film, row0, rows, band, off_rgb, off_p6)
        # the rows around the band still hold their one sample (count 1: the pixel is the sum)
        resolve_check(film, 0, row0, sums[:row0], 0, 0)
        resolve_check(film, row0 + rows, H - row0 - rows, sums[row0 + rows:], 4, 1)
        torch.cuda.synchronize(DEV)
        del keep, keep0, keep1


def test_api_add_and_resolve():
    """Film.add / resolve on tensors: shapes, dtypes, the default rows and nsamples."""
    W, H, n = fc.W_SMALL, fc.H_SMALL, 5
    r = fc.radiance(W, H, n)
    _, want = rt.film_pixels_host(r, W, H, n)
    with rt.Film(W, H) as film:
        film.add(torch.from_numpy(r.copy()).to(DEV))
        rgb, b = film.resolve(p6=True)
        assert rgb.shape == (H, W, 3) and rgb.dtype == torch.float32 and b.shape == (H, W, 3) and b.dtype == torch.uint8
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(want))
        assert np.array_equal(b.cpu().numpy().reshape(-1), p6_body(want))
        band = film.resolve(2, 3)
        assert np.array_equal(bits(band.cpu().numpy()), bits(want[2:5]))
        with pytest.raises(ValueError):
            film.add(torch.zeros(7, dtype=torch.float32, device=DEV))
        with pytest.raises(ValueError):
            film.add(torch.from_numpy(r.copy()))  # a host tensor
    with pytest.raises(rt.RTError):
        film.row_samples(0)  # closed


# ---- passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(5, 11), (3, 5, 8)])
def test_passes_give_the_one_shot_result(split):
    W, H, n = fc.W_SMALL, fc.H_SMALL, 16
    r = fc.radiance(W, H, n)
    _, want = rt.film_pixels_host(r, W, H, n)
    dev_r = torch.from_numpy(r.copy()).to(DEV)
    with rt.Film(W, H) as film:
        film.add(dev_r, nsamples=n)
        one_shot = film.resolve().cpu().numpy()
        assert np.array_equal(bits(one_shot), bits(want))
        for again in range(2):  # clear, then the same result from passes
            film.clear()
            assert film.row_samples(H - 1) == 0
            s0, sums = 0, None
            for k in split:
                film.add(dev_r[:, :, s0:s0 + k].contiguous(), nsamples=k)
                sums, part = rt.film_pixels_host(np.ascontiguousarray(r[:, :, s0:s0 + k]), W, H, k, sums, count_after=s0 + k)
                s0 += k
                # resolved after every pass (progressive display): the pixels so far, the sums undisturbed
                assert np.array_equal(bits(film.resolve().cpu().numpy()), bits(part))
                assert film.row_samples(0) == s0
            rgb, b = film.resolve(p6=True)
            assert np.array_equal(bits(rgb.cpu().numpy()), bits(one_shot))
            assert np.array_equal(b.cpu().numpy().reshape(-1), p6_body(want))


# ---- counts and argument checks ------------------------------------------------------------------
def test_counts_and_argument_checks():
    W, H = fc.W_SMALL, fc.H_SMALL
    lib = L.lib()
    with rt.Film(W, H) as film:
        keep, ptr = upload(fc.radiance(W, H, 3))
        out = Guarded(4 * H * W * 3, 0)
        # no samples yet
        assert lib.rt_film_resolve_device(film._h, 0, H, out.ptr, None, None) == -1 and lib.rt_last_error()
        assert raw_add(film, ptr, 0, 3, 2) == 0 and raw_add(film, ptr, 3, H - 3, 3) == 0
        assert [film.row_samples(y) for y in range(H)] == [2, 2, 2] + [3] * (H - 3)
        out_p6 = Guarded(H * W * 3, 0)
        assert lib.rt_film_resolve_device(film._h, 0, H, out.ptr, out_p6.ptr, None) == -1  # unequal counts
        assert lib.rt_film_resolve_device(film._h, 2, 2, out.ptr, None, None) == -1
        torch.cuda.synchronize(DEV)
        assert out.untouched() and out_p6.untouched()  # a refused resolve writes nothing
        assert lib.rt_film_resolve_device(film._h, 0, 3, out.ptr, None, None) == 0  # (equal ones are fine)
        out2 = Guarded(4 * H * W * 3, 0)
        cases = [
            raw_add(film, None, 0, 1, 1),           # null radiance
            raw_add(film, ptr, 0, 1, 0),            # nsamples < 1
            raw_add(film, ptr, 0, 1, -3),
            raw_add(film, ptr, -1, 1, 1),           # rows outside the image
            raw_add(film, ptr, 0, H + 1, 1),
            raw_add(film, ptr, H, 1, 1),
            raw_add(film, ptr, 0, -1, 1),
            lib.rt_film_resolve_device(film._h, 0, 3, None, None, None),  # both outputs null
            lib.rt_film_resolve_device(film._h, -1, 1, out2.ptr, None, None),
            lib.rt_film_resolve_device(film._h, 3, H, out2.ptr, None, None),
        ]
        assert cases == [-1] * len(cases), cases
        assert raw_add(film, ptr, 0, H, 6_000_000) == -7  # W * rows * nsamples > 2^31-1
        assert raw_add(film, ptr, 2, 0, 4) == 0 and lib.rt_film_resolve_device(film._h, 2, 0, out2.ptr, None, None) == 0
        n = C.c_int64()
        assert lib.rt_film_row_samples(film._h, H, C.byref(n)) == -1 and lib.rt_film_row_samples(film._h, -1, C.byref(n)) == -1
        assert lib.rt_film_row_samples(film._h, 0, None) == -1
        torch.cuda.synchronize(DEV)
        assert out2.untouched()
        assert [film.row_samples(y) for y in range(H)] == [2, 2, 2] + [3] * (H - 3)  # a refused call counts nothing
        del keep
    h = C.c_void_p()
    assert lib.rt_film_create(99, W, H, C.byref(h)) == -1 and not h  # no such device


# ---- camera-ray passes ----------------------------------------------------------------------------
@pytest.mark.parametrize("sample0", [0, 5])
def test_camera_ray_passes_device_equals_host(sample0):
    cam = host_scene("frog.json").camera(37, 11)
    row0, rows, n = 3, 5, 11
    jit = rt.jittered_samples(sample0 + n)[sample0:]
    want_r, want_s = rt.camera_rays(cam, n, jit, row0, rows, sample0=sample0)
    rays, seeds = rt.camera_rays(cam, n, jit, row0, rows, device=0, sample0=sample0)
    assert rays.shape == (37 * rows * n, 6) and seeds.dtype == torch.int32
    assert rays.cpu().numpy().tobytes() == want_r.tobytes()
    assert seeds.cpu().numpy().view(np.uint32).tobytes() == want_s.tobytes()
    # the raw entry into a guarded buffer
    jd = torch.from_numpy(np.ascontiguousarray(jit)).to(DEV)
    g_r, g_s = Guarded(want_r.nbytes, 0), Guarded(want_s.nbytes, 0)
    assert L.lib().rt_camera_rays_pass_device(0, C.byref(cam.c), sample0, n, jd.data_ptr(), row0, rows, g_r.ptr, g_s.ptr,
                                              None) == 0
    torch.cuda.synchronize(DEV)
    assert g_r.read(np.uint8).tobytes() == want_r.tobytes() and g_s.read(np.uint8).tobytes() == want_s.tobytes()


# ---- frames ------------------------------------------------------------------------------------
def _golden(name):
    m = golden_meta(name)
    W, H = m["width"], m["height"]
    hs = host_scene({"c3_small": "frog", "frog_bounce": "frog", "cornell": "cornell"}[name] + ".json")
    cam = hs.camera(W, H)
    b = cam.basis()
    for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"):  # the golden frame's own camera
        assert np.array_equal(bits(b[k]), bits(hexv(m[k]))), (name, k)
    fb = golden_array(name, "fb.f32.gz", F).reshape(H, W, 3)
    return hs, cam, m["spp"], m["max_depth"], bool(m["diffuse_bounce"]), tuple(float(v) for v in hexv(m["miss_color"])), fb


# name -> (pass_spp, band_rows): at least two passes and two bands, neither dividing evenly
FRAMES = {"cornell": (3, 50), "frog_bounce": (3, 32), "c3_small": (5, 40)}


@pytest.mark.parametrize("name", list(FRAMES))
def test_render_rays_gives_the_golden_frame(name):
    hs, cam, spp, depth, diffuse, miss, fb = _golden(name)
    pass_spp, band_rows = FRAMES[name]
    assert depth == {"cornell": 3, "frog_bounce": 8, "c3_small": 1}[name]
    assert -(-spp // pass_spp) >= 2 and -(-cam.pixel_height // band_rows) >= 2
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        rgb, b = ds.render_rays(cam, spp, depth, diffuse, miss, pass_spp=pass_spp, band_rows=band_rows, p6=True)
        got = rgb.cpu().numpy()
        bad = (bits(got) != bits(fb)).any(axis=2)
        assert not bad.any(), (int(bad.sum()), float(np.abs(got - fb).max()))
        assert np.array_equal(b.cpu().numpy().reshape(-1), p6_body(fb))
        # one pass, one band
        whole = ds.render_rays(cam, spp, depth, diffuse, miss)
        assert np.array_equal(bits(whole.cpu().numpy()), bits(fb))
        if name == "c3_small":
            frame = ds.render(cam, spp=spp, max_depth=depth, diffuse_bounce=diffuse, miss_color=miss)
            assert np.array_equal(bits(got), bits(frame))
            ref = gzip.open(GOLDEN / "scenes" / name / "image.ppm.gz").read()
            assert b.cpu().numpy().tobytes() == ref[len(rt.p6_header(cam.pixel_width, cam.pixel_height)):]
        if name == "frog_bounce":
            steps = []

            def same_rays(rays, seeds, row0, rows, sample0, n):
                assert rays.shape == (cam.pixel_width * rows * n, 6) and seeds.shape == (rays.shape[0],)
                steps.append((row0, rows, sample0, n))
                return rays

            with rt.Film(cam.pixel_width, cam.pixel_height) as film:
                hooked = ds.render_rays(cam, spp, depth, diffuse, miss, pass_spp=pass_spp, band_rows=band_rows,
                                        ray_fn=same_rays, film=film)
                assert film.row_samples(0) == spp  # the caller's film was used and left open
            assert np.array_equal(bits(hooked.cpu().numpy()), bits(fb))
            assert steps == [(r0, min(band_rows, 54 - r0), s0, min(pass_spp, spp - s0))
                             for s0 in range(0, spp, pass_spp) for r0 in range(0, 54, band_rows)]
    finally:
        ds.close()


# ---- beside frames -------------------------------------------------------------------------------
def test_film_beside_a_renderers_frames():
    """Three frames in flight on a Renderer while a film adds and resolves on a stream of its own on
    the same device: the frames are the frame rendered alone, the film's pixels the host build's."""
    hs = host_scene("cornell.json")
    cam = hs.camera(64, 48)
    W, H, n = fc.W_SMALL, fc.H_SMALL, 16
    r = fc.radiance(W, H, n)
    _, want = rt.film_pixels_host(r, W, H, n)
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=hs.settings["miss_color"])
    rr = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    film = rt.Film(W, H)
    try:
        kept = rr.render(cam, spp=4, max_depth=1, miss_color=hs.settings["miss_color"]).tobytes()
        dev_r = torch.from_numpy(r.copy()).to(DEV)
        side = torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        tickets = [rr.submit(cam, o) for _ in range(3)]
        with torch.cuda.stream(side):  # Film's default stream is torch's current one
            film.add(dev_r[:, :, :5].contiguous(), nsamples=5)
            film.add(dev_r[:, :, 5:].contiguous(), nsamples=11)
            rgb, b = film.resolve(p6=True)
        for k in tickets:
            addr, nb = rr.wait(k)
            assert bytes((C.c_uint8 * nb).from_address(addr)) == kept, k
        assert rr.scene(0).faults() == 0
        side.synchronize()
        assert np.array_equal(bits(rgb.cpu().numpy()), bits(want))
        assert np.array_equal(b.cpu().numpy().reshape(-1), p6_body(want))
    finally:
        film.close()
        rr.close()
