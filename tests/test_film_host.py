"""The film (rt_film_*, rt_camera_rays_pass_*), the part that needs no device: the
host build of the film's arithmetic (rt_film_pixels_host: the functions the kernels run) against
shade_rays_cases.pixel_sum's restatement of render()'s pixel and against the reference's own golden
frame and P6 image, sample passes against the one-shot sums, camera-ray passes against the whole
frame's rays, and every argument check that answers without a device.  All comparisons are on bit
patterns."""
from __future__ import annotations

import ctypes as C
import gzip

import numpy as np
import pytest

import film_cases as fc
import ray_batches as rb
import shade_rays_cases as sc
from conftest import GOLDEN, golden_array, golden_meta, hexv, host_scene
from film_cases import bits

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L
from oracle import pyoracle as orc

F = np.float32
W, ROWS = fc.W_SMALL, fc.H_SMALL


def test_entry_points_exist():
    lib = L.lib()
    for name in ("rt_film_create", "rt_film_destroy", "rt_film_clear_device", "rt_film_add_device",
                 "rt_film_resolve_device", "rt_film_row_samples", "rt_film_pixels_host", "rt_camera_rays_pass_host",
                 "rt_camera_rays_pass_device"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert callable(rt.Film) and callable(rt.film_pixels_host) and callable(rt.DeviceScene.render_rays)
    assert lib.rt_abi_version() == 3
    hdr = (GOLDEN.parents[1] / "include" / "rt_mi355x.h").read_text()
    added = hdr[hdr.index("#define RT_ABI_VERSION"):hdr.index("enum {")]
    for name in ("rt_film_create", "rt_film_pixels_host", "rt_camera_rays_pass_device"):
        assert name in added, name  # the "added since" list of RT_ABI_VERSION


# ---- random frames -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", fc.NS_HOST)
def test_host_film_equals_pixel_sum(n):
    r = fc.radiance(W, ROWS, n)
    assert (r == 0).sum() >= 16 and (r == 1).sum() >= 16
    assert ((r > 0) & (r < np.finfo(F).tiny)).sum() >= 4  # subnormals
    want_sum, want = fc.reference(r)
    sums, rgb = rt.film_pixels_host(r, W, ROWS, n)
    assert sums.shape == rgb.shape == (ROWS, W, 3)
    assert np.array_equal(bits(sums), bits(want_sum))
    assert np.array_equal(bits(rgb), bits(want))
    # the order is pinned: the same samples added last to first are another frame
    _, rev = fc.reference(np.ascontiguousarray(r[:, :, ::-1]))
    differ = int((bits(rev) != bits(want)).any(axis=2).sum())
    print(f"n = {n}: {differ} of {ROWS * W} pixels change under the reversed order")
    if n >= 3:  # (one sample, or two: a + b is b + a)
        assert differ >= 16
        for seed in range(1, fc.SEEDS[n]):  # the first seed that meets it
            _, a = fc.reference(fc.make_radiance(W, ROWS, n, seed))
            _, b = fc.reference(np.ascontiguousarray(fc.make_radiance(W, ROWS, n, seed)[:, :, ::-1]))
            assert int((bits(a) != bits(b)).any(axis=2).sum()) < 16
    else:
        assert differ == 0


def test_pixel_is_the_double_quotient_of_the_float_count():
    """float(double(sum) / double(float(count))) for counts that are no power of two."""
    s = np.array([[[0.1, 1.0, 2.5]]], F)
    for count in (1, 3, 7, 16, 17, 1000):
        sums = s.copy()
        _, rgb = rt.film_pixels_host(np.zeros((1, 1, 1, 3), F), 1, 1, 1, sums, count_after=count)
        assert np.array_equal(bits(sums), bits(s))  # + 0.0f
        assert np.array_equal(bits(rgb), bits((s.astype(np.float64) / np.float64(F(count))).astype(F)))


# ---- passes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(1, 15), (4, 4, 4, 4), (3, 5, 8)])
def test_sample_passes_give_the_one_shot_frame(split):
    n = sum(split)
    assert n == 16
    r = fc.radiance(W, ROWS, n)
    want_sum, want = fc.reference(r)
    sums, rgb, s0 = None, None, 0
    for k in split:
        part = np.ascontiguousarray(r[:, :, s0:s0 + k])
        sums, rgb = rt.film_pixels_host(part, W, ROWS, k, sums, count_after=s0 + k)
        s0 += k
        assert np.array_equal(bits(sums), bits(fc.pixel_sums(r[:, :, :s0])))  # resolvable after every pass
        assert np.array_equal(bits(rgb), bits(sc.pixel_sum(np.ascontiguousarray(r[:, :, :s0]), ROWS, W, s0)))
    assert np.array_equal(bits(sums), bits(want_sum)) and np.array_equal(bits(rgb), bits(want))


# ---- the reference's own frame -------------------------------------------------------------------
def _c3_small():
    """c3_small's camera and the oracle's radiance of every sample, (H, W, spp, 3).

    Depth 1 reads no seed, so a sample's radiance is a function of its ray alone.  The whole table
    is made by one oracle render per sample s with spp = 1 and the one-entry jitter table
    [jitter[s]]: its pixel is col / float(1) = TraceRayIterative of sample s's ray.  Every 97th ray
    is also shaded by shade_rays_cases.oracle_shade, as tests/test_shade_rays_host.py makes its
    radiances, and must give the same bits (the whole table that way is 332k one-pixel renders)."""
    m = golden_meta("c3_small")
    Wc, Hc, spp = m["width"], m["height"], m["spp"]
    assert m["max_depth"] == 1 and spp == 16
    cam = host_scene("frog.json").camera(Wc, Hc)
    b = cam.basis()
    for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"):
        assert np.array_equal(bits(b[k]), bits(hexv(m[k]))), k
    a = rb.scene_arrays("frog")
    miss = tuple(float(v) for v in hexv(m["miss_color"]))
    oc = orc.camera_from_basis(b["center"], b["pixel00_loc"], b["pixel_delta_u"], b["pixel_delta_v"], Wc, Hc)
    jit = orc.jitter(spp)
    rad = np.zeros((Hc, Wc, spp, 3), F)
    for s in range(spp):
        rad[:, :, s] = orc.render_g(a["P"], oc, a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"],
                                    spp=1, max_depth=1, diffuse_bounce=bool(m["diffuse_bounce"]), miss=miss,
                                    jitter_tab=jit[s:s + 1])
    rays, _, pix = sc.camera_rays(b, Wc, Hc, jit, targets=True)
    flat = rad.reshape(-1, 3)
    for i in range(0, flat.shape[0], 97):
        one, _, _ = sc.oracle_shade(a, rays[i, :3], pix[i], 0, 0, 1, bool(m["diffuse_bounce"]), miss)
        assert np.array_equal(bits(one), bits(flat[i])), i
    return Wc, Hc, spp, rad


def test_golden_frame_and_p6_through_the_film():
    """The oracle's per-sample radiances of c3_small through the host film are the reference's
    framebuffer, and its pixels through encode_p6 are the reference's P6 image; in one add and in
    two passes."""
    Wc, Hc, spp, rad = _c3_small()
    fb = golden_array("c3_small", "fb.f32.gz", F).reshape(Hc, Wc, 3)
    _, rgb = rt.film_pixels_host(rad, Wc, Hc, spp)
    assert np.array_equal(bits(rgb), bits(fb))
    assert (fb > 0).any() and (fb == 0).any()
    sums, _ = rt.film_pixels_host(np.ascontiguousarray(rad[:, :, :5]), Wc, Hc, 5)
    _, rgb2 = rt.film_pixels_host(np.ascontiguousarray(rad[:, :, 5:]), Wc, Hc, spp - 5, sums, count_after=spp)
    assert np.array_equal(bits(rgb2), bits(fb))
    ref = gzip.open(GOLDEN / "scenes" / "c3_small" / "image.ppm.gz").read()
    head = rt.p6_header(Wc, Hc)
    assert ref.startswith(head) and len(ref) == len(head) + Wc * Hc * 3
    assert rt.encode_p6(rgb)[len(head):] == ref[len(head):]


# ---- camera-ray passes ----------------------------------------------------------------------------
def _camera():
    return host_scene("frog.json").camera(37, 11)


def _raw_pass(cam, sample0, n, jit, row0, rows):
    Wc = cam.pixel_width
    rays = np.zeros((Wc * rows * n, 6), F)
    seeds = np.zeros(Wc * rows * n, np.uint32)
    rc = L.lib().rt_camera_rays_pass_host(C.byref(cam.c), sample0, n, jit.ctypes.data, row0, rows, rays.ctypes.data,
                                          seeds.ctypes.data)
    assert rc == 0, L.lib().rt_last_error()
    return rays, seeds


def test_camera_pass_from_sample_0_is_the_existing_call():
    cam = _camera()
    jit = rt.jittered_samples(5)
    for row0, rows in ((0, 11), (3, 5)):
        want_r, want_s = rt.camera_rays(cam, 5, jit, row0, rows)
        got_r, got_s = _raw_pass(cam, 0, 5, jit.reshape(-1), row0, rows)
        assert got_r.tobytes() == want_r.tobytes() and got_s.tobytes() == want_s.tobytes()
    # a null table is the default one, as in rt_camera_rays_host
    rays = np.zeros((37 * 11 * 5, 6), F)
    assert L.lib().rt_camera_rays_pass_host(C.byref(cam.c), 0, 5, None, 0, 11, rays.ctypes.data, None) == 0
    assert rays.tobytes() == rt.camera_rays(cam, 5)[0].tobytes()


def test_camera_passes_interleave_to_the_whole_frame():
    cam = _camera()
    Wc, rows, row0, spp = 37, 5, 3, 16
    jit = rt.jittered_samples(spp)
    want_r, want_s = rt.camera_rays(cam, spp, jit, row0, rows)
    a_r, a_s = rt.camera_rays(cam, 5, jit[:5], row0, rows, sample0=0)
    b_r, b_s = rt.camera_rays(cam, 11, jit[5:], row0, rows, sample0=5)
    got_r = np.concatenate([a_r.reshape(rows, Wc, 5, 6), b_r.reshape(rows, Wc, 11, 6)], axis=2).reshape(-1, 6)
    got_s = np.concatenate([a_s.reshape(rows, Wc, 5), b_s.reshape(rows, Wc, 11)], axis=2).reshape(-1)
    assert got_r.tobytes() == want_r.tobytes() and got_s.tobytes() == want_s.tobytes()
    assert np.array_equal(b_s.reshape(rows, Wc, 11)[2, 30], sc.make_rng_seed(30, row0 + 2, np.arange(5, 16)))
    assert not np.array_equal(b_s, rt.camera_rays(cam, 11, jit[5:], row0, rows)[1])  # (the seeds do move)


def test_cpp_wrappers(tmp_path):
    """rt::film_pixels_host and rt::camera_rays_pass of include/rt_mi355x.hpp (a stand-alone program
    linked against the library) give the C entries' bits; the header compiles without warnings."""
    import subprocess

    from conftest import REPO
    from raytracinginonesemester_amd import build as B

    exe = tmp_path / "film_hpp_main"
    subprocess.run([B.CXX, "-std=c++17", "-O1", *B.FP, "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'include'}",
                    str(REPO / "tests" / "native" / "film_hpp_main.cpp"), "-o", str(exe), f"-L{L.LIB_PATH.parent}",
                    "-lrt_mi355x", f"-Wl,-rpath,{L.LIB_PATH.parent}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    film, rays, refused = r.stdout.split("--\n")
    Wf, rows, n = 5, 3, 7
    i, s = np.meshgrid(np.arange(Wf * rows * 3), np.arange(n), indexing="ij")
    table = (((i * 37 + s * 101) % 256).astype(F) / F(255.0)).reshape(rows, Wf, 3, n).transpose(0, 1, 3, 2)
    want_sum, want = fc.reference(np.ascontiguousarray(table))
    words = np.array([[int(w, 16) for w in line.split()] for line in film.splitlines()], np.uint32)
    assert np.array_equal(words[:, 0], bits(want_sum).reshape(-1)) and np.array_equal(words[:, 1], bits(want).reshape(-1))
    cam = rt.Camera((0.5, 1.0, 4.0), (0.0, 0.5, 0.0), (0.0, 1.0, 0.0), 35.0, 24.0, 9, 6)
    want_r, want_s = rt.camera_rays(cam, 2, np.array([[0.25, -0.125], [-0.375, 0.5]], F), 2, 3, sample0=3)
    words = np.array([[int(w, 16) for w in line.split()] for line in rays.splitlines()], np.uint32)
    assert words.shape == (9 * 3 * 2, 7)
    assert np.array_equal(words[:, :6], want_r.view(np.uint32)) and np.array_equal(words[:, 6], want_s)
    assert refused.strip() == "-1"  # rt::Film(0, 4): RT_ERR_ARG as an rt::Error


# ---- argument checks -----------------------------------------------------------------------------
_BUF = np.zeros(4096, F)
_P = _BUF.ctypes.data
_FILM = C.c_void_p()
_CAM = _camera()
_CP = C.addressof(_CAM.c)


def _fresh():
    _BUF[:] = 0
    L.lib().rt_last_error()


def test_film_calls_refuse_a_null_film_without_a_device():
    lib = L.lib()
    n = C.c_int64(-5)
    assert lib.rt_film_add_device(None, _P, 0, 1, 1, None) == -1 and lib.rt_last_error()
    assert lib.rt_film_add_device(None, None, 0, 1, 1, None) == -1
    assert lib.rt_film_resolve_device(None, 0, 1, _P, _P, None) == -1 and lib.rt_last_error()
    assert lib.rt_film_clear_device(None, None) == -1 and lib.rt_last_error()
    assert lib.rt_film_row_samples(None, 0, C.byref(n)) == -1 and n.value == -5
    lib.rt_film_destroy(None)
    assert not _BUF.any()


def test_film_create_checks_its_arguments_first():
    lib = L.lib()
    h = C.c_void_p(1)
    assert lib.rt_film_create(0, 0, 4, C.byref(h)) == -1 and not h
    assert lib.rt_film_create(0, 4, -1, C.byref(h)) == -1 and not h
    assert lib.rt_film_create(0, 4, 4, None) == -1


# (radiance, width, rows, nsamples, sums, count_after, rgb) -> code
HOST_CASES = {
    "null radiance": ((None, 4, 2, 2, _P, 2, _P), -1),
    "null sums": ((_P, 4, 2, 2, None, 2, _P), -1),
    "nsamples 0": ((_P, 4, 2, 0, _P, 2, _P), -1),
    "nsamples -1": ((_P, 4, 2, -1, _P, 2, _P), -1),
    "width 0": ((_P, 0, 2, 2, _P, 2, _P), -1),
    "rows -1": ((_P, 4, -1, 2, _P, 2, _P), -1),
    "count below this add": ((_P, 4, 2, 2, _P, 1, _P), -1),
    "2^31 samples": ((_P, 1 << 15, 1 << 15, 2, _P, 2, _P), -7),
}


@pytest.mark.parametrize("case", sorted(HOST_CASES))
def test_film_pixels_host_argument_errors(case):
    args, code = HOST_CASES[case]
    _fresh()
    assert L.lib().rt_film_pixels_host(*args) == code, case
    assert L.lib().rt_last_error()
    assert not _BUF.any()


def test_film_pixels_host_of_no_rows_is_ok():
    _fresh()
    assert L.lib().rt_film_pixels_host(_P, 4, 0, 2, _P, 2, None) == 0
    assert not _BUF.any()


# (cam, sample0, nsamples, jitter, row0, rows, rays, seeds) -> code; the device entry takes the same
PASS_CASES = {
    "null camera": ((None, 0, 2, _P, 0, 1, _P, None), -1),
    "null rays": ((_CP, 0, 2, _P, 0, 1, None, None), -1),
    "nsamples 0": ((_CP, 0, 0, _P, 0, 1, _P, None), -1),
    "sample0 -1": ((_CP, -1, 2, _P, 0, 1, _P, None), -1),
    "sample0 + nsamples past int": ((_CP, 0x7FFFFFFF, 2, _P, 0, 1, _P, None), -1),
    "row0 -1": ((_CP, 0, 2, _P, -1, 1, _P, None), -1),
    "rows past the image": ((_CP, 0, 2, _P, 10, 2, _P, None), -1),
    "rows -1": ((_CP, 0, 2, _P, 0, -1, _P, None), -1),
    "2^31 rays": ((_CP, 0, 1 << 24, _P, 0, 11, _P, None), -7),
}


@pytest.mark.parametrize("entry", ["rt_camera_rays_pass_host", "rt_camera_rays_pass_device"])
@pytest.mark.parametrize("case", sorted(PASS_CASES))
def test_camera_pass_argument_errors_need_no_device(entry, case):
    args, code = PASS_CASES[case]
    _fresh()
    if entry.endswith("_device"):
        rc = L.lib().rt_camera_rays_pass_device(0, *args, None)
    else:
        rc = L.lib().rt_camera_rays_pass_host(*args)
    assert rc == code, (case, rc)
    assert L.lib().rt_last_error()
    assert not _BUF.any()


def test_camera_pass_null_table_and_empty_band():
    _fresh()
    lib = L.lib()
    assert lib.rt_camera_rays_pass_host(_CP, 3, 2, None, 0, 1, _P, None) == -1  # a slice of no table
    assert lib.rt_camera_rays_pass_device(0, _CP, 3, 2, None, 0, 1, _P, None, None) == -1
    assert lib.rt_camera_rays_pass_device(0, _CP, 0, 2, None, 0, 1, _P, None, None) == -1
    assert lib.rt_camera_rays_pass_host(_CP, 3, 2, _P, 4, 0, _P, None) == 0  # rows == 0
    assert lib.rt_camera_rays_pass_device(0, _CP, 3, 2, _P, 4, 0, _P, None, None) == 0
    assert not _BUF.any()
