"""Hit records and camera rays (rt_trace_hits*, rt_hit_record_host, rt_camera_rays*; DESIGN.md
§4.19), the part that needs no device: the entry points and layouts, the argument checks (which
answer before any HIP call), the helper's restatement against the reference's own records
(tests/golden/hit_records/), the host build of the record's arithmetic against the helper, the
host build of the camera rays against tests/shade_rays_cases.py's, and what the batches of
tests/test_gpu_trace_hits.py contain, so that no GPU test can pass by emptiness."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import hit_records as hr
import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. entry points and layouts ---------------------------------------------------------------
ENTRIES = ("rt_trace_hits_device", "rt_trace_hits", "rt_trace_hits_variant", "rt_hit_record_host", "rt_camera_rays_host",
           "rt_camera_rays_device")


def test_entry_points_exist():
    lib = L.lib()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert callable(rt.DeviceScene.trace_hits) and callable(rt.DeviceScene.trace_hits_variant)
    assert callable(rt.camera_rays) and callable(rt.hit_record_host) and callable(rt.hit_fields)
    assert lib.rt_trace_hits_variant(None) == rt.RT_RAYS_VARIANT_NONE
    assert lib.rt_abi_version() == 3


def test_hit_layout():
    assert C.sizeof(L.Hit) == 64 == rt.HIT_DTYPE.itemsize == hr.HIT_DTYPE.itemsize
    assert C.sizeof(L.Ray) == 24
    want = {"tri": 0, "t": 4, "u": 8, "v": 12, "p": 16, "normal": 28, "geom_normal": 40, "front_face": 52, "object_id": 56,
            "material": 60}
    assert [f[0] for f in L.Hit._fields_] == list(want) == list(rt.HIT_DTYPE.names)
    for name, off in want.items():
        assert getattr(L.Hit, name).offset == off == rt.HIT_DTYPE.fields[name][1] == hr.HIT_DTYPE.fields[name][1], name
    assert rt.HIT_DTYPE == hr.HIT_DTYPE


# ---- 2. argument errors ------------------------------------------------------------------------
# A scene handle that is never read: every check below answers before the scene is touched.
_FAKE_SCENE = C.create_string_buffer(64)
_RAYS = np.zeros((4, 6), np.float32)
_BUF = np.zeros(4 * 64 + 64, np.uint8)
_ALIGNED = _BUF.ctypes.data + (-_BUF.ctypes.data) % 16
_S, _R = C.addressof(_FAKE_SCENE), _RAYS.ctypes.data
BIN = L.RT_FLAG_BINARY

# (scene, rays, n, flags, hits) -> code
ARG_CASES = {
    "null scene": ((None, _R, 4, 0, _ALIGNED), -1),
    "null rays": ((_S, None, 4, 0, _ALIGNED), -1),
    "null hits": ((_S, _R, 4, 0, None), -1),
    "unknown flag": ((_S, _R, 4, L.RT_FLAG_NO_CULL, _ALIGNED), -1),
    "unknown flag beside BINARY": ((_S, _R, 4, BIN | 8, _ALIGNED), -1),
    "n = 2^31": ((_S, _R, 1 << 31, 0, _ALIGNED), -7),
    "n = 2^40, binary": ((_S, _R, 1 << 40, BIN, _ALIGNED), -7),
}


@pytest.mark.parametrize("entry", ["rt_trace_hits", "rt_trace_hits_device"])
@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_argument_errors_need_no_device(entry, case):
    args, code = ARG_CASES[case]
    rc = getattr(L.lib(), entry)(*args, None)  # kernel_ms / hip_stream
    assert rc == code, (case, rc, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _BUF.any()  # nothing was written


@pytest.mark.parametrize("off", [4, 8, 12])
def test_misaligned_device_records_are_refused(off):
    assert L.lib().rt_trace_hits_device(_S, _R, 4, 0, _ALIGNED + off, None) == -1
    assert b"aligned" in L.lib().rt_last_error()
    assert L.lib().rt_trace_hits_device(_S, _R, 0, BIN, _ALIGNED + off, None) == -1
    assert not _BUF.any()


def test_empty_batch_is_ok_without_a_device():
    for entry in ("rt_trace_hits", "rt_trace_hits_device"):
        assert getattr(L.lib(), entry)(_S, _R, 0, 0, _ALIGNED, None) == 0
        assert getattr(L.lib(), entry)(_S, _R, 0, BIN, _ALIGNED, None) == 0
    ms = C.c_float(7.0)
    assert L.lib().rt_trace_hits(_S, _R, 0, 0, _ALIGNED + 4, C.byref(ms)) == 0 and ms.value == 0.0  # host records: any alignment
    assert not _BUF.any()


# ---- 3. the helper against the reference's own records -----------------------------------------
@pytest.mark.parametrize("name", hr.NAMES)
def test_ref_records_equal_the_reference(name):
    """t, p, normal and front_face of ref_records on the fixture rays are the bits the reference's
    SearchBVH wrote (hit, triangleIdx too: the oracle's traversal is the reference's)."""
    fx = hr.fixture(name)
    b = hr.batch(name)
    pick = hr.fixture_pick()
    assert pick.size == 256 and same_bytes(fx["rays"], b["rays"][pick])
    hit = fx["hit"] != 0
    assert 64 <= hit.sum() <= 224  # hits and misses both
    assert np.array_equal(np.where(hit, fx["tri"], -1), b["idx"][pick])
    rec = hr.ref_records(hr.scene(name), fx["rays"], b["idx"][pick])  # (orc_search_bvh runs in the helper here)
    assert same_bytes(rec, hr.reference(name)[0][pick])
    assert np.array_equal(rec["tri"] >= 0, hit)
    assert same_bytes(rec["t"][hit], fx["t"][hit])
    assert same_bytes(rec["p"][hit], fx["p"][hit])
    assert same_bytes(rec["normal"][hit], fx["normal"][hit])
    assert np.array_equal(rec["front_face"][hit], fx["front"][hit].astype(np.int32))
    # SearchBVH's own miss record: t = -1, p = normal = 0, front_face false
    miss = ~hit
    assert (fx["t"][miss] == -1.0).all() and not fx["p"][miss].any() and not fx["normal"][miss].any() and not fx["front"][miss].any()
    assert (rec["t"][miss] == -1.0).all() and (rec["tri"][miss] == -1).all()
    for k in ("u", "v", "p", "normal", "geom_normal", "front_face", "object_id", "material"):
        assert not rec[k][miss].any(), k


# ---- 4. the host build of the record -----------------------------------------------------------
@pytest.mark.parametrize("name", hr.NAMES)
def test_hit_record_host_equals_ref_records(name):
    """rt_hit_record_host (the kernel's functions, built for the host) on every hit of the batch,
    each ray paired with the triangle it hits: every byte but the ids, u, v and geom_normal
    included; paired with a triangle it misses: a whole miss record."""
    b, s = hr.batch(name), hr.scene(name)
    want, _ = hr.reference(name)
    k = np.flatnonzero(b["idx"] >= 0)
    tris = np.ascontiguousarray(s["tris"], np.float32)
    got = rt.hit_record_host(b["rays"][k], tris[b["idx"][k]])
    exp = want[k].copy()
    assert np.array_equal(got["tri"], np.arange(k.size)) and (got["object_id"] == -1).all() and (got["material"] == -1).all()
    exp["tri"], exp["object_id"], exp["material"] = got["tri"], -1, -1
    bad = np.flatnonzero([g.tobytes() != e.tobytes() for g, e in zip(got, exp)])
    assert bad.size == 0, (bad[:4], got[bad[:4]], exp[bad[:4]])
    # a ray that misses the scene misses every triangle of it
    m = np.flatnonzero(b["idx"] < 0)
    assert m.size >= 256
    got = rt.hit_record_host(b["rays"][m], tris[np.arange(m.size) % tris.shape[0]])
    assert same_bytes(got, hr.ref_records(s, b["rays"][m], b["idx"][m], b["t"][m]))
    assert (got["tri"] == -1).all() and (got["t"] == -1.0).all()


def test_hit_record_host_arguments():
    lib = L.lib()
    out = np.zeros(2, rt.HIT_DTYPE)
    assert lib.rt_hit_record_host(None, None, 0, None) == 0
    assert lib.rt_hit_record_host(None, _R, 2, out.ctypes.data) == -1
    assert lib.rt_hit_record_host(_R, _R, -1, out.ctypes.data) == -1
    assert not out.view(np.uint8).any()
    with pytest.raises(ValueError):
        rt.hit_record_host(np.zeros((2, 6), np.float32), np.zeros((3, 18), np.float32))


# ---- 5. non-emptiness: what the GPU tests' batches contain (seed 1234, 4096 rays) ---------------
def test_batches_contain_every_class():
    flipped = 0
    for name in rb.SCENES:
        rec, cls = hr.reference(name)
        counts = {k: int(v.sum()) for k, v in cls.items()}
        print(name, counts)
        assert counts["hit"] >= 1000, name
        assert counts["back"] >= (8 if name == "frog" else 256), name
        assert counts["hit"] <= 4096 - 256, name  # and misses
        flipped += counts["flipped"]
    assert int(hr.reference("cornell")[1]["degenerate"].sum()) >= 1024
    assert flipped >= 256
    rec, cls = hr.reference(hr.FUZZ_CASE)
    assert cls["hit"].sum() >= 1000
    default = cls["hit"] & (rec["material"] == -1)
    assert default.sum() >= 16
    c = sf.case(hr.FUZZ_CASE)
    nm = c["mats"].size
    oid = rec["object_id"][cls["hit"]]
    assert nm == 7 and (oid < 0).any() and (oid >= nm).any() and ((oid >= 0) & (oid < nm)).sum() >= 256
    assert np.array_equal(rec["material"][cls["hit"]], np.where((oid >= 0) & (oid < nm), oid, -1))
    assert np.unique(rec["material"][cls["hit"]]).size >= 5
    assert hr.FUZZ_RAY_SEED == rb.SEED  # the first seed tried already meets the condition


# ---- 6. camera rays: the host build against the helper the reference's frames pin ----------------
_camera = hr.shape_camera
CAMERA_SHAPES = hr.CAMERA_SHAPES


def helper_rays(case, spp, row0, rows, jitter=None):
    cam = _camera(case)
    W, H = cam.pixel_width, cam.pixel_height
    jit = rt.jittered_samples(spp) if jitter is None else jitter
    rays, seeds = sc.camera_rays(cam.basis(), W, H, jit)
    rows = H - row0 if rows is None else rows
    sl = slice(row0 * W * spp, (row0 + rows) * W * spp)
    return cam, rays[sl], seeds[sl]


@pytest.mark.parametrize("shape", list(CAMERA_SHAPES))
def test_camera_rays_host_equals_the_helper(shape):
    case, spp, row0, rows = CAMERA_SHAPES[shape]
    cam, want_r, want_s = helper_rays(case, spp, row0, rows)
    rays, seeds = rt.camera_rays(cam, spp, row0=row0, rows=rows)
    assert rays.dtype == np.float32 and seeds.dtype == np.uint32
    assert same_bytes(rays, want_r) and same_bytes(seeds, want_s)
    # a caller's table, and no seeds
    jit = (np.random.default_rng(3).random((spp, 2), np.float32) - np.float32(0.5)).astype(np.float32)
    _, want_r, _ = helper_rays(case, spp, row0, rows, jit)
    rays2, _ = rt.camera_rays(cam, spp, jitter=jit, row0=row0, rows=rows)
    assert same_bytes(rays2, want_r) and not same_bytes(rays2, rays)
    raw = np.zeros_like(rays2)
    n_rows = cam.pixel_height - row0 if rows is None else rows
    assert L.lib().rt_camera_rays_host(C.byref(cam.c), spp, jit.ctypes.data, row0, n_rows, raw.ctypes.data, None) == 0
    assert same_bytes(raw, want_r)


def test_camera_rays_argument_errors():
    lib = L.lib()
    cam = _camera("c_l3_d1")  # 48 x 32
    rays = np.zeros((48 * 32 * 2, 6), np.float32)
    seeds = np.zeros(48 * 32 * 2, np.uint32)
    jit = rt.jittered_samples(2)
    c, r, s, j = C.byref(cam.c), rays.ctypes.data, seeds.ctypes.data, jit.ctypes.data
    big = rt.Camera(width=1 << 15, height=1 << 15)
    cases = [((None, 2, j, 0, 32, r, s), -1), ((c, 2, j, 0, 32, None, s), -1), ((c, 0, j, 0, 32, r, s), -1),
             ((c, -3, j, 0, 32, r, s), -1), ((c, 2, j, -1, 4, r, s), -1), ((c, 2, j, 0, 33, r, s), -1),
             ((c, 2, j, 30, 3, r, s), -1), ((c, 2, j, 33, 0, r, s), -1), ((c, 2, j, 0, -1, r, s), -1),
             ((c, 2, j, 2**31 - 1, 2, r, s), -1), ((C.byref(big.c), 2, j, 0, 1 << 15, r, s), -7),
             ((C.byref(big.c), 2, j, 0, 1 << 15, r, None), -7)]
    for args, code in cases:
        assert lib.rt_camera_rays_host(*args) == code, args[1:5]
        assert lib.rt_last_error()
        assert lib.rt_camera_rays_device(0, *args, None) == code, args[1:5]  # the same checks, before any HIP call
    assert lib.rt_camera_rays_device(0, c, 2, None, 0, 32, r, s, None) == -1  # the device entry needs its table
    assert lib.rt_camera_rays_host(c, 2, j, 32, 0, r, s) == 0 and lib.rt_camera_rays_host(c, 2, j, 7, 0, r, None) == 0
    assert lib.rt_camera_rays_device(0, c, 2, j, 7, 0, r, s, None) == 0  # no rows: no launch, no device
    assert not rays.any() and not seeds.any()  # nothing was written
    assert (1 << 15) * (1 << 15) * 2 > 2**31 - 1


def test_cpp_wrapper_camera_rays(tmp_path):
    """rt::camera_rays of include/rt_mi355x.hpp (a stand-alone program linked against the library)
    gives rt_camera_rays_host's rays and seeds; the header compiles without warnings."""
    import subprocess

    from conftest import REPO
    from raytracinginonesemester_amd import build as B

    exe = tmp_path / "hit_records_hpp_main"
    subprocess.run([B.CXX, "-std=c++17", "-O1", *B.FP, "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'include'}",
                    str(REPO / "tests" / "native" / "hit_records_hpp_main.cpp"), "-o", str(exe), f"-L{L.LIB_PATH.parent}",
                    "-lrt_mi355x", f"-Wl,-rpath,{L.LIB_PATH.parent}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    words = np.array([[int(w, 16) for w in line.split()] for line in r.stdout.splitlines()], np.uint32)
    rays, seeds = rt.camera_rays(_camera("c_l3_d1"), 4, row0=5, rows=7)
    assert words.shape == (48 * 7 * 4, 7)
    assert np.array_equal(words[:, :6], rays.view(np.uint32)) and np.array_equal(words[:, 6], seeds)
