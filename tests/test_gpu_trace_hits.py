"""Hit records and device camera rays on the GPU (rt_trace_hits*, rt_camera_rays_device;
DESIGN.md §4.19), bit for bit (bytes, no tolerance):

* parity per scene: every byte of every record against tests/hit_records.py's restatement of the
  reference's HitRecord for the oracle's closest hits, on the LDS variants, the deep kernel and its
  brute-force completion, and on a scene whose object ids leave the material table;
* batch sizes around the block size, a shuffled batch, the device path on a side stream, whole miss
  records over a 0xFF-filled output;
* camera rays made on the device against the host build, and then through trace_hits and shade_rays
  against the reference's own golden frames;
* a batch beside a renderer's frames, and on a clone.

What the batches contain, and the restatement itself against the reference's records, is pinned on
the CPU by tests/test_hit_records_host.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import hit_records as hr
import ray_batches as rb
import shade_rays_cases as sc
from conftest import golden_array, golden_meta, hexv, host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
W_, B_, D_ = L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP
GUARD = 16

_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    if name not in _scenes:
        _scenes[name] = hr.device_scene(name)
    return _scenes[name]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(got, want):
    return np.flatnonzero(np.ascontiguousarray(got).view(np.uint8).reshape(-1, 64)
                          != np.ascontiguousarray(want).view(np.uint8).reshape(-1, 64))


def as_records(t: torch.Tensor) -> np.ndarray:
    return np.ascontiguousarray(t.cpu().numpy()).view(rt.HIT_DTYPE).reshape(-1)


# ---- 1. parity per scene -----------------------------------------------------------------------
# scene -> the variants (flags 0, RT_FLAG_BINARY) the rule must give
VARIANTS = {"cornell": (W_, B_), "frog": (W_, B_), "sphere_single": (W_, B_), "chain24": (W_, B_), "chain48": (D_, D_),
            "chain300": (D_, D_), "chain600": (D_, D_), hr.FUZZ_CASE: (W_, B_)}


@pytest.mark.parametrize("name", hr.NAMES)
def test_records_equal_the_reference(name):
    b = hr.batch(name)
    want, cls = hr.reference(name)
    ds = scene(name)
    for k, flags in enumerate((0, BINARY)):
        got = ds.trace_hits(b["rays"], flags=flags)
        assert got.dtype == rt.HIT_DTYPE and got.shape == (rb.N_RAYS,)
        bad = np.unique(differing(got, want) // 64) if not same_bytes(got, want) else np.zeros(0, int)
        print(f"{name} flags {flags}: variant {ds.trace_hits_variant()}, {int((got['tri'] >= 0).sum())} hits, "
              f"{bad.size} records differ")
        assert bad.size == 0, (bad[:4], got[bad[:4]], want[bad[:4]])
        variant = ds.trace_hits_variant()
        assert variant == sc.rule_variant(hr.scene(name), flags)[0]
        assert variant == VARIANTS[name][k]
        # tri and t are the closest-hit query's
        idx, t = ds.trace_rays(b["rays"], flags=flags)
        assert np.array_equal(got["tri"], idx) and same_bytes(got["t"], t)
        assert np.array_equal(idx, b["idx"])
    deep = ds.traversal_info()["deep"]
    assert deep == (name in ("chain300", "chain600"))
    if name == "chain600":  # the brute-force completion decides some of these (the larger index of the tie)
        perm = hr.scene(name)["perm"]
        assert (want["tri"] == int(perm[3])).sum() >= 64
    if name == hr.FUZZ_CASE:
        hit = cls["hit"]
        assert (got["material"][hit] == -1).sum() >= 16 and (got["material"][hit] >= 0).sum() >= 256
        assert (got["object_id"][hit] != got["material"][hit]).sum() >= 16


# ---- 2. sizes, order, paths --------------------------------------------------------------------
def raw_trace(ds, rays, n, flags=0):
    """rt_trace_hits over the first n rays into records filled with 0xFF, GUARD more behind them."""
    out = np.full((n + GUARD) * 64, 0xFF, np.uint8)
    rc = L.lib().rt_trace_hits(ds.handle, rays.ctypes.data, n, flags, out.ctypes.data, None)
    return rc, out[:n * 64].view(rt.HIT_DTYPE), out[n * 64:]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096])
@pytest.mark.parametrize("name", ["frog", "chain600"])
def test_batch_sizes_and_placement(name, n):
    b = hr.batch(name)
    want, _ = hr.reference(name)
    for flags in (0, BINARY):
        rc, got, guard = raw_trace(scene(name), b["rays"], n, flags)
        assert rc == 0
        assert same_bytes(got, want[:n])
        assert (guard == 0xFF).all()


def test_misses_are_whole_miss_records():
    """Every byte of a miss is written over the 0xFF fill: tri -1, t -1.0f, zero elsewhere."""
    b = hr.batch("frog")
    miss = np.flatnonzero(b["idx"] < 0)
    assert miss.size >= 1024
    rays = np.ascontiguousarray(b["rays"][miss])
    one = np.zeros(1, rt.HIT_DTYPE)
    one["tri"], one["t"] = -1, -1.0
    for flags in (0, BINARY):
        rc, got, guard = raw_trace(scene("frog"), rays, miss.size, flags)
        assert rc == 0 and (guard == 0xFF).all()
        assert got.tobytes() == one.tobytes() * miss.size
    rc, got, _ = raw_trace(scene("chain600"), np.ascontiguousarray(hr.batch("chain600")["rays"][hr.batch("chain600")["idx"] < 0]),
                           int((hr.batch("chain600")["idx"] < 0).sum()))
    assert rc == 0 and got.size >= 1024 and got.tobytes() == one.tobytes() * got.size


def test_a_shuffled_batch_returns_the_shuffled_records():
    """A lane reading another lane's LDS stack, or storing into another lane's record, would show."""
    perm = np.random.default_rng(11).permutation(rb.N_RAYS)
    for name in ("cornell", "chain300"):
        b = hr.batch(name)
        want, _ = hr.reference(name)
        for flags in (0, BINARY):
            assert same_bytes(scene(name).trace_hits(b["rays"][perm], flags=flags), want[perm])


def test_device_path_on_a_side_stream():
    """Rays made by a torch op on a side stream, traced on that stream with no sync in between."""
    name = hr.FUZZ_CASE
    b = hr.batch(name)
    want, _ = hr.reference(name)
    ds = scene(name)
    dev = torch.device("cuda", 0)
    neg = torch.from_numpy(-b["rays"]).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        r = -neg
        hits = ds.trace_hits(r)
        hits_b = ds.trace_hits(r, flags=BINARY)
        assert ds.trace_hits_variant() == B_
    assert hits.is_cuda and hits.shape == (rb.N_RAYS, 16) and hits.dtype == torch.int32
    side.synchronize()
    assert same_bytes(as_records(hits), want) and same_bytes(as_records(hits_b), want)
    assert same_bytes(as_records(hits), ds.trace_hits(b["rays"]))  # the host path
    f = rt.hit_fields(hits)
    assert set(f) == set(rt.HIT_DTYPE.names)
    for k in rt.HIT_DTYPE.names:
        v = f[k].cpu().numpy()
        assert v.dtype == want[k].dtype and same_bytes(v, want[k]), k
    with pytest.raises(ValueError):
        ds.trace_hits(r[:, :5])
    with pytest.raises(ValueError):
        ds.trace_hits(r, timing=True)
    # a misaligned output is refused before anything is launched
    raw = torch.zeros(rb.N_RAYS * 16 + 4, dtype=torch.int32, device=dev)
    assert L.lib().rt_trace_hits_device(ds.handle, r.data_ptr(), rb.N_RAYS, 0, raw.data_ptr() + 4, None) == -1
    torch.cuda.synchronize(dev)
    assert not raw.any().item()


# ---- 3. camera rays ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(hr.CAMERA_SHAPES))
def test_camera_rays_device_equals_host(shape):
    case, spp, row0, rows = hr.CAMERA_SHAPES[shape]
    cam = hr.shape_camera(case)
    want_r, want_s = rt.camera_rays(cam, spp, row0=row0, rows=rows)
    rays, seeds = rt.camera_rays(cam, spp, row0=row0, rows=rows, device=0)
    assert rays.is_cuda and rays.dtype == torch.float32 and seeds.dtype == torch.int32
    assert same_bytes(rays.cpu().numpy(), want_r) and same_bytes(seeds.cpu().numpy().view(np.uint32), want_s)
    # a caller's table on a side stream; no seeds: nothing behind the rays is written
    jit = (np.random.default_rng(5).random((spp, 2), np.float32) - np.float32(0.5)).astype(np.float32)
    want_j, _ = rt.camera_rays(cam, spp, jitter=jit, row0=row0, rows=rows)
    dev = torch.device("cuda", 0)
    n = want_j.shape[0]
    jd = torch.from_numpy(jit).to(dev)
    out = torch.full((n + GUARD, 6), -3.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    n_rows = cam.pixel_height - row0 if rows is None else rows
    assert L.lib().rt_camera_rays_device(0, C.byref(cam.c), spp, jd.data_ptr(), row0, n_rows, out.data_ptr(), None,
                                         side.cuda_stream) == 0
    side.synchronize()
    got = out.cpu().numpy()
    assert same_bytes(got[:n], want_j) and (got[n:] == -3.25).all()
    r2, s2 = rt.camera_rays(cam, spp, jitter=jit, row0=row0, rows=rows, device=0, stream=side.cuda_stream)
    side.synchronize()
    assert same_bytes(r2.cpu().numpy(), want_j) and same_bytes(s2.cpu().numpy().view(np.uint32), want_s)


def _golden_scene(name):
    """(DeviceScene key, camera, spp, depth, diffuse, miss) of a golden frame."""
    m = golden_meta(name)
    W, H = m["width"], m["height"]
    if name.startswith("chain"):
        import chain_bvh  # (tests/golden is on sys.path: ray_batches)

        pos, look, up, f, s = chain_bvh.CAMERA
        cam, key, miss = rt.Camera(pos, look, up, f, s, W, H), name, (0.0, 0.0, 0.0)
    else:
        json_name = {"c3_small": "frog", "frog_bounce": "frog", "cornell": "cornell"}[name]
        cam, key, miss = host_scene(json_name + ".json").camera(W, H), json_name, tuple(hexv(m["miss_color"]))
    b = cam.basis()
    for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"):  # the golden frame's own camera
        assert same_bytes(b[k], hexv(m[k])), (name, k)
    return key, cam, m["spp"], m["max_depth"], bool(m["diffuse_bounce"]), miss


@pytest.mark.parametrize("name", ["c3_small", "cornell", "chain600"])
def test_device_camera_rays_give_the_golden_hits(name):
    """camera_rays -> trace_hits on the device: tri and t of every sample are the reference's own
    hits.i32 / hitt.f32, and the rest of each record is the restated one."""
    key, cam, spp, _, _, _ = _golden_scene(name)
    ds = scene(key)
    rays, _ = rt.camera_rays(cam, spp, device=0)
    f = rt.hit_fields(ds.trace_hits(rays))
    ghi, ght = golden_array(name, "hits.i32.gz", np.int32), golden_array(name, "hitt.f32.gz", np.float32)
    assert rays.shape[0] == ghi.size
    tri, t = f["tri"].cpu().numpy(), f["t"].cpu().numpy()
    assert np.array_equal(tri, ghi), int((tri != ghi).sum())
    assert same_bytes(t, ght)
    assert (ghi >= 0).sum() >= 1000 and (name == "cornell" or (ghi < 0).sum() >= 1000)  # (cornell is closed)
    if name != "c3_small":  # (4096-ray restatements are enough for frog; these frames are small)
        want = hr.ref_records(hr.scene(key), rays.cpu().numpy(), ghi, ght)
        assert same_bytes(as_records(ds.trace_hits(rays)), want)


@pytest.mark.parametrize("name", ["cornell", "frog_bounce"])
def test_device_camera_rays_shade_to_the_golden_frame(name):
    """camera_rays -> shade_rays on the device, summed per pixel: the reference's own frame."""
    key, cam, spp, depth, diffuse, miss = _golden_scene(name)
    assert depth == {"cornell": 3, "frog_bounce": 8}[name]
    rays, seeds = rt.camera_rays(cam, spp, device=0)
    rad = scene(key).shade_rays(rays, seeds, max_depth=depth, diffuse_bounce=diffuse, miss_color=miss)
    H, W = cam.pixel_height, cam.pixel_width
    fb = golden_array(name, "fb.f32.gz", np.float32).reshape(H, W, 3)
    got = sc.pixel_sum(rad.cpu().numpy(), H, W, spp)
    bad = (got.view(np.uint32) != fb.view(np.uint32)).any(axis=2)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - fb).max()))


# ---- 4. beside frames --------------------------------------------------------------------------
def test_records_beside_a_renderers_frames_and_on_a_clone():
    """Three frames in flight on a Renderer while a batch is traced against its scene on a stream of
    its own, and on a clone of that scene: the frames are the frame rendered alone, no device guard
    fires, the records are the reference's."""
    name = "cornell"
    hs = host_scene(name + ".json")
    b = hr.batch(name)
    want, _ = hr.reference(name)
    cam = hs.camera(64, 48)
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=hs.settings["miss_color"])
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    clone = C.c_void_p()
    try:
        kept = r.render(cam, spp=4, max_depth=1, miss_color=hs.settings["miss_color"]).tobytes()
        ds = r.scene(0)
        L.check(L.lib().rt_scene_clone(ds.handle, 0, C.byref(clone)))
        assert L.lib().rt_trace_hits_variant(clone) == L.RT_RAYS_VARIANT_NONE
        dev = torch.device("cuda", 0)
        dev_rays = torch.from_numpy(b["rays"].copy()).to(dev)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        tickets = [r.submit(cam, o) for _ in range(3)]
        with torch.cuda.stream(side):  # the device path: asynchronous beside the frames
            d = ds.trace_hits(dev_rays)
        host = ds.trace_hits(b["rays"])  # the host path
        on_clone = np.zeros(rb.N_RAYS, rt.HIT_DTYPE)
        L.check(L.lib().rt_trace_hits(clone, b["rays"].ctypes.data, rb.N_RAYS, BINARY, on_clone.ctypes.data, None))
        for k in tickets:
            addr, n = r.wait(k)
            assert bytes((C.c_uint8 * n).from_address(addr)) == kept, k
        assert ds.faults() == 0
        torch.cuda.synchronize()
        assert same_bytes(host, want) and same_bytes(as_records(d), want) and same_bytes(on_clone, want)
        assert L.lib().rt_trace_hits_variant(clone) == B_ and ds.trace_hits_variant() == W_
        assert L.lib().rt_trace_rays_variant(clone) == L.lib().rt_shade_rays_variant(clone) == L.RT_RAYS_VARIANT_NONE  # words of their own
    finally:
        if clone:
            L.lib().rt_scene_destroy(clone)
        r.close()
