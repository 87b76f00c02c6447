"""Batched ray queries on the GPU (rt_trace_rays*, include/rt_mi355x.h) against the
oracle's SearchBVH, ray by ray: closest hit (triangle index equal, t equal as bit patterns),
occlusion (IsInShadow's strict `t < max_t`), every batch size around the wave and block sizes,
the device path on a side stream, queries beside a renderer's frames, and degenerate rays.

The batches are tests/ray_batches.py's (4096 rays in four classes per scene; what they contain
is pinned by tests/test_trace_rays_host.py with the oracle alone).  No ray is left out of any
comparison.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import ray_batches as rb
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)
BINARY = L.RT_FLAG_BINARY
SENT_I, SENT_T = np.int32(-77), np.float32(-7.5)
GUARD = 64

_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    if name not in _scenes:
        _scenes[name] = rb.device_scene(name)
    return _scenes[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the traversal the variant rule gives (rt_trace_rays_variant), asserted for these only
VARIANT = {("frog", 0): L.RT_RAYS_VARIANT_WIDE, ("frog", BINARY): L.RT_RAYS_VARIANT_BINARY,
           **{(c, f): L.RT_RAYS_VARIANT_DEEP for c in ("chain48", "chain300", "chain600") for f in (0, BINARY)}}


@pytest.mark.parametrize("flags", [0, BINARY], ids=["wide", "binary"])
@pytest.mark.parametrize("name", rb.SCENES)
def test_closest_hit_equals_search_bvh(name, flags):
    b = rb.batch(name)
    ds = scene(name)
    idx, t = ds.trace_rays(b["rays"], flags=flags)
    bad = np.flatnonzero((idx != b["idx"]) | (bits(t) != bits(b["t"])))
    print(f"{name} flags {flags}: variant {ds.trace_rays_variant()}, {int((idx >= 0).sum())} hits, {bad.size} differ")
    assert bad.size == 0, (bad[:8], idx[bad[:8]], b["idx"][bad[:8]], t[bad[:8]], b["t"][bad[:8]])
    if (name, flags) in VARIANT:
        assert ds.trace_rays_variant() == VARIANT[(name, flags)]
    if name == "chain48":  # DEEP because its per-lane stack does not fit LDS, not because the scene is deep
        assert not ds.traversal_info()["deep"]
    if name in ("chain300", "chain600"):
        assert ds.traversal_info()["deep"]


def occlusion_case(name):
    """max_t per ray from the oracle's (idx, t): hit ray i cycles over [0.5t, t, nextafter(t, +inf),
    2t, 1e-4, FLT_MAX] (t itself and its successor pin the strict <), miss ray i over
    [0, 1, FLT_MAX]; expected = hit and t < max_t."""
    b = rb.batch(name)
    return occlusion_from(b["idx"], b["t"])


def occlusion_from(idx, t):
    i = np.arange(idx.size)
    up = np.nextafter(t, np.float32(np.inf), dtype=np.float32)
    hit_cycle = np.stack([np.float32(0.5) * t, t, up, np.float32(2.0) * t, np.full_like(t, 1e-4), np.full_like(t, FLT_MAX)])
    miss_cycle = np.stack([np.zeros_like(t), np.ones_like(t), np.full_like(t, FLT_MAX)])
    max_t = np.where(idx >= 0, hit_cycle[i % 6, i], miss_cycle[i % 3, i]).astype(np.float32)
    return max_t, (idx >= 0) & (t < max_t)


@pytest.mark.parametrize("flags", [0, BINARY], ids=["wide", "binary"])
@pytest.mark.parametrize("name", rb.SCENES)
def test_occlusion_equals_is_in_shadow(name, flags):
    b = rb.batch(name)
    max_t, want = occlusion_case(name)
    hit = b["idx"] >= 0
    assert want[hit].any() and (~want[hit]).any()  # both outcomes among the hit rays
    got = scene(name).trace_rays(b["rays"], mode="occluded", max_t=max_t, flags=flags)
    assert got.dtype == np.bool_ and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    print(f"{name} flags {flags}: {int(want.sum())} occluded of {int(hit.sum())} hits, {bad.size} differ")
    assert bad.size == 0, (bad[:8], b["t"][bad[:8]], max_t[bad[:8]])


def raw_trace(ds, mode, rays, max_t, n, flags=0, with_t=True):
    """rt_trace_rays over the first n rays into outputs with GUARD sentinel entries behind them."""
    idx = np.full(n + GUARD, SENT_I, np.int32)
    t = np.full(n + GUARD, SENT_T, np.float32) if with_t else None
    rc = L.lib().rt_trace_rays(ds.handle, mode, rays.ctypes.data, None if max_t is None else max_t.ctypes.data, n, flags,
                               idx.ctypes.data, None if t is None else t.ctypes.data, None)
    return rc, idx, t


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095])
def test_batch_sizes_and_placement(n):
    b = rb.batch("frog")
    ds = scene("frog")
    full_idx, full_t = ds.trace_rays(b["rays"])
    max_t, _ = occlusion_case("frog")
    full_occ = ds.trace_rays(b["rays"], mode="occluded", max_t=max_t)
    rc, idx, t = raw_trace(ds, L.RT_RAYS_CLOSEST, b["rays"], None, n)
    assert rc == 0
    assert np.array_equal(idx[:n], full_idx[:n]) and np.array_equal(bits(t[:n]), bits(full_t[:n]))
    assert (idx[n:] == SENT_I).all() and (t[n:] == SENT_T).all()
    rc, idx, _ = raw_trace(ds, L.RT_RAYS_CLOSEST, b["rays"], None, n, with_t=False)  # hit_t may be NULL
    assert rc == 0 and np.array_equal(idx[:n], full_idx[:n]) and (idx[n:] == SENT_I).all()
    rc, occ, _ = raw_trace(ds, L.RT_RAYS_OCCLUDED, b["rays"], max_t, n, with_t=False)
    assert rc == 0 and np.array_equal(occ[:n] != 0, full_occ[:n]) and (occ[n:] == SENT_I).all()
    assert set(np.unique(occ[:n])) <= {0, 1}


@pytest.mark.parametrize("owner", ["scene", "renderer"])
def test_device_path_on_a_side_stream(owner):
    """Rays made by a torch op on a side stream, traced on that stream with no sync in between;
    for a scene of its own and for a scene owned by a Renderer."""
    b = rb.batch("frog")
    max_t, _ = occlusion_case("frog")
    host = scene("frog")
    want_idx, want_t = host.trace_rays(b["rays"])
    want_occ = host.trace_rays(b["rays"], mode="occluded", max_t=max_t)
    a = rb.scene_arrays("frog")
    r = None
    if owner == "renderer":
        r = rt.Renderer(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], devices=(0,))
        ds = r.scene(0)
    else:
        ds = host
    try:
        dev = torch.device("cuda", 0)
        neg = torch.from_numpy(-b["rays"]).to(dev)
        mt2 = torch.from_numpy(max_t * np.float32(0.5)).to(dev)  # (0.5 x then 2 x: exact, FLT_MAX included)
        torch.cuda.synchronize(dev)
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            rays = -neg
            idx, t = ds.trace_rays(rays)
            occ = ds.trace_rays(rays, mode="occluded", max_t=mt2 * 2.0, flags=BINARY)
            assert ds.trace_rays_variant() == L.RT_RAYS_VARIANT_BINARY
        assert idx.is_cuda and idx.dtype == torch.int32 and t.dtype == torch.float32 and occ.dtype == torch.bool
        side.synchronize()
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(bits(t.cpu().numpy()), bits(want_t))
        assert np.array_equal(occ.cpu().numpy(), want_occ)
    finally:
        if r is not None:
            r.close()


def test_queries_beside_a_renderers_frames():
    """Three frames in flight on a Renderer while its scene answers queries: the frames are the
    frame rendered alone, no device guard fires, the queries equal the oracle."""
    name = "sphere_single"
    hs = host_scene(name + ".json")
    b = rb.batch(name)
    cam = hs.camera(64, 48)
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=hs.settings["miss_color"])
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    try:
        kept = r.render(cam, spp=4, max_depth=1, miss_color=hs.settings["miss_color"]).tobytes()
        ds = r.scene(0)
        dev_rays = torch.from_numpy(b["rays"].copy()).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        tickets = [r.submit(cam, o) for _ in range(3)]
        d_idx, d_t = ds.trace_rays(dev_rays)  # the device path: asynchronous beside the frames
        idx, t = ds.trace_rays(b["rays"])     # the host path
        for k in tickets:
            addr, n = r.wait(k)
            assert bytes((C.c_uint8 * n).from_address(addr)) == kept, k
        assert ds.faults() == 0
        torch.cuda.synchronize()
        for gi, gt in ((idx, t), (d_idx.cpu().numpy(), d_t.cpu().numpy())):
            assert np.array_equal(gi, b["idx"]) and np.array_equal(bits(gt), bits(b["t"]))
    finally:
        r.close()


def test_degenerate_rays_terminate_and_write():
    """Zero-direction rays answer as the reference does; NaN rays' outputs are merely written."""
    sl = rb.class_slices()
    pick = np.concatenate([np.arange(s.start, s.start + 64) for s in sl.values()])
    rays = rb.batch("frog")["rays"][pick].copy()
    zero, nan = [3, 70, 130, 200], [10, 90, 150, 255]
    rays[zero, 3:] = 0.0
    rays[nan, 3:] = np.nan
    rays[nan[0], 4:] = 1.0  # (one with a single NaN component)
    finite = np.setdiff1d(np.arange(256), nan)
    assert finite.size == 252
    a = rb.scene_arrays("frog")
    want_idx, want_t = rb.oracle_trace(a["P"], a["nodes"], a["aabbs"], a["tris"], rays[finite])
    assert (want_idx >= 0).any() and (want_idx < 0).any()
    ds = scene("frog")
    for flags in (0, BINARY):
        rc, idx, t = raw_trace(ds, L.RT_RAYS_CLOSEST, rays, None, 256, flags)
        assert rc == 0
        assert np.array_equal(idx[finite], want_idx) and np.array_equal(bits(t[finite]), bits(want_t))
        assert (idx[nan] != SENT_I).all() and (bits(t[nan]) != bits(SENT_T)).all()
        assert (idx[256:] == SENT_I).all() and (t[256:] == SENT_T).all()
        # occlusion: a NaN max_t gives 0 for every ray, hit or not
        rc, occ, _ = raw_trace(ds, L.RT_RAYS_OCCLUDED, rays, np.full(256, np.nan, np.float32), 256, flags, with_t=False)
        assert rc == 0 and (occ[:256] == 0).all() and (occ[256:] == SENT_I).all()
        rc, occ, _ = raw_trace(ds, L.RT_RAYS_OCCLUDED, rays, np.full(256, FLT_MAX, np.float32), 256, flags, with_t=False)
        assert rc == 0 and np.array_equal(occ[finite] != 0, want_idx >= 0) and (occ[nan] != SENT_I).all()


@pytest.mark.parametrize("flags", [0, BINARY], ids=["wide", "binary"])
@pytest.mark.parametrize("kind", rb.VARIANTS)
@pytest.mark.parametrize("base", rb.VARIANT_BASES)
def test_other_magnitudes(base, kind, flags):
    """Closest hit and occlusion on the scenes of ray_batches.variant_arrays (scaled by 2^-10 and
    2^12, shifted by 4096, with a triangle at 2^100 that takes the float box filter away): every
    box decision at magnitudes the shipped scenes do not have, against the oracle ray by ray."""
    a = rb.variant_arrays(base, kind)
    ds = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], 0)
    try:
        idx, t = ds.trace_rays(a["rays"], flags=flags)
        bad = np.flatnonzero((idx != a["idx"]) | (bits(t) != bits(a["t"])))
        print(f"{base} {kind} flags {flags}: {int((idx >= 0).sum())} hits, {bad.size} differ")
        assert bad.size == 0, (bad[:8], idx[bad[:8]], a["idx"][bad[:8]], t[bad[:8]], a["t"][bad[:8]])
        assert (a["idx"] >= 0).sum() > 100
        max_t, want = occlusion_from(a["idx"], a["t"])
        got = ds.trace_rays(a["rays"], mode="occluded", max_t=max_t, flags=flags)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (bad[:8], a["t"][bad[:8]], max_t[bad[:8]])
        assert ds.faults() == 0
    finally:
        ds.close()
