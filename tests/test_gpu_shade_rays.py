"""Radiance queries on the GPU (rt_shade_rays*, include/rt_mi355x.h) against the
reference's TraceRayIterative, bit for bit (uint32 views, no tolerance):

* frames through rays: every sample of tests/shade_fuzz.py's 15 cases as a caller ray with the
  frame's seeds, summed per pixel, against the reference's own render (frame, hits, t);
* caller rays around four scenes against the oracle's one-pixel render, ray by ray;
* batch sizes around the wave and block sizes, a shuffled batch, max_depth <= 0, default seeds,
  no AOV outputs;
* the device path on a side stream, a clone, and a batch beside a renderer's frames.

What the batches contain is pinned by tests/test_shade_rays_host.py with the oracle alone.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
SENT_I, SENT_T, SENT_C = np.int32(-77), np.float32(-7.5), np.float32(-3.25)
GUARD = 64

_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    """One DeviceScene per ray_batches scene or shade_fuzz case."""
    if name not in _scenes:
        if name in sf.CASES:
            c = sf.case(name)
            _scenes[name] = rt.DeviceScene(c["P"], c["nodes"], c["aabbs"], c["tris"], c["triobj"], sf.mats13(c), c["lights"])
        else:
            _scenes[name] = rb.device_scene(name)
    return _scenes[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    """(radiance, idx, t) equal as bit patterns."""
    return (np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])
            and np.array_equal(bits(got[2]), bits(want[2])))


# ---- 1. frames through rays -------------------------------------------------------------------
def _frame_through_rays(name, flags):
    c = sf.case(name)
    pos, look, up, f, s = c["camera"]
    cam = rt.Camera(pos, look, up, f, s, c["W"], c["H"])
    rays, seeds = sc.camera_rays(cam.basis(), c["W"], c["H"], orc.jitter(c["spp"]))
    ds = scene(name)
    rad, idx, t = ds.shade_rays(rays, seeds, max_depth=c["depth"], diffuse_bounce=c["diffuse"], flags=flags, aov=True)
    H, W, spp = c["H"], c["W"], c["spp"]
    sf.check_against_fixture(name, sc.pixel_sum(rad, H, W, spp), idx.reshape(H, W, spp), t.reshape(H, W, spp))
    return ds


@pytest.mark.parametrize("name", list(sf.CASES))
def test_frames_through_rays(name):
    ds = _frame_through_rays(name, 0)
    variant, deep = sc.rule_variant(sc.scene_of_case(sf.case(name)))
    assert deep == (sf.case(name)["base"] == "chain") == ds.traversal_info()["deep"]
    assert ds.shade_rays_variant() == variant == (L.RT_RAYS_VARIANT_DEEP if deep else L.RT_RAYS_VARIANT_WIDE)
    assert ds.trace_rays_variant() == L.RT_RAYS_VARIANT_NONE  # a word of its own


@pytest.mark.parametrize("name", ["s_l3_d1", "s_l1_d4m", "s_l8_d4"])
def test_frames_through_rays_binary(name):
    ds = _frame_through_rays(name, BINARY)
    assert ds.shade_rays_variant() == sc.rule_variant(sc.scene_of_case(sf.case(name)), BINARY)[0] == L.RT_RAYS_VARIANT_BINARY


# ---- 2. caller rays ---------------------------------------------------------------------------
VARIANT = {"cornell": L.RT_RAYS_VARIANT_WIDE, "frog": L.RT_RAYS_VARIANT_WIDE, "chain48": L.RT_RAYS_VARIANT_DEEP,
           "chain300": L.RT_RAYS_VARIANT_DEEP}


@pytest.mark.parametrize("diffuse", [True, False], ids=["diffuse", "mirror"])
@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("name", sc.SCENES)
def test_caller_rays_equal_trace_ray_iterative(name, depth, diffuse):
    b = sc.caller_batch(name)
    want = sc.reference(name, depth, diffuse)
    ds = scene(name)
    for flags in (0, BINARY):
        got = ds.shade_rays(b["rays"], b["seeds"], max_depth=depth, diffuse_bounce=diffuse, miss_color=sc.MISS,
                            flags=flags, aov=True)
        bad = np.flatnonzero((bits(got[0]) != bits(want[0])).any(axis=1) | (got[1] != want[1]) | (bits(got[2]) != bits(want[2])))
        print(f"{name} depth {depth} diffuse {diffuse} flags {flags}: variant {ds.shade_rays_variant()}, "
              f"{int((got[1] >= 0).sum())} hits, {bad.size} differ")
        assert bad.size == 0, (bad[:8], got[0][bad[:8]], want[0][bad[:8]], got[1][bad[:8]], want[1][bad[:8]])
        assert ds.shade_rays_variant() == sc.rule_variant(rb.scene_arrays(name), flags)[0]
        if not flags:
            assert ds.shade_rays_variant() == VARIANT[name]
    if name == "chain48":  # DEEP by the "otherwise" rule, not because the scene is deep
        assert not ds.traversal_info()["deep"]
    if name == "chain300":
        assert ds.traversal_info()["deep"]


# ---- 3. edges ---------------------------------------------------------------------------------
EDGE = dict(max_depth=3, diffuse_bounce=True, miss_color=sc.MISS)


def edge_batch():
    """frog's 4096-ray query batch with a seed per ray (directions of every length: the kernel
    is compared with itself here)."""
    rays = rb.batch("frog")["rays"]
    i = np.arange(rays.shape[0])
    return rays, sc.make_rng_seed(i % 61, i % 7, i % 5)


def full_answer():
    if "edge" not in full_answer.__dict__:
        rays, seeds = edge_batch()
        full_answer.edge = scene("frog").shade_rays(rays, seeds, aov=True, **EDGE)
        rad, idx, _ = full_answer.edge
        d1 = scene("frog").shade_rays(rays, seeds, max_depth=1, miss_color=sc.MISS)
        assert (idx >= 0).sum() > 400 and (idx < 0).sum() > 400
        assert (bits(rad) != bits(d1)).any(axis=1).sum() > 100  # the bounces show
    return full_answer.edge


def raw_shade(ds, rays, seeds, n, depth=3, with_aov=True, flags=0):
    """rt_shade_rays over the first n rays into outputs with GUARD sentinel entries behind them."""
    rad = np.full((n + GUARD, 3), SENT_C, np.float32)
    idx = np.full(n + GUARD, SENT_I, np.int32) if with_aov else None
    t = np.full(n + GUARD, SENT_T, np.float32) if with_aov else None
    o = L.ShadeOpts(depth, 1, L.Vec3(*sc.MISS), flags)
    rc = L.lib().rt_shade_rays(ds.handle, rays.ctypes.data, None if seeds is None else seeds.ctypes.data, n, C.byref(o),
                               rad.ctypes.data, None if idx is None else idx.ctypes.data,
                               None if t is None else t.ctypes.data, None)
    return rc, rad, idx, t


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_and_placement(n):
    rays, seeds = edge_batch()
    full = full_answer()
    rc, rad, idx, t = raw_shade(scene("frog"), rays, seeds, n)
    assert rc == 0
    assert same((rad[:n], idx[:n], t[:n]), tuple(v[:n] for v in full))
    assert (rad[n:] == SENT_C).all() and (idx[n:] == SENT_I).all() and (t[n:] == SENT_T).all()
    # hit_idx / hit_t NULL leaves the radiance unchanged
    rc, rad2, _, _ = raw_shade(scene("frog"), rays, seeds, n, with_aov=False)
    assert rc == 0 and np.array_equal(bits(rad2), bits(rad))


def test_a_shuffled_batch_returns_the_shuffled_answers():
    """A lane reading another lane's LDS stack, or its rng state, would show here."""
    rays, seeds = edge_batch()
    full = full_answer()
    perm = np.random.default_rng(7).permutation(rays.shape[0])
    for flags in (0, BINARY):
        got = scene("frog").shade_rays(rays[perm], seeds[perm], aov=True, flags=flags, **EDGE)
        assert same(got, tuple(v[perm] for v in full))


@pytest.mark.parametrize("depth", [0, -1])
def test_no_depth_no_ray(depth):
    rays, seeds = edge_batch()
    rc, rad, idx, t = raw_shade(scene("frog"), rays, seeds, 300, depth=depth)
    assert rc == 0
    assert (bits(rad[:300]) == 0).all() and (idx[:300] == -1).all() and (t[:300] == -1.0).all()
    assert (rad[300:] == SENT_C).all() and (idx[300:] == SENT_I).all() and (t[300:] == SENT_T).all()


def test_default_seeds_are_42():
    rays, _ = edge_batch()
    ds = scene("frog")
    a = ds.shade_rays(rays[:1024], None, aov=True, **EDGE)
    b = ds.shade_rays(rays[:1024], np.full(1024, 42, np.uint32), aov=True, **EDGE)
    c = ds.shade_rays(rays[:1024], np.full(1024, 43, np.uint32), aov=True, **EDGE)
    assert same(a, b)
    assert (bits(a[0]) != bits(c[0])).any()  # the seed is read


# ---- 4. paths ---------------------------------------------------------------------------------
def test_device_path_on_a_side_stream():
    """Rays made by a torch op on a side stream, shaded on that stream with no sync in between."""
    rays, seeds = edge_batch()
    full = full_answer()
    ds = scene("frog")
    dev = torch.device("cuda", 0)
    neg = torch.from_numpy(-rays).to(dev)
    sd = torch.from_numpy(seeds.view(np.int32).copy()).to(dev)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        r = -neg
        rad, idx, t = ds.shade_rays(r, sd, aov=True, **EDGE)
        only = ds.shade_rays(r, sd, flags=BINARY, **EDGE)
        assert ds.shade_rays_variant() == L.RT_RAYS_VARIANT_BINARY
    assert rad.is_cuda and rad.shape == (rays.shape[0], 3) and rad.dtype == torch.float32
    assert idx.dtype == torch.int32 and t.dtype == torch.float32
    side.synchronize()
    assert same((rad.cpu().numpy(), idx.cpu().numpy(), t.cpu().numpy()), full)
    assert np.array_equal(bits(only.cpu().numpy()), bits(full[0]))


def test_a_clone_gives_the_same_answers():
    rays, seeds = edge_batch()
    full = full_answer()
    h = C.c_void_p()
    L.check(L.lib().rt_scene_clone(scene("frog").handle, 0, C.byref(h)))
    try:
        assert L.lib().rt_shade_rays_variant(h) == L.RT_RAYS_VARIANT_NONE
        rad = np.zeros((rays.shape[0], 3), np.float32)
        idx = np.zeros(rays.shape[0], np.int32)
        t = np.zeros(rays.shape[0], np.float32)
        o = L.ShadeOpts(3, 1, L.Vec3(*sc.MISS), 0)
        L.check(L.lib().rt_shade_rays(h, rays.ctypes.data, seeds.ctypes.data, rays.shape[0], C.byref(o), rad.ctypes.data,
                                      idx.ctypes.data, t.ctypes.data, None))
        assert same((rad, idx, t), full)
        assert L.lib().rt_shade_rays_variant(h) == L.RT_RAYS_VARIANT_WIDE
        assert L.lib().rt_trace_rays_variant(h) == L.RT_RAYS_VARIANT_NONE  # a word of its own
    finally:
        L.lib().rt_scene_destroy(h)


def test_shading_beside_a_renderers_frames():
    """Three frames in flight on a Renderer while a batch is shaded against its scene on a stream
    of its own: the frames are the frame rendered alone, no device guard fires, the radiances
    equal the oracle's."""
    name = "cornell"
    hs = host_scene(name + ".json")
    b = sc.caller_batch(name)
    want = sc.reference(name, 3, True)
    cam = hs.camera(64, 48)
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=hs.settings["miss_color"])
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    try:
        kept = r.render(cam, spp=4, max_depth=1, miss_color=hs.settings["miss_color"]).tobytes()
        ds = r.scene(0)
        dev = torch.device("cuda", 0)
        dev_rays = torch.from_numpy(b["rays"].copy()).to(dev)
        dev_seeds = torch.from_numpy(b["seeds"].view(np.int32).copy()).to(dev)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        tickets = [r.submit(cam, o) for _ in range(3)]
        with torch.cuda.stream(side):  # the device path: asynchronous beside the frames
            d = ds.shade_rays(dev_rays, dev_seeds, max_depth=3, miss_color=sc.MISS, aov=True)
        host = ds.shade_rays(b["rays"], b["seeds"], max_depth=3, miss_color=sc.MISS, aov=True)  # the host path
        for k in tickets:
            addr, n = r.wait(k)
            assert bytes((C.c_uint8 * n).from_address(addr)) == kept, k
        assert ds.faults() == 0
        torch.cuda.synchronize()
        assert same(host, want)
        assert same(tuple(v.cpu().numpy() for v in d), want)
    finally:
        r.close()
