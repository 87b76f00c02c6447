"""Refit of a resident scene on the GPU (rt_scene_create_refittable, rt_scene_refit*,
rt_triangles_from_mesh_device), bit for bit (bytes and digests, no tolerance).

For every scene and deformation of tests/refit_cases.py the refit scene's arrays equal the host
restatement's (rt_debug_scene_refit_pack), and its answers — closest hits, occlusion, hit records,
radiance, frames and their P6 bytes — equal the oracle's on (nodes, numpy refit boxes, new
triangles) and those of a scene made fresh from those arrays.  What the restatement itself must
satisfy is pinned on the CPU by tests/test_refit_host.py.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import ray_batches as rb
import refit_cases as rc
import shade_rays_cases as sc
from conftest import host_scene, oracle_camera

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
F = np.float32
W, H, SPP = 64, 48, 2
N_SHADE = 256
CASES = [(s, d) for s in rc.SCENES for d in rc.DEFORMATIONS]
IDS = [f"{s}-{d}" for s, d in CASES]

_scenes: dict = {}


def make(name, tris=None, aabbs=None, refittable=True):
    a = rc.scene(name)
    return rt.DeviceScene(a["P"], a["nodes"], a["aabbs"] if aabbs is None else aabbs, a["tris"] if tris is None else tris,
                          a["triobj"], a["mats"], a["lights"], 0, refittable=refittable)


def scene(name: str):
    """The module's refittable scene of that name (whatever pose the last test left it in)."""
    if name not in _scenes:
        _scenes[name] = make(name)
    return _scenes[name]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


@pytest.fixture(autouse=True)
def _no_faults():
    yield
    for ds in _scenes.values():
        assert ds.faults() == 0


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def posed(name, kind):
    """(the module's scene refitted to the pose, a scene made fresh from the pose's arrays, the
    oracle's arrays for it)."""
    a = rc.scene(name)
    new, boxes = rc.deformed(name, kind), rc.expected_aabbs(name, kind)
    ds = scene(name)
    ds.refit(new)
    fresh = make(name, new, boxes, refittable=False)
    o = {"P": a["P"], "nodes": a["nodes"], "aabbs": boxes, "tris": new, "triobj": a["triobj"], "mats": a["mats"],
         "lights": a["lights"]}
    return ds, fresh, o


# ---- 1. the arrays --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SCENES)
def test_a_refittable_scene_is_the_plain_scene_plus_its_plan(name):
    a = rc.scene(name)
    ds, plain = make(name), make(name, refittable=False)
    try:
        want = rc.pack(a["P"], a["nodes"], a["aabbs"], a["tris"])
        assert rc.same(ds.digest(), want) and rc.same(plain.digest(), want)
        assert ds.device_bytes > plain.device_bytes
        with pytest.raises(L.RTError) as e:
            plain.refit(a["tris"])
        assert e.value.code == -7  # RT_ERR_UNSUPPORTED
        assert rc.same(plain.digest(), want)
    finally:
        ds.close()
        plain.close()


@pytest.mark.parametrize("name,kind", CASES, ids=IDS)
def test_refit_arrays_are_the_host_restatements(name, kind):
    a = rc.scene(name)
    new = rc.deformed(name, kind)
    ds = scene(name)
    ds.refit(new)
    got = ds.digest()
    assert rc.same(got, rc.refit_pack(name, new))
    if kind in ("identity", "times2"):  # a plain pack gives the same bytes (exact scaling keeps every choice)
        assert rc.same(got, rc.pack(a["P"], a["nodes"], rc.expected_aabbs(name, kind), new))


@pytest.mark.parametrize("name", rc.SCENES)
def test_refit_there_and_back(name):
    A, B = rc.deformed(name, "wobble"), rc.deformed(name, "wobble_b")
    ds = scene(name)
    ds.refit(A)
    first = ds.digest()
    ds.refit(B)
    assert rc.same(ds.digest(), rc.refit_pack(name, B)) and not rc.same(ds.digest(), first)
    ds.refit(A)
    assert rc.same(ds.digest(), first) and rc.same(first, rc.refit_pack(name, A))


# ---- 2. the queries -------------------------------------------------------------------------------
def occlusion_case(idx, t):
    """max_t per ray: a hit's cycles over 0.5 t, t, nextafter(t), 2 t, a miss's over 0, 1, FLT_MAX;
    expected: hit and t < max_t (IsInShadow's strict test)."""
    i = np.arange(idx.size)
    tt = np.where(idx >= 0, t, F(1)).astype(F)
    hit_cycle = np.stack([tt * F(0.5), tt, np.nextafter(tt, F(np.inf)), tt * F(2)])
    miss_cycle = np.stack([np.zeros_like(tt), np.ones_like(tt), np.full_like(tt, np.finfo(F).max)])
    max_t = np.where(idx >= 0, hit_cycle[i % 4, i], miss_cycle[i % 3, i]).astype(F)
    return max_t, (idx >= 0) & (t < max_t)


def hit_records(o, rays, idx):
    """The records rt_trace_hits must give: rt_hit_record_host's arithmetic on each hit ray and its
    triangle, the ids as assignMaterialToHit reads them; a miss is tri -1, t -1, zero elsewhere."""
    want = np.zeros(idx.size, rt.HIT_DTYPE)
    want["tri"], want["t"] = -1, F(-1)
    k = np.flatnonzero(idx >= 0)
    if k.size:
        rec = rt.hit_record_host(rays[k], o["tris"][idx[k]])
        assert (rec["tri"] >= 0).all()
        oid = np.ascontiguousarray(o["triobj"], np.int32)[idx[k]]
        rec["tri"], rec["object_id"] = idx[k], oid
        rec["material"] = np.where((oid >= 0) & (oid < len(o["mats"])), oid, -1)
        want[k] = rec
    return want


def shade_batch(o, light, seed=1):
    """N_SHADE unit rays around the pose (make_rays' classes A, B and C aimed at float32 points, as
    shade_rays_cases.make_caller_batch makes them), with per-ray seeds."""
    q = N_SHADE // 3 + 1
    raw = rb.make_rays(o["aabbs"], o["tris"], light, 4 * q, seed)
    pick = np.concatenate([np.arange(q), np.arange(q, 2 * q - 1), np.arange(2 * q, 3 * q - 1)])[:N_SHADE]
    org = np.ascontiguousarray(raw[pick, :3], F)
    p = (org + raw[pick, 3:]).astype(F)
    i = np.arange(pick.size)
    x, y = sc.pixel_of(i)
    return org, p, sc.unit_rays(org, p), sc.make_rng_seed(x, y, np.zeros_like(i))


@pytest.mark.parametrize("name,kind", CASES, ids=IDS)
def test_refit_scene_answers_ray_queries_as_the_oracle(name, kind):
    ds, fresh, o = posed(name, kind)
    try:
        light = rc.scene(name)["light"]
        rays = rb.make_rays(o["aabbs"], o["tris"], light, rb.N_RAYS, rb.SEED)  # around the NEW root box
        idx, t = rb.oracle_trace(o["P"], o["nodes"], o["aabbs"], o["tris"], rays)
        max_t, occ = occlusion_case(idx, t)
        want_hits = hit_records(o, rays, idx)
        print(f"{name} {kind}: {int((idx >= 0).sum())} hits, {int(occ.sum())} occluded")
        for flags in (0, BINARY):
            for s in (ds, fresh):
                gi, gt = s.trace_rays(rays, flags=flags)
                assert np.array_equal(gi, idx) and same_bytes(gt, t), (flags, s is ds)
                assert np.array_equal(s.trace_rays(rays, mode="occluded", max_t=max_t, flags=flags), occ)
                assert same_bytes(s.trace_hits(rays, flags=flags), want_hits)
        org, p, urays, seeds = shade_batch(o, light)
        want = np.zeros((N_SHADE, 3), F)
        for i in range(N_SHADE):
            x, y = sc.pixel_of(i)
            want[i] = sc.oracle_shade(o, org[i], p[i], x, y, 3, True, sc.MISS)[0]
        for s in (ds, fresh):
            got = s.shade_rays(urays, seeds, max_depth=3, miss_color=sc.MISS)
            assert same_bytes(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    finally:
        fresh.close()


# ---- 3. frames ------------------------------------------------------------------------------------
def frame(ds, cam, depth, miss):
    """(float bits, P6 bytes) of a frame rendered into device memory."""
    opts, _jit = ds.make_opts(spp=SPP, max_depth=depth, miss_color=miss)
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    p6 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    ds.render_device(cam, opts, rgb.data_ptr(), p6_dev_ptr=p6.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), p6.cpu().numpy()


def oracle_frame(o, cam, depth, miss):
    from oracle import pyoracle as orc

    ref = orc.render_g(o["P"], oracle_camera(cam), o["nodes"], o["aabbs"], o["tris"], o["triobj"], o["mats"], o["lights"],
                       spp=SPP, max_depth=depth, miss=miss)
    return ref, orc.ppm_quantize(ref, 255, True, True).astype(np.uint8).reshape(H, W, 3)


@pytest.mark.parametrize("name,kind", CASES, ids=IDS)
def test_refit_scene_renders_the_oracles_frames(name, kind):
    ds, fresh, o = posed(name, kind)
    try:
        cams = {"front": rc.camera(name, kind, W, H), "aside": rc.camera(name, kind, W, H, aside=True)}
        if kind == "moved":  # the camera left behind sees nothing of the scene any more
            cams["old"] = rc.camera(name, kind, W, H, follow=False)
        for cname, cam in cams.items():
            for depth in (1, 3):
                ref, ref6 = oracle_frame(o, cam, depth, sc.MISS)
                rgb, p6 = frame(ds, cam, depth, sc.MISS)
                live, total = ds.live_tiles()
                print(f"{name} {kind} {cname} depth {depth}: {live} of {total} tiles live")
                assert same_bytes(rgb, ref) and same_bytes(p6, ref6), (cname, depth)
                frgb, fp6 = frame(fresh, cam, depth, sc.MISS)
                assert same_bytes(frgb, ref) and same_bytes(fp6, ref6), (cname, depth)
                assert fresh.live_tiles() == (live, total)  # the same boxes cull the same tiles
                if cname == "old":
                    assert same_bytes(rgb, np.broadcast_to(np.array(sc.MISS, F), (H, W, 3)))
                # part of the frame is culled (cornell's camera is inside the box; at x + 4096 the tile
                # bounds are too coarse to clear the root box at this distance)
                if cname == "aside" and name in ("frog", "sphere_single") and kind != "shift4096":
                    assert 0 < live < total
                assert same_bytes(ds.render(cam, spp=SPP, max_depth=depth, miss_color=sc.MISS), ref)
    finally:
        fresh.close()


# ---- 4. meshes on the device ----------------------------------------------------------------------
def _frog_mesh():
    hs = host_scene("frog.json")
    return hs, np.ascontiguousarray(hs.positions, F), np.ascontiguousarray(hs.indices, np.uint32).reshape(-1, 3)


def test_triangles_from_mesh_are_the_hosts():
    hs, pos, idx = _frog_mesh()
    dev = torch.device("cuda", 0)
    tpos = torch.from_numpy(pos).to(dev)
    tidx = torch.from_numpy(idx.view(np.int32)).to(dev)
    assert hs.normals is not None
    nrm = np.ascontiguousarray(hs.normals, F)
    with_n = rt.triangles_from_mesh(tpos, tidx, torch.from_numpy(nrm).to(dev))
    assert with_n.is_cuda and same_bytes(with_n.cpu().numpy(), hs.triangles)
    without = rt.triangles_from_mesh(pos, idx).cpu().numpy()
    want = np.ascontiguousarray(hs.triangles, F).copy()
    want[:, 9:] = 0
    assert same_bytes(without, want)
    bad = idx.copy()
    bad[len(bad) // 2, 1] = pos.shape[0]  # one past the vertices
    with pytest.raises(L.RTError) as e:
        rt.triangles_from_mesh(pos, bad)
    assert e.value.code == -1  # RT_ERR_ARG


def test_device_loop_deform_mesh_refit_render():
    """Positions deformed in a tensor -> triangles_from_mesh -> refit -> render: nothing but the frame
    leaves the GPU, and it is the oracle's."""
    hs, pos, idx = _frog_mesh()
    a = rc.scene("frog")
    dev = torch.device("cuda", 0)
    tpos = torch.from_numpy(pos).to(dev)
    tidx = torch.from_numpy(idx.view(np.int32)).to(dev)
    tnrm = torch.from_numpy(np.ascontiguousarray(hs.normals, F)).to(dev)
    moved = tpos.clone()
    moved[:, 0] += 0.05 * torch.sin(4.0 * tpos[:, 2])
    tris = rt.triangles_from_mesh(moved, tidx, tnrm)
    ds = scene("frog")
    ds.refit(tris)
    new = tris.cpu().numpy()
    assert not same_bytes(new, a["tris"])
    o = {"P": a["P"], "nodes": a["nodes"], "aabbs": rc.numpy_refit_aabbs(a["nodes"], new), "tris": new,
         "triobj": a["triobj"], "mats": a["mats"], "lights": a["lights"]}
    assert rc.same(ds.digest(), rc.refit_pack("frog", new))
    cam = rc.camera("frog", "identity", W, H)
    for depth in (1, 3):
        ref, ref6 = oracle_frame(o, cam, depth, sc.MISS)
        rgb, p6 = frame(ds, cam, depth, sc.MISS)
        assert same_bytes(rgb, ref) and same_bytes(p6, ref6)


# ---- 5. clones, refusals, streams -----------------------------------------------------------------
def test_a_clone_refits_to_the_same_arrays():
    ds = scene("cornell")
    ds.refit(rc.deformed("cornell", "wobble"))
    h = C.c_void_p()
    L.check(L.lib().rt_scene_clone(ds.handle, 0, C.byref(h)))
    clone = rt.DeviceScene._borrow(h.value, ds.num_triangles, None)
    try:
        assert rc.same(clone.digest(), ds.digest())
        assert clone.device_bytes == ds.device_bytes
        B = rc.deformed("cornell", "wobble_b")
        clone.refit(B)
        assert rc.same(clone.digest(), rc.refit_pack("cornell", B))
        assert rc.same(ds.digest(), rc.refit_pack("cornell", rc.deformed("cornell", "wobble")))  # the source stays
        assert clone.faults() == 0
    finally:
        L.lib().rt_scene_destroy(h)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_vertex_that_is_not_finite_leaves_the_scene_untouched(bad):
    ds = scene("frog")
    ds.refit(rc.deformed("frog", "wobble"))
    before = ds.digest()
    t = rc.deformed("frog", "moved").copy()
    t[len(t) - 1, 8] = bad
    with pytest.raises(L.RTError) as e:
        ds.refit(t)
    assert e.value.code == -1  # RT_ERR_ARG
    with pytest.raises(L.RTError) as e:
        ds.refit(torch.from_numpy(t).to("cuda"))
    assert e.value.code == -1
    assert rc.same(ds.digest(), before)


def test_refit_on_a_side_stream_then_a_frame_on_the_default_stream():
    name, kind = "frog", "moved"
    a = rc.scene(name)
    new = rc.deformed(name, kind)
    ds = scene(name)
    ds.refit(rc.deformed(name, "identity"))
    cam = rc.camera(name, kind, W, H)
    frame(ds, rc.camera(name, "identity", W, H), 1, sc.MISS)  # (a frame of the old pose first: streams and lists in use)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tris = torch.from_numpy(new.copy()).to("cuda")
    side.synchronize()
    ms = ds.refit(tris, stream=side.cuda_stream, timing=True)
    assert ms > 0
    o = {"P": a["P"], "nodes": a["nodes"], "aabbs": rc.expected_aabbs(name, kind), "tris": new, "triobj": a["triobj"],
         "mats": a["mats"], "lights": a["lights"]}
    ref, ref6 = oracle_frame(o, cam, 1, sc.MISS)
    rgb, p6 = frame(ds, cam, 1, sc.MISS)
    assert same_bytes(rgb, ref) and same_bytes(p6, ref6)
    assert rc.same(ds.digest(), rc.refit_pack(name, new))
