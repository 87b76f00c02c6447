"""Rebuild of a resident scene on the GPU (rt_scene_rebuild*), bit for bit (bytes
and digests, no tolerance).

After a rebuild the scene's tree is rt_build_bvh_triangles of the pose, its arrays and facts are
rt_debug_scene_pack's of (tree, pose), its plan refits as rt_debug_scene_refit_pack says, and its
answers — closest hits, occlusion, hit records, radiance, a frame and its P6 bytes — are the oracle's
on (tree, pose) and those of a scene made fresh from those arrays.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import ray_batches as rb
import rebuild_cases as rbc
import refit_cases as rc
import shade_rays_cases as sc
from conftest import host_scene
from test_gpu_refit import hit_records, occlusion_case, oracle_frame, same_bytes, shade_batch

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
F = np.float32
W, H, SPP = 96, 54, 4
N_RAYS = 1024
N_SHADE = 256
CASES = [(s, k) for s in rbc.DEVICE_SCENES for k in rbc.poses_of(s)]
IDS = [f"{s}-{k}" for s, k in CASES]
ANSWER_CASES = [("sphere_single", "wobble"), ("cornell", "wobble"), ("frog", "wobble"), ("frog", "flat"), ("ties", "identity"),
                ("same500", "identity"), ("soup65", "identity"), ("soup1025", "identity")]

_scenes: dict = {}


def make(name, refittable=True, nodes=None, aabbs=None, tris=None):
    a = rbc.scene(name)
    return rt.DeviceScene(a["P"], a["nodes"] if nodes is None else nodes, a["aabbs"] if aabbs is None else aabbs,
                          a["tris"] if tris is None else tris, a["triobj"], a["mats"], a["lights"], 0, refittable=refittable)


def scene(name: str):
    """The module's refittable scene of that name (whatever the last test left under it)."""
    if name not in _scenes:
        _scenes[name] = make(name)
    return _scenes[name]


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()
    rt.reset_tuning()


@pytest.fixture(autouse=True)
def _no_faults():
    yield
    for ds in _scenes.values():
        assert ds.faults() == 0


def check_rebuilt(ds, name, kind, path=L.RT_REBUILD_DEVICE):
    """rebuild(pose) gave the host's tree and the host pack's words and arrays, by the wanted path."""
    nodes, aabbs = ds.rebuild(rbc.pose(name, kind), tree=True)
    want_nodes, want_aabbs = rbc.tree(name, kind)
    assert same_bytes(nodes, want_nodes), "nodes"
    assert same_bytes(aabbs, want_aabbs), "aabbs"
    diff = rbc.differences(ds.digest(), rbc.expected(name, kind))
    assert not diff, f"{name} {kind}: differs from rt_debug_scene_pack in {diff}"
    assert ds.rebuild_path == path, f"{name} {kind}: path {ds.rebuild_path}, wanted {path}"


# ---- 1. the arrays --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", CASES, ids=IDS)
def test_rebuilt_arrays_are_the_host_packs(name, kind):
    ds = scene(name)
    assert ds.rebuild_path in (L.RT_REBUILD_NONE, L.RT_REBUILD_DEVICE, L.RT_REBUILD_HOST)
    check_rebuilt(ds, name, kind)
    a = rbc.scene(name)
    assert ds.device_bytes > 0 and ds.num_triangles == a["P"]


def test_device_bytes_follow_the_new_sizes():
    ds = scene("cornell")
    check_rebuilt(ds, "cornell", "wobble")
    nodes, aabbs = rbc.tree("cornell", "wobble")
    fresh = make("cornell", nodes=nodes, aabbs=aabbs, tris=rbc.pose("cornell", "wobble"))
    try:
        assert ds.device_bytes == fresh.device_bytes
        assert rc.same(ds.digest(), fresh.digest())
    finally:
        fresh.close()


# ---- 2. the plan ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rbc.DEVICE_SCENES)
def test_a_rebuilt_scene_refits_by_its_new_plan_and_rebuilds_back(name):
    kind = "wobble" if name in rbc.SHIPPED else "identity"
    ds = scene(name)
    check_rebuilt(ds, name, kind)
    first = ds.digest()
    ds.refit(rbc.pose(name, "wobble_b"))
    diff = rbc.differences(ds.digest(), rbc.refit_expected(name, kind, "wobble_b"))
    assert not diff, f"{name}: the refit of the rebuilt scene differs from rt_debug_scene_refit_pack in {diff}"
    assert not rc.same(ds.digest(), first)
    check_rebuilt(ds, name, kind)
    assert rc.same(ds.digest(), first)


# ---- 3. the answers -------------------------------------------------------------------------------
def camera_of(name, kind, o):
    if name in rbc.SHIPPED:
        return rc.camera(name, kind, W, H)
    lo, hi = o["aabbs"][0, :3].astype(np.float64), o["aabbs"][0, 3:].astype(np.float64)
    c, e = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    return rt.Camera(tuple(c + np.array([0.3 * e, 0.2 * e, 2.5 * e])), tuple(c), (0.0, 1.0, 0.0), 30.0, 24.0, W, H)


def frame(ds, cam, depth, miss):
    opts, _jit = ds.make_opts(spp=SPP, max_depth=depth, miss_color=miss)
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    p6 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    ds.render_device(cam, opts, rgb.data_ptr(), p6_dev_ptr=p6.data_ptr())
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), p6.cpu().numpy()


def oracle_frame_wh(o, cam, depth, miss):
    from conftest import oracle_camera
    from oracle import pyoracle as orc

    ref = orc.render_g(o["P"], oracle_camera(cam), o["nodes"], o["aabbs"], o["tris"], o["triobj"], o["mats"], o["lights"],
                       spp=SPP, max_depth=depth, miss=miss)
    return ref, orc.ppm_quantize(ref, 255, True, True).astype(np.uint8).reshape(H, W, 3)


@pytest.mark.parametrize("name,kind", ANSWER_CASES, ids=[f"{s}-{k}" for s, k in ANSWER_CASES])
def test_a_rebuilt_scene_answers_as_the_oracle_on_the_new_tree(name, kind):
    ds = scene(name)
    check_rebuilt(ds, name, kind)
    o = rbc.oracle_arrays(name, kind)
    fresh = make(name, refittable=False, nodes=o["nodes"], aabbs=o["aabbs"], tris=o["tris"])
    try:
        light = rbc.scene(name)["light"]
        rays = rb.make_rays(o["aabbs"], o["tris"], light, N_RAYS, rb.SEED)
        idx, t = rb.oracle_trace(o["P"], o["nodes"], o["aabbs"], o["tris"], rays)
        max_t, occ = occlusion_case(idx, t)
        want_hits = hit_records(o, rays, idx)
        print(f"{name} {kind}: {int((idx >= 0).sum())} of {N_RAYS} rays hit, {int(occ.sum())} occluded")
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
        cam = camera_of(name, kind, o)
        ref, ref6 = oracle_frame_wh(o, cam, 3, sc.MISS)
        for s in (ds, fresh):
            rgb, p6 = frame(s, cam, 3, sc.MISS)
            assert same_bytes(rgb, ref) and same_bytes(p6, ref6), s is ds
    finally:
        fresh.close()


# ---- 4. the arity fallback and the cut knobs -----------------------------------------------------------
KNOBS = [({"frustum_stack_cap": 128}, 5), ({"frustum_stack_cap": 60}, 4), ({"frustum_stack_cap": 40}, 3),
         ({"frustum_stack_cap": 25}, 2), ({"frustum_arity": 3}, 3), ({"frustum_arity": 2}, 2),
         ({"cull_boxes": 8, "cut_sub": 4}, 5)]


@pytest.mark.parametrize("knobs,f_log2", KNOBS, ids=["-".join(f"{k}{v}" for k, v in kn.items()) for kn, _ in KNOBS])
def test_rebuild_under_the_record_and_cut_knobs(knobs, f_log2):
    ds = scene("cornell")
    try:
        for k, v in knobs.items():
            rt.set_tuning(k, v)
        assert int(rbc.expected("cornell", "wobble")[0][8]) == f_log2
        check_rebuilt(ds, "cornell", "wobble")
        assert int(ds.digest()[0][8]) == f_log2
    finally:
        rt.reset_tuning()


# ---- 5. the host path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("knob,value", [("record_greedy", 1), ("wide4_greedy", 2)])
def test_other_record_rules_take_the_host_path(knob, value):
    ds = scene("cornell")
    try:
        rt.set_tuning(knob, value)
        check_rebuilt(ds, "cornell", "wobble", path=L.RT_REBUILD_HOST)
    finally:
        rt.reset_tuning()


def test_a_single_triangle_takes_the_host_path():
    check_rebuilt(scene("p1"), "p1", "identity", path=L.RT_REBUILD_HOST)


def test_quantised_records_are_refused_and_nothing_changes():
    ds = scene("cornell")
    check_rebuilt(ds, "cornell", "identity")
    before = ds.digest()
    try:
        rt.set_tuning("quant_records", 1)
        with pytest.raises(L.RTError) as e:
            ds.rebuild(rbc.pose("cornell", "wobble"))
        assert e.value.code == -7  # RT_ERR_UNSUPPORTED
    finally:
        rt.reset_tuning()
    assert rc.same(ds.digest(), before)


def test_a_scene_that_is_not_refittable_is_refused():
    a = rbc.scene("cornell")
    plain = make("cornell", refittable=False)
    try:
        before = plain.digest()
        for tris in (a["tris"], torch.from_numpy(np.array(a["tris"])).to("cuda")):
            with pytest.raises(L.RTError) as e:
                plain.rebuild(tris)
            assert e.value.code == -7
        assert rc.same(plain.digest(), before) and plain.rebuild_path == L.RT_REBUILD_NONE
    finally:
        plain.close()


# ---- 6. the weights -----------------------------------------------------------------------------------
def test_device_box_weights_are_the_hosts_bit_for_bit():
    aabbs = rbc.scene("frog")["aabbs"]
    rng = np.random.default_rng(rbc.SEED)
    special = np.zeros((8, 6), F)
    special[0] = (1, 2, 3, 1, 2, 3)                # zero extent
    special[1] = (0, 0, 0, 1, 0, 0)                # one extent
    special[2] = (-1e30, -1e30, -1e30, 1e30, 1e30, 1e30)
    special[3] = (0, 0, 0, 1e30, 1e-30, 1e30)
    special[4] = (0, 0, 0, 3e38, 3e38, 3e38)
    special[5] = (1, 1, 1, 0, 2, 2)                # a negative extent counts 0
    special[6] = (-0.0, 0.0, -0.0, 0.0, -0.0, 0.0)
    special[7] = (0, 0, 0, 1e-20, 1e-20, 1e-20)
    pw = (1 << np.arange(1, 31)).astype(np.int64)
    leaves = np.unique(np.concatenate([np.arange(1, 4097), pw - 1, pw, pw + 1])).astype(np.uint32)
    boxes = np.vstack([aabbs[rng.integers(0, aabbs.shape[0], leaves.size - 2 * len(special))], special, special])
    boxes = np.ascontiguousarray(boxes[rng.permutation(leaves.size)], F)
    lib = L.lib()
    for rule in (1, 2):
        host, dev = np.zeros(leaves.size, np.float64), np.zeros(leaves.size, np.float64)
        L.check(lib.rt_debug_box_weight_host(L.ptr(boxes), L.ptr(leaves), rule, leaves.size, L.ptr(host)))
        L.check(lib.rt_debug_box_weight_batch(0, L.ptr(boxes), L.ptr(leaves), rule, leaves.size, L.ptr(dev)))
        bad = np.flatnonzero(host.view(np.uint64) != dev.view(np.uint64))
        print(f"rule {rule}: {leaves.size} weights, {bad.size} differ")
        assert bad.size == 0, [(int(leaves[i]), boxes[i].tolist(), host[i].hex(), dev[i].hex()) for i in bad[:4]]


# ---- 7. untouched on error ----------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_vertex_that_is_not_finite_leaves_the_scene_untouched(bad):
    ds = scene("sphere_single")
    check_rebuilt(ds, "sphere_single", "wobble")
    before = ds.digest()
    o = rbc.oracle_arrays("sphere_single", "wobble")
    rays = rb.make_rays(o["aabbs"], o["tris"], rbc.scene("sphere_single")["light"], N_RAYS, rb.SEED)
    hits = ds.trace_rays(rays)
    t = rbc.pose("sphere_single", "flat").copy()
    t[len(t) // 2, 4] = bad
    for tris in (t, torch.from_numpy(t).to("cuda")):
        with pytest.raises(L.RTError) as e:
            ds.rebuild(tris)
        assert e.value.code == -1  # RT_ERR_ARG
    assert rc.same(ds.digest(), before)
    again = ds.trace_rays(rays)
    assert np.array_equal(again[0], hits[0]) and same_bytes(again[1], hits[1])


# ---- 8. around it ---------------------------------------------------------------------------------
def test_a_clone_of_a_rebuilt_scene_rebuilds_to_the_same_arrays():
    ds = scene("cornell")
    check_rebuilt(ds, "cornell", "wobble")
    h = C.c_void_p()
    L.check(L.lib().rt_scene_clone(ds.handle, 0, C.byref(h)))
    clone = rt.DeviceScene._borrow(h.value, ds.num_triangles, None)
    try:
        assert rc.same(clone.digest(), ds.digest()) and clone.device_bytes == ds.device_bytes
        check_rebuilt(clone, "cornell", "flat")
        clone.refit(rbc.pose("cornell", "wobble_b"))
        assert rc.same(clone.digest(), rbc.refit_expected("cornell", "flat", "wobble_b"))
        assert rc.same(ds.digest(), rbc.expected("cornell", "wobble"))  # the source stays
        assert clone.faults() == 0
    finally:
        L.lib().rt_scene_destroy(h)


def test_rebuild_on_a_side_stream_then_a_frame_on_the_default_stream():
    name, kind = "sphere_single", "shift4096"
    ds = scene(name)
    check_rebuilt(ds, name, "identity")
    frame(ds, rc.camera(name, "identity", W, H), 1, sc.MISS)  # (a frame of the old pose first: streams and lists in use)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        tris = torch.from_numpy(np.array(rbc.pose(name, kind))).to("cuda")
    side.synchronize()
    ms, nodes, aabbs = ds.rebuild(tris, stream=side.cuda_stream, timing=True, tree=True)
    assert ms > 0
    o = rbc.oracle_arrays(name, kind)
    assert same_bytes(nodes.cpu().numpy().view(np.uint32), o["nodes"]) and same_bytes(aabbs.cpu().numpy(), o["aabbs"])
    cam = rc.camera(name, kind, W, H)
    ref, ref6 = oracle_frame_wh(o, cam, 1, sc.MISS)
    rgb, p6 = frame(ds, cam, 1, sc.MISS)
    assert same_bytes(rgb, ref) and same_bytes(p6, ref6)
    assert not rbc.differences(ds.digest(), rbc.expected(name, kind))
    assert ds.rebuild_path == L.RT_REBUILD_DEVICE


def test_device_loop_deform_mesh_rebuild_render():
    """Positions deformed in a tensor -> triangles_from_mesh -> rebuild -> render: no host copy of the
    geometry on the way in, and the frame is the oracle's on the host tree of those triangles."""
    hs = host_scene("frog.json")
    a = rbc.scene("frog")
    dev = torch.device("cuda", 0)
    tpos = torch.from_numpy(np.ascontiguousarray(hs.positions, F)).to(dev)
    tidx = torch.from_numpy(np.ascontiguousarray(hs.indices, np.uint32).reshape(-1, 3).view(np.int32)).to(dev)
    tnrm = torch.from_numpy(np.ascontiguousarray(hs.normals, F)).to(dev)
    moved = tpos.clone()
    moved[:, 0] += 0.05 * torch.sin(4.0 * tpos[:, 2])
    tris = rt.triangles_from_mesh(moved, tidx, tnrm)
    ds = scene("frog")
    ds.rebuild(tris)
    assert ds.rebuild_path == L.RT_REBUILD_DEVICE
    new = tris.cpu().numpy()
    nodes, aabbs = rt.build_bvh_triangles(new)
    assert not rbc.differences(ds.digest(), rc.pack(a["P"], nodes, aabbs, new))
    o = {"P": a["P"], "nodes": nodes, "aabbs": aabbs, "tris": new, "triobj": a["triobj"], "mats": a["mats"], "lights": a["lights"]}
    cam = rc.camera("frog", "identity", W, H)
    ref, ref6 = oracle_frame_wh(o, cam, 3, sc.MISS)
    rgb, p6 = frame(ds, cam, 3, sc.MISS)
    assert same_bytes(rgb, ref) and same_bytes(p6, ref6)
