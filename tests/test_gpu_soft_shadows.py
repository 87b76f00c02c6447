"""Soft shadows from spherical area lights on the GPU (rt_light_visibility_device,
rt_path_step_vis_device), with no tolerance against tests/soft_shadow_cases.py's
numpy model (uint32 views; the model is pinned on the CPU by tests/test_soft_shadows_host.py):

* the visibilities and the rng afterwards on every scene and shape set, in WIDE, BINARY and DEEP,
  at every built group size and at 0; samples below, at and across the group size;
* batch sizes around the wave, the block and the groups of a wave, guard words, permuted ids, ids
  of RT_PATH_NONE;
* the staged path: all-point shapes are shade_rays, soft shapes are the model's path, a
  render_rays frame is the model's frame;
* a refitted and a rebuilt scene, a side stream beside frames, a clone's own variant word;
* argument errors launch nothing; non-finite records leave every byte written.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import path_cases as pc
import ray_batches as rb
import refit_cases as rc
import shade_fuzz as sf
import shade_rays_cases as sc
import soft_shadow_cases as ss

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
DEV = torch.device("cuda", 0)
GROUPS = (0,) + tuple(L.LIGHT_VIS_GROUPS)
F, U = np.float32, np.uint32
_scenes: dict = {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("soft_shadows_gpu")


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name, scene_dir):
    if name not in _scenes:
        a = ss.scene_arrays(name, scene_dir)
        _scenes[name] = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"])
    return _scenes[name]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, F).view(U)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == U:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(DEV)


def hits_tensor(rec):
    return dev(np.ascontiguousarray(rec).view(np.int32).reshape(-1, 16))


def state_of(seeds):
    n = len(seeds)
    return rt.PathState(torch.zeros((n, 3), dtype=torch.float32, device=DEV), torch.ones((n, 3), dtype=torch.float32, device=DEV),
                        dev(np.asarray(seeds, U)))


def run_vis(ds, rec, seeds, shp, ids=None, **kw):
    st = state_of(seeds)
    vis = ds.light_visibility(hits_tensor(rec), st, None if ids is None else dev(np.asarray(ids, U)), shp, **kw)
    return vis.cpu().numpy(), st.rng.cpu().numpy().view(U)


def variants_of(a):
    v = {0: sc.rule_variant(a)[0]}
    if sc.rule_variant(a, BINARY)[0] != v[0]:
        v[BINARY] = sc.rule_variant(a, BINARY)[0]
    return v


def sweep_kinds(name):
    return ss.SHAPE_SETS + (tuple(f"s{s}" for s in ss.SWEEP) if name in ("penumbra", "s_l1_d4m") else ())


# ---- 1. the stage against the model -------------------------------------------------------------
@pytest.mark.parametrize("name", ss.SCENES)
def test_visibility_and_rng_equal_the_model(name, scene_dir):
    """Every shape set (on two one-light scenes every sample count of the sweep as well: below, at
    and across each group size), every variant the scene has, every group size and 0."""
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    nl = e["lights"].size
    assert ds.num_lights == nl
    hits = hits_tensor(e["rec"])
    for kind in sweep_kinds(name):
        want = ss.model(name, kind)
        shp = ss.shapes(kind, nl)
        for flags, variant in variants_of(e["scene"]).items():
            for g in GROUPS:
                st = state_of(e["seeds"])
                vis = ds.light_visibility(hits, st, None, shp, lanes_per_entry=g, flags=flags)
                assert ds.light_visibility_variant() == variant
                bad = (bits(vis) != bits(want["vis"])).any(axis=1)
                assert not bad.any(), (name, kind, flags, g, int(bad.sum()), np.flatnonzero(bad)[:4])
                assert np.array_equal(st.rng.cpu().numpy().view(U), want["rng"]), (name, kind, flags, g)
    assert ds.faults() == 0


def test_the_scenes_cover_the_three_variants(scene_dir):
    seen = set()
    for name in ss.SCENES:
        seen |= set(variants_of(ss.entries(name, scene_dir)["scene"]).values())
    assert seen == {L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP}
    v = ss.model("penumbra", "s64")["vis"]
    assert ((v > 0) & (v < 1)).sum() >= 32  # the fractions are exercised, not only 0 and 1


# ---- 2. batch sizes, guard words, ids ------------------------------------------------------------
# 3: the last group of a wave stays partial at every group size (8 entries per wave at G = 8, 2 at
# G = 32); 13: a partial wave at G = 8 that is more than one wave at G = 32.
@pytest.mark.parametrize("m", (1, 3, 13, 63, 64, 65, 257, 4096))
def test_batch_sizes_guard_words_and_ids(m, scene_dir):
    name = "s_l3_d1"
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    n, nl = e["rec"].shape[0], e["lights"].size
    want = ss.model(name, "mixed")
    shp = ss.shapes("mixed", nl)
    k = np.arange(m) % n  # past the entries: from their start again, as paths of their own
    hits = hits_tensor(e["rec"][k])
    rs = np.random.default_rng(m)
    perm = rs.permutation(m).astype(U)
    none = perm.copy()
    none[rs.random(m) < 0.3] = L.RT_PATH_NONE
    for ids in (None, perm, none):
        for g in GROUPS:
            seeds = np.zeros(m + 2, U)  # two state words no entry names
            seeds[:] = 0xDEADBEEF
            own = np.arange(m) if ids is None else ids
            live = own != L.RT_PATH_NONE
            seeds[own[live]] = e["seeds"][k][live]
            st = state_of(seeds)
            buf = torch.full((m * nl + 64,), float("nan"), dtype=torch.float32, device=DEV)
            vis = buf[:m * nl].view(m, nl)
            sh = ds._shape_tensor(shp, "test")
            L.check(L.lib().rt_light_visibility_device(ds.handle, m, hits.data_ptr(), None if ids is None else dev(ids).data_ptr(),
                                                       sh.data_ptr(), st.rng.data_ptr(), g, 0, vis.data_ptr(),
                                                       torch.cuda.current_stream(DEV).cuda_stream))
            torch.cuda.synchronize()
            assert torch.isnan(buf[m * nl:]).all(), (m, g)  # the guard words
            exp = np.where(live[:, None], want["vis"][k], F(0.0))
            assert np.array_equal(bits(vis), bits(exp)), (m, g, ids is None)
            exp_rng = seeds.copy()
            exp_rng[own[live]] = want["rng"][k][live]
            assert np.array_equal(st.rng.cpu().numpy().view(U), exp_rng), (m, g)


# ---- 3. the staged path --------------------------------------------------------------------------
def staged(ds, rays, seeds, depth, diffuse, shp, g=0, flags=0):
    """The path from the primitives, every depth through the two new stages."""
    state = ds.path_begin(rays.shape[0], seeds)
    cur, ids = rays.clone(), None
    for d in range(depth):
        last = d + 1 == depth
        hits = ds.trace_hits(cur, flags)
        vis = ds.light_visibility(hits, state, ids, shp, lanes_per_entry=g, flags=flags)
        nxt, alive = ds.path_step(cur, hits, state, ids, None, diffuse, sc.MISS, flags, last=last, vis=vis)
        if last:
            break
        cur, ids, count = rt.compact_paths(alive, nxt, ids)
        if count == 0:
            break
    return rt.path_finish(state)


@pytest.mark.parametrize("depth", (1, 4))
@pytest.mark.parametrize("name", ("cornell", "s_l8_d4", "chain600"))
def test_all_point_shapes_are_shade_rays(name, depth, scene_dir):
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    rays, seeds = dev(e["rays"]), dev(e["seeds"])
    shp = ss.shapes("point", e["lights"].size)
    mono = ds.shade_rays(rays, seeds, max_depth=depth, diffuse_bounce=True, miss_color=sc.MISS)
    got = ds.trace_paths(rays, seeds, depth, True, sc.MISS, light_shapes=shp)
    assert np.array_equal(bits(got), bits(mono))
    for g in L.LIGHT_VIS_GROUPS:  # ... and through the two new stages themselves
        assert np.array_equal(bits(staged(ds, rays, seeds, depth, True, shp, g)), bits(mono)), g
    if name == "cornell" and depth in sc.DEPTHS:  # (its entries are the caller batch the oracle shaded)
        assert np.array_equal(bits(mono), bits(sc.reference(name, depth, True)[0]))


@pytest.mark.parametrize("name, kind", [("penumbra", "s8"), ("s_l3_d1", "mixed"), ("cornell", "soft")])
def test_soft_paths_at_depth_4_are_the_models(name, kind, scene_dir):
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    n = 256
    shp = ss.shapes(kind, e["lights"].size)
    want = ss.cpu_staged_soft_path(e["scene"], e["rays"][:n], e["seeds"][:n], 4, True, sc.MISS, shp)
    got = ds.trace_paths(dev(e["rays"][:n]), dev(e["seeds"][:n]), 4, True, sc.MISS, light_shapes=shp)
    assert np.array_equal(bits(got), bits(want))
    hard = ds.trace_paths(dev(e["rays"][:n]), dev(e["seeds"][:n]), 4, True, sc.MISS)
    assert (bits(hard) != bits(want)).any()
    assert ds.faults() == 0


def test_a_render_rays_frame_is_the_models_frame(scene_dir):
    """48 x 32 at spp 4 of the penumbra scene, depth 2, film included."""
    hs = ss.penumbra(scene_dir)["hs"]
    ds = scene("penumbra", scene_dir)
    W, H, spp = 48, 32, 4
    cam = hs.camera(W, H)
    shp = hs.light_shapes
    assert shp["radius"][0] > 0 and shp["shadow_samples"][0] == 8
    rays, seeds = rt.camera_rays(cam, spp)
    rad = ss.cpu_staged_soft_path(ss.penumbra()["arrays"], rays, seeds, 2, False, (0, 0, 0), shp)
    want = rt.film_pixels_host(rad, W, H, spp)[1]
    got = ds.render_rays(cam, spp, 2, False, light_shapes=shp)
    assert np.array_equal(bits(got).reshape(H, W, 3), bits(want).reshape(H, W, 3))
    banded = ds.render_rays(cam, spp, 2, False, light_shapes=shp, pass_spp=2, band_rows=10)
    assert np.array_equal(bits(banded), bits(got))
    plain = ds.render_rays(cam, spp, 2, False)
    assert (bits(plain) != bits(got)).any()
    assert np.array_equal(bits(ds.render_rays(cam, spp, 2, False, light_shapes=ss.shapes("point", 1))), bits(plain))


# ---- 4. scene states -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("cornell", "wobble"), ("chain300", "times2")])
def test_refitted_and_rebuilt_scenes(name, kind):
    a = rc.scene(name)
    new = rc.deformed(name, kind)
    ds = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], 0, refittable=True)
    try:
        lights = np.ascontiguousarray(a["lights"], rt.LIGHT_DTYPE)
        shp = ss.shapes("soft", lights.size)
        for step in ("refit", "rebuild"):
            if step == "refit":
                ds.refit(new)
                nodes, aabbs = a["nodes"], rt.refit_aabbs(a["nodes"], new)
            else:
                ds.rebuild(new)
                nodes, aabbs = rt.build_bvh_triangles(new)
            o = {"P": a["P"], "nodes": np.ascontiguousarray(nodes).view(U).reshape(-1, 4),
                 "aabbs": np.ascontiguousarray(aabbs, F).reshape(-1, 6), "tris": new, "triobj": a["triobj"], "mats": a["mats"],
                 "lights": lights}
            r = rb.make_rays(o["aabbs"], new, a["light"], 512, rb.SEED)  # around the NEW root box
            idx, _ = rb.oracle_trace(o["P"], o["nodes"], o["aabbs"], new, r)
            rec = pc.records(o, r, idx)
            seeds = (np.arange(512, dtype=np.uint64) * np.uint64(40503) + np.uint64(7)).astype(U)
            want = ss.model_visibility(o, rec, lights, shp, seeds)
            assert (want["vis"] > 0).any() and (want["vis"] < 1).any() and (want["rng"] != seeds).any()
            if name == "cornell":
                assert ((want["vis"] > 0) & (want["vis"] < 1)).any()
            for flags in (0, BINARY):
                for g in GROUPS:
                    vis, rng = run_vis(ds, rec, seeds, shp, lanes_per_entry=g, flags=flags)
                    assert np.array_equal(bits(vis), bits(want["vis"])) and np.array_equal(rng, want["rng"]), (step, flags, g)
    finally:
        ds.close()


def test_a_side_stream_beside_frames_of_the_same_scene(scene_dir):
    name = "penumbra"
    hs = ss.penumbra(scene_dir)["hs"]
    e = ss.entries(name, scene_dir)
    want = ss.model(name, "s64")
    shp = ss.shapes("s64", 1)
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        cam = hs.camera(64, 48)
        opts, _jit = ds.make_opts(spp=4, max_depth=2)
        frames = [torch.zeros((48, 64, 3), dtype=torch.float32, device=DEV) for _ in range(4)]
        ds.render_device(cam, opts, frames[0].data_ptr())
        hits = hits_tensor(e["rec"])
        st = state_of(e["seeds"])
        side = torch.cuda.Stream(DEV)
        torch.cuda.synchronize(DEV)
        for f in frames[1:]:
            ds.render_device(cam, opts, f.data_ptr())
        with torch.cuda.stream(side):
            vis = ds.light_visibility(hits, st, None, shp)
        side.synchronize()
        torch.cuda.synchronize(DEV)
        assert np.array_equal(bits(vis), bits(want["vis"])) and np.array_equal(st.rng.cpu().numpy().view(U), want["rng"])
        assert ds.faults() == 0
        for f in frames[1:]:
            assert torch.equal(f, frames[0])
    finally:
        ds.close()


def test_a_clone_has_a_variant_word_of_its_own(scene_dir):
    name = "cornell"
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    want = ss.model(name, "soft")
    shp = ss.shapes("soft", e["lights"].size)
    ds.light_visibility(hits_tensor(e["rec"]), state_of(e["seeds"]), None, shp, flags=BINARY)
    assert ds.light_visibility_variant() == L.RT_RAYS_VARIANT_BINARY
    h = C.c_void_p()
    L.check(L.lib().rt_scene_clone(ds.handle, 0, C.byref(h)))
    try:
        assert L.lib().rt_light_visibility_variant(h) == L.RT_RAYS_VARIANT_NONE
        clone = rt.DeviceScene._borrow(h.value, ds.num_triangles, None)
        vis, rng = run_vis(clone, e["rec"], e["seeds"], shp)
        assert np.array_equal(bits(vis), bits(want["vis"])) and np.array_equal(rng, want["rng"])
        assert L.lib().rt_light_visibility_variant(h) == L.RT_RAYS_VARIANT_WIDE
        assert ds.light_visibility_variant() == L.RT_RAYS_VARIANT_BINARY and ds.path_step_variant() in (0, 1, 2, 3)
    finally:
        L.lib().rt_scene_destroy(h)


# ---- 5. bad inputs ---------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(scene_dir):
    name = "s_l3_d1"
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    nl = e["lights"].size
    m = 64
    hits = hits_tensor(e["rec"][:m])
    st = state_of(e["seeds"][:m])
    shp = ds._shape_tensor(ss.shapes("soft", nl), "test")
    vis = torch.full((m, nl), -7.0, dtype=torch.float32, device=DEV)
    before = st.rng.clone()
    lib = L.lib()

    def call(hits_p=hits.data_ptr(), ids_p=None, shp_p=shp.data_ptr(), rng_p=st.rng.data_ptr(), g=0, flags=0,
             vis_p=vis.data_ptr(), mm=m):
        return lib.rt_light_visibility_device(ds.handle, mm, hits_p, ids_p, shp_p, rng_p, g, flags, vis_p, None)

    assert call(g=2) == -1 and call(g=64) == -1 and call(g=-1) == -1 and call(flags=1) == -1 and call(flags=16) == -1
    assert call(hits_p=None) == -1 and call(shp_p=None) == -1 and call(rng_p=None) == -1 and call(vis_p=None) == -1
    assert call(hits_p=hits.data_ptr() + 4) == -1 and call(vis_p=vis.data_ptr() + 2) == -1
    assert call(mm=1 << 31) == -7
    big = ss.shapes("soft", nl)
    big["shadow_samples"][nl - 1] = 257
    assert call(shp_p=ds._shape_tensor(big, "test").data_ptr()) == -7 and "shadow_samples" in lib.rt_last_error().decode()
    assert call(mm=0) == 0
    torch.cuda.synchronize()
    assert (vis == -7.0).all() and torch.equal(st.rng, before)  # nothing ran
    with pytest.raises(ValueError):
        ds.light_visibility(hits[:, :15].contiguous(), st)
    with pytest.raises(ValueError):
        ds.light_visibility(hits, st, light_shapes=ss.shapes("soft", nl + 1))
    with pytest.raises(ValueError):
        ds.path_step(dev(e["rays"][:m]), hits, st, vis=vis[:, :1].contiguous())
    assert call() == 0 and ds.light_visibility(hits[:0], st).shape == (0, nl)


def test_non_finite_records_leave_every_byte_written(scene_dir):
    name = "s_l3_d1"
    e = ss.entries(name, scene_dir)
    ds = scene(name, scene_dir)
    nl = e["lights"].size
    k = np.flatnonzero(e["rec"]["tri"] >= 0)[:240]
    rec = np.array(e["rec"][k])
    bad = (np.nan, np.inf, -np.inf, 1e38, -1e38, 0.0)
    for i in range(rec.shape[0]):
        f = ("p", "normal")[i % 2]
        rec[f][i, (i // 2) % 3] = bad[(i // 6) % len(bad)]
    rec["normal"][200:220] = 0.0
    rec["p"][220:240] = e["lights"]["position"][1]  # the point sits on a light
    for kind in ("mixed", "soft"):
        for g in GROUPS:
            st = state_of(e["seeds"][k])
            buf = torch.full((rec.shape[0] * nl + 16,), -7.0, dtype=torch.float32, device=DEV)
            vis = buf[:rec.shape[0] * nl].view(-1, nl)
            sh = ds._shape_tensor(ss.shapes(kind, nl), "test")
            L.check(L.lib().rt_light_visibility_device(ds.handle, rec.shape[0], hits_tensor(rec).data_ptr(), None, sh.data_ptr(),
                                                       st.rng.data_ptr(), g, 0, vis.data_ptr(), None))
            torch.cuda.synchronize()
            v = vis.cpu().numpy()
            assert ((v >= 0) & (v <= 1)).all() and (buf[rec.shape[0] * nl:] == -7.0).all(), (kind, g)
            # the host build draws the same numbers for the same words
            rng = np.array(e["seeds"][k], U)
            rt.light_samples_host(rec, e["lights"], ss.shapes(kind, nl), rng)
            assert np.array_equal(st.rng.cpu().numpy().view(U), rng), (kind, g)
            nxt, alive = ds.path_step(dev(e["rays"][k]), hits_tensor(rec), st, vis=vis.contiguous(), miss_color=sc.MISS)
            torch.cuda.synchronize()
            assert nxt.shape == (rec.shape[0], 6) and int(alive.max()) <= 1
    assert ds.faults() == 0
