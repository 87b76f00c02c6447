"""The closest-point query on the GPU (rt_closest_points*), bytes and no tolerance:

* parity per scene with the host build (which tests/test_closest_points_host.py holds against the
  model of tests/closest_point_cases.py): every point class, unbounded and with per-point bounds,
  the 4-ary and the binary records, the deep kernel and the completion of a lane whose stack filled
  up; the variant rule;
* batch sizes around the wave and the block, outputs pre-filled with a pattern, a null evals;
* a refitted and a rebuilt scene against the model;
* a call on a side stream beside frames of the same scene;
* argument errors on a live scene, a clone's own variant word;
* non-finite points;
* the pruning: the walk evaluates a small part of the scene.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import closest_point_cases as cp
import refit_cases as rc
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
W_, B_, D_ = L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP
# scene -> the variants (flags 0, RT_FLAG_BINARY) the rule must give
VARIANTS = {"sphere_single": (W_, B_), "frog": (W_, B_), "cornell": (W_, B_), "chain24": (W_, B_), "chain300": (D_, D_),
            "chain600": (D_, D_), "small": (W_, B_), "scaled": (W_, B_), cp.MOVED: (W_, B_)}
GUARD = 16
FILL = 0xA5
F32 = np.float32

_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    if name not in _scenes:
        _scenes[name] = cp.device_scene(name)
    return _scenes[name]


@pytest.fixture(scope="module")
def host():
    """rt.closest_points_host on the scene's 4096 points per (scene, bound), computed once."""
    memo = {}

    def get(name, bound="none"):
        if (name, bound) not in memo:
            a = cp.arrays(name)
            memo[name, bound] = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], cp.points(name),
                                                       cp.max_d2(name, bound))
        return memo[name, bound]

    return get


# ---- 1. parity per scene -----------------------------------------------------------------------
@pytest.mark.parametrize("bound", cp.BOUNDS)
@pytest.mark.parametrize("name", cp.SCENES)
def test_device_equals_the_host_build(name, bound, host):
    ds = scene(name)
    q = cp.points(name)
    md = cp.max_d2(name, bound)
    want = host(name, bound)
    n_leaf = cp.leaves(cp.arrays(name))["tri"].size
    for i, flags in enumerate((0, BINARY)):
        got = ds.closest_points(q, max_d2=md, flags=flags, evals=True)
        bad = cp.differing_points(got[:6], want)
        assert bad.size == 0, (name, bound, flags, bad[:4], [g[bad[:4]] for g in got[:6]], [w[bad[:4]] for w in want])
        assert all(cp.same_bytes(g, w) for g, w in zip(got[:6], want))
        assert ds.closest_points_variant() == VARIANTS[name][i]
        ev = got[6]
        assert ev.dtype == np.uint32 and (ev <= n_leaf).all()
        for c, sl in cp.class_slices().items():
            print(f"{name} {bound} variant {VARIANTS[name][i]} class {c}: mean evals {ev[sl].mean():.2f} of {n_leaf} leaves, "
                  f"most {int(ev[sl].max())}")
        if name == "chain600" and bound == "none":
            # a near-first walk down the chain pushes a leaf per level: some lane fills the 512
            # entries and takes the completion, whose count is every leaf
            assert (ev == n_leaf).sum() >= 1
            assert (ev < n_leaf).sum() >= 1
    assert ds.traversal_info()["deep"] == (name in ("chain300", "chain600"))


# ---- 2. sizes, padding, a null evals -----------------------------------------------------------
def raw_query(ds, q, n, flags=0, max_d2=None, evals=True):
    """rt_closest_points over the first n points into outputs filled with FILL, GUARD entries more
    behind each; the records start 4 bytes into their buffer (the host entry needs no alignment)."""
    rec = np.full(4 + (n + GUARD) * 32, FILL, np.uint8)
    ev = np.full((n + GUARD) * 4, FILL, np.uint8)
    rc_ = L.lib().rt_closest_points(ds.handle, q.ctypes.data, None if max_d2 is None else max_d2.ctypes.data, n, flags,
                                    rec.ctypes.data + 4, ev.ctypes.data if evals else None, None)
    return rc_, rec[4:4 + n * 32].view(rt.POINT_HIT_DTYPE), rec[4 + n * 32:], ev[:n * 4].view(np.uint32), ev[n * 4:]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
@pytest.mark.parametrize("name", ["frog", "small", "chain600"])
def test_batch_sizes_and_placement(name, n, host):
    q = cp.points(name)
    for bound in cp.BOUNDS:
        md = cp.max_d2(name, bound)
        want = host(name, bound)
        for flags in (0, BINARY):
            rc_, rec, g1, ev, g2 = raw_query(scene(name), q, n, flags, md)
            assert rc_ == 0
            for f, w in zip(cp.FIELDS, want):
                assert cp.same_bytes(np.ascontiguousarray(rec[f]), w[:n]), (bound, flags, f)
            assert (g1 == FILL).all() and (g2 == FILL).all()
            assert (ev >= 1).any() or (rec["tri"] < 0).all()
            # a null evals: the same records, and the evals buffer is not touched
            rc_, rec2, g1, ev2, _ = raw_query(scene(name), q, n, flags, md, evals=False)
            assert rc_ == 0 and rec2.tobytes() == rec.tobytes() and (g1 == FILL).all()
            assert (ev2.view(np.uint8) == FILL).all()


def test_the_miss_record_is_written_whole():
    """Bounds of 0, NaN and -1 for far points: the miss record over the fill pattern."""
    miss = np.zeros(1, rt.POINT_HIT_DTYPE)
    miss["tri"], miss["d2"], miss["region"] = -1, -1.0, -1
    for name in ("cornell", "chain300"):
        q = np.ascontiguousarray(cp.points(name)[cp.class_slices()["d"]][:300])
        md = np.zeros(300, F32)
        md[1::3] = np.nan
        md[2::3] = -1.0
        for flags in (0, BINARY):
            rc_, rec, g1, ev, g2 = raw_query(scene(name), q, 300, flags, md)
            assert rc_ == 0 and rec.tobytes() == miss.tobytes() * 300
            assert (g1 == FILL).all() and (g2 == FILL).all()


# ---- 3. refit and rebuild ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("cornell", "wobble"), ("chain300", "times2"), ("frog", "wobble")])
def test_refitted_and_rebuilt_scenes(name, kind):
    a = rc.scene(name)
    new = rc.deformed(name, kind)
    ds = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], 0, refittable=True)
    n = 256 if name == "frog" else 1024
    try:
        for step in ("refit", "rebuild"):
            if step == "refit":
                ds.refit(new)
                nodes, aabbs = a["nodes"], rt.refit_aabbs(a["nodes"], new)
            else:
                ds.rebuild(new)
                nodes, aabbs = rt.build_bvh_triangles(new)
            o = {"P": a["P"], "nodes": np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4),
                 "aabbs": np.ascontiguousarray(aabbs, F32).reshape(-1, 6), "tris": np.ascontiguousarray(new, F32).reshape(-1, 18)}
            q = cp.make_points(o, n, seed=31)  # around the NEW root box, on the NEW triangles
            m = cp.model_answers(o, q)
            md = cp.bounds_around(m)
            m2 = cp.model_answers(o, q, md)
            assert (m["tri"] >= 0).all() and (m2["tri"] < 0).sum() >= n // 8
            for flags in (0, BINARY):
                for mm, bound in ((m, None), (m2, md)):
                    got = ds.closest_points(q, max_d2=bound, flags=flags)
                    bad = cp.differing_points(got, cp.as_tuple(mm))
                    assert bad.size == 0, (step, flags, bad[:4], [g[bad[:4]] for g in got], [w[bad[:4]] for w in cp.as_tuple(mm)])
    finally:
        ds.close()


# ---- 4. streams --------------------------------------------------------------------------------
def test_a_side_stream_beside_frames_of_the_same_scene(host):
    """Frames in flight on the scene's own streams while a batch runs on a side stream, device
    tensors in and out: the same bytes as the host build, and the frames are the frame alone."""
    name = "cornell"
    hs = host_scene(name + ".json")
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        q = cp.points(name)
        md = cp.max_d2(name, "around")
        want = host(name, "around")
        cam = hs.camera(64, 48)
        opts, _jit = ds.make_opts(spp=4, max_depth=2, miss_color=hs.settings["miss_color"])
        dev = torch.device("cuda", 0)
        frames = [torch.zeros((48, 64, 3), dtype=torch.float32, device=dev) for _ in range(4)]
        ds.render_device(cam, opts, frames[0].data_ptr())
        torch.cuda.synchronize(dev)
        neg = torch.from_numpy(-q).to(dev)
        dmd = torch.from_numpy(md.copy()).to(dev)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        for f in frames[1:]:
            ds.render_device(cam, opts, f.data_ptr())
        with torch.cuda.stream(side):
            pts = -neg
            got = ds.closest_points(pts, max_d2=dmd)
            got_b = ds.closest_points(pts, max_d2=dmd, flags=BINARY, evals=True)
        assert got[0].is_cuda and got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[5].dtype == torch.int32
        assert got[2].shape == (q.shape[0], 3) and got[0].shape == got[1].shape == got[5].shape == (q.shape[0],)
        side.synchronize()
        torch.cuda.synchronize(dev)
        for g in (got, got_b[:6]):
            assert all(cp.same_bytes(x.cpu().numpy(), w) for x, w in zip(g, want))
        assert (got_b[6].cpu().numpy() >= 0).all()
        assert all(cp.same_bytes(x, w) for x, w in zip(ds.closest_points(q, max_d2=md), want))  # the host path
        assert ds.faults() == 0
        for f in frames[1:]:
            assert torch.equal(f, frames[0])
        with pytest.raises(ValueError):
            ds.closest_points(pts[:, :2])
        with pytest.raises(ValueError):
            ds.closest_points(pts, timing=True)
        with pytest.raises(ValueError):
            ds.closest_points(pts, max_d2=dmd[:5])
        with pytest.raises(ValueError):
            ds.closest_points(q[:, :2])
        c0 = ds.closest_points(pts[:0])
        assert c0[0].shape == (0,) and c0[2].shape == (0, 3)
        out = ds.closest_points(q, timing=True)
        assert out[-1] > 0 and all(cp.same_bytes(x, w) for x, w in zip(out[:6], host(name)))
    finally:
        ds.close()


# ---- 5. arguments on a live scene --------------------------------------------------------------
def test_argument_errors_launch_nothing():
    ds = scene("frog")
    lib = L.lib()
    dev = torch.device("cuda", 0)
    n = 256
    pts = torch.from_numpy(cp.points("frog")[:n].copy()).to(dev)
    rec = torch.full((n * 8 + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ev = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    Q, H, E = pts.data_ptr(), rec.data_ptr(), ev.data_ptr()
    ds.closest_points(cp.points("frog")[:8])
    before = ds.closest_points_variant()
    assert before == W_
    cases = [((None, Q, None, n, 0, H, E), -1), ((ds.handle, None, None, n, 0, H, E), -1),
             ((ds.handle, Q, None, n, 0, None, E), -1), ((ds.handle, Q, None, n, 8, H, E), -1),
             ((ds.handle, Q, None, n, 0, H + 4, E), -1), ((ds.handle, Q + 2, None, n, 0, H, E), -1),
             ((ds.handle, Q, None, 1 << 31, 0, H, E), -7)]
    for args, code in cases:
        assert lib.rt_closest_points_device(*args, None) == code, args
        assert lib.rt_last_error()
    assert lib.rt_closest_points_device(ds.handle, Q, None, 0, 0, H, E, None) == 0  # no points: no launch
    torch.cuda.synchronize(dev)
    assert (rec == 0x5A5A5A5A).all().item() and (ev == 0x5A5A5A5A).all().item()
    assert ds.closest_points_variant() == before
    # a clone keeps a word of its own
    clone = C.c_void_p()
    L.check(lib.rt_scene_clone(ds.handle, 0, C.byref(clone)))
    try:
        assert lib.rt_closest_points_variant(clone) == L.RT_RAYS_VARIANT_NONE
        assert lib.rt_closest_points_device(clone, Q, None, n, BINARY, H, E, None) == 0
        torch.cuda.synchronize(dev)
        assert lib.rt_closest_points_variant(clone) == B_ and ds.closest_points_variant() == before
        assert lib.rt_trace_multi_hits_variant(clone) == L.RT_RAYS_VARIANT_NONE
        a = cp.arrays("frog")
        want = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], cp.points("frog")[:n])
        got = rec[:n * 8].cpu().numpy().view(rt.POINT_HIT_DTYPE)
        for f, w in zip(cp.FIELDS, want):
            assert cp.same_bytes(np.ascontiguousarray(got[f]), w), f
        assert (rec[n * 8:] == 0x5A5A5A5A).all().item()
    finally:
        lib.rt_scene_destroy(clone)


# ---- 6. unspecified inputs ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["frog", "chain600"])
def test_non_finite_points_return_and_fill_every_output(name):
    ds = scene(name)
    n = 512
    q = cp.points(name)[:n].copy()
    q[0::8, 0] = np.nan
    q[1::8, 1] = np.inf
    q[2::8] = -np.inf
    q[3::8] = np.nan
    q[4::8, 2] = F32(3e38)
    md = np.full(n, np.inf, F32)
    md[::5] = np.nan
    for flags in (0, BINARY):
        for bound in (None, md):
            rc_, rec, g1, ev, g2 = raw_query(ds, q, n, flags, bound)
            assert rc_ == 0
            assert (g1 == FILL).all() and (g2 == FILL).all()
            won = rec["tri"] >= 0
            assert ((rec["region"] >= 0) == won).all() and (rec["region"] <= 6).all() and (rec["tri"] < ds.num_triangles).all()
            assert (rec["d2"][~won] == -1.0).all() and not rec["p"][~won].any() and not rec["v"][~won].any()
            assert not won[0::8].any() and not won[3::8].any()  # a NaN coordinate: a NaN D never wins
            assert (ev <= cp.leaves(cp.arrays(name))["tri"].size).all()
            # the finite points beside them are answered as ever
            a = cp.arrays(name)
            fin = np.flatnonzero(np.isfinite(q).all(axis=1) & (np.abs(q) < 1e30).all(axis=1))
            want = rt.closest_points_host(a["nodes"], a["aabbs"], a["tris"], q[fin], None if bound is None else bound[fin])
            for f, w in zip(cp.FIELDS, want):
                assert cp.same_bytes(np.ascontiguousarray(rec[f][fin]), w), f
    assert ds.faults() == 0


# ---- 7. the walk prunes ------------------------------------------------------------------------
def test_the_walk_evaluates_a_small_part_of_frog():
    """Classes a and b: the mean number of triangles a lane evaluates stays below P/20 (a scan of
    every leaf would be P).  tests/test_closest_points_host.py shows the floor, the leaves whose own
    box is no further than the answer, far below that."""
    ds = scene("frog")
    P = int(cp.arrays("frog")["P"])
    sl = cp.class_slices()
    q = np.ascontiguousarray(np.vstack([cp.points("frog")[sl["a"]], cp.points("frog")[sl["b"]]]))
    m = cp.model("frog")
    ms = cp.class_slices(m["idx"].size)
    floor = np.concatenate([m["floor"][ms["a"]], m["floor"][ms["b"]]]).mean()
    per = ms["a"].stop - ms["a"].start  # the model answers the first `per` points of each class
    for flags in (0, BINARY):
        ev = ds.closest_points(q, flags=flags, evals=True)[6]
        on_model = np.concatenate([ev[:per], ev[1024:1024 + per]]).mean()
        print(f"frog classes a, b, flags {flags}: mean evals {ev.mean():.2f} (a {ev[:1024].mean():.2f}, b {ev[1024:].mean():.2f}), "
              f"most {int(ev.max())}; on the model's points {on_model:.2f} against the floor's mean {floor:.2f}: "
              f"ratio {on_model / floor:.2f}; P/20 = {P / 20:.0f}")
        assert ev.min() >= 1 and ev.mean() < P / 20
