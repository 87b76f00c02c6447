"""The multi-hit query on the GPU (rt_trace_multi_hits*), bytes and no tolerance:

* parity per scene with the host build (which tests/test_multi_hit_host.py holds against the model
  of tests/multi_hit_cases.py): every k of KS, the 4-ary and the binary records, the deep kernel and
  its brute-force completion, unbounded and with per-ray bounds; the variant rule;
* batch sizes around the wave and the block, outputs pre-filled with a pattern, k = 0 with no
  records at all;
* the closest-hit query's answer inside the list;
* a refitted and a rebuilt scene;
* a call on a side stream beside frames of the same scene;
* argument errors on a live scene.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import multi_hit_cases as mh
import ray_batches as rb
import refit_cases as rc
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
W_, B_, D_ = L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP
# scene -> the variants (flags 0, RT_FLAG_BINARY) the rule must give
VARIANTS = {"sphere_single": (W_, B_), "frog": (W_, B_), "cornell": (W_, B_), "chain24": (W_, B_), "chain300": (D_, D_),
            "chain600": (D_, D_), "small": (W_, B_), "scaled": (W_, B_)}
GUARD = 16
FILL = 0xA5

_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    if name not in _scenes:
        _scenes[name] = mh.device_scene(name)
    return _scenes[name]


@pytest.fixture(scope="module")
def host():
    """rt.multi_hits_host per (scene, k, bound), computed once."""
    memo = {}

    def get(name, k, bound="none"):
        if (name, k, bound) not in memo:
            a = mh.arrays(name)
            mt = None if bound == "none" else mh.model(name, bound)["max_t"]
            memo[name, k, bound] = rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], mh.rays(name), k, mt)
        return memo[name, k, bound]

    return get


# ---- 1. parity per scene -----------------------------------------------------------------------
@pytest.mark.parametrize("bound", mh.BOUNDS)
@pytest.mark.parametrize("name", mh.SCENES)
def test_device_equals_the_host_build(name, bound, host):
    ds = scene(name)
    r = mh.rays(name)
    mt = None if bound == "none" else mh.model(name, bound)["max_t"]
    for i, flags in enumerate((0, BINARY)):
        for k in mh.KS:
            got, want = ds.trace_multi_hits(r, k, max_t=mt, flags=flags), host(name, k, bound)
            bad = mh.differing_rays(got, want)
            assert bad.size == 0, (name, bound, flags, k, bad[:4], got[0][bad[:4]], want[0][bad[:4]])
            assert all(mh.same_bytes(g, w) for g, w in zip(got, want))
            assert ds.multi_hits_variant() == VARIANTS[name][i]
        assert np.array_equal(ds.count_hits(r, max_t=mt, flags=flags), host(name, 0, bound)[0])
    c = host(name, 0, bound)[0]
    print(f"{name} {bound}: variants {VARIANTS[name]}, {int(c.sum())} hits, most {int(c.max())}")
    assert ds.traversal_info()["deep"] == (name in ("chain300", "chain600"))


# ---- 2. sizes, padding, k = 0 ------------------------------------------------------------------
def raw_trace(ds, rays, n, k, flags=0, max_t=None, hits=True, count=True):
    """rt_trace_multi_hits over the first n rays into outputs filled with FILL, GUARD entries more
    behind each; the records start 4 bytes into their buffer (the host entry needs no alignment)."""
    rec = np.full(4 + (n * k + GUARD) * 16, FILL, np.uint8)
    cnt = np.full((n + GUARD) * 4, FILL, np.uint8)
    rc_ = L.lib().rt_trace_multi_hits(ds.handle, rays.ctypes.data, None if max_t is None else max_t.ctypes.data, n, k, flags,
                                      rec.ctypes.data + 4 if hits else None, cnt.ctypes.data if count else None, None)
    return rc_, rec[4:4 + n * k * 16].view(rt.MULTI_HIT_DTYPE).reshape(n, k), rec[4 + n * k * 16:], \
        cnt[:n * 4].view(np.int32), cnt[n * 4:]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
@pytest.mark.parametrize("name", ["frog", "small", "chain600"])
def test_batch_sizes_and_placement(name, n, host):
    r = mh.rays(name)
    for flags in (0, BINARY):
        for k in (1, 5, 32):  # 256-thread blocks and, for k > 16, 128-thread ones
            want = host(name, k)
            rc_, rec, g1, cnt, g2 = raw_trace(scene(name), r, n, k, flags)
            assert rc_ == 0
            assert np.array_equal(cnt, want[0][:n])
            for f, w in zip(("tri", "t", "u", "v"), want[1:]):
                assert mh.same_bytes(np.ascontiguousarray(rec[f]), w[:n]), (k, f)
            assert (g1 == FILL).all() and (g2 == FILL).all()


@pytest.mark.parametrize("name", ["sphere_single", "chain300"])
def test_every_output_byte_is_written(name, host):
    """Slots past count hold the miss entry over the fill pattern; count alone, records alone."""
    r = mh.rays(name)
    n = 4096
    miss = np.zeros(1, rt.MULTI_HIT_DTYPE)
    miss["tri"], miss["t"] = -1, -1.0
    for flags in (0, BINARY):
        for k in (2, 8, 32):
            want = host(name, k)
            rc_, rec, g1, cnt, g2 = raw_trace(scene(name), r, n, k, flags)
            assert rc_ == 0 and np.array_equal(cnt, want[0][:n])
            past = np.arange(k)[None, :] >= np.minimum(cnt, k)[:, None]
            assert past.sum() >= 1000 and (~past).sum() >= 1000
            assert rec[past].tobytes() == miss.tobytes() * int(past.sum())
            assert (rec["tri"][~past] >= 0).all()
            # records alone (a null count), and nothing else is touched
            rc_, rec2, g1, cnt2, _ = raw_trace(scene(name), r, n, k, flags, count=False)
            assert rc_ == 0 and rec2.tobytes() == rec.tobytes() and (g1 == FILL).all() and (cnt2.view(np.uint8) == FILL).all()


@pytest.mark.parametrize("name", ["frog", "chain600"])
def test_k_zero_counts_without_records(name, host):
    r = mh.rays(name)
    for bound in mh.BOUNDS:
        mt = None if bound == "none" else mh.model(name, bound)["max_t"]
        for flags in (0, BINARY):
            rc_, rec, g1, cnt, g2 = raw_trace(scene(name), r, 4096, 0, flags, max_t=mt, hits=False)
            assert rc_ == 0 and np.array_equal(cnt, host(name, 0, bound)[0][:4096])
            assert np.array_equal(cnt, host(name, 8, bound)[0][:4096])  # the same counts as with a list
            assert (g1 == FILL).all() and (g2 == FILL).all()


# ---- 3. beside the closest-hit query -----------------------------------------------------------
@pytest.mark.parametrize("name", mh.SCENES)
def test_the_closest_hit_is_in_the_list(name):
    ds = scene(name)
    r = mh.rays(name)
    for flags in (0, BINARY):
        idx, t = ds.trace_rays(r, flags=flags)
        count, tri, tt, _, _ = ds.trace_multi_hits(r, 32, flags=flags)
        assert np.array_equal(count > 0, idx >= 0)
        hit = idx >= 0
        assert (tt[hit, 0] <= t[hit]).all()
        whole = hit & (count <= 32)
        assert whole.sum() >= 64  # at least a wave of rays whose whole hit set is in the list
        at = (tri[whole] == idx[whole][:, None]) & (tt[whole].view(np.uint32) == t[whole].view(np.uint32)[:, None])
        assert at.any(axis=1).all(), np.flatnonzero(whole)[~at.any(axis=1)][:4]


# ---- 4. refit and rebuild ----------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("cornell", "wobble"), ("chain300", "times2"), ("frog", "wobble")])
def test_refitted_and_rebuilt_scenes(name, kind):
    a = rc.scene(name)
    new = rc.deformed(name, kind)
    ds = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], 0, refittable=True)
    try:
        for step in ("refit", "rebuild"):
            if step == "refit":
                ds.refit(new)
                nodes, aabbs = a["nodes"], rt.refit_aabbs(a["nodes"], new)
            else:
                ds.rebuild(new)
                nodes, aabbs = rt.build_bvh_triangles(new)
            o = {"P": a["P"], "nodes": np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4),
                 "aabbs": np.ascontiguousarray(aabbs, np.float32).reshape(-1, 6), "tris": new}
            r = rb.make_rays(o["aabbs"], new, a["light"], 1024, rb.SEED)  # around the NEW root box
            m = mh.model_lists(o, r)
            mt = mh.bounds_around(m)
            m2 = mh.model_lists(o, r, mt)
            assert m["count"].sum() >= 256
            for flags in (0, BINARY):
                for k in (0, 4, 32):
                    for mm, bound in ((m, None), (m2, mt)):
                        got, want = ds.trace_multi_hits(r, k, max_t=bound, flags=flags), mh.take(mm, k)
                        bad = mh.differing_rays(got, want)
                        assert bad.size == 0, (step, flags, k, bad[:4], got[0][bad[:4]], want[0][bad[:4]])
    finally:
        ds.close()


# ---- 5. streams --------------------------------------------------------------------------------
def test_a_side_stream_beside_frames_of_the_same_scene(host):
    """Frames in flight on the scene's own streams while a batch runs on a side stream, device
    tensors in and out: the same bytes as the host path alone, and the frames are the frame alone."""
    name = "cornell"
    hs = host_scene(name + ".json")
    ds = rt.DeviceScene.from_host(hs, device=0)
    try:
        a = mh.arrays(name)
        r = mh.rays(name)
        mt = mh.model(name, "around")["max_t"]
        want = rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], r, 8, mt)
        cam = hs.camera(64, 48)
        opts, _jit = ds.make_opts(spp=4, max_depth=2, miss_color=hs.settings["miss_color"])
        dev = torch.device("cuda", 0)
        frames = [torch.zeros((48, 64, 3), dtype=torch.float32, device=dev) for _ in range(4)]
        ds.render_device(cam, opts, frames[0].data_ptr())
        torch.cuda.synchronize(dev)
        neg = torch.from_numpy(-r).to(dev)
        dmt = torch.from_numpy(mt.copy()).to(dev)
        side = torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        for f in frames[1:]:
            ds.render_device(cam, opts, f.data_ptr())
        with torch.cuda.stream(side):
            rays = -neg
            got = ds.trace_multi_hits(rays, 8, max_t=dmt)
            got_b = ds.trace_multi_hits(rays, 8, max_t=dmt, flags=BINARY)
            cnt = ds.count_hits(rays, max_t=dmt)
        assert got[0].is_cuda and got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
        assert got[1].shape == got[2].shape == got[3].shape == got[4].shape == (r.shape[0], 8)
        side.synchronize()
        torch.cuda.synchronize(dev)
        for g in (got, got_b):
            assert all(mh.same_bytes(x.cpu().numpy(), w) for x, w in zip(g, want))
        assert np.array_equal(cnt.cpu().numpy(), want[0])
        assert all(mh.same_bytes(x, w) for x, w in zip(ds.trace_multi_hits(r, 8, max_t=mt), want))  # the host path
        assert ds.faults() == 0
        for f in frames[1:]:
            assert torch.equal(f, frames[0])
        with pytest.raises(ValueError):
            ds.trace_multi_hits(rays[:, :5], 4)
        with pytest.raises(ValueError):
            ds.trace_multi_hits(rays, 4, timing=True)
        with pytest.raises(ValueError):
            ds.trace_multi_hits(rays, 33)
        c0 = ds.trace_multi_hits(rays[:0], 4)
        assert c0[0].shape == (0,) and c0[1].shape == (0, 4)
        out, ms = ds.count_hits(r, timing=True)
        assert ms > 0 and np.array_equal(out, host(name, 0)[0])
    finally:
        ds.close()


# ---- 6. arguments on a live scene --------------------------------------------------------------
def test_argument_errors_launch_nothing():
    ds = scene("frog")
    lib = L.lib()
    dev = torch.device("cuda", 0)
    n = 256
    rays = torch.from_numpy(mh.rays("frog")[:n].copy()).to(dev)
    rec = torch.full((n * 4 * 4 + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    cnt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    R, H, N = rays.data_ptr(), rec.data_ptr(), cnt.data_ptr()
    before = ds.multi_hits_variant()
    cases = [((None, R, None, n, 4, 0, H, N), -1), ((ds.handle, None, None, n, 4, 0, H, N), -1),
             ((ds.handle, R, None, n, 33, 0, H, N), -1), ((ds.handle, R, None, n, -1, 0, H, N), -1),
             ((ds.handle, R, None, n, 4, 0, None, None), -1), ((ds.handle, R, None, n, 0, 0, H, None), -1),
             ((ds.handle, R, None, n, 4, 8, H, N), -1), ((ds.handle, R, None, n, 4, 0, H + 4, N), -1),
             ((ds.handle, R, None, 1 << 31, 0, 0, None, N), -7), ((ds.handle, R, None, 1 << 27, 16, 0, H, N), -7)]
    for args, code in cases:
        assert lib.rt_trace_multi_hits_device(*args, None) == code, args
        assert lib.rt_last_error()
    assert lib.rt_trace_multi_hits_device(ds.handle, R, None, 0, 4, 0, H, N, None) == 0  # no rays: no launch
    torch.cuda.synchronize(dev)
    assert (rec == 0x5A5A5A5A).all().item() and (cnt == 0x5A5A5A5A).all().item()
    assert ds.multi_hits_variant() == before
    # a clone keeps a word of its own
    clone = C.c_void_p()
    L.check(lib.rt_scene_clone(ds.handle, 0, C.byref(clone)))
    try:
        assert lib.rt_trace_multi_hits_variant(clone) == L.RT_RAYS_VARIANT_NONE
        assert lib.rt_trace_multi_hits_device(clone, R, None, n, 4, BINARY, H, N, None) == 0
        torch.cuda.synchronize(dev)
        assert lib.rt_trace_multi_hits_variant(clone) == B_ and ds.multi_hits_variant() == before
        assert lib.rt_trace_hits_variant(clone) == L.RT_RAYS_VARIANT_NONE
        a = mh.arrays("frog")
        want = rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], mh.rays("frog")[:n], 4)
        got = rec[:n * 16].cpu().numpy().view(rt.MULTI_HIT_DTYPE).reshape(n, 4)
        assert np.array_equal(cnt.cpu().numpy(), want[0])
        for f, w in zip(("tri", "t", "u", "v"), want[1:]):
            assert mh.same_bytes(np.ascontiguousarray(got[f]), w), f
    finally:
        lib.rt_scene_destroy(clone)
