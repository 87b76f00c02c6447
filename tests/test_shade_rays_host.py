"""Radiance queries (rt_shade_rays*, include/rt_mi355x.h), the part that needs no device: the
entry points exist, their argument checks answer before any HIP call, and the helper module of
the GPU tests (tests/shade_rays_cases.py) is pinned with the oracle alone: its camera rays are the
reference's, its per-ray references add up to the reference's own frames, and its caller-ray
batches contain what tests/test_gpu_shade_rays.py relies on, so that no GPU test can pass by
emptiness."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L
from oracle import pyoracle as orc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_entry_points_exist():
    lib = L.lib()
    for name in ("rt_shade_opts_default", "rt_shade_rays_device", "rt_shade_rays", "rt_shade_rays_variant"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert callable(rt.DeviceScene.shade_rays) and callable(rt.DeviceScene.shade_rays_variant)
    assert rt.ShadeOpts is L.ShadeOpts and C.sizeof(L.ShadeOpts) == 24
    assert lib.rt_shade_rays_variant(None) == rt.RT_RAYS_VARIANT_NONE
    assert lib.rt_abi_version() == 3
    o = L.ShadeOpts(7, 7, L.Vec3(7, 7, 7), 7)
    lib.rt_shade_opts_default(C.byref(o))
    assert (o.max_depth, o.diffuse_bounce, tuple(o.miss_color), o.flags) == (1, 1, (0.0, 0.0, 0.0), 0)
    lib.rt_shade_opts_default(None)


# A scene handle that is never read: every check below answers before the scene is touched.
_FAKE_SCENE = C.create_string_buffer(64)
_RAYS = np.zeros((4, 6), np.float32)
_SEEDS = np.zeros(4, np.uint32)
_RAD = np.zeros((4, 3), np.float32)
_IDX = np.zeros(4, np.int32)
_T = np.zeros(4, np.float32)
_S, _R, _SD, _C, _I, _TT = (C.addressof(_FAKE_SCENE), _RAYS.ctypes.data, _SEEDS.ctypes.data, _RAD.ctypes.data,
                            _IDX.ctypes.data, _T.ctypes.data)


def _opts(flags=0, depth=1):
    o = L.ShadeOpts()
    L.lib().rt_shade_opts_default(C.byref(o))
    o.flags, o.max_depth = flags, depth
    return o


_O, _O_NOCULL, _O_BIN8, _O_BIN = _opts(), _opts(L.RT_FLAG_NO_CULL), _opts(L.RT_FLAG_BINARY | 8), _opts(L.RT_FLAG_BINARY)
_OP = {k: C.addressof(v) for k, v in (("ok", _O), ("nocull", _O_NOCULL), ("bin8", _O_BIN8), ("bin", _O_BIN))}

# (scene, rays, seeds, n, opt, radiance, hit_idx, hit_t) -> code
ARG_CASES = {
    "null scene": ((None, _R, _SD, 4, _OP["ok"], _C, _I, _TT), -1),
    "null rays": ((_S, None, _SD, 4, _OP["ok"], _C, _I, _TT), -1),
    "null opts": ((_S, _R, _SD, 4, None, _C, _I, _TT), -1),
    "null radiance": ((_S, _R, _SD, 4, _OP["ok"], None, _I, _TT), -1),
    "null radiance, no aov, no seeds": ((_S, _R, None, 4, _OP["bin"], None, None, None), -1),
    "unknown flag": ((_S, _R, _SD, 4, _OP["nocull"], _C, _I, _TT), -1),
    "unknown flag beside BINARY": ((_S, _R, _SD, 4, _OP["bin8"], _C, _I, _TT), -1),
    "n = 2^31": ((_S, _R, _SD, 1 << 31, _OP["ok"], _C, _I, _TT), -7),
    "n = 2^40, binary, no aov": ((_S, _R, None, 1 << 40, _OP["bin"], _C, None, None), -7),
}


@pytest.mark.parametrize("entry", ["rt_shade_rays", "rt_shade_rays_device"])
@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_argument_errors_need_no_device(entry, case):
    args, code = ARG_CASES[case]
    rc = getattr(L.lib(), entry)(*args, None)  # kernel_ms / hip_stream
    assert rc == code, (case, rc, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _RAD.any() and not _IDX.any() and not _T.any()  # nothing was written


def test_empty_batch_is_ok_without_a_device():
    for entry in ("rt_shade_rays", "rt_shade_rays_device"):
        assert getattr(L.lib(), entry)(_S, _R, _SD, 0, _OP["ok"], _C, _I, _TT, None) == 0
        assert getattr(L.lib(), entry)(_S, _R, None, 0, _OP["bin"], _C, None, None, None) == 0
    assert not _RAD.any() and not _IDX.any() and not _T.any()


def test_make_rng_seed():
    assert sc.make_rng_seed(0, 0, 0) == 0 and sc.make_rng_seed(1, 0, 0) == 73856093
    assert sc.make_rng_seed(63, 35, 127) == ((63 * 73856093) ^ (35 * 19349663) ^ (127 * 83492791)) & 0xFFFFFFFF
    i = np.arange(sc.N_CALLER)
    x, y = sc.pixel_of(i)
    assert x.max() < 8 and y.max() < 8 and np.unique(sc.make_rng_seed(x, y, 0 * i)).size == 64


# ---- camera rays: the helper's rays are the reference's ------------------------------------------
def _case_camera(name):
    c = sf.case(name)
    pos, look, up, f, s = c["camera"]
    return rt.Camera(pos, look, up, f, s, c["W"], c["H"])


def case_rays(name):
    c = sf.case(name)
    return sc.camera_rays(_case_camera(name).basis(), c["W"], c["H"], orc.jitter(c["spp"]))


@pytest.mark.parametrize("name", [n for n in sf.CASES if sf.CASES[n][6] <= 16])
def test_camera_rays_reproduce_the_fixture_hits(name):
    """orc_search_bvh on camera_rays equals the reference's per-sample hit indices and t."""
    c = sf.case(name)
    rays, seeds = case_rays(name)
    assert rays.shape == (c["H"] * c["W"] * c["spp"], 6) and seeds.shape == (rays.shape[0],) and seeds.dtype == np.uint32
    _, ghi, ght = sf.fixture_frames(name)
    idx, t = rb.oracle_trace(c["P"], c["nodes"], c["aabbs"], c["tris"], rays)
    assert np.array_equal(idx, ghi.reshape(-1)), int((idx != ghi.reshape(-1)).sum())
    assert np.array_equal(bits(t), bits(ght.reshape(-1)))
    n = np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1)
    assert np.abs(n - 1.0).max() < 1e-6  # unit directions: the only ones the oracle can state


def test_camera_ray_seeds_follow_the_sample_order():
    _, seeds = sc.camera_rays(_case_camera("c_l3_d2").basis(), 32, 24, orc.jitter(5))
    k = ((7 * 32) + 30) * 5 + 3  # y = 7, x = 30, s = 3
    assert seeds[k] == sc.make_rng_seed(30, 7, 3) and seeds[0] == 0 and seeds[1] == 83492791


@pytest.mark.parametrize("name", ["c_l3_d1", "s_l0_d1"])
def test_per_ray_references_add_up_to_the_fixture_frame(name):
    """pixel_sum over oracle_shade's radiances is the reference's own frame (depth 1: no seed is
    read, every ray takes pixel (0, 0)); its AOV is the fixture's."""
    c = sf.case(name)
    assert c["depth"] == 1
    rays, _, pix = sc.camera_rays(_case_camera(name).basis(), c["W"], c["H"], orc.jitter(c["spp"]), targets=True)
    assert np.array_equal(bits(sc.unit_rays(rays[:, :3], pix)), bits(rays))
    scene = sc.scene_of_case(c)
    rad = np.zeros((rays.shape[0], 3), np.float32)
    idx = np.zeros(rays.shape[0], np.int32)
    t = np.zeros(rays.shape[0], np.float32)
    for i in range(rays.shape[0]):
        rad[i], idx[i], t[i] = sc.oracle_shade(scene, rays[i, :3], pix[i], 0, 0, 1, c["diffuse"], (0.0, 0.0, 0.0))
    fb, ghi, ght = sf.fixture_frames(name)
    assert np.array_equal(idx, ghi.reshape(-1)) and np.array_equal(bits(t), bits(ght.reshape(-1)))
    assert np.array_equal(bits(sc.pixel_sum(rad, c["H"], c["W"], c["spp"])), bits(fb))
    assert (fb > 0).any() and (fb == 0).any()


def test_variant_rule_of_the_test_scenes():
    """The kernels the GPU tests reach: the LDS variants on the sphere cases, cornell and frog,
    DEEP on the deep chains and, by the "otherwise" rule, on the 48-level chain (not a deep scene)."""
    W, B, D = L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP
    for name in ("cornell", "frog"):
        a = rb.scene_arrays(name)
        assert sc.rule_variant(a) == (W, False) and sc.rule_variant(a, L.RT_FLAG_BINARY) == (B, False)
    assert sc.rule_variant(rb.scene_arrays("chain48")) == (D, False)
    assert sc.rule_variant(rb.scene_arrays("chain48"), L.RT_FLAG_BINARY) == (D, False)
    assert sc.rule_variant(rb.scene_arrays("chain300")) == (D, True)
    s = sc.scene_of_case(sf.case("s_l1_d1"))
    assert sc.rule_variant(s) == (W, False) and sc.rule_variant(s, L.RT_FLAG_BINARY) == (B, False)
    assert sc.rule_variant(sc.scene_of_case(sf.case("c_l3_d2"))) == (D, True)


# ---- caller rays ----------------------------------------------------------------------------
# name -> hit fraction, shadow rays cast, of them occluded, depth-3 bounce rays of the rays in
# column x = 0, fraction of the hit rays whose depth-3 radiance differs from depth 1 (diffuse on),
# the same with mirror-only bounces, hit rays with a clamped component, misses
FIGURES = {
    "cornell": (0.691, 144, 21, 29, 0.989, 0.989, 12, 79),
    "frog": (0.309, 19, 7, 8, 1.000, 0.000, 6, 177),
    "chain48": (0.641, 42, 35, 39, 1.000, 0.000, 1, 92),
    "chain300": (0.676, 45, 36, 41, 1.000, 0.000, 5, 83),
}


@pytest.mark.parametrize("name", sc.SCENES)
def test_caller_batches_contain_what_the_gpu_tests_rely_on(name):
    """The non-emptiness conditions; with mirror-only bounces frog's and the chains' depth adds
    nothing (kr = 0: the throughput is spent at once), which is a path the kernel has too."""
    f = sc.conditions(name)
    print(name, f)
    assert 0.2 <= f["hit_frac"] <= 0.8
    assert f["shadow_cast"] > 0 and 0 < f["shadow_occluded"] < f["shadow_cast"]
    assert f["bounce_x0"] > 0
    assert f["differs_d3"] >= 0.05
    assert f["clamped"] >= 1 and f["misses"] >= 1
    assert sc.meets(f)
    for seed in range(1, sc.RAY_SEEDS[name]):  # the first seed that meets them
        assert not sc.meets(sc.conditions(name, seed))
    hf, cast, occ, bx0, d3, d3m, cl, miss = FIGURES[name]
    assert abs(f["hit_frac"] - hf) < 5e-4 and abs(f["differs_d3"] - d3) < 5e-4 and abs(f["differs_d3_mirror"] - d3m) < 5e-4
    assert (f["shadow_cast"], f["shadow_occluded"], f["bounce_x0"], f["clamped"], f["misses"]) == (cast, occ, bx0, cl, miss), \
        "the batch is not the one the conditions were computed for"


@pytest.mark.parametrize("name", sc.SCENES)
def test_caller_batch_shape_and_aov(name):
    """256 finite unit rays, 64 distinct seeds, and orc_search_bvh(o, d) on them equals the
    one-pixel render's AOV (the render traces the ray the batch holds)."""
    b = sc.caller_batch(name)
    rays = b["rays"]
    assert rays.shape == (sc.N_CALLER, 6) and rays.dtype == np.float32 and np.isfinite(rays).all()
    assert np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    assert np.array_equal(rays[:, :3], b["o"]) and np.unique(b["seeds"]).size == 64
    a = rb.scene_arrays(name)
    idx, t = rb.oracle_trace(a["P"], a["nodes"], a["aabbs"], a["tris"], rays)
    for depth, diffuse in ((1, True), (3, False)):
        _, ridx, rt_ = sc.reference(name, depth, diffuse)
        assert np.array_equal(idx, ridx) and np.array_equal(bits(t), bits(rt_))
    # a miss's radiance is the miss colour, at every depth
    rad3, _, _ = sc.reference(name, 3, True)
    assert np.array_equal(rad3[idx < 0], np.broadcast_to(np.array(sc.MISS, np.float32), rad3[idx < 0].shape))
