"""Batched ray queries (rt_trace_rays*, include/rt_mi355x.h), the part that needs no device: the
entry points exist, their argument checks answer before any HIP call, and the ray batches of
tests/ray_batches.py contain what the GPU tests (tests/test_gpu_trace_rays.py) rely on, shown
with the oracle alone so that no GPU test can pass by emptiness."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ray_batches as rb

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L


def test_entry_points_exist():
    lib = L.lib()
    for name in ("rt_trace_rays_device", "rt_trace_rays", "rt_trace_rays_variant"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    assert callable(rt.DeviceScene.trace_rays) and callable(rt.DeviceScene.trace_rays_variant)
    assert (rt.RT_RAYS_CLOSEST, rt.RT_RAYS_OCCLUDED) == (0, 1)
    assert (rt.RT_RAYS_VARIANT_NONE, rt.RT_RAYS_VARIANT_WIDE, rt.RT_RAYS_VARIANT_BINARY,
            rt.RT_RAYS_VARIANT_DEEP) == (0, 1, 2, 3)
    assert lib.rt_trace_rays_variant(None) == rt.RT_RAYS_VARIANT_NONE


# A scene handle that is never read: every check below answers before the scene is touched.
_FAKE_SCENE = C.create_string_buffer(64)
_RAYS = np.zeros((4, 6), np.float32)
_MAXT = np.ones(4, np.float32)
_IDX = np.zeros(4, np.int32)
_T = np.zeros(4, np.float32)
_S, _R, _M, _I, _TT = C.addressof(_FAKE_SCENE), _RAYS.ctypes.data, _MAXT.ctypes.data, _IDX.ctypes.data, _T.ctypes.data

# (scene, mode, rays, max_t, n, flags, hit_idx, hit_t) -> code
ARG_CASES = {
    "null scene": ((None, 0, _R, None, 4, 0, _I, _TT), -1),
    "null rays": ((_S, 0, None, None, 4, 0, _I, _TT), -1),
    "null output": ((_S, 0, _R, None, 4, 0, None, _TT), -1),
    "null output, occluded": ((_S, 1, _R, _M, 4, 0, None, None), -1),
    "closest with max_t": ((_S, 0, _R, _M, 4, 0, _I, _TT), -1),
    "occluded without max_t": ((_S, 1, _R, None, 4, 0, _I, None), -1),
    "occluded with hit_t": ((_S, 1, _R, _M, 4, 0, _I, _TT), -1),
    "unknown mode": ((_S, 2, _R, None, 4, 0, _I, _TT), -1),
    "unknown flag": ((_S, 0, _R, None, 4, L.RT_FLAG_NO_CULL, _I, _TT), -1),
    "unknown flag beside BINARY": ((_S, 0, _R, None, 4, L.RT_FLAG_BINARY | 8, _I, _TT), -1),
    "n = 2^31": ((_S, 0, _R, None, 1 << 31, 0, _I, _TT), -7),
    "n = 2^40, occluded": ((_S, 1, _R, _M, 1 << 40, L.RT_FLAG_BINARY, _I, None), -7),
}


@pytest.mark.parametrize("entry", ["rt_trace_rays", "rt_trace_rays_device"])
@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_argument_errors_need_no_device(entry, case):
    args, code = ARG_CASES[case]
    rc = getattr(L.lib(), entry)(*args, None)  # kernel_ms / hip_stream
    assert rc == code, (case, rc, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _IDX.any() and not _T.any()  # nothing was written


def test_empty_batch_is_ok_without_a_device():
    for entry in ("rt_trace_rays", "rt_trace_rays_device"):
        assert getattr(L.lib(), entry)(_S, 0, _R, None, 0, 0, _I, _TT, None) == 0
        assert getattr(L.lib(), entry)(_S, 1, _R, _M, 0, L.RT_FLAG_BINARY, _I, None, None) == 0


def test_python_mode_names():
    unbound = object.__new__(rt.DeviceScene)  # the mode is checked before the scene is touched
    with pytest.raises(ValueError):
        unbound.trace_rays(_RAYS, mode="nearest")


# The variant rule of every caller query (rt::SceneMeta::query_variant through rt_debug_query_variant),
# row by row: (wide, lane_stack, lane_wide, deep) -> (variant with flags 0, with RT_FLAG_BINARY).
# deep gives DEEP; else wide and lane_wide without the flag give WIDE; else lane_stack gives BINARY;
# else DEEP.
_W, _B, _D = L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP
VARIANT_RULE = {
    (0, 0, 0, 0): (_D, _D),
    (0, 0, 0, 1): (_D, _D),
    (0, 0, 1, 0): (_D, _D),  # lane_wide says nothing without the 4-ary records
    (0, 0, 1, 1): (_D, _D),
    (0, 1, 0, 0): (_B, _B),
    (0, 1, 0, 1): (_D, _D),
    (0, 1, 1, 0): (_B, _B),
    (0, 1, 1, 1): (_D, _D),
    (1, 0, 0, 0): (_D, _D),
    (1, 0, 0, 1): (_D, _D),
    (1, 0, 1, 0): (_W, _D),  # the flag takes WIDE away and the binary stack does not fit LDS
    (1, 0, 1, 1): (_D, _D),
    (1, 1, 0, 0): (_B, _B),
    (1, 1, 0, 1): (_D, _D),
    (1, 1, 1, 0): (_W, _B),  # frog
    (1, 1, 1, 1): (_D, _D),
}


def test_variant_rule_row_by_row():
    assert "rt_debug_query_variant" in L.SIGNATURES
    assert (_W, _B, _D) == (1, 2, 3) and len(VARIANT_RULE) == 16
    for facts, want in VARIANT_RULE.items():
        got = tuple(L.lib().rt_debug_query_variant(*facts, flags) for flags in (0, L.RT_FLAG_BINARY))
        assert got == want, (facts, got, want)
    # any non-zero int is true, and only the BINARY bit of flags is read
    assert L.lib().rt_debug_query_variant(7, -1, 2, 0, 0) == _W
    assert L.lib().rt_debug_query_variant(1, 1, 1, 0, L.RT_FLAG_BINARY | 8) == _B
    assert L.lib().rt_debug_query_variant(1, 1, 1, 0, 8) == _W


HIT_FRACTION = {"sphere_single": 0.398, "frog": 0.272, "cornell": 0.710, "chain24": 0.498, "chain48": 0.525,
                "chain300": 0.548, "chain600": 0.550}
TIE_WINNERS = {"chain24": (162, 58), "chain48": (150, 56), "chain300": (114, 49), "chain600": (26, 132)}


def test_generator_shape_and_classes():
    a = rb.scene_arrays("frog")
    rays = rb.make_rays(a["aabbs"], a["tris"], a["light"], rb.N_RAYS, rb.SEED)
    assert rays.shape == (rb.N_RAYS, 6) and rays.dtype == np.float32 and np.isfinite(rays).all()
    assert np.array_equal(rays, rb.batch("frog")["rays"])  # deterministic
    sl = rb.class_slices()
    d = rays[:, 3:].astype(np.float64)
    n = np.linalg.norm(d, axis=1)
    assert n[sl["A"]].min() < 0.1 and n[sl["A"]].max() > 10.0  # unnormalised on purpose
    assert np.allclose(n[sl["B"]], 1.0, atol=1e-6) and np.allclose(n[sl["C"]], 1.0, atol=1e-6)
    dd = np.abs(rays[sl["D"], 3:])
    assert ((dd == 1.0).sum(axis=1) == 1).all()
    small = dd[dd != 1.0]
    assert (small < 1e-8).all() and (small == 0).any() and (small > 0).any()  # both below intersectAABB's 1e-8


@pytest.mark.parametrize("name", rb.SCENES)
def test_batches_contain_what_the_gpu_tests_rely_on(name):
    b = rb.batch(name)
    hit = b["idx"] >= 0
    frac = float(hit.mean())
    print(f"{name}: hit fraction {frac:.3f}")
    assert 0.2 <= frac <= 0.8
    assert abs(frac - HIT_FRACTION[name]) < 5e-4, "the batch is not the one the conditions were computed for"
    assert np.array_equal(b["t"] == -1.0, ~hit) and (b["t"][hit] >= np.float32(1e-4)).all()
    a = rb.scene_arrays(name)
    assert b["idx"].max() < a["P"]
    for cls, s in rb.class_slices().items():
        k = int(hit[s].sum())
        print(f"  class {cls}: {k} hits of {hit[s].size}")
        assert 0 < k < hit[s].size, f"class {cls} has no {'hit' if k == 0 else 'miss'}"
    if name in TIE_WINNERS:  # both winners of the duplicated triangle (chain_bvh: levels 0 and 3)
        p0, p3 = int(a["perm"][0]), int(a["perm"][3])
        got = (int((b["idx"] == p0).sum()), int((b["idx"] == p3).sum()))
        print(f"  perm[0] / perm[3] winners: {got}")
        assert got == TIE_WINNERS[name]
