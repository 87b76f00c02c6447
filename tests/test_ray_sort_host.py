"""Sorting caller rays for coherence (rt_ray_*, rt_gather_device, rt_scatter_device),
the part that needs no device: the key's host build against a float32 numpy restatement of its
definition (include/rt_mi355x.h), item for item on uint32, on the seven caller batches of
tests/ray_batches.py and a table of special rays and boxes; the host order against numpy's stable
argsort; and every argument rule that answers before any HIP call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ray_batches as rb
from ray_sort_cases import (BIG, CASES, INF, NAN, SPECIAL_BOXES, SPECIAL_RAYS, half_box, np_keys, root_box)

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

F = np.float32


@pytest.mark.parametrize("name", rb.SCENES)
def test_host_keys_equal_the_numpy_restatement(name):
    rays = rb.batch(name)["rays"]
    assert rays.shape == (rb.N_RAYS, 6)
    for box in (root_box(name), half_box(root_box(name))):
        for mode, b in CASES:
            got = rt.ray_keys(rays, box, mode, b)
            want = np_keys(rays, box, mode, b)
            assert got.dtype == np.uint32 and np.array_equal(got, want), (name, mode, b, np.flatnonzero(got != want)[:4])
            assert int(got.max()) < 2 ** rt.ray_key_bits(mode, b)
    # the half box clamps on both sides of every axis, the root box on neither for some ray
    hb = half_box(root_box(name))
    o = rays[:, :3]
    assert ((o < hb[:3]).any(axis=0) & (o > hb[3:]).any(axis=0)).all()


def test_the_batches_spread_over_the_keys():
    """The restatement and the host build could agree on a constant: the batches fill many cells."""
    rays = rb.batch("frog")["rays"]
    for mode, b in CASES:
        distinct = np.unique(rt.ray_keys(rays, root_box("frog"), mode, b)).size
        assert distinct >= min(2 ** rt.ray_key_bits(mode, b), 64) // 2, (mode, b, distinct)


@pytest.mark.parametrize("box", SPECIAL_BOXES)
def test_special_rays_and_boxes(box):
    bx = np.array(SPECIAL_BOXES[box], F)
    for mode, b in CASES:
        got = rt.ray_keys(SPECIAL_RAYS, bx, mode, b)
        want = np_keys(SPECIAL_RAYS, bx, mode, b)
        assert np.array_equal(got, want), (box, mode, b, np.flatnonzero(got != want))


def test_special_cells_by_hand():
    """What the definition says in words, for a few of the entries above, at b = 2 (4 cells per axis)."""
    unit = np.array(SPECIAL_BOXES["unit"], F)

    def cells(ray, box=unit, mode="origin"):
        key = int(rt.ray_keys(np.array([ray], F), box, mode, 2)[0])
        n = 3 if mode == "origin" else 6
        return [sum(((key >> (n * j + n - 1 - c)) & 1) << j for j in range(2)) for c in range(n)]

    assert cells([NAN, 0.5, 0.5, 0, 0, 1]) == [0, 2, 2]  # NaN: cell 0
    assert cells([INF, 0.5, -INF, 0, 0, 1]) == [3, 2, 0]  # +inf: the last cell, -inf: the first
    assert cells([1.0, -0.0, 0.25, 0, 0, 1]) == [3, 0, 1]  # hi itself clamps to the last cell
    assert cells([0.5, 0.75, 0.25, 0, 0, 1], np.array(SPECIAL_BOXES["flat_x"], F)) == [0, 3, 1]  # 0 / 0 -> 0
    assert cells([0.75, 0.5, 0.5, 0, 0, 1], np.array(SPECIAL_BOXES["flat_x"], F))[0] == 3  # x / 0 -> the last cell
    assert cells([0.25, 0.5, 0.5, 0, 0, 1], np.array(SPECIAL_BOXES["flat_x"], F))[0] == 0  # -x / 0 -> the first
    assert cells([0.5, 0.5, 0.5, 0, 0, 0], mode="origin_dir")[3:] == [0, 0, 0]  # a zero direction: 0 / 0
    assert cells([0.5, 0.5, 0.5, BIG, 1, 1], mode="origin_dir")[3:] == [2, 2, 2]  # the squared length overflows: u = d / inf = 0
    assert cells([0.5, 0.5, 0.5, 0, 0, 1], mode="origin_dir")[3:] == [2, 2, 3]
    assert cells([0.5, 0.5, 0.5, -1, 0, 0], mode="origin_dir")[3:] == [0, 2, 2]


# ---- the order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("frog", "chain300"))
def test_host_order_is_the_stable_argsort(name):
    rays = rb.batch(name)["rays"]
    box = root_box(name)
    for mode, b in CASES:
        sorted_rays, order = rt.sort_rays(rays, box, mode, b)
        keys = np_keys(rays, box, mode, b)
        want = np.argsort(keys, kind="stable")
        assert order.dtype == np.int32 and np.array_equal(order, want), (name, mode, b)
        assert np.array_equal(sorted_rays.view(np.uint32), rays[want].view(np.uint32))
    # b = 1: eight keys, ties on almost every ray
    assert np.unique(np_keys(rays, box, "origin", 1)).size <= 8


def test_host_order_small_sizes():
    rays = rb.batch("cornell")["rays"]
    box = root_box("cornell")
    for n in (1, 2, 63, 64, 65, 257):
        _, order = rt.sort_rays(rays[:n], box, "origin", 2)
        assert np.array_equal(order, np.argsort(np_keys(rays[:n], box, "origin", 2), kind="stable"))
    s, order = rt.sort_rays(rays[:0], box, "origin_dir", 5)
    assert s.shape == (0, 6) and order.shape == (0,)


# ---- entry points and argument rules -------------------------------------------------------------
NAMES = ("rt_scene_bounds", "rt_ray_key_bits", "rt_ray_keys_host", "rt_ray_keys_device", "rt_ray_sort_host",
         "rt_ray_sort_scratch_bytes", "rt_ray_sort_device", "rt_gather_device", "rt_scatter_device")


def test_entry_points_exist():
    lib = L.lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    for name in ("ray_keys", "ray_key_bits", "sort_rays", "gather", "scatter"):
        assert callable(getattr(rt, name)), name
    assert callable(rt.DeviceScene.bounds)
    assert (rt.RT_SORT_ORIGIN, rt.RT_SORT_ORIGIN_DIR) == (0, 1)
    assert lib.rt_abi_version() == 3
    hpp = (rb.HERE.parent / "include" / "rt_mi355x.hpp").read_text()
    for name in NAMES:
        assert name + "(" in hpp, name


def test_key_bits():
    lib = L.lib()
    for b in range(1, 11):
        assert lib.rt_ray_key_bits(L.RT_SORT_ORIGIN, b) == 3 * b
    for b in range(1, 6):
        assert lib.rt_ray_key_bits(L.RT_SORT_ORIGIN_DIR, b) == 6 * b
    for mode, b in ((0, 0), (0, 11), (0, -1), (1, 0), (1, 6), (2, 1), (-1, 1)):
        assert lib.rt_ray_key_bits(mode, b) == -1, (mode, b)  # RT_ERR_ARG
        assert b"RT_SORT_ORIGIN" in lib.rt_last_error()
    assert rt.ray_key_bits("origin", 10) == 30 and rt.ray_key_bits("origin_dir", 5) == 30
    for mode, b in (("origin", 11), ("origin", 0), ("origin_dir", 6), ("morton", 1)):
        with pytest.raises(ValueError):
            rt.ray_keys(np.zeros((1, 6), F), [0, 0, 0, 1, 1, 1], mode, b)


# Host buffers no failing call may touch: every check answers before any access and any HIP call.
_BUF = np.zeros(4096, np.uint32)
_P = _BUF.ctypes.data
_P16 = _P + (-_P) % 16
_BOX = L.AABB(L.Vec3(0, 0, 0), L.Vec3(1, 1, 1))
_BX = C.addressof(_BOX)
ARG, UNSUPPORTED = -1, -7
TOO_MANY = 2 ** 31


def test_host_call_arguments():
    lib = L.lib()
    rays, out = np.zeros((4, 6), F), np.full(8, 0xAAAAAAAA, np.uint32)
    r, o = rays.ctypes.data, out.ctypes.data
    for fn in (lib.rt_ray_keys_host, lib.rt_ray_sort_host):
        assert fn(r, 4, 0, 5, _BX, o) == 0
        assert (out[4:] == 0xAAAAAAAA).all()
        assert fn(None, 0, 0, 5, None, None) == 0  # n == 0: nothing is read
        for mode, b in ((0, 0), (0, 11), (1, 6), (2, 5), (-1, 5)):
            assert fn(r, 4, mode, b, _BX, _P) == ARG
            assert fn(r, 0, mode, b, _BX, _P) == ARG  # a bad mode is an error for any n
        assert fn(None, 4, 0, 5, _BX, _P) == ARG
        assert fn(r, 4, 0, 5, None, _P) == ARG
        assert fn(r, 4, 0, 5, _BX, None) == ARG
        assert fn(r, TOO_MANY, 0, 5, _BX, _P) == UNSUPPORTED
        assert b"2^31-1" in lib.rt_last_error()
    assert not _BUF.any()


def test_scratch_bytes():
    lib = L.lib()
    f = lib.rt_ray_sort_scratch_bytes
    assert f(0, 0, 5) == 0 and f(TOO_MANY, 0, 5) == 0 and f(100, 0, 11) == 0 and f(100, 2, 1) == 0
    last = 0
    for n in (1, 64, 4096, 2 ** 20 + 3, 2 ** 31 - 1):
        s = f(n, 1, 5)
        assert s >= 5 * 4 * n and s >= last  # keys, sorted keys, indices, and the sort's two temporaries
        assert s == f(n, 0, 1)  # one reservation per n
        last = s


def test_device_call_arguments_answer_without_a_device():
    lib = L.lib()
    # keys and sort: n == 0, the bad modes, the nulls and the count, before any HIP call
    assert lib.rt_ray_keys_device(0, None, 0, 0, 5, None, None, None) == 0
    assert lib.rt_ray_sort_device(0, None, 0, 1, 5, None, None, None, None, None) == 0
    for mode, b in ((0, 0), (0, 11), (1, 6), (2, 5)):
        assert lib.rt_ray_keys_device(0, _P, 4, mode, b, _BX, _P + 1024, None) == ARG
        assert lib.rt_ray_sort_device(0, _P, 4, mode, b, _BX, _P + 1024, None, _P + 2048, None) == ARG
    for args in ((None, 4, 0, 5, _BX, _P + 1024), (_P, 4, 0, 5, None, _P + 1024), (_P, 4, 0, 5, _BX, None),
                 (_P + 2, 4, 0, 5, _BX, _P + 1024), (_P, 4, 0, 5, _BX, _P + 1025)):
        assert lib.rt_ray_keys_device(0, *args, None) == ARG, args
    assert lib.rt_ray_keys_device(0, _P, TOO_MANY, 0, 5, _BX, _P + 1024, None) == UNSUPPORTED
    ok = dict(rays=_P, n=4, mode=0, bits=5, box=_BX, order=_P + 1024, out=_P + 2048, scratch=_P + 4096)
    for bad in (dict(rays=None), dict(box=None), dict(order=None), dict(scratch=None), dict(rays=_P + 1), dict(order=_P + 1026),
                dict(out=_P + 2049), dict(out=_P + 4 * 24 - 4), dict(out=_P)):
        a = {**ok, **bad}
        rc = lib.rt_ray_sort_device(0, a["rays"], a["n"], a["mode"], a["bits"], a["box"], a["order"], a["out"], a["scratch"], None)
        assert rc == ARG, bad
    assert lib.rt_ray_sort_device(0, _P, TOO_MANY, 0, 5, _BX, _P + 1024, None, _P + 4096, None) == UNSUPPORTED
    # gather and scatter
    for fn in (lib.rt_gather_device, lib.rt_scatter_device):
        assert fn(0, None, 0, 24, None, None, None) == 0
        for eb in (0, 1, 2, 3, 6, 26, 68, 128, 2 ** 32 + 24):
            assert fn(0, _P, 4, eb, _P + 1024, _P + 2048, None) == ARG, eb
            assert fn(0, _P, 0, eb, _P + 1024, _P + 2048, None) == ARG, eb
        for args in ((None, 4, 24, _P + 1024, _P + 2048), (_P, 4, 24, None, _P + 2048), (_P, 4, 24, _P + 1024, None),
                     (_P + 1, 4, 24, _P + 1024, _P + 2048), (_P, 4, 24, _P + 1026, _P + 2048), (_P, 4, 24, _P + 1024, _P + 2050),
                     (_P, 4, 24, _P + 1024, _P), (_P, 4, 24, _P + 1024, _P + 92), (_P + 92, 4, 24, _P + 1024, _P)):
            assert fn(0, *args, None) == ARG, args
        assert fn(0, _P, TOO_MANY, 4, _P + 1024, _P + 2048, None) == UNSUPPORTED
    assert not _BUF.any()


def test_scene_bounds_arguments():
    lib = L.lib()
    assert lib.rt_scene_bounds(None, _BX) == ARG
    fake = C.create_string_buffer(64)
    assert lib.rt_scene_bounds(C.addressof(fake), None) == ARG
