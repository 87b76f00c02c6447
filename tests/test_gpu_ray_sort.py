"""Sorting caller rays for coherence on the GPU (rt_ray_*, rt_gather_device, rt_scatter_device;
DESIGN.md §4.25).  Every comparison is on uint32 views, with no tolerance:

* device keys equal host keys item for item;
* the device order is numpy's stable argsort of the keys and rays_out is rays[order], for sizes
  around the wave, block and sort-tile sizes, with few distinct keys (ties on almost every ray: the
  stability is what is tested), the maximum bits, and one batch past 2^20;
* gather and scatter against numpy indexing for every element size the library moves, aligned
  and 4 bytes off a 16-byte boundary, and scatter(gather(x)) == x;
* trace_rays, trace_hits, shade_rays and trace_paths with ``sort=`` equal the unsorted calls and
  the oracle's answers of tests/ray_batches.py, on scenes of the WIDE, BINARY and DEEP variants;
* a sort and query chain on a side stream; DeviceScene.bounds() after refit and rebuild.

The key itself is pinned by tests/test_ray_sort_host.py against a numpy restatement.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ray_batches as rb
import ray_sort_cases as rs
import rebuild_cases as rbc
import refit_cases as rc
from ray_sort_cases import half_box, root_box

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

F = np.float32
BINARY = L.RT_FLAG_BINARY
DEV = torch.device("cuda", 0)
SIZES = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096)
MODES = {"origin": (1, 2, 10), "origin_dir": (1, 2, 5)}
SORTS = ("origin", "origin_dir", True)
QUERY_SCENES = ("sphere_single", "frog", "cornell", "chain48", "chain300")
MISS = (0.25, 0.5, 0.125)
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


def u32(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(DEV)


def seeds_for(n):
    return np.random.default_rng(77).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


# ---- keys -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("frog", "chain300"))
def test_device_keys_equal_host_keys(name):
    rays = rb.batch(name)["rays"]
    box = root_box(name)
    d = dev(rays)
    for bx in (box, half_box(box)):
        for mode, bits in ((m, b) for m in MODES for b in MODES[m]):
            want = rt.ray_keys(rays, bx, mode, bits)
            got = rt.ray_keys(d, bx, mode, bits)
            assert got.dtype == torch.int32 and np.array_equal(u32(got), want), (name, mode, bits)
    # an array 4 bytes off an 8-byte boundary takes the kernel's dword loads
    flat = torch.zeros(rays.size + 1, dtype=torch.float32, device=DEV)
    flat[1:] = d.reshape(-1)
    off = flat[1:].view(-1, 6)
    assert off.data_ptr() % 8 == 4
    assert np.array_equal(u32(rt.ray_keys(off, box, "origin_dir", 5)), rt.ray_keys(rays, box, "origin_dir", 5))


def test_device_keys_of_special_rays():
    d = dev(rs.SPECIAL_RAYS)
    for box in rs.SPECIAL_BOXES.values():
        bx = np.array(box, F)
        for mode, bits in rs.CASES:
            assert np.array_equal(u32(rt.ray_keys(d, bx, mode, bits)), rt.ray_keys(rs.SPECIAL_RAYS, bx, mode, bits)), (box, mode, bits)


# ---- order and sorted rays ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_device_order_is_the_stable_argsort(n):
    rays = rb.batch("frog")["rays"][:n]
    box = root_box("frog")
    d = dev(rays)
    for mode, bits in ((m, b) for m in MODES for b in MODES[m]):
        keys = rt.ray_keys(rays, box, mode, bits)
        want = np.argsort(keys, kind="stable")
        out, order = rt.sort_rays(d, box, mode, bits)
        assert order.dtype == torch.int32 and np.array_equal(order.cpu().numpy(), want), (n, mode, bits)
        assert np.array_equal(u32(out), u32(rays[want])), (n, mode, bits)
    if n >= 256:  # b = 1, 2: at most 8 / 64 origin keys, so nearly every ray ties with another
        assert np.unique(rt.ray_keys(rays, box, "origin", 1)).size <= 8
        assert np.unique(rt.ray_keys(rays, box, "origin", 2)).size <= 64


def test_a_large_batch_and_an_empty_one():
    base = rb.batch("frog")["rays"]
    n = 2 ** 20 + 3
    rays = np.ascontiguousarray(np.tile(base, (n // base.shape[0] + 1, 1))[:n])
    box = root_box("frog")
    want = np.argsort(rt.ray_keys(rays, box, "origin", 2), kind="stable")
    out, order = rt.sort_rays(dev(rays), box, "origin", 2)
    assert np.array_equal(order.cpu().numpy(), want)
    assert np.array_equal(u32(out), u32(rays[want]))
    out, order = rt.sort_rays(dev(rays[:0]), box, "origin", 2)
    assert out.shape == (0, 6) and order.shape == (0,)
    assert rt.ray_keys(dev(rays[:0]), box).shape == (0,)
    e = torch.empty((0, 6), dtype=torch.float32, device=DEV)
    assert rt.gather(e, order).shape == (0, 6) and rt.scatter(e, order).shape == (0, 6)


# ---- gather and scatter ---------------------------------------------------------------------------
@pytest.mark.parametrize("elem_bytes", (4, 12, 24, 52, 64))
def test_gather_and_scatter_equal_numpy_indexing(elem_bytes):
    w = elem_bytes // 4
    rng = np.random.default_rng(elem_bytes)
    for n in SIZES + (70001,):
        x = rng.integers(0, 2 ** 32, (n, w), dtype=np.uint64).astype(np.uint32)
        perm = rng.permutation(n).astype(np.int32)
        inv = np.empty_like(x)
        inv[perm] = x
        order = dev(perm)
        for offset in ((0,) if elem_bytes % 16 == 0 else (0, 1)):
            # offset 1: input and output 4 bytes off a 16-byte boundary
            buf = torch.zeros(n * w + 5, dtype=torch.int32, device=DEV)
            buf[offset:offset + n * w] = dev(x).reshape(-1)
            xin = buf[offset:offset + n * w].view(n, w)
            out = torch.zeros(n * w + 5, dtype=torch.int32, device=DEV)[offset:offset + n * w].view(n, w)
            assert xin.data_ptr() % 16 == 4 * offset and out.data_ptr() % 16 == 4 * offset
            g = rt.gather(xin, order, out=out)
            assert g.data_ptr() == out.data_ptr() and np.array_equal(u32(g), x[perm]), (n, offset)
            back = rt.scatter(g, order)
            assert np.array_equal(u32(back), x), (n, offset)
            s = rt.scatter(xin, order, out=out)
            assert np.array_equal(u32(s), inv), (n, offset)
    # other shapes and dtypes with the same row bytes
    if elem_bytes == 12:
        x = rng.random((257, 3), dtype=np.float32)
        perm = rng.permutation(257).astype(np.int32)
        assert np.array_equal(u32(rt.gather(dev(x), dev(perm))), u32(x[perm]))
    with pytest.raises(ValueError):
        rt.gather(torch.zeros((4, 17), dtype=torch.int32, device=DEV), dev(np.arange(4, dtype=np.int32)))
    with pytest.raises(ValueError):
        rt.gather(torch.zeros((4, 3), dtype=torch.uint8, device=DEV), dev(np.arange(4, dtype=np.int32)))


def test_an_order_entry_outside_the_batch_is_skipped():
    x = dev(np.arange(8 * 6, dtype=np.int32).reshape(8, 6))
    order = dev(np.array([3, 2, 1, 0, 100, -1, 7, 6], np.int32))
    out = torch.full((8, 6), -5, dtype=torch.int32, device=DEV)
    got = rt.gather(x, order, out=out).cpu().numpy()
    xs = x.cpu().numpy()
    assert np.array_equal(got[[0, 1, 2, 3, 6, 7]], xs[[3, 2, 1, 0, 7, 6]]) and (got[4:6] == -5).all()


# ---- queries with sort= ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, BINARY], ids=["wide", "binary"])
@pytest.mark.parametrize("name", QUERY_SCENES)
def test_sorted_queries_equal_the_unsorted_and_the_oracle(name, flags):
    b = rb.batch(name)
    ds = scene(name)
    rays = dev(b["rays"])
    n = rays.shape[0]
    idx0, t0 = ds.trace_rays(rays, flags=flags)
    assert np.array_equal(idx0.cpu().numpy(), b["idx"]) and np.array_equal(u32(t0), u32(b["t"]))
    up = np.nextafter(b["t"], F(np.inf), dtype=F)
    max_t = np.where(b["idx"] >= 0, np.where(np.arange(n) % 2 == 0, b["t"], up), F(1.0)).astype(F)
    mt = dev(max_t)
    occ0 = ds.trace_rays(rays, mode="occluded", max_t=mt, flags=flags)
    assert np.array_equal(occ0.cpu().numpy(), (b["idx"] >= 0) & (b["t"] < max_t))
    hits0 = ds.trace_hits(rays, flags=flags)
    seeds = dev(seeds_for(n))
    shade0 = {d: ds.shade_rays(rays, seeds, max_depth=d, miss_color=MISS, flags=flags, aov=True) for d in (1, 2, 3)}
    variant = ds.trace_hits_variant()
    for sort in SORTS:
        idx, t = ds.trace_rays(rays, flags=flags, sort=sort)
        assert np.array_equal(idx.cpu().numpy(), b["idx"]) and np.array_equal(u32(t), u32(b["t"])), (name, sort)
        occ = ds.trace_rays(rays, mode="occluded", max_t=mt, flags=flags, sort=sort)
        assert occ.dtype == torch.bool and torch.equal(occ, occ0), (name, sort)
        hits = ds.trace_hits(rays, flags=flags, sort=sort)
        assert torch.equal(hits, hits0), (name, sort)
        assert np.array_equal(hits[:, 0].cpu().numpy(), b["idx"]) and np.array_equal(u32(hits[:, 1]), u32(b["t"]))
        assert ds.trace_hits_variant() == variant
        for d, (rad0, i0, tt0) in shade0.items():
            rad, i1, tt1 = ds.shade_rays(rays, seeds, max_depth=d, miss_color=MISS, flags=flags, aov=True, sort=sort)
            assert np.array_equal(u32(rad), u32(rad0)), (name, sort, d)
            assert np.array_equal(i1.cpu().numpy(), b["idx"]) and np.array_equal(u32(tt1), u32(b["t"]))
            assert torch.equal(i1, i0) and np.array_equal(u32(tt1), u32(tt0))
        # without seeds and without AOVs
        assert np.array_equal(u32(ds.shade_rays(rays, None, max_depth=2, miss_color=MISS, flags=flags, sort=sort)),
                              u32(ds.shade_rays(rays, None, max_depth=2, miss_color=MISS, flags=flags)))
    if name in ("cornell", "sphere_single"):  # paths survive the first segment there: the seeds matter
        assert not np.array_equal(u32(shade0[1][0]), u32(shade0[3][0]))


def test_the_query_scenes_cover_the_three_variants():
    import shade_rays_cases as sc

    seen = set()
    for name in QUERY_SCENES:
        a = rb.scene_arrays(name)
        seen |= {sc.rule_variant(a)[0], sc.rule_variant(a, BINARY)[0]}
    assert seen == {L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP}


def test_sort_is_for_the_device_path():
    ds = scene("frog")
    rays = rb.batch("frog")["rays"]
    with pytest.raises(ValueError):
        ds.trace_rays(rays, sort="origin")
    with pytest.raises(ValueError):
        ds.trace_hits(rays, sort=True)
    with pytest.raises(ValueError):
        ds.shade_rays(rays, sort="origin_dir")
    with pytest.raises(ValueError):
        ds.trace_hits(dev(rays), sort="morton")
    assert np.array_equal(ds.bounds(), root_box("frog"))


# ---- trace_paths(sort=...) ----------------------------------------------------------------------------
@pytest.mark.parametrize("diffuse", [True, False], ids=["diffuse", "mirror"])
@pytest.mark.parametrize("name", ("cornell", "sphere_single"))
def test_sorted_paths_equal_the_unsorted_and_the_monolith(name, diffuse):
    ds = scene(name)
    b = rb.batch(name)
    rays, seeds = dev(b["rays"]), dev(seeds_for(b["rays"].shape[0]))
    mono = ds.shade_rays(rays, seeds, max_depth=4, diffuse_bounce=diffuse, miss_color=MISS)
    base = ds.trace_paths(rays, seeds, 4, diffuse, MISS)
    assert np.array_equal(u32(base), u32(mono))
    # with the diffuse bounce paths survive the first segment: depth 4 differs from depth 1 (without it
    # a path goes on only from a material with kr > 0, which sphere_single has none of)
    assert not diffuse or not np.array_equal(u32(mono), u32(ds.shade_rays(rays, seeds, max_depth=1, diffuse_bounce=diffuse, miss_color=MISS)))
    table = dev(np.ascontiguousarray(rb.scene_arrays(name)["mats"], F).reshape(-1, 13))
    default = dev(np.ascontiguousarray(rt.default_material(), F).reshape(1, 13))
    seen = []

    def own_table(hits, cur, ids, depth):
        m = hits[:, 15].long()
        inside = (m >= 0) & (m < table.shape[0])
        seen.append((depth, ids.clone(), cur.clone()))
        return torch.where(inside[:, None], table[m.clamp(0, table.shape[0] - 1)], default)

    for sort in SORTS:
        for compact in (True, False):
            got = ds.trace_paths(rays, seeds, 4, diffuse, MISS, compact=compact, sort=sort)
            assert np.array_equal(u32(got), u32(mono)), (name, sort, compact)
            seen.clear()
            got = ds.trace_paths(rays, seeds, 4, diffuse, MISS, material_fn=own_table, compact=compact, sort=sort)
            assert np.array_equal(u32(got), u32(mono)), (name, sort, compact, "material_fn")
            # the hook saw the sorted entries with their ids: at the first depth a permutation whose
            # entry k is the caller's ray ids[k]
            depth, ids, cur = seen[0]
            assert depth == 0 and np.array_equal(np.sort(ids.cpu().numpy()), np.arange(rays.shape[0]))
            assert torch.equal(cur, rays[ids.long()])
            assert not torch.equal(cur, rays)


# ---- streams and bounds -----------------------------------------------------------------------------
def test_a_sorted_chain_on_a_side_stream():
    ds = scene("frog")
    b = rb.batch("frog")
    rays, seeds = dev(b["rays"]), dev(seeds_for(b["rays"].shape[0]))
    box = ds.bounds()
    want_sorted, want_order = rt.sort_rays(rays, box, "origin_dir", 5)
    want_hits = ds.trace_hits(rays)
    want_rad = ds.shade_rays(rays, seeds, max_depth=3, miss_color=MISS)
    torch.cuda.synchronize(DEV)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        srt, order = rt.sort_rays(rays, box, "origin_dir", 5)
        hits = rt.scatter(ds.trace_hits(srt), order)
        hits2 = ds.trace_hits(rays, sort="origin_dir")
        rad = ds.shade_rays(rays, seeds, max_depth=3, miss_color=MISS, sort=True)
        sd = rt.gather(seeds, order)
        rad2 = rt.scatter(ds.shade_rays(srt, sd, max_depth=3, miss_color=MISS), order)
    # the same chain with the stream given by handle, from the default stream
    side.synchronize()
    srt3, order3 = rt.sort_rays(rays, box, "origin_dir", 5, stream=side.cuda_stream)
    hits3 = ds.trace_hits(rays, stream=side.cuda_stream, sort="origin")
    side.synchronize()
    assert torch.equal(order, want_order) and torch.equal(srt, want_sorted)
    assert torch.equal(order3, want_order) and torch.equal(srt3, want_sorted)
    for h in (hits, hits2, hits3):
        assert torch.equal(h, want_hits)
    for r in (rad, rad2):
        assert np.array_equal(u32(r), u32(want_rad))


@pytest.mark.parametrize("name", ("sphere_single", "cornell"))
def test_bounds_follow_refit_and_rebuild(name):
    a = rc.scene(name)
    ds = rt.DeviceScene(a["P"], a["nodes"], a["aabbs"], a["tris"], a["triobj"], a["mats"], a["lights"], refittable=True)
    try:
        assert np.array_equal(u32(ds.bounds()), u32(a["aabbs"][0]))
        for kind in ("wobble", "moved", "flat"):
            tris = rc.deformed(name, kind)
            ds.refit(tris)
            want = rt.refit_aabbs(a["nodes"], tris)[0]
            assert np.array_equal(u32(ds.bounds()), u32(want)), (name, kind)
            assert not np.array_equal(u32(want), u32(a["aabbs"][0]))
        for kind in ("wobble", "shift4096"):
            tris = rbc.pose(name, kind)
            nodes, aabbs = ds.rebuild(tris, tree=True)
            assert np.array_equal(u32(ds.bounds()), u32(aabbs[0])), (name, kind)
            assert np.array_equal(u32(aabbs[0]), u32(rbc.tree(name, kind)[1][0]))
        # a sorted query in the new box answers as the unsorted one
        rays = dev(rb.batch(name)["rays"] + np.array([4096, 0, 0, 0, 0, 0], F))
        assert torch.equal(ds.trace_hits(rays, sort=True), ds.trace_hits(rays))
    finally:
        ds.close()
