"""Path stages for caller hits on the GPU (rt_path_*, include/rt_mi355x.h), bit for
bit (uint32 views, no tolerance) against the oracle and the reference's fixtures:

* staged equals monolith equals reference: trace_paths on the caller batches of four scenes (WIDE,
  BINARY and DEEP between them) and on three shading-fuzz frames;
* per-hit materials: a scene uploaded with its own table, shaded with a second table through
  material_fn, against the oracle's render with that table;
* `direct`, batch sizes around the wave and block sizes, shuffled entries and ids, aliased next
  rays, dead entries, RT_PATH_LAST with null outputs;
* the stable compaction against numpy.flatnonzero;
* a staged batch on a side stream beside a renderer's frames, and on a clone.

What the batches and tables contain is pinned by tests/test_shade_rays_host.py and
tests/test_path_stages_host.py with the oracle alone.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

import path_cases as pc
import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc
from conftest import host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

pytestmark = pytest.mark.gpu

BINARY = L.RT_FLAG_BINARY
DEV = torch.device("cuda", 0)
_scenes: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _close_scenes():
    yield
    for ds in _scenes.values():
        ds.close()
    _scenes.clear()


def scene(name: str):
    """One DeviceScene per ray_batches scene or shade_fuzz case (uploaded with its own table)."""
    if name not in _scenes:
        if name in sf.CASES:
            c = sf.case(name)
            _scenes[name] = rt.DeviceScene(c["P"], c["nodes"], c["aabbs"], c["tris"], c["triobj"], sf.mats13(c), c["lights"])
        else:
            _scenes[name] = rb.device_scene(name)
    return _scenes[name]


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def wrap(m):
    """Entries 0..m-1 of a batch as indices into the 256-ray caller batch (past it: from its start again)."""
    return np.arange(m) % sc.N_CALLER


def dev_batch(name, m=None):
    b = sc.caller_batch(name)
    k = wrap(sc.N_CALLER if m is None else m)
    return (torch.from_numpy(b["rays"][k].copy()).to(DEV), torch.from_numpy(b["seeds"][k].view(np.int32).copy()).to(DEV))


def staged(ds, rays, seeds, depth, diffuse=True, entry_ids=None, n_paths=None, alias=False, compact=True, flags=0):
    """A path in stages from the primitives: entry k of `rays` is path entry_ids[k] (None: k) of
    n_paths.  Returns the clamped radiance by path id."""
    n = rays.shape[0] if n_paths is None else n_paths
    state = ds.path_begin(n, seeds)
    cur, ids = rays.clone(), entry_ids
    for d in range(depth):
        last = d + 1 == depth
        hits = ds.trace_hits(cur, flags)
        nxt, alive = ds.path_step(cur, hits, state, ids, None, diffuse, sc.MISS, flags, last=last,
                                  next_rays=cur if alias and not last else None)
        if last:
            assert nxt is None and alive is None
            break
        if alias:
            assert nxt.data_ptr() == cur.data_ptr()
        if compact:
            cur, ids, count = rt.compact_paths(alive, nxt, ids)
            if count == 0:
                break
        else:
            own = ids if ids is not None else torch.arange(cur.shape[0], dtype=torch.int32, device=DEV)
            cur, ids = nxt, torch.where(alive != 0, own, torch.full_like(own, -1))
    return rt.path_finish(state)


# ---- 1. staged equals monolith equals reference ----------------------------------------------------
@pytest.mark.parametrize("diffuse", [True, False], ids=["diffuse", "mirror"])
@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("name", sc.SCENES)
def test_trace_paths_equals_the_reference(name, depth, diffuse):
    ds = scene(name)
    rays, seeds = dev_batch(name)
    want = sc.reference(name, depth, diffuse)[0]
    a = rb.scene_arrays(name)
    variants = {0: sc.rule_variant(a)[0]}
    if sc.rule_variant(a, BINARY)[0] != variants[0]:
        variants[BINARY] = sc.rule_variant(a, BINARY)[0]
    mono = ds.shade_rays(rays, seeds, max_depth=depth, diffuse_bounce=diffuse, miss_color=sc.MISS)
    assert np.array_equal(bits(mono), bits(want))
    for flags, variant in variants.items():
        for compact in (True, False):
            got = ds.trace_paths(rays, seeds, depth, diffuse, sc.MISS, compact=compact, flags=flags)
            assert ds.path_step_variant() == variant
            bad = (bits(got) != bits(want)).any(axis=1)
            assert not bad.any(), (name, depth, diffuse, flags, compact, int(bad.sum()), np.flatnonzero(bad)[:4])


def test_the_scenes_cover_the_three_variants():
    seen = set()
    for name in sc.SCENES:
        a = rb.scene_arrays(name)
        seen |= {sc.rule_variant(a)[0], sc.rule_variant(a, BINARY)[0]}
    assert seen == {L.RT_RAYS_VARIANT_WIDE, L.RT_RAYS_VARIANT_BINARY, L.RT_RAYS_VARIANT_DEEP}


def test_default_seeds_and_no_depth():
    ds = scene("frog")
    rays, _ = dev_batch("frog")
    assert ds.trace_paths(rays, None, 0).abs().sum().item() == 0 and ds.trace_paths(rays[:0], None, 3).shape == (0, 3)
    got = ds.trace_paths(rays, None, 3, True, sc.MISS)
    mono = ds.shade_rays(sc.caller_batch("frog")["rays"], None, max_depth=3, miss_color=sc.MISS)  # seeds 42: the host path
    assert np.array_equal(bits(got), bits(mono))


def _case_camera(name):
    c = sf.case(name)
    pos, look, up, f, s = c["camera"]
    return rt.Camera(pos, look, up, f, s, c["W"], c["H"])


@pytest.mark.parametrize("name", pc.FIXTURE_CASES)
def test_fuzz_frames_through_trace_paths(name):
    """camera_rays -> trace_paths -> Film is the reference's frame; the first segment's records
    carry the reference's primary hits and t."""
    c = sf.case(name)
    ds, cam = scene(name), _case_camera(name)
    H, W, spp = c["H"], c["W"], c["spp"]
    rays, seeds = rt.camera_rays(cam, spp, device=0)
    rad = ds.trace_paths(rays, seeds, c["depth"], c["diffuse"])
    with rt.Film(W, H) as film:
        film.add(rad)
        rgb = film.resolve().cpu().numpy()
    f = rt.hit_fields(ds.trace_hits(rays))
    sf.check_against_fixture(name, rgb, f["tri"].cpu().numpy().reshape(H, W, spp), f["t"].cpu().numpy().reshape(H, W, spp))


def test_render_rays_with_a_material_fn_that_returns_none():
    name = "s_l1_d4m"
    c = sf.case(name)
    ds, cam = scene(name), _case_camera(name)
    calls = []

    def fn(hits, rays, ids, depth):
        calls.append((tuple(hits.shape), tuple(rays.shape), tuple(ids.shape), depth))
        return None

    plain = ds.render_rays(cam, c["spp"], c["depth"], c["diffuse"])
    hooked = ds.render_rays(cam, c["spp"], c["depth"], c["diffuse"], material_fn=fn)
    assert np.array_equal(bits(hooked), bits(plain)) and np.array_equal(bits(plain), bits(sf.fixture_frames(name)[0]))
    assert [k[3] for k in calls] == list(range(len(calls))) and 1 < len(calls) <= c["depth"]
    assert all(k[0] == (k[2][0], 16) and k[1] == (k[2][0], 6) for k in calls) and calls[0][2][0] == c["H"] * c["W"] * c["spp"]
    assert calls[1][2][0] < calls[0][2][0]  # compacted


# ---- 2. per-hit materials ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.TABLE_B_CASES)
def test_per_hit_materials(name):
    """The scene holds the case's own table; material_fn hands every hit B[hit.material] (the
    Material() defaults for -1): the frame is the oracle's render of the case with table B."""
    c = sf.case(name)
    ds, cam = scene(name), _case_camera(name)
    B = pc.table_b(name)
    nm = B.shape[0]
    T = torch.from_numpy(np.vstack([B, pc.default_material()[None, :]])).to(DEV)
    seen = set()

    def fn(hits, rays, ids, depth):
        mat = rt.hit_fields(hits)["material"].long()
        seen.update(np.unique(mat.cpu().numpy()).tolist())
        return T[torch.where(mat >= 0, mat, torch.full_like(mat, nm))]

    got = ds.render_rays(cam, c["spp"], c["depth"], c["diffuse"], material_fn=fn)
    want, _ = pc.oracle_render_with_b(name)
    bad = (bits(got) != bits(want)).any(axis=2)
    assert not bad.any(), f"{name}: {int(bad.sum())} pixels differ from the oracle's render with table B"
    own = sf.fixture_frames(name)[0]
    assert (bits(got) != bits(own)).any(), "table B changed nothing"
    assert -1 in seen and seen >= set(range(nm))  # the defaults and every entry were handed out


# ---- 3. direct, placement ------------------------------------------------------------------------------
def test_direct_is_what_the_step_adds():
    name = "cornell"
    ds = scene(name)
    rays, seeds = dev_batch(name)
    state = ds.path_begin(rays.shape[0], seeds)
    hits = ds.trace_hits(rays)
    nxt, alive, direct = ds.path_step(rays, hits, state, miss_color=sc.MISS, direct=True)
    hit = (rt.hit_fields(hits)["tri"] >= 0).cpu().numpy()
    rad, direct = state.radiance.cpu().numpy(), direct.cpu().numpy()
    assert hit.any() and (~hit).any() and direct[hit].any()
    assert np.array_equal(rad[hit], direct[hit]) and not direct[~hit].any()
    assert np.array_equal(rad[~hit], np.broadcast_to(np.array(sc.MISS, np.float32), rad[~hit].shape))
    want = sc.reference(name, 1, True)[0]  # the unclamped sum of one depth, clamped, is the depth-1 radiance
    assert np.array_equal(bits(rt.path_finish(state)), bits(want))
    # a dead entry's next ray is its input ray, byte for byte; a live one's is new
    dead = (alive == 0).cpu().numpy()
    assert dead[~hit].all() and (~dead).any()
    assert np.array_equal(bits(nxt)[dead], bits(rays)[dead]) and (bits(nxt)[~dead] != bits(rays)[~dead]).any(axis=1).all()


@pytest.mark.parametrize("m", pc.PLACEMENT_SIZES)
def test_batch_sizes(m):
    """m entries: the first m answers, and not a byte past entry m of the outputs."""
    name = "frog"
    ds = scene(name)
    rays, seeds = dev_batch(name, m)
    want = sc.reference(name, 3, True)[0][wrap(m)]
    assert np.array_equal(bits(ds.trace_paths(rays, seeds, 3, True, sc.MISS)), bits(want))
    assert np.array_equal(bits(ds.trace_paths(rays, seeds, 3, True, sc.MISS, compact=False, flags=BINARY)), bits(want))
    state = ds.path_begin(m, seeds)
    big = torch.full((m + 64, 6), -3.25, dtype=torch.float32, device=DEV)
    hits = ds.trace_hits(rays)
    nxt, alive = ds.path_step(rays, hits, state, miss_color=sc.MISS, next_rays=big[:m])
    assert nxt.data_ptr() == big.data_ptr() and alive.shape == (m,) and int(alive.max()) <= 1
    assert (big[m:] == -3.25).all() and (big[:m] != -3.25).any(dim=1).all()


def test_shuffled_entries_with_shuffled_ids():
    name = "cornell"
    ds = scene(name)
    rays, seeds = dev_batch(name)
    want = sc.reference(name, 3, True)[0]
    perm = torch.from_numpy(np.random.default_rng(5).permutation(sc.N_CALLER)).to(DEV)
    ids = perm.to(torch.int32)
    for compact in (True, False):
        got = staged(ds, rays[perm].contiguous(), seeds, 3, entry_ids=ids, compact=compact)  # seeds stay by path id
        assert np.array_equal(bits(got), bits(want)), compact
    # a shuffled batch through trace_paths returns the shuffled answers
    got = ds.trace_paths(rays[perm].contiguous(), seeds[perm].contiguous(), 3, True, sc.MISS)
    assert np.array_equal(bits(got), bits(want[perm.cpu().numpy()]))


@pytest.mark.parametrize("name", ["frog", "chain300"])
def test_next_rays_aliased_onto_rays(name):
    ds = scene(name)
    rays, seeds = dev_batch(name)
    want = sc.reference(name, 3, True)[0]
    for compact in (True, False):
        assert np.array_equal(bits(staged(ds, rays, seeds, 3, alias=True, compact=compact)), bits(want)), compact
    assert np.array_equal(bits(rays), sc.caller_batch(name)["rays"].view(np.uint32))  # staged() works on a copy


def test_last_with_null_outputs_and_with_outputs():
    name = "cornell"
    ds = scene(name)
    rays, seeds = dev_batch(name)
    want = sc.reference(name, 1, True)[0]
    hits = ds.trace_hits(rays)
    state = ds.path_begin(rays.shape[0], seeds)
    assert ds.path_step(rays, hits, state, miss_color=sc.MISS, last=True) == (None, None)
    assert np.array_equal(bits(rt.path_finish(state)), bits(want))
    assert np.array_equal(state.rng.cpu().numpy(), seeds.cpu().numpy()) and (state.throughput == 1).all()  # no draw
    state = ds.path_begin(rays.shape[0], seeds)
    out = torch.full_like(rays, -3.25)
    nxt, alive = ds.path_step(rays, hits, state, miss_color=sc.MISS, last=True, next_rays=out)
    assert not alive.any() and np.array_equal(bits(nxt), bits(rays))
    assert np.array_equal(bits(rt.path_finish(state)), bits(want))


def test_finish_keeps_nan_and_negative_zero():
    ds = scene("frog")
    state = ds.path_begin(3)
    v = np.array([[np.nan, -0.0, 2.0], [-1.0, 0.5, 1.0], [1.5, -np.inf, np.inf]], np.float32)
    state.radiance.copy_(torch.from_numpy(v))
    assert np.array_equal(bits(rt.path_finish(state)), bits(pc.clamp01(v)))


# ---- 4. compaction ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", pc.COMPACT_SIZES)
def test_compaction_against_flatnonzero(m):
    k = torch.arange(m, dtype=torch.int32, device=DEV)
    rays = (k[:, None] * 6 + torch.arange(6, dtype=torch.int32, device=DEV)[None, :]).view(torch.float32).contiguous()  # any bits
    ids_in = (k * 7 + 3).contiguous()
    rays_h, ids_h = rays.cpu().numpy().view(np.uint32), ids_in.cpu().numpy()
    for kind in pc.PATTERNS:
        flags = pc.flags_pattern(kind, m)
        nz = np.flatnonzero(flags)
        alive = torch.from_numpy(flags).to(DEV)
        for with_ids in (False, True):
            out_r, out_i, count = rt.compact_paths(alive, rays, ids_in if with_ids else None)
            assert count == nz.size and out_r.shape == (count, 6) and out_i.shape == (count,), (kind, with_ids, count, nz.size)
            assert np.array_equal(out_i.cpu().numpy(), ids_h[nz] if with_ids else nz.astype(np.int32)), (kind, with_ids)
            assert np.array_equal(out_r.cpu().numpy().view(np.uint32), rays_h[nz]), (kind, with_ids)


def test_compaction_past_one_scan_tile():
    """2048 * 2048 + 1 entries: the first size whose tile counts need a second scan level."""
    m = 2048 * 2048 + 1
    assert L.lib().rt_path_compact_scratch_bytes(m) == 4 * (2049 + 2)
    k = torch.arange(m, dtype=torch.int32, device=DEV)
    rays = k[:, None].expand(m, 6).contiguous().view(torch.float32)
    ids_in = (k * 7 + 3).contiguous()
    for kind in ("last", "random_0.5"):
        flags = pc.flags_pattern(kind, m)
        nz = torch.from_numpy(np.flatnonzero(flags)).to(DEV)
        out_r, out_i, count = rt.compact_paths(torch.from_numpy(flags).to(DEV), rays, ids_in)
        assert count == nz.shape[0], (kind, count)
        assert torch.equal(out_i, ids_in[nz]) and torch.equal(out_r.view(torch.int32), rays.view(torch.int32)[nz]), kind


def test_compaction_refuses_overlapping_buffers():
    m = 100
    alive = torch.ones(m, dtype=torch.uint8, device=DEV)
    rays = torch.zeros((2 * m, 6), dtype=torch.float32, device=DEV)
    ids = torch.zeros(2 * m, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    scratch = torch.zeros(16, dtype=torch.int32, device=DEV)
    lib = L.lib()
    st = torch.cuda.current_stream(DEV).cuda_stream
    r, i = rays.data_ptr(), ids.data_ptr()
    ok = lib.rt_path_compact_device(0, m, alive.data_ptr(), r, i, r + 24 * m, i + 4 * m, count.data_ptr(), scratch.data_ptr(), st)
    assert ok == 0 and count.item() == m
    count.fill_(-5)
    for ro, io in ((r, i + 4 * m), (r + 24 * (m - 1), i + 4 * m), (r + 24 * m, i), (r + 24 * m, i + 4 * (m - 1))):
        assert lib.rt_path_compact_device(0, m, alive.data_ptr(), r, i, ro, io, count.data_ptr(), scratch.data_ptr(), st) == -1
    torch.cuda.synchronize()
    assert count.item() == -5


# ---- 5. beside frames, on a clone --------------------------------------------------------------------------
def test_staged_paths_beside_a_renderers_frames():
    """Three frames in flight on a Renderer while a batch runs in stages against its scene on a
    stream of its own: the frames are the frame rendered alone, no device guard fires, the radiances
    equal the oracle's."""
    name = "cornell"
    hs = host_scene(name + ".json")
    want = sc.reference(name, 3, True)[0]
    cam = hs.camera(64, 48)
    o, _jit = rt.DeviceScene.make_opts(spp=4, max_depth=1, miss_color=hs.settings["miss_color"])
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3)
    try:
        kept = r.render(cam, spp=4, max_depth=1, miss_color=hs.settings["miss_color"]).tobytes()
        ds = r.scene(0)
        rays, seeds = dev_batch(name)
        side = torch.cuda.Stream(DEV)
        torch.cuda.synchronize()
        tickets = [r.submit(cam, o) for _ in range(3)]
        with torch.cuda.stream(side):
            got = ds.trace_paths(rays, seeds, 3, True, sc.MISS)
        for k in tickets:
            addr, n = r.wait(k)
            assert bytes((C.c_uint8 * n).from_address(addr)) == kept, k
        assert ds.faults() == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(got), bits(want))
    finally:
        r.close()


def test_a_clone_gives_the_same_answers():
    name = "frog"
    rays, seeds = dev_batch(name)
    want = sc.reference(name, 3, True)[0]
    h = C.c_void_p()
    L.check(L.lib().rt_scene_clone(scene(name).handle, 0, C.byref(h)))
    try:
        assert L.lib().rt_path_step_variant(h) == L.RT_RAYS_VARIANT_NONE
        clone = rt.DeviceScene._borrow(h.value, scene(name).num_triangles, None)
        assert np.array_equal(bits(clone.trace_paths(rays, seeds, 3, True, sc.MISS)), bits(want))
        assert L.lib().rt_path_step_variant(h) == L.RT_RAYS_VARIANT_WIDE
    finally:
        L.lib().rt_scene_destroy(h)
