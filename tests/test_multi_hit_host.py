"""The multi-hit query on the CPU (rt_multi_hits_host), bytes and no tolerance:

* the host build against tests/multi_hit_cases.py's model, record for record and count for count,
  for every scene, every k of KS, unbounded and with a per-ray max_t drawn around the model's own
  hit distances;
* a sub-sample of the records' t against the oracle's intersectTriangle (orc_intersect_g);
* the properties that tie the query to SearchBVH's closest hit;
* what the inputs contain, asserted on the model (not on the code under test);
* the argument rules of the host build and of the device entries, which answer before any HIP call.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import multi_hit_cases as mh

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L


def host(name, k, max_t=None, r=None):
    a = mh.arrays(name)
    return rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], mh.rays(name) if r is None else r, k, max_t)


# ---- 1. the host build equals the model --------------------------------------------------------
@pytest.mark.parametrize("bound", mh.BOUNDS)
@pytest.mark.parametrize("name", mh.SCENES)
def test_host_build_equals_the_model(name, bound):
    m = mh.model(name, bound)
    assert mh.rays(name).shape[0] >= 4096
    for k in mh.KS:
        got, want = host(name, k, m["max_t"]), mh.take(m, k)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape
        bad = mh.differing_rays(got, want)
        assert bad.size == 0, (name, bound, k, bad[:4], got[0][bad[:4]], want[0][bad[:4]])
        assert all(mh.same_bytes(g, w) for g, w in zip(got, want))
    print(f"{name} {bound}: {int(m['count'].sum())} hits, most {int(m['count'].max())}, "
          f"{int((m['count'] > 32).sum())} rays past k = 32, {int(m['overflow'].sum())} overflowed")


def test_bounds_are_around_the_hit_distances():
    """The per-ray max_t really cuts at, just below and far from a hit: what each kind leaves."""
    for name in ("frog", "small", "chain300"):
        m0, m1 = mh.model(name, "none"), mh.model(name, "around")
        mt, n = m1["max_t"], m0["count"].size
        kind = np.arange(n) % 4
        hit = m0["count"] > 0
        assert (m1["count"][kind == 2] == 0).all() and (mt[kind == 2] < 1e-4).all()
        assert np.array_equal(m1["count"][kind == 3], m0["count"][kind == 3]) and np.isinf(mt[kind == 3]).all()
        # exactly a hit's t: that hit counts (t <= tmax) where its boxes still pass (a flat box's
        # slab parameter, computed in double, may lie above a t that Moller-Trumbore rounded down
        # in float: the reference would not open it either); one ulp below: it does not
        at, below = hit & (kind == 0), hit & (kind == 1)
        assert at.sum() >= 100 and below.sum() >= 100
        last = m1["start"][1:] - 1
        kept = at & (m1["count"] > 0)
        on_bound = m1["t"][last[kept]].view(np.uint32) == mt[kept].view(np.uint32)
        print(f"{name}: of {int(at.sum())} rays bounded at a hit's t, {int(on_bound.sum())} keep that hit")
        assert on_bound.sum() >= 100
        assert (m1["count"][below] < m0["count"][below]).all()
        some = (at | below) & (m1["count"] > 0)
        assert (m1["t"][last[some]] <= mt[some]).all()


# ---- 2. t against the oracle's intersectTriangle ------------------------------------------------
@pytest.mark.parametrize("name", ["frog", "cornell", "small", "chain600"])
def test_t_is_the_oracles_t(name):
    from oracle import pyoracle as orc

    m = mh.model(name, "none")
    a, r = mh.arrays(name), mh.rays(name)
    count, tri, t, _, _ = host(name, 8)
    rays_, slots = np.nonzero(tri >= 0)
    pick = np.random.default_rng(3).choice(rays_.size, min(256, rays_.size), replace=False)
    assert pick.size >= 200
    for i, j in zip(rays_[pick], slots[pick]):
        hit, tt = orc.intersect_g(a["tris"][tri[i, j]], r[i, 3:6], origin=r[i, 0:3], tmin=1e-4)
        assert hit[0] == 1 and mh.same_bytes(tt[:1], t[i, j:j + 1]), (i, j)
    assert np.array_equal(count, m["count"])


# ---- 3. the closest hit -------------------------------------------------------------------------
@pytest.mark.parametrize("name", mh.SCENES)
def test_closest_hit_properties(name):
    """SearchBVH's hit is a member of S, count > 0 exactly when it hits, hits[0].t <= its t."""
    c = mh.closest(name)
    n = c["idx"].size
    count, tri, t, _, _ = (x[:n] for x in host(name, 1))
    hit = c["idx"] >= 0
    assert hit.sum() >= 256
    assert np.array_equal(count > 0, hit)
    assert (t[hit, 0] <= c["t"][hit]).all() and (t[hit, 0] >= np.float32(1e-4)).all()
    m = mh.model(name, "none")
    key = (m["ray"].astype(np.int64) << 32) | m["tri"].astype(np.int64)
    want = (np.flatnonzero(hit).astype(np.int64) << 32) | c["idx"][hit].astype(np.int64)
    pos = np.searchsorted(np.sort(key), want)
    assert (np.sort(key)[np.minimum(pos, key.size - 1)] == want).all()
    at = np.argsort(key)[np.minimum(pos, key.size - 1)]
    assert mh.same_bytes(m["t"][at], c["t"][hit])  # the same t bits as the closest-hit query


# ---- 4. what the inputs contain (asserted on the model) ---------------------------------------
def test_frog_has_rays_with_many_hits():
    import ray_batches as rb

    m = mh.model("frog", "none")
    a = m["count"][rb.class_slices()["A"]]
    assert (a > 2).mean() >= 0.01, float((a > 2).mean())


def test_lattice_lists_hold_ties():
    m = mh.model("small", "none")
    _, _, t, _, _ = mh.take(m, 8)
    hit = m["count"] > 0
    tie = ((t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0)).any(axis=1)
    assert hit.sum() >= 1000 and tie[hit].mean() >= 0.25, float(tie[hit].mean())
    # and equal t is ordered by triangle index
    _, tri, t, _, _ = mh.take(m, 32)
    eq = (t[:, 1:] == t[:, :-1]) & (t[:, 1:] > 0)
    assert eq.sum() >= 1000 and (tri[:, 1:][eq] > tri[:, :-1][eq]).all()


def test_the_axis_ray_of_the_chains():
    m3, m6 = mh.model("chain300", "none"), mh.model("chain600", "none")
    assert m3["count"][-1] >= 256 and not m3["overflow"].any()
    assert m6["overflow"][-1] and m6["count"][-1] > m6["dfs_count"][-1] > 0
    assert m6["count"][-1] == 600
    # rays past k = 32, and overflowed rays, are common in the batch itself
    assert (m6["count"] > 32).sum() >= 256 and m6["overflow"][:-1].sum() >= 64
    assert (m6["count"][m6["overflow"]] >= m6["dfs_count"][m6["overflow"]]).all()


@pytest.mark.parametrize("name", mh.CHAINS)
def test_the_duplicated_triangle_is_a_tie_ordered_by_index(name):
    perm = mh.arrays(name)["perm"]
    lo, hi = int(perm[0]), int(perm[3])
    assert lo < hi
    _, tri, t, _, _ = mh.take(mh.model(name, "none"), 4)
    both = (tri[:, 0] == lo) & (tri[:, 1] == hi)
    assert both.sum() >= 64
    assert mh.same_bytes(t[both, 0], t[both, 1])
    assert not ((tri[:, :-1] == hi) & (tri[:, 1:] == lo)).any()


# ---- 5. arguments -------------------------------------------------------------------------------
# A scene handle that is never read: every check below answers before the scene is touched.
_FAKE_SCENE = C.create_string_buffer(64)
_RAYS = np.zeros((4, 6), np.float32)
_BUF = np.zeros(4 * 32 * 16 + 64, np.uint8)
_CNT = np.zeros(4, np.int32)
_ALIGNED = _BUF.ctypes.data + (-_BUF.ctypes.data) % 16
_S, _R, _N = C.addressof(_FAKE_SCENE), _RAYS.ctypes.data, _CNT.ctypes.data
BIN = L.RT_FLAG_BINARY

# (scene, rays, max_t, n, k, flags, hits, count) -> code
ARG_CASES = {
    "null scene": ((None, _R, None, 4, 4, 0, _ALIGNED, _N), -1),
    "null rays": ((_S, None, None, 4, 4, 0, _ALIGNED, _N), -1),
    "k = -1": ((_S, _R, None, 4, -1, 0, _ALIGNED, _N), -1),
    "k = 33": ((_S, _R, None, 4, 33, 0, _ALIGNED, _N), -1),
    "both outputs null": ((_S, _R, None, 4, 4, 0, None, None), -1),
    "k = 0 and no count": ((_S, _R, None, 4, 0, 0, _ALIGNED, None), -1),
    "k > 0 and no hits": ((_S, _R, None, 4, 4, 0, None, _N), -1),
    "unknown flag": ((_S, _R, None, 4, 4, L.RT_FLAG_NO_CULL, _ALIGNED, _N), -1),
    "unknown flag beside BINARY": ((_S, _R, None, 4, 4, BIN | 8, _ALIGNED, _N), -1),
    "n = 2^31": ((_S, _R, None, 1 << 31, 0, 0, None, _N), -7),
    "n k = 2^31": ((_S, _R, None, 1 << 26, 32, BIN, _ALIGNED, _N), -7),
}


@pytest.mark.parametrize("entry", ["rt_trace_multi_hits", "rt_trace_multi_hits_device"])
@pytest.mark.parametrize("case", sorted(ARG_CASES))
def test_argument_errors_need_no_device(entry, case):
    args, code = ARG_CASES[case]
    rc = getattr(L.lib(), entry)(*args, None)  # kernel_ms / hip_stream
    assert rc == code, (case, rc, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _BUF.any() and not _CNT.any()  # nothing was written


def test_no_rays_no_launch_and_misaligned_records():
    lib = L.lib()
    for entry in (lib.rt_trace_multi_hits, lib.rt_trace_multi_hits_device):
        assert entry(_S, _R, None, 0, 4, 0, _ALIGNED, _N, None) == 0  # no rays: no launch, no device
        assert entry(_S, _R, None, 0, 0, BIN, None, _N, None) == 0
    for off in (4, 8, 12):
        assert lib.rt_trace_multi_hits_device(_S, _R, None, 4, 4, 0, _ALIGNED + off, _N, None) == -1
        assert b"aligned" in lib.rt_last_error()
    assert lib.rt_trace_multi_hits_variant(None) == rt.RT_RAYS_VARIANT_NONE
    assert rt.RT_MULTI_HIT_MAX_K == 32 and rt.MULTI_HIT_DTYPE.itemsize == 16
    assert [rt.MULTI_HIT_DTYPE.fields[f][1] for f in ("tri", "t", "u", "v")] == [0, 4, 8, 12]
    assert not _BUF.any() and not _CNT.any()


def test_host_build_arguments():
    lib = L.lib()
    a = mh.arrays("sphere_single")
    nd, bx, tr = (a[k].ctypes.data for k in ("nodes", "aabbs", "tris"))
    P = int(a["P"])
    ok = (P, nd, bx, tr, _R, None, 4)
    assert lib.rt_multi_hits_host(*ok, 4, _ALIGNED, _N) == 0
    assert lib.rt_multi_hits_host(*ok, 4, _ALIGNED + 4, None) == 0  # host records need no alignment
    assert lib.rt_multi_hits_host(*ok, 0, None, _N) == 0
    for args in ((*ok, 33, _ALIGNED, _N), (*ok, -1, _ALIGNED, _N), (*ok, 4, None, _N), (*ok, 0, None, None),
                 (0, nd, bx, tr, _R, None, 4, 4, _ALIGNED, _N), (P, None, bx, tr, _R, None, 4, 4, _ALIGNED, _N),
                 (P, nd, bx, tr, None, None, 4, 4, _ALIGNED, _N)):
        assert lib.rt_multi_hits_host(*args) == -1, args
    bad = a["nodes"].copy()
    bad[0, 1] = 2 * P + 5  # a child outside the array
    assert lib.rt_multi_hits_host(P, bad.ctypes.data, bx, tr, _R, None, 4, 4, _ALIGNED, _N) == -1
    if P > 1:
        loop = a["nodes"].copy()
        loop[0, 1] = 0  # the root its own child
        r = np.ascontiguousarray(mh.rays("sphere_single")[:4])
        assert lib.rt_multi_hits_host(P, loop.ctypes.data, bx, tr, r.ctypes.data, None, 4, 4, _ALIGNED, _N) == -1
    with pytest.raises(ValueError):
        rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((2, 5), np.float32), 4)
    with pytest.raises(ValueError):
        rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((2, 6), np.float32), 33)
    with pytest.raises(ValueError):
        rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((2, 6), np.float32), 4, max_t=np.zeros(3, np.float32))
    c, tri, t, u, v = rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], np.zeros((0, 6), np.float32), 4)
    assert c.shape == (0,) and tri.shape == t.shape == u.shape == v.shape == (0, 4)


def test_unspecified_inputs_terminate_and_fill_every_output():
    """NaN and infinite rays and bounds: the call returns and writes every slot (values unspecified)."""
    a = mh.arrays("cornell")
    r = mh.rays("cornell")[:64].copy()
    r[0::4, 3] = np.nan
    r[1::4, 0] = np.inf
    r[2::4, 3:6] = 0.0
    mt = np.full(64, np.nan, np.float32)
    mt[::2] = -1.0
    for max_t in (None, mt):
        count, tri, t, u, v = rt.multi_hits_host(a["nodes"], a["aabbs"], a["tris"], r, 4, max_t)
        assert (count >= 0).all()
        filled = np.arange(4)[None, :] < np.minimum(count, 4)[:, None]
        assert (tri[filled] >= 0).all() and (tri[~filled] == -1).all() and (t[~filled] == -1.0).all()
