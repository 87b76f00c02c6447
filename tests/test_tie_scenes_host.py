"""The tie scenes of tests/tie_scenes.py contain what they are for, shown with the oracle alone (no
GPU), and the oracle is pinned to the reference on them.  These are conditions the generator's
seeds must meet, not measurements of the code under test: tests/test_gpu_ties.py compares the
kernels with the oracle on exactly these batches, and could pass by emptiness otherwise.

Measured (classify's brute-force float32 restatement against the oracle's SearchBVH; 4096 rays):

  batch   hit    >=2 tied  >=4 tied  winner smallest/largest/neither  t above  oracle misses,  near tie
                                     (of the tied rays)               bf min   one accepts    (1-3 ulp)
  small   0.945  0.919     0.469     0.385 / 0.213 / 0.402            5        1              0.030
  large   0.946  0.934     0.573     0.332 / 0.206 / 0.462            6        4              0.019
  scaled  0.941  0.752     0.303     0.324 / 0.360 / 0.316            33       14             0.379

  ("t above bf min": the oracle's t exceeds the smallest accepted t: the closer triangle's flat box
  has a slab parameter, computed in double, above a bestT that Moeller-Trumbore rounded down in
  float, so the reference never opens it.  The scaled scene is the small one times 3: exact ties
  turn into near ties, so it is held to the near-tie share instead of the tie floors.)

  frame     hit samples  with a second triangle at the same t  winner smallest/largest/neither  t above bf min
  small_d1  0.681        0.595                                 1571 / 1680 / 483                124
  small_d3  0.523        0.516                                 822 / 672 / 166                  13
  large_d1  0.611        0.705                                 1675 / 2176 / 619                99

  soup (96x72, spp 1 and 4 alike)  hit    winners with a verbatim copy
  mixed                            1.000  0.672
  edge_on                          0.580  0.999
  around                           1.000  0.902
  slivers                          0.740  1.000

  (A few near triangles cover most of a mixed or around image (5 and 3 distinct winners), so the
  share of winners with copies swings with the soup's seed; the 12 large repeated triangles win
  nearly every hit sample of the edge_on and slivers soups.)

HW1 chunk boundaries: a tile's bin list is filled through an atomic cursor (hw1_fill_kernel), so
its order is not a function of the scene and "the tied pair straddles a 32-entry chunk boundary"
cannot be stated on the CPU.  What is stated here instead: some tile's candidate list (the
triangles whose projected bounding rectangle meets the 16x4 tile; a subset of it is what the
kernel lists) is longer than 256 entries and holds a tied pair, and the chunk sweep of
tests/test_gpu_ties.py (16, 32, 64, 256 entries, every fuse setting) runs on these soups.
"""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import hit_records as hr
import shade_fuzz as sf
import tie_scenes as ts
from conftest import golden_meta, hexv
from test_gpu_trace_rays import occlusion_from

import raytracinginonesemester_amd as rt

NAMES = list(ts.SCENES)
HIT_FRACTION = {"small": 0.945, "large": 0.946, "scaled": 0.941}


def test_generator_is_deterministic_and_shaped():
    a = ts.scene("small")
    b = ts.lattice_scene(*ts.SCENES["small"][:3])
    for k in ("nodes", "aabbs", "tris", "triobj", "mats", "lights"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert 300 <= a["P"] <= 400 and 3000 <= ts.scene("large")["P"] <= 10000
    rays = ts.lattice_rays(a, ts.N_RAYS, ts.SCENES["small"][3])
    assert rays.shape == (ts.N_RAYS, 6) and rays.dtype == np.float32 and np.isfinite(rays).all()
    assert np.array_equal(rays, ts.batch("small")["rays"])
    # the plane's vertices are multiples of 0.5; the root box is not flat
    assert np.array_equal(a["tris"][:, :9] * 2, np.round(a["tris"][:, :9] * 2))
    assert a["aabbs"][0, 2] == -1.0 and a["aabbs"][0, 5] == 0.0
    # an eighth repeated verbatim (all 18 floats), an eighth with rotated vertices, far apart in index
    for kind, same in ((1, True), (2, False)):
        copies = np.flatnonzero(a["kind"] == kind)
        assert copies.size == (a["P"] - 2 * copies.size) // 8
        orig = np.array([np.flatnonzero((a["group"] == a["group"][c]) & (a["kind"] == 0))[0] for c in copies])
        assert (a["tris"][copies].tobytes() == a["tris"][orig].tobytes()) == same
        assert np.array_equal(np.sort(a["tris"][copies, :9].reshape(-1, 3, 3), axis=1),
                              np.sort(a["tris"][orig, :9].reshape(-1, 3, 3), axis=1))
        assert np.abs(copies - orig).mean() > a["P"] / 8
    # unnormalised directions: t is 1/s
    d = rays[:, 3:].astype(np.float64)
    assert set(np.round(-d[:, 2] / rays[:, 2], 6)) == {0.5, 1.0, 2.0, 3.0}
    s3 = ts.scene("scaled")
    assert np.array_equal(s3["tris"][:, :9], a["tris"][:, :9] * np.float32(3.0)) and np.array_equal(s3["nodes"], a["nodes"])
    assert int((a["lights"]["position"][:, 2] > 0).sum()) == 3 and int((a["lights"]["position"][:, 2] == 0).sum()) == 1


@pytest.mark.parametrize("name", NAMES)
def test_lattice_batches_meet_the_floors(name):
    b = ts.batch(name)
    hit = b["idx"] >= 0
    f = ts.figures(ts.classes(name), hit)
    print(name, {k: round(v, 3) for k, v in f.items()})
    assert abs(f["hit"] - HIT_FRACTION[name]) < 5e-4, "the batch is not the one the figures were recorded for"
    if name == "scaled":  # exact ties turned into near ties
        assert f["near"] >= 0.10 and f["tied2"] >= 0.5
    else:
        assert f["tied2"] >= 0.80 and f["tied4"] >= 0.40
        assert f["near"] >= 0.01
    assert min(f["smallest"], f["largest"], f["neither"]) >= 0.10
    assert f["above_min"] >= 4
    assert f["miss_but_accepts"] >= 1
    for cls, s in ts.class_slices().items():
        k = int(hit[s].sum())
        print(f"  class {cls}: {k} hits of {hit[s].size}")
        assert 0 < k < hit[s].size, f"class {cls} has no {'hit' if k == 0 else 'miss'}"
    assert np.array_equal(b["t"] == -1.0, ~hit) and b["idx"].max() < ts.scene(name)["P"]


@pytest.mark.parametrize("name", NAMES)
def test_occlusion_outcomes_at_t_and_its_successor(name):
    """occlusion_from's cycle puts max_t = t on hit ray i with i % 6 == 1 and nextafter(t) with
    i % 6 == 2: the strict t < max_t answers no for the first and yes for the second, and both kinds
    have tied rays among them."""
    b = ts.batch(name)
    max_t, want = occlusion_from(b["idx"], b["t"])
    hit = b["idx"] >= 0
    at_t = hit & (max_t == b["t"])
    above = hit & (max_t == np.nextafter(b["t"], np.float32(np.inf), dtype=np.float32))
    assert at_t.sum() > 400 and above.sum() > 400
    assert not want[at_t].any() and want[above].all()
    tied = ts.classes(name)["tied"] >= 2
    assert (at_t & tied).sum() > 100 and (above & tied).sum() > 100
    assert want[hit].any() and (~want[hit]).any() and not want[~hit].any()


@pytest.mark.parametrize("name", NAMES)
def test_hit_record_branches_occur(name):
    b = ts.batch(name)
    rec, cls = hr.records_and_classes(ts.scene(name), b["rays"], b["idx"], b["t"])
    got = {k: int(cls[k].sum()) for k in ("hit", "back", "degenerate", "flipped")}
    print(name, got)
    assert min(got.values()) >= 16
    assert (rec["material"][cls["hit"]] == -1).any() and (rec["material"][cls["hit"]] >= 0).any()


# ---- frames ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ts.FRAME_CASES))
def test_frames_are_full_of_ties(name):
    c = ts.frame_case(name)
    rgb, hi, ht = sf.oracle_render(c, aov=True)
    rays, _ = rt.camera_rays(ts.frame_camera(name), c["spp"])
    cl = ts.classify(ts.scene(c["scene"]), rays, hi.reshape(-1), ht.reshape(-1))
    hit = hi.reshape(-1) >= 0
    tied = float((cl["tied"][hit] >= 2).mean())
    winners = [int((cl["winner"] == w).sum()) for w in (ts.SMALLEST, ts.LARGEST, ts.NEITHER)]
    print(name, "hit", round(float(hit.mean()), 3), "tied", round(tied, 3), "winners", winners, "above the minimum",
          int(cl["above_min"].sum()))
    assert 0.3 <= hit.mean() <= 0.9  # hits and misses
    assert tied >= 0.20
    assert winners[0] > 0 and winners[1] > 0
    assert (rgb >= 1.0).mean() <= 0.25 and rgb.mean() > 0.02
    if c["depth"] > 1:  # the bounces show where they can: from the lower layer up against the plane (0.074 of the pixels)
        d1 = sf.oracle_render(c, depth=1)
        assert ((d1.view(np.uint32) != rgb.view(np.uint32)).any(axis=2)).mean() > 0.05


@pytest.mark.parametrize("name", list(ts.FRAME_CASES))
def test_frame_generator_and_oracle_are_pinned_to_the_reference(name):
    """The case's arrays and camera are the fixture's, and orc.render_g reproduces the reference's
    own render() + SearchBVH on it bit for bit: frame, hit indices and t."""
    from oracle import pyoracle as orc

    c = ts.frame_case(name)
    meta = golden_meta("ties_" + name)
    assert sf.input_sha256(c) == {k: meta["sha256"][k] for k in sf.INPUTS}
    assert (meta["width"], meta["height"], meta["spp"], meta["max_depth"], bool(meta["diffuse_bounce"])) == \
        (c["W"], c["H"], c["spp"], c["depth"], c["diffuse"])
    assert meta["num_lights"] == 4 and meta["num_materials"] == 5
    pos, look, up, f, s = c["camera"]
    cam = orc.camera(pos, look, up, f, s, c["W"], c["H"])
    for k, v in (("center", cam.center), ("pixel00_loc", cam.pixel00), ("pixel_delta_u", cam.du),
                 ("pixel_delta_v", cam.dv)):
        assert np.array_equal(np.array([v.x, v.y, v.z], np.float32).view(np.uint32), hexv(meta[k]).view(np.uint32)), k
    rgb, hi, ht = sf.oracle_render(c, aov=True)
    ts.check_against_fixture(name, rgb, hi, ht)


def test_oracle_records_are_pinned_to_the_reference():
    """The reference's own hit records of the first 64 rays of each class of the small batch
    (tests/golden/hit_records/lattice10): the oracle's winner and hit_records' restated record are
    the bits SearchBVH wrote."""
    fx = hr.fixture(ts.HIT_RECORDS_NAME)
    b = ts.batch("small")
    pick = hr.fixture_pick()
    assert fx["rays"].tobytes() == b["rays"][pick].tobytes()
    hit = fx["hit"] != 0
    assert hit.sum() >= 64 and (~hit).sum() >= 8
    assert np.array_equal(np.where(hit, fx["tri"], -1), b["idx"][pick])
    rec = hr.ref_records(ts.scene("small"), fx["rays"], b["idx"][pick], b["t"][pick])
    assert rec["t"][hit].tobytes() == fx["t"][hit].tobytes()
    assert rec["p"][hit].tobytes() == fx["p"][hit].tobytes()
    assert rec["normal"][hit].tobytes() == fx["normal"][hit].tobytes()
    assert np.array_equal(rec["front_face"][hit], fx["front"][hit].astype(np.int32))
    assert (fx["t"][~hit] == -1.0).all()
    assert (ts.classes("small")["tied"][pick] >= 2).sum() >= 128  # the fixture's rays are tied rays


# ---- HW1 ------------------------------------------------------------------------------------------
def test_soup_copies_are_verbatim_and_spread():
    for kind in ts.SOUP_KINDS:
        s = ts.dup_soup(kind)
        g = s["group"]
        M = g.size
        v = s["positions"].reshape(M, 9)
        nn = s["normals"].reshape(M, 9)
        members = [np.flatnonzero(g == k) for k in np.unique(g)]
        copied = [m for m in members if m.size > 1]
        assert sum(m.size == 1 for m in members) == ts.N_SOUP - ts.N_SOUP // 4
        assert len(copied) == ts.N_SOUP // 4 + ts.N_LARGE and max(m.size for m in copied) == 4
        gaps = []
        for m in copied:
            assert all(v[i].tobytes() == v[m[0]].tobytes() and nn[i].tobytes() == nn[m[0]].tobytes() for i in m[1:])
            gaps += list(np.diff(m))
        gaps = np.array(gaps)
        # copies within a 16-entry chunk's reach and past 16, 32, 64 and 256 indices
        for lo, hi_ in ((1, 16), (16, 32), (32, 64), (64, 256), (256, M)):
            assert ((gaps >= lo) & (gaps < hi_)).sum() >= 8, (kind, lo)
        first_is_original = sum(int(m[0] == np.flatnonzero(g == g[m[0]])[0]) for m in copied)
        assert first_is_original == len(copied)


def _candidates(s, cam, tile):
    """Triangles in front of the camera whose projected bounding rectangle meets the 16x4 tile."""
    b = cam.basis()
    c, p00, du, dv = (np.asarray(b[k], np.float64) for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"))
    w = np.cross(du, dv)
    M = s["group"].size
    v = s["positions"].reshape(M, 3, 3).astype(np.float64) - c
    depth = v @ w
    plane = (p00 - c) @ w
    front = (depth * np.sign(plane) > 1e-9).all(axis=1)
    with np.errstate(all="ignore"):
        q = v * (plane / depth)[:, :, None] - (p00 - c)
        x, y = (q @ du) / (du @ du), (q @ dv) / (dv @ dv)
    tx, ty = tile
    return np.flatnonzero(front & (x.max(axis=1) >= 16 * tx) & (x.min(axis=1) <= 16 * tx + 16)
                          & (y.max(axis=1) >= 4 * ty) & (y.min(axis=1) <= 4 * ty + 4))


@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("kind", ts.SOUP_KINDS)
def test_hw1_oracle_keeps_the_first_index(kind, spp):
    """At least a tenth of the hit samples are won by a triangle that has verbatim copies (their t
    is the same in every bit), and the oracle's winner is the smallest index of them: the
    reference's rule, asserted of the oracle and not assumed."""
    s = ts.dup_soup(kind)
    g = s["group"]
    size = np.bincount(g)[g]
    first = np.full(g.max() + 1, -1)
    first[g[::-1]] = np.arange(g.size)[::-1]
    rgb, hi, ht = ts.soup_reference(kind, spp)
    w = hi.reshape(-1)[hi.reshape(-1) >= 0]
    tied = size[w] > 1
    print(kind, spp, "hit", round(float((hi >= 0).mean()), 3), "tied", round(float(tied.mean()), 3))
    assert (hi >= 0).mean() > 0.3 and tied.mean() >= 0.10
    assert np.array_equal(first[g[w]], w)
    # some tile has a long candidate list with a tied winner in it (see the module docstring)
    cam = ts.soup_camera(kind)
    longest = 0
    for ty in range(0, 18):
        for tx in range(0, 6):
            tile_w = hi[4 * ty:4 * ty + 4, 16 * tx:16 * tx + 16].reshape(-1)
            tile_w = tile_w[tile_w >= 0]
            if tile_w.size and (size[tile_w] > 1).any():
                longest = max(longest, _candidates(s, cam, (tx, ty)).size)
    assert longest > (256 if kind in ("mixed", "around") else 24), longest


def test_hw1_big_frame_soup_is_tied_too():
    """The smaller soup of the 640x480 GPU case, at 96x72: the same conditions."""
    n = ts.N_SOUP_BIG_FRAME
    g = ts.dup_soup("edge_on", n=n)["group"]
    size = np.bincount(g)[g]
    first = np.full(g.max() + 1, -1)
    first[g[::-1]] = np.arange(g.size)[::-1]
    hi = ts.soup_reference("edge_on", 1, n=n)[1].reshape(-1)
    w = hi[hi >= 0]
    assert (hi >= 0).mean() > 0.3 and (size[w] > 1).mean() >= 0.10 and np.array_equal(first[g[w]], w)


def test_hw1_other_index_rules_give_other_frames():
    """Taking the largest tied index instead changes the hit AOV on every soup: the comparisons of
    tests/test_gpu_ties.py can fail."""
    for kind in ts.SOUP_KINDS:
        g = ts.dup_soup(kind)["group"]
        last = np.full(g.max() + 1, -1)
        last[g] = np.arange(g.size)
        hi = ts.soup_reference(kind, 1)[1].reshape(-1)
        w = hi[hi >= 0]
        assert (last[g[w]] != w).mean() >= 0.10


# ---- the comparisons can fail -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "large"])
def test_other_rules_give_other_answers(name):
    """The brute-force minimum (with either index rule) is not the reference's answer: it differs on
    the rays whose t lies above that minimum, on the rays the oracle misses, and on most tied rays."""
    b, cl = ts.batch(name), ts.classes(name)
    differs_t = cl["min_t"].view(np.uint32) != b["t"].view(np.uint32)
    assert differs_t.sum() >= cl["above_min"].sum() + cl["miss_but_accepts"].sum() >= 5
    assert (differs_t[cl["above_min"]]).all() and differs_t[cl["miss_but_accepts"]].all()
    assert ((cl["min_idx"] != b["idx"]) & (cl["tied"] >= 2)).mean() > 0.3


def test_fixture_files_are_what_meta_says():
    for name in ts.FRAME_CASES:
        meta = golden_meta("ties_" + name)
        for a, k in zip(ts.fixture_frames(name), ("fb.f32", "hits.i32", "hitt.f32")):
            assert hashlib.sha256(a.tobytes()).hexdigest() == meta["sha256"][k], (name, k)
