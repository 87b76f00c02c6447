"""hw1_rect against the oracle, triangle by triangle, on the CPU (rt_hw1_rects_host: the host build
of the functions hw1_rect_count_kernel runs; tests/test_gpu_hw1_binning.py shows the device's
rectangles equal to these).

The binned HW1 path lists triangle k only in the tiles of its range.  It is exact if and only if
every sample at which ray_intersection accepts triangle k lies in a listed tile; a frame shows
that only where k would also have won.  Here the oracle renders each triangle alone, so every
accepted sample of every triangle is checked (containment), and the floors below keep the check
from passing by emptiness.  They are conditions on the generator's seeds (tests/hw1_cases.py), met
by the oracle alone.

Measured with the oracle (accepted samples; 120 triangles, 4 spp, the default table):

  case                          mixed    around    shell (404)
  96x72 base                    55,200   421,560   33,552
  97x71 base                    54,840   420,024   33,264
  97x71 4 mm                    11,764   410,316   13,592
  97x71 300 mm                  87,832   407,736   29,788
  97x71 axis look               34,844   422,196   16,748
  97x71 rolled                  54,600   413,360   33,472
  97x71 inside the soup         18,664   159,984   14,260
  97x71 far                     -        -         2,592
  97x71 scaled 2^-10            53,432   420,000   30,500
  97x71 scaled 2^12             54,784   419,276   33,288
  97x71 shifted 4096            54,840   420,036   33,404
  1x400 / 400x1                 3,820 / 104   25,000 / 20,388   1,884 / 820

  edge_on 0, slivers 4 and 0, tiny 60 and 48 at 96x72 and 97x71: those soups accept next to nothing
  by design and carry no floor.  The 40 random cameras: 706,784 over 80 triangles each.  The special
  soup: 587,020 and 584,716; the in-plane soup: 359,424 and 358,124.

Known cost cliff, recorded and not tested: at focal lengths up to about 13 mm, and for any image
one row high, every triangle is listed in every tile (list fill 1.000 in the 4 mm and 400x1 cases
above): the image's directions then span so wide a range that the half-planes' slack covers it.
The frames stay exact; the lists are as long as brute force's.  DESIGN.md §4.7.
"""
from __future__ import annotations

import numpy as np
import pytest

import hw1_cases as hc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import configs

MIXED_FLOOR, AROUND_FLOOR, RANDOM_FLOOR, SPECIAL_FLOOR = 10_000, 100_000, 300_000, 300_000
# The sum over triangles of the tiles in their range (the bin list's total) at the parent of the
# commit that added this test, by rt_hw1_rects_host, whose arithmetic that commit did not touch.
# A tighter hw1_rect lowers these; nothing may raise them.  They may only go down.
TIGHTNESS = {"c2": 69_373, "mixed": 900, "edge_on": 2349, "around": 2481, "slivers": 4253, "tiny": 237,
             "shell": 816}


def missed(c: dict, acc: np.ndarray, tiles: np.ndarray) -> list:
    """(triangle, its tile range, the accepted pixels outside it) for every triangle with one."""
    out = []
    for k in range(acc.shape[0]):
        ys, xs = np.nonzero(acc[k].any(axis=2))
        tx0, tx1, ty0, ty1 = (int(v) for v in tiles[k])
        ok = (xs // hc.TW >= tx0) & (xs // hc.TW <= tx1) & (ys // hc.TH >= ty0) & (ys // hc.TH <= ty1)
        if not ok.all():
            out.append((k, (tx0, tx1, ty0, ty1), list(zip(xs[~ok][:4].tolist(), ys[~ok][:4].tolist())), int((~ok).sum())))
    return out


def contained(c: dict) -> int:
    """Asserts containment for the case; returns the oracle's accepted-sample count."""
    assert hc.in_unit(c["jitter"])
    acc = hc.accepted(c)
    rects, tiles = rt.hw1_rects_host(c["positions"], c["indices"], c["camera"])
    bad = missed(c, acc, tiles)
    assert not bad, f"{c['name']}: accepted samples outside their triangle's tile range: {bad[:4]}"
    # the rectangle itself holds a position ix in {x, x + 1}, iy in {y, y + 1} of every accepted sample
    for k in range(acc.shape[0]):
        ys, xs = np.nonzero(acc[k].any(axis=2))
        if ys.size:
            assert rects[k, 0] <= xs.min() + 1 and xs.max() <= rects[k, 2], (c["name"], k)
            assert rects[k, 1] <= ys.min() + 1 and ys.max() <= rects[k, 3], (c["name"], k)
    return int(acc.sum())


@pytest.mark.parametrize("args", hc.FIXED_CASES, ids=lambda a: "-".join(str(v) for v in a))
def test_accepted_samples_lie_in_the_tile_range(args):
    c = hc.case(*args)
    total = contained(c)
    kind, W, H = args[:3]
    if W * H >= 96 * 71:  # the frames of at least 96x72x4 samples (97x71 has 55 pixels fewer)
        floor = {"mixed": MIXED_FLOOR, "around": AROUND_FLOOR}.get(kind)
        if floor is not None:
            assert total >= floor, (c["name"], total)


@pytest.mark.parametrize("kind", ["mixed", "around", "tiny"])
def test_corner_table_is_contained(kind):
    """{0, 0.99999994}^2: x + 0.99999994 rounds to x + 1 from x = 1 on, the ix = x + 1 the
    rectangles allow for."""
    c = hc.case(kind, 96, 72, jitter="corners")
    total = contained(c)
    assert total >= {"mixed": MIXED_FLOOR, "around": AROUND_FLOOR, "tiny": 1}[kind]


def test_random_cameras():
    total = 0
    for i in range(hc.N_RANDOM):
        total += contained(hc.random_camera_case(i))
    assert total >= RANDOM_FLOOR, total


@pytest.mark.parametrize("W,H", [(96, 72), (97, 71)])
@pytest.mark.parametrize("which", ["special", "inplane"])
def test_special_and_inplane_soups(which, W, H):
    total = contained(hc.soup_case(which, W, H))
    if which == "special":
        assert total >= SPECIAL_FLOOR, total
    else:
        assert total > 0


def test_out_of_range_tables_leave_the_rectangles():
    """Why rt_render_hw1_device sends such tables to the brute-force kernel: with
    ((-3.25, 1.5), (7, -3.25), (1.5, 7)) accepted samples fall outside their triangle's tiles."""
    for kind in ("mixed", "around", "tiny"):
        c = hc.case(kind, 96, 72, jitter="wild")
        assert not hc.in_unit(c["jitter"])
        _, tiles = rt.hw1_rects_host(c["positions"], c["indices"], c["camera"])
        assert missed(c, hc.accepted(c), tiles), kind
    for name, inside in (("default", True), ("corners", True), ("centred", False), ("wild", False), ("three", False)):
        assert hc.in_unit(hc.jitter_table(name, hc.JITTER[name])) == inside, name


def test_case_contents():
    """What the generators produce, pinned: kinds, counts, the special soup's rows."""
    assert hc.KINDS == ("mixed", "edge_on", "around", "slivers", "tiny", "shell")
    assert len(hc.FIXED_CASES) == 12 + 5 * 3 + 1 + 3 * 3 + 2 * 3 and len(set(hc.FIXED_CASES)) == len(hc.FIXED_CASES)
    assert {a[3] for a in hc.FIXED_CASES} == set(hc.CAMERAS) and {a[4] for a in hc.FIXED_CASES} == set(hc.XFORMS)
    for kind in hc.SOUP_KINDS:
        s = hc.soup(kind)
        assert s["positions"].shape == (3 * hc.N_SOUP, 3) and s["positions"].dtype == np.float32
        assert np.array_equal(s["indices"].reshape(-1), np.arange(3 * hc.N_SOUP))
        assert np.isfinite(s["positions"]).all() and np.isfinite(s["normals"]).all()
        assert s["positions"].tobytes() == hc.case(kind, 97, 71)["positions"].tobytes()
    tiny = hc.soup("tiny")["positions"].reshape(-1, 3, 3)
    assert np.abs(tiny - tiny.mean(axis=1, keepdims=True)).max() < 0.06
    sh = hc.soup("shell")["positions"].reshape(-1, 3, 3).astype(np.float64)
    assert sh.shape[0] == hc.N_SHELL + hc.N_AROUND == 404
    dist = np.linalg.norm(sh[:hc.N_SHELL].mean(axis=1) - np.array(hc.BASE_POS), axis=1)
    assert 1.5 < dist.min() and dist.max() < 6.5
    assert hc.soup("shell", cam_key="far")["positions"].tobytes() != hc.soup("shell")["positions"].tobytes()
    # scaled and shifted scenes: the same triangles, transformed in double and rounded once
    base = hc.case("mixed", 97, 71)["positions"]
    assert np.array_equal(hc.case("mixed", 97, 71, xform="large")["positions"], base * np.float32(4096.0))
    assert np.array_equal(hc.case("mixed", 97, 71, xform="small")["positions"], base * np.float32(2.0 ** -10))
    assert np.array_equal(hc.case("mixed", 97, 71, xform="shifted")["positions"], (base.astype(np.float64) + 4096.0).astype(np.float32))
    # the special soup's rows
    sp = hc.special_soup()["positions"].reshape(60, 3, 3)
    centre = hc.camera("base", 96, 72).basis()["center"]
    rows = hc.SPECIAL_ROWS
    assert [rows[k] for k in rows] == [(0, 20), (20, 30), (30, 40), (40, 45), (45, 50), (50, 55), (55, 60)]
    assert (sp[0:20, 0] == centre).all() and not (sp[20:, 0] == centre).all(axis=1).any()
    e1, e2 = (sp[20:30, j].astype(np.float64) - sp[20:30, 0] for j in (1, 2))
    area = np.linalg.norm(np.cross(e1, e2), axis=1)
    assert (area[:6] == 0).all() and (area[6:] < 1e-5 * np.linalg.norm(e1, axis=1)[6:] * np.linalg.norm(e2, axis=1)[6:]).all()
    assert np.abs(sp[30:40]).max() > 1e12 and np.isfinite(sp[:40]).all()
    for (a, b), test in ((rows["two_100"], lambda r: (r == np.float32(2.0 ** 100))), (rows["nan"], np.isnan),
                         (rows["inf"], np.isposinf), (rows["near_max"], lambda r: (r == np.float32(3e38)))):
        assert (test(sp[a:b]).reshape(b - a, -1).sum(axis=1) == 1).all()
    ip = hc.inplane_soup()["positions"]
    assert ip.shape == (180, 3) and (ip[:, 2] == centre[2]).all()
    # the column scene: 512 triangles, every one some tiles tall at the tallest frame
    col = hc.column_case(1, 131073)
    assert col["indices"].shape == (hc.N_COLUMN, 3) and col["spp"] == 2 and np.isfinite(col["positions"]).all()
    assert [hc.ntiles(W, H) for W, H in hc.THRESHOLD_SHAPES] == [5120, 5121, 8192, 8193, 32768, 32769, 2 * 2561]
    # the random cameras: every frame width and height class, a one-row and a narrow frame among them
    shapes = [(c["camera"].pixel_width, c["camera"].pixel_height) for c in map(hc.random_camera_case, range(hc.N_RANDOM))]
    assert all(1 <= W <= 129 and 1 <= H <= 59 for W, H in shapes)
    assert any(H == 1 for _, H in shapes) and any(W < 16 for W, _ in shapes) and any(W % 16 and H % 4 for W, H in shapes)
    assert all(hc.random_camera_case(i)["indices"].shape[0] == hc.N_RANDOM_TRIS for i in range(hc.N_RANDOM))


def test_empty_and_whole_image_ranges():
    """The two ends of the host entry's answer: a triangle behind the camera has the empty range
    (0, -1, 0, -1) and an empty rectangle; one with a NaN vertex has the whole image."""
    cam = hc.camera("base", 97, 71)
    behind = np.array([[0.3, -6.0, 0.7], [0.5, -6.0, 0.7], [0.3, -6.0, 0.9]], np.float32)
    nan = behind.copy()
    nan[1, 1] = np.nan
    pos = np.concatenate([behind, nan])
    rects, tiles = rt.hw1_rects_host(pos, np.arange(6, dtype=np.uint32).reshape(2, 3), cam)
    assert tuple(tiles[0]) == (0, -1, 0, -1) and (rects[0, 0] > rects[0, 2] or rects[0, 1] > rects[0, 3])
    assert tuple(rects[1]) == (-2, -2, 98, 72) and tuple(tiles[1]) == (0, 6, 0, 17)
    assert hc.range_area(tiles) == 7 * 18
    with pytest.raises(rt.RTError):
        rt._lib.check(rt._lib.lib().rt_hw1_rects_host(None, None, None, 0, None, None))
    with pytest.raises(rt.RTError):  # (a null scene: refused before any HIP call)
        rt._lib.check(rt._lib.lib().rt_hw1_debug_bins(None, None, None, None, 0, None, 0))


def c2_tiles():
    c = configs.HW1_CONFIGS["c2"]
    mesh = rt.MeshHW1(configs.MESHES / c["mesh"])
    cam = rt.Camera(c["position"], c["look_at"], c["up"], c["focal_mm"], c["sensor_mm"], c["width"], c["height"], hw1=True)
    return rt.hw1_rects_host(mesh.positions, mesh.indices, cam)[1]


@pytest.mark.parametrize("name", list(TIGHTNESS))
def test_tightness_is_pinned(name):
    """An hw1_rect that returned the whole image would pass every parity test; the list total it
    leads to is pinned.  It may only go down."""
    if name == "c2":
        tiles = c2_tiles()
    else:
        c = hc.case(name, 96, 72)
        tiles = rt.hw1_rects_host(c["positions"], c["indices"], c["camera"])[1]
    assert hc.range_area(tiles) == TIGHTNESS[name]
