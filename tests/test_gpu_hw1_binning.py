"""The HW1 binning on the device (csrc/rt_hw1.hip: hw1_rect_count_kernel -> scan -> hw1_fill_kernel
-> render_hw1_chunks_kernel) on the cases of tests/hw1_cases.py.

The reference is the oracle (orc.render_hw1) and everything is bit for bit: "the oracle's frame"
means hit index, t bits, float pixel bits and P6 bytes.  tests/test_hw1_rects_host.py shows on the
CPU that the host build of hw1_rect holds every sample the oracle accepts, triangle by triangle;
here the device's rectangles are shown equal to the host's, the lists equal to the rectangles, and
the frames equal to the oracle's at the shapes where the passes take other paths: partial tiles,
one-pixel-wide and -high images, the tile counts on either side of each scan form's limit.

Measured on an MI355X (the oracle's figures; thresholds in the tests):
  odd shapes, 97x71x3 of shell + 4 around: hit share 0.884, 22 distinct winners
  column scene, 2 spp:  H      tiles   hit share  winners  list total (capacity 65,536)
                        20480   5120   0.918      316      13,312
                        20481   5121   0.918      318      13,315
                        32768   8192   0.900      317      19,389
                        32769   8193   0.900      317      19,400
                        131072  32768  0.846      340      62,675
                        131073  32769  0.846      339      62,669
                        17x10244 5122  0.938      313      15,788
Caller tables outside [0,1), before they took the brute-force kernel: test_caller_jitter_tables.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest
import torch

import hw1_cases as hc
from test_hw1_rects_host import TIGHTNESS

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import configs

pytestmark = pytest.mark.gpu

BINNED = {0: "render_hw1_chunks_kernel<false>", 1: "render_hw1_chunks_kernel<false>",
          2: "render_hw1_chunks_kernel<true>", 3: "render_hw1_chunks_kernel<true>"}
BRUTE = "render_hw1_kernel"


def bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def scene_of(c) -> rt.HW1Scene:
    return rt.HW1Scene(c["positions"], c["normals"], c["indices"])


def frame(hs, c, brute=False):
    """One rt_render_hw1_device frame of the case: (rgb, p6, hit index, t), flat."""
    cam, spp = c["camera"], c["spp"]
    n = cam.pixel_width * cam.pixel_height
    rgb = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    p6 = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
    hi = torch.zeros(n * spp, dtype=torch.int32, device="cuda")
    ht = torch.zeros(n * spp, dtype=torch.float32, device="cuda")
    hs.render_device(cam, *hc.LIGHT, spp, rgb_ptr=rgb.data_ptr(), p6_ptr=p6.data_ptr(), hit_idx_ptr=hi.data_ptr(),
                     hit_t_ptr=ht.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, jitter=c["jitter"],
                     brute=brute)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), p6.cpu().numpy(), hi.cpu().numpy(), ht.cpu().numpy()


@lru_cache(maxsize=None)
def ref_case(*args, **kw):
    return hc.reference(hc.case(*args, **kw))


@lru_cache(maxsize=None)
def ref_column(W, H):
    return hc.reference(hc.column_case(W, H))


def check_frame(c, got, ref, what="", p6_too=True):
    """got is the oracle's frame."""
    rgb, p6, hi, ht = got
    r_rgb, r_hi, r_ht = ref
    cam, spp = c["camera"], c["spp"]
    bad = np.flatnonzero(hi.reshape(-1) != r_hi.reshape(-1))
    if bad.size:
        px = bad // spp
        lost = np.unique(r_hi.reshape(-1)[bad])
        raise AssertionError(
            f"{c['name']} {what}: {bad.size} of {hi.size} samples have another winner, in {np.unique(px).size} pixels "
            f"(x {int((px % cam.pixel_width).min())}..{int((px % cam.pixel_width).max())}, "
            f"y {int((px // cam.pixel_width).min())}..{int((px // cam.pixel_width).max())}); the oracle's winners there: "
            f"{lost[:12].tolist()} ({lost.size} triangles); got {hi.reshape(-1)[bad[:8]].tolist()} for "
            f"{r_hi.reshape(-1)[bad[:8]].tolist()}")
    assert np.array_equal(bits(ht), bits(r_ht)), (c["name"], what, "t")
    assert np.array_equal(bits(rgb), bits(r_rgb)), (c["name"], what, "pixels")
    if p6_too and p6 is not None:
        body = rt.encode_p6(r_rgb)[len(rt.p6_header(cam.pixel_width, cam.pixel_height)):]
        assert np.asarray(p6).tobytes() == body, (c["name"], what, "P6")


def check_bins(hs, c, what=""):
    """The latest frame's binning state against the host build: the device's rectangles are the
    host's, each tile's list (as a sorted set) is the set of triangles whose range holds the tile,
    and the totals agree.  Returns the list total."""
    cam = c["camera"]
    W, H = cam.pixel_width, cam.pixel_height
    rects, tiles = rt.hw1_rects_host(c["positions"], c["indices"], cam)
    b = hs.bins()
    diff = np.flatnonzero((b["rects"] != rects).any(axis=1))
    assert diff.size == 0, (c["name"], what, "device rectangles differ from the host's", diff[:8].tolist(),
                            b["rects"][diff[:4]].tolist(), rects[diff[:4]].tolist())
    sets = hc.tile_sets(tiles, W, H)
    total = hc.range_area(tiles)
    off = b["offsets"].astype(np.int64)
    assert off.size == hc.ntiles(W, H) + 1 and off[0] == 0
    assert np.array_equal(np.diff(off), np.array([len(s) for s in sets], np.int64)), (c["name"], what, "tile counts")
    assert int(off[-1]) == hs.list_info()[1] == b["total"] == total, (c["name"], what, int(off[-1]), hs.list_info(), total)
    assert b["complete"] and b["list"].size == total, (c["name"], what, "the list outgrew its capacity")
    lst = b["list"].astype(np.int64)
    for t, s in enumerate(sets):
        got = np.sort(lst[off[t]:off[t + 1]])
        assert np.array_equal(got, np.array(s, np.int64)), (c["name"], what, "tile", t, got[:8].tolist(), s[:8])
    return total


def all_rect_cases():
    for a in hc.FIXED_CASES:
        yield hc.case(*a)
    for i in range(hc.N_RANDOM):
        yield hc.random_camera_case(i)
    for which in ("special", "inplane"):
        for W, H in ((96, 72), (97, 71)):
            yield hc.soup_case(which, W, H)


@pytest.mark.parametrize("fuse", [0, 3])
def test_device_rectangles_and_lists_are_the_hosts(fuse, tune):
    """Every case of tests/test_hw1_rects_host.py: the read-back of one frame equals the host
    entry, rectangle for rectangle, and every tile's list is what the rectangles say."""
    tune(hw1_fuse=fuse)
    for c in all_rect_cases():
        hs = scene_of(c)
        try:
            frame(hs, c)
            assert hs.kernel_name() == BINNED[fuse]
            check_bins(hs, c, f"fuse {fuse}")
        finally:
            hs.close()


@pytest.mark.parametrize("chunk", [16, 32])
@pytest.mark.parametrize("fuse", [0, 3])
def test_odd_frame_shapes(fuse, chunk, tune):
    """Partial tiles, one tile, one pixel, one row, one column: shell + 4 around, 1 and 3 samples, two
    frames in a row on the same buffers, one scene walking the shapes (its buffers laid out anew
    at every change)."""
    tune(hw1_fuse=fuse, hw1_chunk=chunk)
    _, r_hi, _ = ref_case("shell", 97, 71, spp=3)
    share, winners = float((r_hi >= 0).mean()), np.unique(r_hi[r_hi >= 0]).size
    print(f"97x71x3: hit share {share:.3f}, {winners} distinct winners")
    assert share >= 0.5 and winners >= 20
    hs = scene_of(hc.case("shell", 97, 71, spp=3))
    try:
        for W, H in hc.ODD_SHAPES:
            for spp in (1, 3):
                c = hc.case("shell", W, H, spp=spp)
                for k in range(2):
                    check_frame(c, frame(hs, c), ref_case("shell", W, H, spp=spp), f"fuse {fuse} chunk {chunk} frame {k}")
                assert hs.kernel_name() == BINNED[fuse]
            check_bins(hs, c, f"fuse {fuse} chunk {chunk}")
    finally:
        hs.close()


@pytest.mark.parametrize("fuse", [2, 3])
@pytest.mark.parametrize("W,H", hc.THRESHOLD_SHAPES, ids=lambda v: str(v))
def test_tile_count_thresholds(W, H, fuse, tune):
    """The column scene in frames of 5120 / 5121, 8192 / 8193 and 32768 / 32769 tiles, one on either
    side of each scan form's limit (the fused wave scan with bit 0 of hw1_fuse, then 8, 32 and any
    number of tiles per thread), and 17 x 10244: two tile columns, the second one pixel wide."""
    tune(hw1_fuse=fuse)
    c = hc.column_case(W, H)
    ref = ref_column(W, H)
    share, winners = float((ref[1] >= 0).mean()), np.unique(ref[1][ref[1] >= 0]).size
    print(f"{W}x{H}: {hc.ntiles(W, H)} tiles, hit share {share:.3f}, {winners} distinct winners")
    assert share >= 0.5 and winners >= 100
    hs = scene_of(c)
    try:
        cap0 = hs.list_info()[0]
        for k in range(2):
            check_frame(c, frame(hs, c), ref, f"fuse {fuse} frame {k}")
            cap, total = hs.list_info()
            print(f"  frame {k}: list total {total} of {cap}")
            assert cap == cap0 and 0 < total < cap0
            assert hs.kernel_name() == BINNED[fuse]
        check_bins(hs, c, f"fuse {fuse}")
    finally:
        hs.close()


def test_cameras_and_magnitudes():
    """Every camera, scale and shift, 97x71x2 of the shell about that camera's axis + 4 around."""
    for cam, xf in [(k, "none") for k in hc.CAMERAS] + [("base", x) for x in hc.XFORMS if x != "none"]:
        c = hc.case("shell", 97, 71, cam, xf, spp=2)
        hs = scene_of(c)
        try:
            check_frame(c, frame(hs, c), ref_case("shell", 97, 71, cam, xf, spp=2))
            assert hs.kernel_name() == BINNED[2]
        finally:
            hs.close()


@pytest.mark.parametrize("W,H", [(96, 72), (97, 71)])
@pytest.mark.parametrize("which", ["special", "inplane"])
def test_special_and_inplane_soups(which, W, H):
    """A vertex at the camera centre, degenerate, huge, NaN and inf triangles; the camera in every
    triangle's plane: binned and brute force agree in every byte, hit index and t are the oracle's,
    and so are the pixels (a NaN pixel compared as a position, not by its payload)."""
    c = hc.soup_case(which, W, H)
    r_rgb, r_hi, r_ht = hc.reference(c)
    hs = scene_of(c)
    try:
        a = frame(hs, c)
        assert hs.kernel_name() == BINNED[2]
        b = frame(hs, c, brute=True)
        assert hs.kernel_name() == BRUTE
    finally:
        hs.close()
    for x, y, what in zip(a, b, ("pixels", "P6", "hit index", "t")):
        assert x.tobytes() == y.tobytes(), (c["name"], what, "binned against brute force")
    rgb, _p6, hi, ht = a
    assert np.array_equal(hi, r_hi.reshape(-1)) and np.array_equal(bits(ht), bits(r_ht))
    nan = np.isnan(r_rgb.reshape(-1))
    assert np.array_equal(np.isnan(rgb), nan)
    assert np.array_equal(bits(rgb)[~nan], bits(r_rgb)[~nan])


@pytest.mark.parametrize("table", list(hc.JITTER))
def test_caller_jitter_tables(table):
    """Every table through HW1Scene.render_device and rt.render_hw1 gives the oracle's frame with
    that table.  hw1_rect assumes ix = (int)(x + j) in {x, x + 1}: a table with an entry outside [0,1)
    takes the brute-force kernel, and the next default-table frame of the scene is the binned one's
    again.

    Before that rule (rt_hw1.hip of the parent commit on an MI355X), the mixed soup of 120 triangles
    at 96x72, samples whose winner was not the oracle's:
      ((-3.25, 1.5), (7, -3.25), (1.5, 7)): 97 of 20,736, in 97 pixels (x 11..95, y 10..60), hits of
        9 triangles (13, 16, 30, 34, 44, 55, 70, 110, 113) given to the triangle behind them;
      ((3, 3),): 2 of 6,912, pixels (94, 71) and (95, 71), triangle 27's hits given to 15.
    The centred table lost nothing there (it is outside [0,1) too and takes the exact path now)."""
    spp = hc.JITTER[table]
    inside = hc.in_unit(hc.jitter_table(table, spp))
    for kind in ("mixed", "around", "tiny"):
        c = hc.case(kind, 96, 72, jitter=table)
        ref = ref_case(kind, 96, 72, jitter=table)
        hs = scene_of(c)
        try:
            check_frame(c, frame(hs, c), ref, "render_device")
            assert hs.kernel_name() == (BINNED[2] if inside else BRUTE), (table, hs.kernel_name())
            d = hc.case(kind, 96, 72)
            check_frame(d, frame(hs, d), ref_case(kind, 96, 72), "the default table after it")
            assert hs.kernel_name() == BINNED[2]
        finally:
            hs.close()
        rgb, hi, ht = rt.render_hw1(c["positions"], c["normals"], c["indices"], c["camera"], *hc.LIGHT, spp=spp,
                                    jitter=c["jitter"], aov=True)
        check_frame(c, (rgb, None, hi, ht), ref, "rt.render_hw1")


@pytest.mark.parametrize("name", list(TIGHTNESS))
def test_list_totals_are_the_pinned_ones(name):
    """list_info()'s total of one frame: the integers tests/test_hw1_rects_host.py pins."""
    if name == "c2":
        cfg = configs.HW1_CONFIGS["c2"]
        mesh = rt.MeshHW1(configs.MESHES / cfg["mesh"])
        cam = rt.Camera(cfg["position"], cfg["look_at"], cfg["up"], cfg["focal_mm"], cfg["sensor_mm"], cfg["width"],
                        cfg["height"], hw1=True)
        c = {"positions": mesh.positions, "normals": mesh.normals, "indices": mesh.indices, "camera": cam, "spp": 1,
             "jitter": None, "name": "c2"}
    else:
        c = hc.case(name, 96, 72)
    hs = scene_of(c)
    try:
        frame(hs, c)
        assert hs.list_info()[1] == TIGHTNESS[name]
    finally:
        hs.close()
