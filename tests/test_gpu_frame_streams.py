"""Frame streams (RT_TUNE_FRAME_STREAMS): an rt_renderer single frame's gate wait,
cull, cut and render kernel on one of two streams of the scene, alternating by frame.

The schedule orders work and computes nothing, so the oracle is the same renderer with the knob
at 0 (the prep-stream schedule, which the rest of the suite pins to the reference's goldens):
every delivered frame is byte-equal to it.  One full-size c3 frame is also held against
tests/golden/scenes/c3_full.

Frog at 16 spp has 4x4-pixel tiles: 256x144 is 2,304 tiles = 9,216 wave items, just more than the
7,168 first items of the persistent grid (the queues hand out items, the gate item is a dequeued
one); 64x36 is 144 tiles (no wave dequeues, and the gate must still open).
"""
from __future__ import annotations

import ctypes as C
import gzip
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN, host_scene

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib

SPP = 16
BIG, SMALL = (256, 144), (64, 36)


def _cams(hs, wh):
    """Two cameras, the second moved by (4, 0, 3) mm."""
    base = hs.camera(*wh)
    return [base, rt.Camera(tuple(np.add(base.pos, (0.004, 0.0, 0.003))), base.look_at, base.up,
                            base.focal_length_mm, base.sensor_height_mm, *wh)]


def _opts(hs, spp=SPP, max_depth=1):
    return rt.DeviceScene.make_opts(spp=spp, max_depth=max_depth, miss_color=hs.settings["miss_color"],
                                    diffuse_bounce=hs.settings.get("diffuse_bounce", True))[0]


def _frame(r, t):
    addr, n = r.wait(t)
    return bytes((C.c_uint8 * n).from_address(addr))


def _singles(r, cams, o):
    """Each camera's frame, rendered alone with the knob at 0."""
    rt.set_tuning("frame_streams", 0)
    return [_frame(r, r.submit(c, o)) for c in cams]


def _pipelined(r, cams, o, order, depth):
    """Frames of cams[order[i]] kept `depth` in flight: [(camera index, delivered bytes)]."""
    pend, got = [], []
    for k in order:
        pend.append((k, r.submit(cams[k], o)))
        if len(pend) >= depth:
            kk, t = pend.pop(0)
            got.append((kk, _frame(r, t)))
    got += [(kk, _frame(r, t)) for kk, t in pend]
    return got


def _check(got, want, what=""):
    assert len(got) > 0
    for i, (kk, b) in enumerate(got):
        assert b == want[kk], f"{what} frame {i} (camera {kk}) differs from the knob-0 frame"


ORDER = [0, 1, 1, 0, 1, 0, 0, 1, 0, 1]


def test_knob_is_listed_round_trips_and_resets():
    """Host only: RT_TUNE_FRAME_STREAMS is in _lib.TUNE under the header's id, a value set is read
    back, and a reset restores the default."""
    assert _lib.TUNE["frame_streams"] == 25
    rt.reset_tuning()
    try:
        assert rt.get_tuning("frame_streams") is None
        for v in (0.0, 1.0):
            rt.set_tuning("frame_streams", v)
            assert rt.get_tuning("frame_streams") == v
        rt.set_tuning("frame_streams", None)
        assert rt.get_tuning("frame_streams") is None
        rt.set_tuning("frame_streams", 0)
    finally:
        rt.reset_tuning()
    assert rt.get_tuning("frame_streams") is None


@pytest.mark.gpu
@pytest.mark.parametrize("wh", [BIG, SMALL])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_pipelined_frames_equal_the_prep_stream_schedule(wh, depth, tune):
    """Depth 1, 2, 3; P6 and float delivery; two alternating cameras: every delivered frame is the
    knob-0 frame of its camera."""
    hs = host_scene("frog.json")
    cams, o = _cams(hs, wh), _opts(hs)
    for deliver in (rt.RT_DELIVER_P6, rt.RT_DELIVER_F32):
        r = rt.Renderer.from_host(hs, devices=(0,), depth=depth, deliver=deliver)
        try:
            want = _singles(r, cams, o)
            assert want[0] != want[1]
            tune(frame_streams=1)
            _check(_pipelined(r, cams, o, ORDER, depth), want, f"deliver {deliver}")
        finally:
            r.close()


@pytest.mark.gpu
def test_full_size_frame_is_the_reference_frame(tune):
    """c3 (1920x1080x16) on the frame streams, three frames in flight: the reference's own P6."""
    hs = host_scene("frog.json")
    ppm = gzip.open(GOLDEN / "scenes" / "c3_full" / "image.ppm.gz").read()
    tune(frame_streams=1)
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        cam, o = hs.camera(1920, 1080), _opts(hs)
        ts = [r.submit(cam, o) for _ in range(3)]
        for t in ts:
            assert _frame(r, t) == ppm[17:]
    finally:
        r.close()


def _long_run(frames: int) -> int:
    """The child process of the long gate run: its exit status is the number of wrong frames."""
    hs = host_scene("frog.json")
    cams, o = _cams(hs, BIG), _opts(hs)
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        want = _singles(r, cams, o)
        rt.set_tuning("frame_streams", 1)
        rt.set_tuning("prepass_gate", 0.5)
        got = _pipelined(r, cams, o, [(k * 7 // 3) & 1 for k in range(frames)], 3)
        bad = sum(b != want[kk] for kk, b in got) + abs(len(got) - frames)
    finally:
        r.close()
    print(f"long run: {len(got)} frames, {bad} wrong", flush=True)
    return min(bad, 100)


@pytest.mark.gpu
def test_long_gate_run_every_frame():
    """400 frames at depth 3 with the gate on (0.5) and the frame streams on, every frame compared.
    A gate word overwritten by the wrong kernel would stall a frame stream for good, so the run
    has a process of its own and a wall-clock bound: a stall fails the test."""
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "400"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "long run: 400 frames, 0 wrong" in p.stdout


@pytest.mark.gpu
def test_resize_and_knob_flip_mid_run(tune):
    """256x144 -> 64x36 -> 256x144 on the frame streams (a new list layout: the serialising path),
    then the knob flipped between the frames of one renderer, nothing waited for in between."""
    hs = host_scene("frog.json")
    o = _opts(hs)
    cams = {wh: _cams(hs, wh) for wh in (BIG, SMALL)}
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        want = {}
        for wh in (BIG, SMALL, BIG):
            want[wh] = _singles(r, cams[wh], o)
        tune(frame_streams=1)
        for wh in (BIG, SMALL, BIG):
            _check(_pipelined(r, cams[wh], o, [0, 1, 0, 1], 3), want[wh], f"{wh}")
        pend = []
        for i, knob in enumerate([1, 1, 0, 0, 1, 0, 1, 1]):
            tune(frame_streams=knob)
            pend.append((i & 1, r.submit(cams[BIG][i & 1], o)))
            if len(pend) >= 3:
                kk, t = pend.pop(0)
                assert _frame(r, t) == want[BIG][kk], f"frame {i - 2} around a knob flip"
        for kk, t in pend:
            assert _frame(r, t) == want[BIG][kk]
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("scene,wh,spp,max_depth", [("frog.json", SMALL, SPP, 8), ("heightfield_c5.json", (384, 216), 4, 1)])
def test_other_kernels_on_the_frame_streams(scene, wh, spp, max_depth, tune):
    """The bounce kernels (max_depth 8) and the big-scene kernel (the c5 heightfield at its fixture's
    size): three pipelined frames, knob 1 against knob 0."""
    hs = host_scene(scene)
    cams, o = _cams(hs, wh), _opts(hs, spp=spp, max_depth=max_depth)
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        want = _singles(r, cams, o)
        tune(frame_streams=1)
        _check(_pipelined(r, cams, o, [0, 1, 0], 3), want)
    finally:
        r.close()


@pytest.mark.gpu
def test_rejected_frame_arms_no_gate_wait(tune):
    """A frame refused before its launch (spp 0: RT_ERR_ARG) between two good frames: the next
    frame waits for no gate that nobody opens, and delivers."""
    hs = host_scene("frog.json")
    cams, o = _cams(hs, BIG), _opts(hs)
    bad = _opts(hs)
    bad.spp = 0
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        want = _singles(r, cams, o)
        tune(frame_streams=1)
        t0 = r.submit(cams[0], o)
        with pytest.raises(rt.RTError) as e:
            r.submit(cams[1], bad)
        assert e.value.code == -1
        t1 = r.submit(cams[1], o)
        t2 = r.submit(cams[0], o)
        assert [_frame(r, t) for t in (t0, t1, t2)] == [want[0], want[1], want[0]]
    finally:
        r.close()


@pytest.mark.gpu
def test_times_after_pipelined_frames(tune):
    """After 12 pipelined frames on the frame streams the scene's time readers return the timed
    frames' values and the renderer's frame latency covers its delivery."""
    hs = host_scene("frog.json")
    cams, o = _cams(hs, BIG), _opts(hs)
    tune(frame_streams=1)
    r = rt.Renderer.from_host(hs, devices=(0,), depth=3, deliver=rt.RT_DELIVER_P6)
    try:
        assert len(_pipelined(r, cams, o, [k & 1 for k in range(12)], 3)) == 12
        sc = r.scene(0)
        for name in ("kernel_times", "prepass_times", "frame_times"):
            v = getattr(sc, name)(8)
            assert 0 < len(v) <= 8 and np.all(np.isfinite(v)) and np.all(v > 0), (name, v)
        f, d = r.times(rt.RT_TIME_FRAME, 8), r.times(rt.RT_TIME_DELIVER, 8)
        assert len(f) == 8 and len(d) == 8 and np.all(f >= d), (f, d)
    finally:
        r.close()


if __name__ == "__main__":
    sys.exit(_long_run(int(sys.argv[1])))
