"""Path stages for caller hits (rt_path_*, include/rt_mi355x.h), the part that needs no device: the
entry points exist, their argument checks answer before any HIP call, the step's arithmetic (host
build, rt_path_step_host) driven through a staged path on the CPU equals the oracle's
TraceRayIterative bit for bit, and the second material tables of tests/test_gpu_path_stages.py show
in the oracle's renders, so that no per-hit material test can pass by a table that changes nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import path_cases as pc
import ray_batches as rb
import shade_fuzz as sf
import shade_rays_cases as sc

import raytracinginonesemester_amd as rt
from raytracinginonesemester_amd import _lib as L

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_entry_points_exist():
    lib = L.lib()
    for name in ("rt_path_opts_default", "rt_path_begin_device", "rt_path_step_device", "rt_path_step_variant",
                 "rt_path_step_host", "rt_path_compact_scratch_bytes", "rt_path_compact_device", "rt_path_finish_device"):
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    for name in ("path_begin", "path_step", "path_step_variant", "trace_paths"):
        assert callable(getattr(rt.DeviceScene, name)), name
    assert callable(rt.compact_paths) and callable(rt.path_finish) and callable(rt.path_step_host)
    assert C.sizeof(L.PathOpts) == 20 and C.sizeof(L.PathStateT) == 24
    assert lib.rt_path_step_variant(None) == rt.RT_RAYS_VARIANT_NONE
    assert lib.rt_abi_version() == 3
    # a bit of its own: no RT_FLAG_* uses it
    assert L.RT_PATH_LAST & (L.RT_FLAG_NO_CULL | L.RT_FLAG_BINARY) == 0 and L.RT_PATH_LAST == 16
    o = L.PathOpts(7, L.Vec3(7, 7, 7), 7)
    lib.rt_path_opts_default(C.byref(o))
    assert (o.diffuse_bounce, tuple(o.miss_color), o.flags) == (1, (0.0, 0.0, 0.0), 0)
    lib.rt_path_opts_default(None)


# ---- argument checks ------------------------------------------------------------------------------
# A scene handle that is never read, and host buffers no call may write: every check answers first.
_FAKE_SCENE = C.create_string_buffer(64)
_BUF = np.zeros(4096, np.uint32)
_S, _P = C.addressof(_FAKE_SCENE), _BUF.ctypes.data
_P16 = _P + (-_P) % 16
_STATE = L.PathStateT(_P, _P, _P)
_ST = C.addressof(_STATE)
_STATE_NO_RNG = L.PathStateT(_P, _P, None)


def _opts(flags=0):
    o = L.PathOpts()
    L.lib().rt_path_opts_default(C.byref(o))
    o.flags = flags
    return o


_OPTS = {"ok": _opts(), "last": _opts(L.RT_PATH_LAST), "bin_last": _opts(L.RT_FLAG_BINARY | L.RT_PATH_LAST),
         "nocull": _opts(L.RT_FLAG_NO_CULL), "bit8": _opts(L.RT_FLAG_BINARY | 8), "bit32": _opts(32)}
_OP = {k: C.addressof(v) for k, v in _OPTS.items()}

# (scene, m, rays, hits, mats, ids, opt, state, next, alive, direct) -> code
STEP_CASES = {
    "null scene": ((None, 4, _P, _P16, None, None, _OP["ok"], _ST, _P, _P, None), -1),
    "null rays": ((_S, 4, None, _P16, None, None, _OP["ok"], _ST, _P, _P, None), -1),
    "null hits": ((_S, 4, _P, None, None, None, _OP["ok"], _ST, _P, _P, None), -1),
    "null opts": ((_S, 4, _P, _P16, None, None, None, _ST, _P, _P, None), -1),
    "null state": ((_S, 4, _P, _P16, None, None, _OP["ok"], None, _P, _P, None), -1),
    "null state member": ((_S, 4, _P, _P16, None, None, _OP["ok"], C.addressof(_STATE_NO_RNG), _P, _P, None), -1),
    "unknown flag": ((_S, 4, _P, _P16, None, None, _OP["nocull"], _ST, _P, _P, None), -1),
    "unknown flag beside BINARY": ((_S, 4, _P, _P16, None, None, _OP["bit8"], _ST, _P, _P, None), -1),
    "unknown flag 32": ((_S, 4, _P, _P16, None, None, _OP["bit32"], _ST, _P, _P, None), -1),
    "m = 2^31": ((_S, 1 << 31, _P, _P16, None, None, _OP["ok"], _ST, _P, _P, None), -7),
    "m = 2^40, last, no outputs": ((_S, 1 << 40, _P, _P16, _P, _P, _OP["bin_last"], _ST, None, None, None), -7),
    "hits not 16-byte aligned": ((_S, 4, _P, _P16 + 4, None, None, _OP["ok"], _ST, _P, _P, None), -1),
    "no next rays without LAST": ((_S, 4, _P, _P16, None, None, _OP["ok"], _ST, None, _P, None), -1),
    "no alive without LAST": ((_S, 4, _P, _P16, None, None, _OP["ok"], _ST, _P, None, None), -1),
}


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_step_argument_errors_need_no_device(case):
    args, code = STEP_CASES[case]
    rc = L.lib().rt_path_step_device(*args, None)
    assert rc == code, (case, rc, L.lib().rt_last_error())
    assert L.lib().rt_last_error()
    assert not _BUF.any()


def test_empty_batches_are_ok_without_a_device():
    lib = L.lib()
    assert lib.rt_path_step_device(_S, 0, _P, _P16, None, None, _OP["ok"], _ST, _P, _P, None, None) == 0
    assert lib.rt_path_step_device(_S, 0, _P, _P16, _P, _P, _OP["bin_last"], _ST, None, None, _P, None) == 0
    assert lib.rt_path_begin_device(0, 0, None, _ST, None) == 0
    assert lib.rt_path_finish_device(0, 0, _P, None) == 0
    assert lib.rt_path_step_host(0, _P, _P, None, None, None, 0, None, 0, None, _OP["ok"], _ST, _P, _P, None) == 0
    assert lib.rt_path_compact_scratch_bytes(0) == 0
    assert not _BUF.any()


def test_begin_finish_and_compact_check_their_arguments_first():
    lib = L.lib()
    assert lib.rt_path_begin_device(0, 4, None, None, None) == -1 and lib.rt_last_error()
    assert lib.rt_path_begin_device(0, 4, None, C.addressof(_STATE_NO_RNG), None) == -1
    assert lib.rt_path_begin_device(0, 1 << 31, None, _ST, None) == -7
    assert lib.rt_path_finish_device(0, 4, None, None) == -1 and lib.rt_last_error()
    assert lib.rt_path_finish_device(0, 1 << 31, _P, None) == -7
    m = 100
    a, ri, ii, ro, io, cnt, scr = (_P + o for o in (0, 256, 2656, 4096, 6496, 8192, 8256))
    ok = (0, m, a, ri, ii, ro, io, cnt, scr, None)

    def call(**kw):
        names = ("device", "m", "alive", "rays_in", "ids_in", "rays_out", "ids_out", "count", "scratch", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.rt_path_compact_device(*[args[k] for k in names])

    for k in ("alive", "rays_in", "rays_out", "ids_out", "count", "scratch"):
        assert call(**{k: None}) == -1, k
    assert call(m=1 << 31) == -7
    assert call(scratch=scr + 1) == -1
    # outputs that overlap inputs, by a whole array or by their last / first bytes
    assert call(rays_out=ri) == -1 and call(ids_out=ii) == -1
    assert call(rays_out=ri + 24 * m - 4) == -1 and call(rays_out=ri - 24 * m + 4) == -1
    assert call(ids_out=a + m - 1) == -1 and call(rays_out=a) == -1 and call(ids_out=ri) == -1
    assert call(count=ii) == -1 and call(scratch=a + 96) == -1
    assert not _BUF.any()


def test_compact_scratch_bytes():
    f = L.lib().rt_path_compact_scratch_bytes
    assert f(1) == 4 and f(2048) == 4 and f(2049) == 8 and f(65537) == 4 * 33 and f(1048577) == 4 * 513
    assert f(2048 * 2048) == 4 * 2048 and f(2048 * 2048 + 1) == 4 * (2049 + 2)
    assert f((1 << 31) - 1) == 4 * ((1 << 20) + 512) and f(1 << 31) == 0


# ---- the step's arithmetic: a staged path on the CPU is the oracle's TraceRayIterative ---------------
@pytest.mark.parametrize("diffuse", [True, False], ids=["diffuse", "mirror"])
@pytest.mark.parametrize("depth", sc.DEPTHS)
@pytest.mark.parametrize("name", sc.SCENES)
def test_cpu_staged_path_equals_the_reference(name, depth, diffuse):
    b = sc.caller_batch(name)
    scene = rb.scene_arrays(name)
    rad, (idx, t) = pc.cpu_staged_path(scene, b["rays"], b["seeds"], depth, diffuse, sc.MISS)
    want, widx, wt = sc.reference(name, depth, diffuse)
    assert np.array_equal(idx, widx) and np.array_equal(bits(t), bits(wt))
    bad = (bits(rad) != bits(want)).any(axis=1)
    assert not bad.any(), f"{name} depth {depth}: {int(bad.sum())} of {bad.size} rays differ, first {np.flatnonzero(bad)[:4]}"


def test_host_step_conventions():
    """What the GPU placement tests rely on, on the host build: a dead entry keeps its input ray,
    `direct` is what the step added from a fresh state, a miss adds the miss colour, an entry
    without a path touches nothing, and next_rays may be the rays themselves."""
    name = "cornell"
    b, scene = sc.caller_batch(name), rb.scene_arrays(name)
    rays = np.array(b["rays"])
    n = rays.shape[0]
    idx, _ = rb.oracle_trace(scene["P"], scene["nodes"], scene["aabbs"], scene["tris"], rays)
    rec = pc.records(scene, rays, idx)
    lights = np.ascontiguousarray(scene["lights"], rt.LIGHT_DTYPE)
    occ = pc.shadow_answers(scene, rec, lights)
    state = lambda: (np.zeros((n, 3), F), np.ones((n, 3), F), np.array(b["seeds"], np.uint32))  # noqa: E731
    rad, thr, rng = state()
    nxt, alive, direct = rt.path_step_host(rays, rec, rad, thr, rng, occ, lights, scene["mats"], miss_color=sc.MISS)
    hit = idx >= 0
    assert alive[hit].any() and not alive[~hit].any() and (~hit).any()
    dead = alive == 0
    assert np.array_equal(bits(nxt[dead]), bits(rays[dead])) and (bits(nxt[~dead]) != bits(rays[~dead])).any(axis=1).all()
    assert np.array_equal(rad[hit], direct[hit]) and not direct[~hit].any()
    assert np.array_equal(rad[~hit], np.broadcast_to(np.array(sc.MISS, F), rad[~hit].shape))
    assert np.array_equal(thr[~hit], np.ones_like(thr[~hit])) and np.array_equal(rng[~hit], b["seeds"][~hit])
    # RT_PATH_LAST: the same radiance, no draw, nothing alive
    rad2, thr2, rng2 = state()
    nxt2, alive2, direct2 = rt.path_step_host(rays, rec, rad2, thr2, rng2, occ, lights, scene["mats"], miss_color=sc.MISS, last=True)
    assert np.array_equal(bits(rad2), bits(rad)) and np.array_equal(bits(direct2), bits(direct)) and not alive2.any()
    assert np.array_equal(rng2, b["seeds"]) and (thr2 == 1).all() and np.array_equal(bits(nxt2), bits(rays))
    # shuffled entries with shuffled ids, every fourth entry without a path
    perm = np.random.default_rng(3).permutation(n)
    ids = perm.astype(np.uint32)
    ids[::4] = L.RT_PATH_NONE
    rad3, thr3, rng3 = state()
    nxt3, alive3, direct3 = rt.path_step_host(rays[perm], rec[perm], rad3, thr3, rng3, occ[perm], lights, scene["mats"], ids=ids,
                                              miss_color=sc.MISS)
    on = ids != L.RT_PATH_NONE
    assert np.array_equal(bits(nxt3[on]), bits(nxt[perm][on])) and np.array_equal(alive3[on], alive[perm][on])
    assert np.array_equal(bits(direct3[on]), bits(direct[perm][on]))
    assert np.array_equal(bits(nxt3[~on]), bits(rays[perm][~on])) and not alive3[~on].any() and not direct3[~on].any()
    used = np.zeros(n, bool)
    used[perm[on]] = True
    assert np.array_equal(bits(rad3[used]), bits(rad[used])) and np.array_equal(rng3[used], rng[used])
    assert not rad3[~used].any() and (thr3[~used] == 1).all() and np.array_equal(rng3[~used], b["seeds"][~used])


def test_finish_clamp_of_the_helper_keeps_nan_and_negative_zero():
    c = pc.clamp01(np.array([[np.nan, -0.0, 2.0], [-1.0, 0.5, 1.0]], F))
    assert np.isnan(c[0, 0]) and bits(c[0, 1]) == 0x80000000 and c[0, 2] == 1 and tuple(c[1]) == (0.0, 0.5, 1.0)


# ---- per-hit materials: the second tables show -------------------------------------------------------
@pytest.mark.parametrize("name", pc.TABLE_B_CHECKED)
def test_second_material_table_changes_the_frame(name):
    """From the oracle alone: the case rendered with table B differs from the case as shipped in at
    least 90 % of the pixels that hold a hit, and is finite."""
    assert set(pc.TABLE_B_CASES) <= set(pc.TABLE_B_CHECKED)
    c = sf.case(name)
    rgb_b, hi = pc.oracle_render_with_b(name)
    rgb_a = sf.oracle_render(c)
    assert np.isfinite(rgb_b).all()
    hit_px = (hi >= 0).any(axis=2)
    frac = float(((bits(rgb_a) != bits(rgb_b)).any(axis=2) & hit_px).sum()) / max(int(hit_px.sum()), 1)
    print(name, frac)
    assert hit_px.any() and frac >= 0.9, frac
    assert pc.table_b(name).shape == (c["mats"].size, 13) and not np.array_equal(pc.table_b(name), sf.mats13(c))


def test_neg_table_b_ends_paths():
    """s_l3_d4's table B keeps the 'neg' table's kd + kr <= 0 entry, and primary hits carry it."""
    b = pc.table_b("s_l3_d4")
    assert b[3, 3] + b[3, 9] <= 0
    _, hi = pc.oracle_render_with_b("s_l3_d4")
    assert (sf.primary_material(sf.case("s_l3_d4"), hi) == 3).any()


# ---- the C++ wrappers ---------------------------------------------------------------------------------
def test_cpp_wrappers(tmp_path):
    """rt::path_step_host of include/rt_mi355x.hpp (a stand-alone program linked against the library)
    gives the C entry's bits over two depths; the device wrappers refuse bad arguments as
    rt::Error; the header compiles without warnings."""
    import subprocess

    from conftest import REPO
    from raytracinginonesemester_amd import build as B

    exe = tmp_path / "path_hpp_main"
    subprocess.run([B.CXX, "-std=c++17", "-O1", *B.FP, "-Wall", "-Wextra", "-Werror", f"-I{REPO / 'include'}",
                    str(REPO / "tests" / "native" / "path_hpp_main.cpp"), "-o", str(exe), f"-L{L.LIB_PATH.parent}",
                    "-lrt_mi355x", f"-Wl,-rpath,{L.LIB_PATH.parent}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    d0, d1, refused = r.stdout.split("--\n")
    rays = np.array([[0, 0, 3, 0, 0, -1], [1, 0.5, 3, 0, 0, -1], [2, 0, 3, 0, 0.6, 0.8], [3, 0, 3, 1, 0, 0]], F)
    rec = np.zeros(4, rt.HIT_DTYPE)
    for k, (tri, p, n, mat) in enumerate([(5, (0, 0, 0), (0, 0, 2), 1), (9, (1, 0.5, 0), (0, 0.6, 0.8), 7),
                                          (-1, (0, 0, 0), (0, 0, 0), 0), (2, (3, 0, 0), (0, 0, 1), 0)]):
        rec[k] = (tri, -1.0 if tri < 0 else 1.0, 0, 0, p, n, n, 1, mat, mat)
    table = np.stack([rt.default_material(), rt.default_material()])
    table[1] = [0.25, 0.5, 0.75, 0.5, 0.04, 0.04, 0.04, 0.5, 7.3, 0.5, 0.0, 0.125, 0.0]
    lights = np.array([((1, 2, 4), (1, 0.9, 0.8), 2), ((-2, 1, 3), (0.3, 0.3, 1.0), 1)], rt.LIGHT_DTYPE)
    occ = np.array([[0, 1], [1, 0], [0, 0], [0, 0]], np.uint8)
    ids = np.array([2, 0, 1, L.RT_PATH_NONE], np.uint32)
    rad, thr, rng = np.zeros((3, 3), F), np.ones((3, 3), F), np.array([42, 7, 99], np.uint32)
    for depth, text in enumerate((d0, d1)):
        nxt, alive, direct = rt.path_step_host(rays, rec, rad, thr, rng, occ, lights, table, ids=ids,
                                               miss_color=(0.25, 0.5, 0.125), last=depth == 1)
        words = [[int(w, 16) for w in line.split()] for line in text.splitlines()]
        ent, st = np.array(words[:4], np.uint32), np.array(words[4:], np.uint32)
        assert ent.shape == (4, 10) and st.shape == (3, 7)
        assert np.array_equal(ent[:, :6], bits(nxt)) and np.array_equal(ent[:, 6], alive) and np.array_equal(ent[:, 7:], bits(direct))
        assert np.array_equal(st[:, :3], bits(rad)) and np.array_equal(st[:, 3:6], bits(thr)) and np.array_equal(st[:, 6], rng)
        if depth == 0:
            assert alive[0] == 1 and alive[2] == 0 and alive[3] == 0 and direct[0].any() and rad[2].any()
    assert refused.split() == ["-1", "-1", "-1", "-1"]
