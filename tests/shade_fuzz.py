"""Shading fuzz cases: random material tables, object ids and light sets (TEST DATA GENERATOR).

The four shading copies of csrc/rt_shade.hpp (shade_d1, paired_bounces_resume, paired_bounces,
the generic depth loop) otherwise only ever see the shipped scenes' tables: a few materials
constant over whole objects, one light (cornell two), ids in range.  The cases here give them
1/5/7-entry, "negative" and empty tables, a random id per triangle (neighbouring lanes differ, a
tenth of the ids outside the table) and 0/1/2/3/5/8 lights with intensities 0 and -1 among them,
over two bases:

* ``sphere``: sphere.json's own arrays (host_scene) and its shipped camera at 64x36;
* ``chain``: chain_bvh.chain_scene(600)'s tree (the MODE_DEEP kernels, the reference's stack
  overflow and brute-force completion) over other triangles, see chain_rings.

Everything is drawn from splitmix64 (no dependence on numpy's generators), in float32.
tests/golden/gen_golden.py gen_shade sends a case through the reference's render() (ref_g
arrays, miss colour 0); tests/test_shade_fuzz.py pins the generator and the oracle to those
fixtures, tests/test_gpu_shade_fuzz.py the GPU.  No NaN or infinite inputs.
"""
from __future__ import annotations

import hashlib
import sys
from functools import lru_cache
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
if str(GOLDEN) not in sys.path:
    sys.path.insert(0, str(GOLDEN))
import chain_bvh  # noqa: E402
from chain_bvh import LIGHT, MAT  # noqa: E402

INT_MAX, INT_MIN = 2**31 - 1, -(2**31)
U = "U"  # a uniform draw among a field's edge values
KD = (0.0, 0.25, 1.0, U)
KS = (0.0, 0.5, 1.0, U)
SHININESS = (0.0, 0.5, 1.0, 7.3, 32.0, 1000.0, 1e5, U)  # U: (0, 300)
KR = (0.0, 1e-5, 0.3, 0.95, U)
EMISSION = (0.0, 0.0, 0.2, 2.0)  # times a uniform colour
INTENSITY = (0, 1, 2, 3, 5, -1)
LIGHT_COUNTS = (0, 1, 2, 3, 5, 8)
INPUTS = ("nodes.bin", "aabbs.bin", "tris.bin", "triobj.bin", "mats.bin", "lights.bin")

# name -> base, table, ids, lights, W, H, spp, max_depth, diffuse_bounce, seed
# table: entries, or "neg" (5 entries, three of them negative), or 0 (empty, ids present).
# Seeds: the first of 1, 2, ... whose case meets tests/test_shade_fuzz.py's visibility conditions.
CASES = {
    "s_l0_d1": ("sphere", 5, "per_triangle", 0, 64, 36, 4, 1, True, 1),
    "s_l1_d1": ("sphere", 7, "per_triangle", 1, 64, 36, 16, 1, True, 3),
    "s_l2_d1": ("sphere", "neg", "per_object", 2, 64, 36, 5, 1, True, 11),
    "s_l3_d1": ("sphere", 5, "per_triangle", 3, 64, 36, 64, 1, True, 1),
    "s_l5_d1": ("sphere", 1, "per_object", 5, 64, 36, 128, 1, True, 6),
    "s_l8_d1": ("sphere", 0, "per_object", 8, 64, 36, 4, 1, True, 1),
    "s_l0_d4": ("sphere", 7, "per_triangle", 0, 64, 36, 64, 4, True, 1),
    "s_l1_d4": ("sphere", 5, "per_triangle", 1, 64, 36, 16, 4, True, 3),
    "s_l1_d4m": ("sphere", 7, "per_triangle", 1, 64, 36, 4, 4, False, 5),
    "s_l2_d4": ("sphere", 5, "per_triangle", 2, 64, 36, 4, 4, False, 4),
    "s_l3_d4": ("sphere", "neg", "per_triangle", 3, 64, 36, 16, 4, True, 1),
    "s_l5_d4": ("sphere", 7, "per_object", 5, 64, 36, 128, 4, True, 6),
    "s_l8_d4": ("sphere", 5, "per_object", 8, 64, 36, 16, 4, False, 16),
    "c_l3_d1": ("chain", 5, "per_triangle", 3, 48, 32, 4, 1, True, 1),
    "c_l3_d2": ("chain", 5, "per_triangle", 3, 32, 24, 5, 2, True, 1),
}
FIELDS = ("base", "table", "ids", "num_lights", "W", "H", "spp", "depth", "diffuse", "seed")


class Rng:
    """splitmix64; floats are 24-bit fractions, exact in float32."""

    def __init__(self, seed: int):
        self.s = (0x9E3779B97F4A7C15 * (seed + 1)) & (2**64 - 1)

    def next(self) -> int:
        self.s = (self.s + 0x9E3779B97F4A7C15) & (2**64 - 1)
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return z ^ (z >> 31)

    def u(self) -> float:
        return (self.next() >> 40) / float(1 << 24)

    def below(self, n: int) -> int:
        return self.next() % n

    def pick(self, options, lo=0.0, hi=1.0):
        v = options[self.below(len(options))]
        return lo + (hi - lo) * self.u() if v is U else v


def _seed(name: str, seed: int) -> int:
    return int.from_bytes(hashlib.sha256(f"{name}:{seed}".encode()).digest()[:6], "little")


def material_table(rng: Rng, table) -> np.ndarray:
    n = 5 if table == "neg" else int(table)
    m = np.zeros(n, MAT)
    for i in range(n):
        m["albedo"][i] = [1.3 * rng.u() for _ in range(3)]
        m["spec"][i] = [1.3 * rng.u() for _ in range(3)]
        m["kd"][i] = rng.pick(KD)
        m["ks"][i] = rng.pick(KS)
        m["shininess"][i] = rng.pick(SHININESS, 0.0, 300.0)
        m["kr"][i] = rng.pick(KR)
        e = rng.pick(EMISSION)
        m["emission"][i] = [e * rng.u() for _ in range(3)]
    if table == "neg":
        m["shininess"][1] = -2.0
        m["ks"][2] = -0.5
        m["kd"][3], m["kr"][3] = -1.0, 0.5  # kd + kr <= 0: the path ends (query.h:196-199)
    return m


def object_ids(rng: Rng, own: np.ndarray, nm: int, mode: str) -> np.ndarray:
    own = np.asarray(own, np.int32)
    if mode == "per_object":
        return (own % nm).astype(np.int32) if nm > 0 else own.copy()
    assert mode == "per_triangle" and nm > 0
    out = np.zeros(own.size, np.int64)
    outside = (-1, nm, nm + 5, INT_MAX, INT_MIN)
    for t in range(own.size):
        out[t] = outside[rng.below(5)] if rng.below(10) == 0 else rng.below(nm)
    return out.astype(np.int32)


def light_set(rng: Rng, n: int, lo, hi) -> np.ndarray:
    lt = np.zeros(n, LIGHT)
    for i in range(n):
        lt["position"][i] = [lo[a] + (hi[a] - lo[a]) * rng.u() for a in range(3)]
        lt["color"][i] = [1.2 * rng.u() for _ in range(3)]
        lt["intensity"][i] = INTENSITY[rng.below(len(INTENSITY))]
    return lt


def chain_rings(P: int = 600) -> dict:
    """chain_bvh.chain_scene(P)'s tree over other triangles.  As shipped the chain shows its
    camera one triangle (level 0 hides the rest) and every bounce ray leaves the scene, so no
    material table or depth could be seen in it.  Here level k's triangle is scaled so that it
    looks 0.2 + 1.4 k / (P - 2) times level 0's size from the camera: the levels show as
    concentric rings a fraction of a pixel wide (neighbouring samples hit different triangles),
    all still cover the image centre (the DFS stack still grows by one per level there, and the
    reference still overflows and completes by brute force), level 3 still repeats level 0.  The
    last level is a ceiling behind the camera (z = 6, facing down) that catches the bounce rays."""
    d = chain_bvh.chain_scene(P)
    perm = d["perm"]
    tris = np.zeros((P, 18), np.float32)
    nn = 2 * P - 1
    aabbs = np.zeros((nn, 6), np.float32)
    cam_z = np.float32(chain_bvh.CAMERA[0][2])
    for k in range(P):
        kk = 0 if k == 3 else k
        if k == P - 1:
            v = np.array([(-20.0, -20.0, 6.0), (20.0, -20.0, 6.0), (0.0, 20.0, 6.0)], np.float32)
            n = (0.0, 0.0, -1.0)
        else:
            z = np.float32(-0.01 * kk)
            s = np.float32(2.0) * np.float32(0.2 + 1.4 * kk / (P - 2)) * (cam_z - z) / cam_z
            v = np.array([(-s, -s, z), (s, -s, z), (0.0, s, z)], np.float32)
            n = (0.0, 0.0, 1.0)
        t = int(perm[k])
        tris[t, 0:9] = v.reshape(-1)
        tris[t, 9:18] = n * 3
        aabbs[P - 1 + k] = np.concatenate([v.min(axis=0), v.max(axis=0)])
    nodes = d["nodes"]
    for i in range(P - 2, -1, -1):
        le, ri = int(nodes[i]["left"]), int(nodes[i]["right"])
        aabbs[i] = np.concatenate([np.minimum(aabbs[le, :3], aabbs[ri, :3]), np.maximum(aabbs[le, 3:], aabbs[ri, 3:])])
    return {"nodes": nodes.view(np.uint32).reshape(-1, 4).copy(), "aabbs": aabbs, "tris": tris,
            "own_ids": np.zeros(P, np.int32), "camera": chain_bvh.CAMERA,
            # lights between the stack of rings (z <= 0) and the ceiling
            "light_box": ((-4.0, -4.0, 0.5), (4.0, 4.0, 5.5))}


def sphere_base() -> dict:
    from conftest import host_scene

    hs = host_scene("sphere.json")
    i = hs.info
    lo, hi = hs.aabbs[0, :3].astype(np.float64), hs.aabbs[0, 3:].astype(np.float64)
    up = np.array(tuple(i.cam_up), np.float64)
    h = float(np.dot(hi - lo, np.abs(up)))  # the scene box grown by its height
    return {"nodes": hs.nodes.copy(), "aabbs": hs.aabbs.copy(), "tris": hs.triangles.copy(),
            "own_ids": hs.tri_object_ids.copy(),
            "camera": (tuple(i.cam_position), tuple(i.cam_look_at), tuple(i.cam_up), float(i.focal_length_mm),
                       float(i.sensor_height_mm)),
            "light_box": (tuple(lo - h), tuple(hi + h))}


@lru_cache(maxsize=None)
def _base(kind: str) -> dict:
    return sphere_base() if kind == "sphere" else chain_rings(600)


def make_case(name: str, seed=None) -> dict:
    spec = dict(zip(FIELDS, CASES[name]))
    if seed is not None:
        spec["seed"] = seed
    b = _base(spec["base"])
    rng = Rng(_seed(name, spec["seed"]))
    mats = material_table(rng, spec["table"])
    ids = object_ids(rng, b["own_ids"], mats.size, spec["ids"])
    lights = light_set(rng, spec["num_lights"], *b["light_box"])
    c = dict(spec)
    c.update(name=name, nodes=b["nodes"], aabbs=b["aabbs"], tris=b["tris"], triobj=ids, mats=mats, lights=lights,
             camera=b["camera"], P=int(b["tris"].shape[0]))
    return c


@lru_cache(maxsize=None)
def case(name: str) -> dict:
    """The named case: arrays in the layouts of chain_bvh (nodes (2P-1, 4) uint32, aabbs, tris,
    triobj int32, mats MAT, lights LIGHT), camera tuple, W, H, spp, depth, diffuse.  Shared:
    do not modify."""
    return make_case(name)


def input_bytes(c: dict) -> dict:
    return {"nodes.bin": np.ascontiguousarray(c["nodes"], np.uint32).tobytes(),
            "aabbs.bin": np.ascontiguousarray(c["aabbs"], np.float32).tobytes(),
            "tris.bin": np.ascontiguousarray(c["tris"], np.float32).tobytes(),
            "triobj.bin": np.ascontiguousarray(c["triobj"], np.int32).tobytes(),
            "mats.bin": c["mats"].tobytes(), "lights.bin": c["lights"].tobytes()}


def input_sha256(c: dict) -> dict:
    return {k: hashlib.sha256(v).hexdigest() for k, v in input_bytes(c).items()}


def write_arrays(c: dict, out_dir) -> None:
    """The files oracle/_ref/ref_g `arrays` reads."""
    o = Path(out_dir)
    for k, v in input_bytes(c).items():
        (o / k).write_bytes(v)
    pos, look, up, f, s = c["camera"]
    (o / "camera.txt").write_text(" ".join(float(v).hex() for v in [*pos, *look, *up, f, s]) + "\n")


def mats13(c: dict):
    """The table as (n, 13) float32 rows, or None when it is empty."""
    return c["mats"].view(np.float32).reshape(-1, 13) if c["mats"].size else None


def oracle_render(c: dict, lights=None, depth=None, **kw):
    """orc.render_g of the case (miss colour 0), optionally with other lights or depth."""
    from oracle import pyoracle as orc

    pos, look, up, f, s = c["camera"]
    cam = orc.camera(pos, look, up, f, s, c["W"], c["H"])
    lt = c["lights"] if lights is None else lights
    return orc.render_g(c["P"], cam, c["nodes"], c["aabbs"], c["tris"], c["triobj"], mats13(c), lt, spp=c["spp"],
                        max_depth=c["depth"] if depth is None else depth, diffuse_bounce=c["diffuse"], **kw)


def primary_material(c: dict, hits: np.ndarray) -> np.ndarray:
    """Table entry of each hit sample's primary hit; -1: the default material, -2: a miss."""
    nm = c["mats"].size
    ids = c["triobj"].astype(np.int64)[np.maximum(hits, 0)]
    ent = np.where((ids >= 0) & (ids < nm), ids, -1)
    return np.where(hits >= 0, ent, -2)


def visibility(c: dict) -> dict:
    """The figures of tests/test_shade_fuzz.py's visibility conditions, from the oracle alone."""
    rgb, hi, _ = oracle_render(c, aov=True)
    hit_px = (hi >= 0).any(axis=2)
    nhp = max(int(hit_px.sum()), 1)
    out = {"finite": bool(np.isfinite(rgb).all()), "hit_frac": float((hi >= 0).mean()),
           "clamped_frac": float((rgb >= 1.0).mean())}
    pm = primary_material(c, hi)
    nh = max(int((pm >= -1).sum()), 1)
    out["entry_frac"] = [float((pm == e).sum()) / nh for e in range(c["mats"].size)]
    out["default_frac"] = float((pm == -1).sum()) / nh
    changed = lambda other: float(((other.view(np.uint32) != rgb.view(np.uint32)).any(axis=2) & hit_px).sum()) / nhp  # noqa: E731
    L = c["lights"]
    out["drop_light"] = []
    for i in range(L.size):
        if int(L[i]["intensity"]) == 0:
            # an intensity-0 light adds exactly 0: it shows as itself at intensity 1 would
            lit = L.copy()
            lit["intensity"][i] = 1
            out["drop_light"].append(changed(oracle_render(c, lights=lit)))
        else:
            out["drop_light"].append(changed(oracle_render(c, lights=np.delete(L, i))))
    out["no_lights"] = changed(oracle_render(c, lights=L[:0])) if L.size else None
    out["depth1"] = changed(oracle_render(c, depth=1)) if c["depth"] > 1 else None
    return out


def fixture_frames(name):
    """(fb, hits or None, t or None) of the fixture; the 64 and 128 spp AOVs are kept by sha256."""
    from conftest import golden_array

    c = case(name)
    W, H, spp = c["W"], c["H"], c["spp"]
    fb = golden_array("shade_" + name, "fb.f32.gz", np.float32).reshape(H, W, 3)
    if spp > 16:
        return fb, None, None
    return (fb, golden_array("shade_" + name, "hits.i32.gz", np.int32).reshape(H, W, spp),
            golden_array("shade_" + name, "hitt.f32.gz", np.float32).reshape(H, W, spp))


def check_against_fixture(name, rgb, hi, ht):
    """Frame, hit indices and t equal the reference's bit for bit (no tolerance)."""
    from conftest import golden_meta

    meta = golden_meta("shade_" + name)
    fb, ghi, ght = fixture_frames(name)
    hi, ht = np.ascontiguousarray(hi, np.int32), np.ascontiguousarray(ht, np.float32)
    if ghi is not None:
        assert np.array_equal(hi, ghi), f"{name}: {int((hi != ghi).sum())} primary hits differ"
        assert np.array_equal(ht.view(np.uint32), ght.view(np.uint32)), f"{name}: hit t differs"
    assert hashlib.sha256(hi.tobytes()).hexdigest() == meta["sha256"]["hits.i32"], f"{name}: hit indices"
    assert hashlib.sha256(ht.tobytes()).hexdigest() == meta["sha256"]["hitt.f32"], f"{name}: hit t"
    rgb = np.ascontiguousarray(rgb, np.float32)
    assert np.isfinite(rgb).all(), f"{name}: non-finite frame"
    bad = rgb.view(np.uint32) != fb.view(np.uint32)
    assert not bad.any(), (f"{name}: {int(bad.any(axis=2).sum())} pixels differ, "
                           f"max-abs {float(np.abs(rgb - fb).max())}")
