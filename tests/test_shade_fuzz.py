"""Shading fuzz cases on the CPU (tests/shade_fuzz.py): the generator and the oracle pinned to
the reference's fixtures, and the conditions under which a case can fail at all.

Goldens: tests/golden/scenes/shade_<name>, the reference's own render() + SearchBVH on the
case's arrays (tests/golden/gen_golden.py gen_shade, oracle/_ref/ref_g arrays, miss colour 0).
Bar: bit-exact frame, hit indices and t.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
import pytest

from conftest import golden_meta, hexv

import shade_fuzz as sf

NAMES = list(sf.CASES)


@lru_cache(maxsize=None)
def vis(name):
    return sf.visibility(sf.case(name))


def test_case_list_covers_the_issue():
    """Every light count at depth 1 and above on the sphere base, both bounce modes, every spp
    class at depth 1 and above, every table kind and id mode, the chain base with 3 lights."""
    cs = [sf.case(n) for n in NAMES]
    sph = [c for c in cs if c["base"] == "sphere"]
    for deep in (False, True):
        sel = [c for c in sph if (c["depth"] > 1) == deep]
        assert {c["num_lights"] for c in sel} == set(sf.LIGHT_COUNTS)
        assert {c["spp"] for c in cs if (c["depth"] > 1) == deep} == {4, 5, 16, 64, 128}
    assert {c["diffuse"] for c in sph if c["depth"] > 1} == {True, False}
    assert {c["table"] for c in cs} == {0, 1, 5, 7, "neg"}
    assert {c["ids"] for c in cs} == {"per_object", "per_triangle"}
    assert {(c["num_lights"], c["table"], c["depth"]) for c in cs if c["base"] == "chain"} == {(3, 5, 1), (3, 5, 2)}
    for c in cs:
        assert c["lights"].size == c["num_lights"]
        for a in ("aabbs", "tris"):
            assert np.isfinite(c[a]).all()
        assert np.isfinite(c["mats"].view(np.float32)).all()
        assert np.isfinite(c["lights"]["position"]).all() and np.isfinite(c["lights"]["color"]).all()


@pytest.mark.parametrize("name", NAMES)
def test_generator_is_pinned(name):
    """Each case's arrays hash to its fixture's meta.json, and its camera is the fixture's."""
    from oracle import pyoracle as orc

    c = sf.case(name)
    meta = golden_meta("shade_" + name)
    assert sf.input_sha256(c) == {k: meta["sha256"][k] for k in sf.INPUTS}
    assert (meta["width"], meta["height"], meta["spp"], meta["max_depth"], bool(meta["diffuse_bounce"])) == \
        (c["W"], c["H"], c["spp"], c["depth"], c["diffuse"])
    assert meta["num_lights"] == c["num_lights"] and meta["num_materials"] == c["mats"].size
    pos, look, up, f, s = c["camera"]
    cam = orc.camera(pos, look, up, f, s, c["W"], c["H"])
    for k, v in (("center", cam.center), ("pixel00_loc", cam.pixel00), ("pixel_delta_u", cam.du),
                 ("pixel_delta_v", cam.dv)):
        assert np.array_equal(np.array([v.x, v.y, v.z], np.float32).view(np.uint32), hexv(meta[k]).view(np.uint32)), k


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_pinned(name):
    """orc.render_g on the case equals the reference bit for bit (uint32 view), AOVs included."""
    rgb, hi, ht = sf.oracle_render(sf.case(name), aov=True)
    sf.check_against_fixture(name, rgb, hi, ht)


@pytest.mark.parametrize("name", NAMES)
def test_case_is_not_blind(name):
    """A case could not pass by showing nothing: enough samples hit, few values sit at the clamp,
    every table entry and the default material are primary hits (per_triangle), every light
    changes the frame, so do the lights together and the depth.  (A light of intensity 0 adds
    exactly 0 to every sample, so dropping it cannot change a frame; it counts as seen where the
    same light at intensity 1 would change the frame.)"""
    c, v = sf.case(name), vis(name)
    assert v["finite"]
    assert v["hit_frac"] >= 0.5, v["hit_frac"]
    assert v["clamped_frac"] <= 0.25, v["clamped_frac"]
    if c["ids"] == "per_triangle":
        assert min(v["entry_frac"]) >= 0.03, v["entry_frac"]
        assert v["default_frac"] >= 0.03, v["default_frac"]
    assert all(d > 0.0 for d in v["drop_light"]), v["drop_light"]
    if c["num_lights"]:
        assert v["no_lights"] >= 0.3, v["no_lights"]
    if c["depth"] > 1:
        assert v["depth1"] >= 0.1, v["depth1"]


def _seen_entries(name):
    """Table entries that are the primary hit of at least 3 % of the hit samples."""
    c, v = sf.case(name), vis(name)
    return [c["mats"][e] for e in range(c["mats"].size) if v["entry_frac"][e] >= 0.03]


def test_edge_values_are_seen():
    """Intensity 0 and -1, kd + kr <= 0, kr = 1e-5 (the throughput cut, on a mirror bounce) and
    shininess 0 / 0.5 / negative each occur on a light or material that is seen; the empty table
    and the ids outside a table too."""
    inten = {int(i) for n in NAMES for i in sf.case(n)["lights"]["intensity"]}  # every light is seen (above)
    assert {0, -1} <= inten
    bounce = [m for n in NAMES if sf.case(n)["depth"] > 1 for m in _seen_entries(n)]
    assert any(m["kd"] + m["kr"] <= 0.0 for m in bounce)
    assert any(m["kd"] < 0.0 for m in bounce)
    mirror = [m for n in NAMES if sf.case(n)["depth"] > 1 and not sf.case(n)["diffuse"] for m in _seen_entries(n)]
    assert any(m["kr"] == np.float32(1e-5) and m["spec"].max() * m["kr"] < 1e-4 for m in mirror)
    every = [m for n in NAMES for m in _seen_entries(n)]
    for s in (0.0, 0.5, -2.0):
        assert any(m["shininess"] == np.float32(s) and m["ks"] != 0.0 for m in every), s
    assert any(m["ks"] < 0.0 for m in every)
    empty = [n for n in NAMES if sf.case(n)["table"] == 0]
    assert empty and all(vis(n)["default_frac"] == 1.0 and sf.case(n)["triobj"].max() > 0 for n in empty)
    for n in NAMES:
        c = sf.case(n)
        if c["ids"] == "per_triangle":
            nm = c["mats"].size
            assert {-1, nm, nm + 5, sf.INT_MAX, sf.INT_MIN} <= set(c["triobj"].tolist())
