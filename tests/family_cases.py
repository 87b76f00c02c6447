"""Cases for the wave-family entry test (rt_debug_family_test_host / _batch: family_axis +
family_entry_passes, what family_dirs and frustum_loop call) with its two references (TEST DATA
GENERATOR, a helper module: no tests here).

A wave is 64 rays with one origin, `active` bytes, a bestT per lane, the scene bound bmax and 32
boxes (entry k tested as lane k tests it).

Sound side: the rays themselves.  Entry k must pass whenever some live lane's own
box_cases.ref_aabb(ray, box k, [1e-4, that lane's bestT]) passes: `any_pass`.

Tight side: model_pass, a float64 restatement of the documented rule with exact 1/d, the widening
2^-18 (twice the builds' 2^-19) and the loose rule as written.  The builds' float error (b - o,
v_rcp_f32, the product: < 2^-22 relative) is far inside the extra 2^-19, so whatever the model
rejects the builds must reject.

family_case(name) gives a named set {rays (W, 64, 6), active (W, 64) uint8, best_t (W, 64),
bmax (W, 3), boxes (W, 32, 6), band (W, 32), side (W, 32), any_pass (W, 32), model_pass (W, 32),
model_loose (W,)}, computed once and read-only.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import raytracinginonesemester_amd as rt
from box_cases import F32, FLT_MAX, TMIN, ref_aabb
from tile_cases import BANDS, TILE_CASES, _cameras, _perp

QUADS = ((2, 2, 16), (4, 4, 4), (8, 8, 1))  # (pixels wide, high, spp): 64 rays
FAMILY_CASES = tuple("camera_" + k for k in TILE_CASES) + ("free",)
KW_MODEL = 2.0 ** -18


# ---- the tight-side model -----------------------------------------------------------------
def model(rays, active, best_t, bmax, boxes):
    """(pass (W, 32) bool, loose (W,) bool): the documented rule in float64, widening 2^-18."""
    rays, best_t, bmax, boxes = (np.asarray(a, F32) for a in (rays, best_t, bmax, boxes))
    live = np.asarray(active) != 0
    W = rays.shape[0]
    o = rays[:, 0, :3]
    nr, fr = np.zeros((W, 32, 3)), np.zeros((W, 32, 3))
    loose = np.zeros(W, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            d = rays[:, :, 3 + a]
            dl = np.where(live, d, np.inf).min(axis=1)
            dh = np.where(live, d, -np.inf).max(axis=1)
            fin = (bmax[:, a] + np.abs(o[:, a])) < F32(1e30)  # float32, as the builds
            ok = ((dl >= F32(1e-8)) | (dh <= F32(-1e-8))) & fin
            lz = ~ok & fin
            loose |= lz
            dl64, dh64 = dl.astype(np.float64), dh.astype(np.float64)
            u0 = np.where(ok, 1.0 / dl64, np.where(lz, np.where(dh > 0, 1.0 / dh64, np.inf), -np.inf))
            u1 = np.where(ok, 1.0 / dh64, np.where(lz, np.where(dl < 0, 1.0 / dl64, -np.inf), np.inf))
            lo = boxes[:, :, a].astype(np.float64) - o[:, None, a].astype(np.float64)
            hi = boxes[:, :, 3 + a].astype(np.float64) - o[:, None, a].astype(np.float64)
            px, py, qx, qy = lo * u0[:, None], lo * u1[:, None], hi * u0[:, None], hi * u1[:, None]
            n_ = np.fmin(np.fmin(px, py), np.fmin(qx, qy))
            f_ = np.fmax(np.fmax(px, py), np.fmax(qx, qy))
            la = ((u0 > 0) & (u1 < 0))[:, None]  # the loose axis' one-sided bound
            nr[:, :, a] = np.where(la, np.fmax(px, qy), n_)
            fr[:, :, a] = np.where(la, np.inf, f_)
        Lc = np.fmax(np.fmax(nr[:, :, 0], nr[:, :, 1]), nr[:, :, 2])
        Hc = np.fmin(np.fmin(fr[:, :, 0], fr[:, :, 1]), fr[:, :, 2])
        Lc = Lc - np.abs(Lc) * KW_MODEL
        Hc = Hc + np.abs(Hc) * KW_MODEL
        tmax_w = np.where(live, best_t, 0).astype(np.float64).max(axis=1)
        ok_ = np.fmax(Lc, float(TMIN)) <= np.fmin(Hc, tmax_w[:, None])
    return ok_, loose


# ---- the sound-side reference -------------------------------------------------------------
def any_lane_passes(rays, active, best_t, boxes):
    """(W, 32): some live lane's ref_aabb(ray, box k, [1e-4, its bestT]) passes."""
    W = rays.shape[0]
    out = np.zeros((W, 32), bool)
    step = 256
    for i in range(0, W, step):
        r, b, t, a = rays[i:i + step], boxes[i:i + step], best_t[i:i + step], active[i:i + step]
        k = r.shape[0]
        rr = np.broadcast_to(r[:, None, :, :], (k, 32, 64, 6)).reshape(-1, 6)
        bb = np.broadcast_to(b[:, :, None, :], (k, 32, 64, 6)).reshape(-1, 6)
        tmm = np.empty((k, 32, 64, 2), F32)
        tmm[..., 0] = TMIN
        tmm[..., 1] = t[:, None, :]
        ok = ref_aabb(rr, bb, tmm.reshape(-1, 2)).reshape(k, 32, 64)
        out[i:i + k] = (ok & (a[:, None, :] != 0)).any(axis=2)
    return out


# ---- waves ----------------------------------------------------------------------------------
def _camera_waves(rng, kind):
    """Camera quads (QUADS) of the tile cases' cameras: a quad across the image centre (on the
    camera's own axis planes: direction components cross zero, the loose form, for the cameras
    along an axis), one at a corner and one free."""
    for k, (cam, scale) in enumerate(_cameras(rng, kind)):
        W, H = cam.pixel_width, cam.pixel_height
        if W < 8 or H < 8:
            continue
        w, h, spp = QUADS[k % 3]
        places = [((W - w) // 2, (H - h) // 2), (0, H - h), (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)))]
        for (x0, y0) in places:
            rays, _ = rt.camera_rays(cam, spp=spp, row0=y0, rows=h)
            yield rays.reshape(h, W, spp, 6)[:, x0:x0 + w].reshape(64, 6).copy(), scale


def _free_waves(rng, n):
    """One origin, directions over a hemisphere (intervals crossing zero on two and three axes) or
    a cone around an axis, some lanes with |d| < 1e-8 on an axis, at several magnitudes."""
    for k in range(n):
        scale = float(rng.choice([1.0, 2.0 ** -10, 2.0 ** 12, 1e-3, 1e3]))
        o = rng.normal(size=3) * scale * float(rng.choice([0.0, 1.0, 3.0]))
        d = rng.normal(size=(64, 3))
        kind = k % 4
        if kind == 0:  # a hemisphere around a free pole
            pole = rng.normal(size=3)
            d = np.where((d @ pole)[:, None] < 0, -d, d)
        elif kind == 1:  # a narrow cone around an axis: two intervals cross zero
            d = d * 0.05 + np.roll(np.array([1.0, 0.0, 0.0]), k % 3) * (1 if k % 8 < 4 else -1)
        elif kind == 2:  # one sign on every axis
            d = np.abs(d) * rng.choice([-1.0, 1.0], size=3) + 0.01 * rng.choice([-1.0, 1.0], size=3)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        if kind == 3 or k % 5 == 0:  # lanes with a parallel component
            sel = rng.random((64, 3)) < 0.1
            d[sel] = rng.choice([0.0, -0.0, 5e-9, -5e-9, 9.9e-9, 1.01e-8, -1.01e-8], size=sel.sum())
        yield np.concatenate([np.tile(o, (64, 1)), d], axis=1).astype(F32), scale


def _wave_boxes(rng, rays, live, scale):
    """32 boxes: most with a corner off a live lane's ray by a band's relative offset, on both
    sides (tile_cases' construction), flat boxes on 1-3 axes, boxes around the origin, free boxes."""
    o = rays[0, :3].astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    lanes = np.flatnonzero(live)
    dmean = d[lanes].mean(axis=0)
    boxes = np.zeros((32, 6))
    band = np.full(32, -1, np.int64)
    side = np.zeros(32, np.int64)
    aim = np.zeros(32, np.int64)
    for i in range(32):
        L = int(rng.choice(lanes))
        aim[i] = L
        dn = d[L] / max(np.linalg.norm(d[L]), 1e-30)
        t = scale * float(rng.choice([0.3, 1.0, 2.0, 5.0]) * rng.uniform(0.5, 1.5))
        size = scale * float(rng.choice([1e-3, 0.1, 1.0]))
        q = o + t * dn
        if i < 24:
            band[i], side[i] = (i // 2) % 6, 1 if i % 2 == 0 else -1
            if rng.random() < 0.5 and lanes.size > 1:  # away from the family's mean direction
                nrm = dn - dmean * (dn @ dmean) / max(dmean @ dmean, 1e-30)
                nrm = nrm - dn * (nrm @ dn)
            else:
                nrm = _perp(rng, dn)
            nn = np.linalg.norm(nrm)
            nrm = nrm / nn if nn > 1e-12 else _perp(rng, dn)
            corner = q + side[i] * BANDS[band[i]] * t * nrm
            sg = np.where(nrm >= 0, 1.0, -1.0)
            boxes[i, :3], boxes[i, 3:] = np.minimum(corner, corner + sg * size), np.maximum(corner, corner + sg * size)
        elif i < 27:  # flat on 1, 2, 3 axes
            h = np.where(rng.random(3).argsort() < i - 23, 0.0, size)
            boxes[i, :3], boxes[i, 3:] = q - h, q + h
        elif i < 29:  # the origin inside the box, or on its face
            h = np.abs(rng.normal(size=3)) * size + size
            c = o + (h * rng.choice([0.0, 0.5, 1.0]) * rng.choice([-1.0, 1.0], size=3))
            boxes[i, :3], boxes[i, 3:] = c - h, c + h
        else:
            c = o + t * (dn + rng.normal(size=3) * float(rng.choice([0.01, 0.3, 2.0])))
            h = np.abs(rng.normal(size=3)) * size
            boxes[i, :3], boxes[i, 3:] = c - h, c + h
    return np.ascontiguousarray(boxes, F32), band, side, aim


def _entry_t(ray, box):
    """The reference's entry parameter of the ray at the box (float64), as float32."""
    with np.errstate(all="ignore"):
        o, d = ray[:3].astype(np.float64), ray[3:].astype(np.float64)
        t0 = (box[:3].astype(np.float64) - o) / d
        t1 = (box[3:].astype(np.float64) - o) / d
        t = np.fmax.reduce(np.fmin(t0, t1))
    return F32(t) if np.isfinite(t) and t > 0 else F32(1.0)


def _build(rng, waves):
    R, A, T, M, B, band, side = [], [], [], [], [], [], []
    for w, (rays, sc) in enumerate(waves):
        live = np.zeros(64, np.uint8)
        if w % 3 == 0:  # one live lane, half the lanes, all 64
            live[int(rng.integers(0, 64))] = 1
        elif w % 3 == 1:
            live[rng.permutation(64)[:32]] = rng.choice(np.array([1, 2, 255], np.uint8))
        else:
            live[:] = 1
        boxes, bd, sd, aim = _wave_boxes(rng, rays, live != 0, sc)
        mode = (w // 3) % 6
        t_aim = _entry_t(rays[aim[0]], boxes[0])
        if mode == 0:
            bt = np.full(64, FLT_MAX, F32)
        elif mode == 1:
            bt = np.full(64, t_aim, F32)
        elif mode == 2:
            bt = np.full(64, np.nextafter(t_aim, F32(np.inf)), F32)
        elif mode == 3:
            bt = np.full(64, np.nextafter(t_aim, F32(0)), F32)
        elif mode == 4:
            bt = np.full(64, TMIN, F32)
        else:  # per lane: no hit yet, or a hit somewhere along the way
            bt = np.where(rng.random(64) < 0.5, FLT_MAX, sc * rng.uniform(0.1, 6.0, size=64)).astype(F32)
        bm = np.abs(boxes).max(axis=0).reshape(2, 3).max(axis=0) * float(rng.choice([1.0, 16.0, 1024.0]))
        if w % 11 == 5:  # an axis of coordinates near the float range: no bound there
            bm[int(rng.integers(0, 3))] = float(rng.choice([1e30, 3e38]))
        R.append(rays), A.append(live), T.append(bt), M.append(bm.astype(F32)), B.append(boxes)
        band.append(bd), side.append(sd)
    case = {"rays": np.ascontiguousarray(R, F32), "active": np.ascontiguousarray(A, np.uint8),
            "best_t": np.ascontiguousarray(T, F32), "bmax": np.ascontiguousarray(M, F32),
            "boxes": np.ascontiguousarray(B, F32), "band": np.array(band), "side": np.array(side)}
    case["any_pass"] = any_lane_passes(case["rays"], case["active"], case["best_t"], case["boxes"])
    case["model_pass"], case["model_loose"] = model(case["rays"], case["active"], case["best_t"], case["bmax"], case["boxes"])
    for v in case.values():
        v.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def family_case(name: str) -> dict:
    rng = np.random.default_rng([41, FAMILY_CASES.index(name)])
    if name == "free":
        return _build(rng, list(_free_waves(rng, 900)))
    waves = []
    for _ in range(5):  # 5 draws of the cameras
        waves += list(_camera_waves(rng, name[len("camera_"):]))
    return _build(rng, waves)


def describe(case, idx, limit=3):
    """The first `limit` (wave, entry) pairs of idx (an (m, 2) array) as hex floats."""
    out = []
    for w, k in np.asarray(idx)[:limit]:
        live = np.flatnonzero(case["active"][w])
        out.append("wave %d entry %d: origin %s box %s bmax %s live lanes %s\n  dirs %s\n  bestT %s" % (
            w, k, [float(x).hex() for x in case["rays"][w, 0, :3]], [float(x).hex() for x in case["boxes"][w, k]],
            [float(x).hex() for x in case["bmax"][w]], live.tolist(),
            [[float(x).hex() for x in case["rays"][w, l, 3:]] for l in live[:4]],
            [float(x).hex() for x in case["best_t"][w, live[:4]]]))
    return "\n".join(out)


# ---- what both builds must satisfy (the host tests and the GPU tests call these) -------------
def _call(entry, device, rays, active, best_t, bmax, boxes, n=None):
    from raytracinginonesemester_amd import _lib

    n = rays.shape[0] if n is None else n
    out = np.full((n, 32), -1, np.int32)
    loose = np.full(n, -1, np.int32)
    args = [np.ascontiguousarray(rays, F32), None if active is None else np.ascontiguousarray(active, np.uint8),
            np.ascontiguousarray(best_t, F32), np.ascontiguousarray(bmax, F32), np.ascontiguousarray(boxes, F32)]
    ptrs = [None if a is None else a.ctypes.data for a in args]
    fn = getattr(_lib.lib(), entry)
    _lib.check(fn(*(([0] if device else []) + ptrs + [n, out.ctypes.data, loose.ctypes.data])))
    return out, loose


def host_fn(*a, **k):
    return _call("rt_debug_family_test_host", False, *a, **k)


def device_fn(*a, **k):
    return _call("rt_debug_family_test_batch", True, *a, **k)


def check_set(fn, name):
    """Both sides on one set; prints the rejected shares (not asserted)."""
    c = family_case(name)
    out, loose = fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"])
    assert np.isin(out, (0, 1)).all()
    assert np.array_equal(loose, c["model_loose"].astype(np.int32)), name
    bad = np.argwhere(c["any_pass"] & (out == 0))
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} of {out.size} entries rejected although a live lane's "
                               f"own test passes\n" + describe(c, bad))
    bad = np.argwhere(~c["model_pass"] & (out == 1))
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} of {out.size} entries pass although the 2^-18 model "
                               f"rejects them\n" + describe(c, bad))
    miss = ~c["any_pass"]
    print(f"{name}: {out.shape[0]} waves, loose {float(loose.mean()):.3f}, all-lanes-miss {float(miss.mean()):.3f}; "
          f"of those rejected: build {float((out[miss] == 0).mean()):.4f}, model {float((~c['model_pass'][miss]).mean()):.4f}")
    return out, loose


def check_inactive_lanes(fn, name):
    """What the inactive lanes hold (other directions, NaN, another bestT) changes no answer, and
    `active` NULL is all lanes live."""
    c = family_case(name)
    rng = np.random.default_rng(43)
    out, loose = fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"])
    off = c["active"] == 0
    rays, bt = c["rays"].copy(), c["best_t"].copy()
    junk = rng.normal(size=rays[..., 3:].shape).astype(F32)
    junk[rng.random(junk.shape) < 0.1] = np.nan
    rays[..., 3:][off] = junk[off]
    bt[off] = rng.choice(np.array([0.0, 1e-5, 3.4028235e38, np.nan], F32), size=int(off.sum()))
    out2, loose2 = fn(rays, c["active"], bt, c["bmax"], c["boxes"])
    assert np.array_equal(out, out2) and np.array_equal(loose, loose2)
    full = (c["active"] != 0).all(axis=1)
    assert full.any()
    out3, loose3 = fn(c["rays"][full], None, c["best_t"][full], c["bmax"][full], c["boxes"][full])
    assert np.array_equal(out3, out[full]) and np.array_equal(loose3, loose[full])


def check_short_batches(fn, name="free"):
    """1, 3 and 5 waves (a block holds 4: a partial last block); nothing is written past n."""
    c = family_case(name)
    out, loose = fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"])
    for n in (1, 3, 5, 63, 65):
        o, l = fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"], n)
        assert np.array_equal(o, out[:n]) and np.array_equal(l, loose[:n]), n


# ---- waves of degenerate cameras (tests/camera_cases.py): sound side only --------------------
# What a frame of a camera outside 1e-12 <= |D| <= ~1.8e19 can bring to a wave: lanes that hold
# get_ray's fallback (0, 0, 1) beside ordinary directions, lanes with a zero direction (|D|^2
# overflowed), and 64 identical lanes (intervals of zero width).  NaN lanes are outside the
# family's contract: its min / max drop them, and render_frame sends such a frame to the lane
# kernel (camera_class).  A zero direction is parallel on every axis, so the lane's own test is the
# inside test of the origin on all three.
DEGENERATE_CASES = ("mixed_fallback", "zero_lanes", "identical")


def _degenerate_waves(rng, name):
    import camera_cases as cc

    def quads(c, spp_of_quad):
        w, h, spp = spp_of_quad
        tab = c["table"] if c["spp"] == spp else rt.jittered_samples(spp)
        rays, _ = rt.camera_rays(c["cam"], spp=spp, jitter=tab)
        rays = rays.reshape(c["H"], c["W"], spp, 6)
        for y0 in range(0, c["H"] - h + 1, h):
            for x0 in range(0, c["W"] - w + 1, w):
                yield rays[y0:y0 + h, x0:x0 + w].reshape(64, 6).copy()

    fb = np.array([0.0, 0.0, 1.0], F32)
    if name == "mixed_fallback":
        # every quad of the threshold and plane frames that holds both kinds, then ordinary
        # camera quads with lanes overwritten by the fallback
        for cname in cc.names_of("threshold") + cc.names_of("plane"):
            for q in QUADS:
                for r in quads(cc.case(cname), q):
                    f = cc.is_fallback(r[:, 3:])
                    if f.any() and not f.all():
                        yield r, 1.0
        for k, (r, sc) in enumerate(_camera_waves(rng, "free")):
            if k % 7 == 0:
                r[rng.random(64) < float(rng.choice([0.02, 0.5, 0.98])), 3:] = fb
                yield r, sc
    elif name == "zero_lanes":
        for cname in ("ov_partial_du", "ov_partial_du_1e28", "ov_sphere_partial_dv", "ov_sensor_1e25"):
            for r in quads(cc.case(cname), QUADS[1]):
                yield r, 1.0
        for k, (r, sc) in enumerate(_camera_waves(rng, "inside")):
            if k % 7 == 0:
                r[rng.random(64) < float(rng.choice([0.02, 0.5, 1.0])), 3:] = rng.choice(np.array([0.0, -0.0], F32))
                yield r, sc
    else:
        for cname in cc.names_of("fallback") + ("co_du0_dv0", "co_up_zero", "ov_pos_1e20"):
            c = cc.case(cname)
            for q in QUADS[1:]:
                for i, r in enumerate(quads(c, q)):
                    if i % 5 == 0:
                        yield r, 1.0
        for k, (r, sc) in enumerate(_camera_waves(rng, "axis")):
            if k % 7 == 0:
                r[:, 3:] = r[int(rng.integers(0, 64)), 3:]
                yield r, sc


def _build_degenerate(rng, waves):
    import camera_cases as cc

    scene_boxes = np.concatenate([np.asarray(cc.scene(s)["aabbs"], F32).reshape(-1, 6)[:15]
                                  for s in ("above_origin", "sphere_single", "cornell")])
    R, A, T, M, B = [], [], [], [], []
    for w, (rays, sc) in enumerate(waves):
        live = np.ones(64, np.uint8)
        if w % 3 == 1:
            live[rng.permutation(64)[:32]] = 0
        nonzero = (rays[:, 3:] != 0).any(axis=1)
        aim = (live != 0) & nonzero
        if not aim.any():  # only zero directions: boxes around the origin and the scenes' own
            boxes = np.tile(scene_boxes[rng.integers(0, scene_boxes.shape[0], size=32)], (1, 1)).astype(F32)
            o = rays[0, :3]
            h = (np.abs(rng.normal(size=(8, 3))) * sc + 0.01 * sc).astype(F32)
            off = (h * rng.choice([0.0, 0.5, 1.0, 1.5], size=(8, 3)) * rng.choice([-1.0, 1.0], size=(8, 3))).astype(F32)
            boxes[:8, :3], boxes[:8, 3:] = o + off - h, o + off + h
        else:
            boxes, _bd, _sd, _aim = _wave_boxes(rng, rays, aim, sc)
            boxes = boxes.copy()
            boxes[24:] = scene_boxes[rng.integers(0, scene_boxes.shape[0], size=8)]
        mode = w % 4
        if mode == 0:
            bt = np.full(64, FLT_MAX, F32)
        elif mode == 1:
            bt = np.full(64, TMIN, F32)
        else:
            bt = np.where(rng.random(64) < 0.5, FLT_MAX, sc * rng.uniform(0.1, 6.0, size=64)).astype(F32)
        bm = np.maximum(np.abs(boxes).max(axis=0).reshape(2, 3).max(axis=0), np.abs(scene_boxes).max()) * 2.0
        R.append(rays), A.append(live), T.append(bt), M.append(bm.astype(F32)), B.append(boxes)
    case = {"rays": np.ascontiguousarray(R, F32), "active": np.ascontiguousarray(A, np.uint8),
            "best_t": np.ascontiguousarray(T, F32), "bmax": np.ascontiguousarray(M, F32),
            "boxes": np.ascontiguousarray(B, F32)}
    assert np.isfinite(case["rays"]).all()
    case["any_pass"] = any_lane_passes(case["rays"], case["active"], case["best_t"], case["boxes"])
    for v in case.values():
        v.setflags(write=False)
    return case


@lru_cache(maxsize=None)
def degenerate_case(name: str) -> dict:
    rng = np.random.default_rng([45, DEGENERATE_CASES.index(name)])
    return _build_degenerate(rng, list(_degenerate_waves(rng, name)))


def check_degenerate(fn, name):
    """Sound side: no entry rejected while some live lane's own test passes it."""
    c = degenerate_case(name)
    out, loose = fn(c["rays"], c["active"], c["best_t"], c["bmax"], c["boxes"])
    assert np.isin(out, (0, 1)).all()
    live = c["active"] != 0
    d = c["rays"][..., 3:]
    import camera_cases as cc

    fb = cc.is_fallback(d.reshape(-1, 3)).reshape(live.shape) & live
    zero = (d == 0).all(axis=2) & live
    same = np.array([(np.unique(d[w][live[w]].view(np.uint32), axis=0).shape[0] == 1) for w in range(d.shape[0])])
    print(f"{name}: {out.shape[0]} waves (with fallback lanes {int(fb.any(axis=1).sum())}, mixed "
          f"{int((fb.any(axis=1) & ~(fb | ~live).all(axis=1)).sum())}, with zero lanes {int(zero.any(axis=1).sum())}, "
          f"identical {int(same.sum())}), loose {float(loose.mean()):.3f}, some lane passes {float(c['any_pass'].mean()):.3f}, "
          f"rejected of the rest {float((out[~c['any_pass']] == 0).mean()):.3f}")
    assert out.shape[0] >= 40 and c["any_pass"].any() and (~c["any_pass"]).any()
    if name == "mixed_fallback":
        assert (fb.any(axis=1) & ~(fb | ~live).all(axis=1)).sum() >= 20
    elif name == "zero_lanes":
        assert zero.any(axis=1).sum() >= 20 and (zero | ~live).all(axis=1).any()
    else:
        assert same.sum() >= 20
    bad = np.argwhere(c["any_pass"] & (out == 0))
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} of {out.size} entries rejected although a live lane's own "
                               f"test passes\n" + describe(c, bad))
    return out, loose
