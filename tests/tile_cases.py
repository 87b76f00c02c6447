"""Cases for the tile test (rt_debug_tile_test_host / _batch: tile_dirs_f + tile_misses_box_f, the
function tile_cull_kernel and tile_cut_kernel call) with its two references (TEST DATA GENERATOR,
a helper module: no tests here).

Sound side: the rays themselves.  A tile's rays are rt.camera_rays' (the reference's get_ray
arithmetic on the host) under TABLE16, 16 jitter entries that span the one-pixel pad: the four
corners (+-1, +-1), (-0.5, 0.49999997), the centre and ten random entries in [-1, 1].  Each goes
through box_cases.ref_aabb (float64, tmin 1e-4, tmax FLT_MAX).  Where any ray of the tile passes,
the test must not say "missed": `any_pass`.

Tight side: model_cull, a float64 restatement of the documented rule with every margin doubled
(pad terms 2 * (16 ulp + 1.1e-5 * scale), slacks 2e-4, parallel threshold 2e-6, inside tolerance
2e-4).  The device forms' float error is a few ulps (6e-8 relative) of the same terms, the doubled
margins add 1e-5 and up, so whatever the model culls the builds must cull.  One term of the rule
is not monotone in the margins: the absolute slack 1e-4 * mag * max |1/D| takes its maximum over
the axes in use, and a wider interval takes an axis that nearly reaches 0 out of use.  The model's
maximum therefore also runs over the axes the undoubled rule uses (model_cull); without that it
culls items the rule as documented keeps (a camera 4096 from the origin, an 80 x 48 image: the
slack falls from 397 to 4.3).

tile_case(name) gives a named set: a list of groups, one per (camera, rectangle), each with the
camera, `tiles` (n, 4) int32 = (x0, x1, y0, y1), `boxes` (n, 6), `band` (n,) (index into BANDS,
-1 for the other kinds), `side` (n,) (+1 outside, -1 inside, 0 other), `any_pass`, `model_cull`;
computed once and read-only.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import raytracinginonesemester_amd as rt
from box_cases import F32, FLT_MAX, TMIN, ref_aabb

BANDS = (1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
RECTS = ((1, 1), (2, 2), (4, 4), (8, 8), (16, 4), (64, 1))
IMAGES = ((1, 1), (80, 48), (1920, 1080), (3840, 2160))
FOCALS = (8.0, 35.0, 600.0)
# (scale, shift): the unit scene, scene and camera scaled by 2^-10 and 2^12, and shifted by 4096
TRANSFORMS = ((1.0, 0.0), (2.0 ** -10, 0.0), (2.0 ** 12, 0.0), (1.0, 4096.0))
# a set per kind of camera (test_gpu_parity._fuzz_cameras' kinds), each with every transform, image
# size and focal length
TILE_CASES = ("axis", "inside", "grazing", "free")
BOXES_PER_GROUP = 108
EPS32 = 2.0 ** -23


def _table16():
    rng = np.random.default_rng(21)
    t = [(1, 1), (1, -1), (-1, 1), (-1, -1), (-0.5, 0.49999997), (0, 0)]
    t += [tuple(v) for v in rng.uniform(-1, 1, size=(10, 2))]
    return np.ascontiguousarray(t, F32)


TABLE16 = _table16()
TABLE16.setflags(write=False)


# ---- the tight-side model -----------------------------------------------------------------
def model_cull(cam, tiles, boxes):
    """tile_misses_box_f(tile_dirs_f(cam, tile), box) in float64 with every margin doubled."""
    b = cam.basis()
    c, p0, du, dv = (b[k].astype(np.float64) for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"))
    tiles = np.asarray(tiles, np.float64)
    bx = np.asarray(boxes, F32).astype(np.float64)
    n = tiles.shape[0]
    pxl, pxh, pyl, pyh = tiles[:, 0] - 1, tiles[:, 1] + 1, tiles[:, 2] - 1, tiles[:, 3] + 1
    pxm, pym = np.maximum(np.abs(pxl), np.abs(pxh)), np.maximum(np.abs(pyl), np.abs(pyh))
    Dl, Dh, Dl1, Dh1 = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for a in range(3):
        base = p0[a] - c[a]
        u0, u1, v0, v1 = pxl * du[a], pxh * du[a], pyl * dv[a], pyh * dv[a]
        ulp = 2 * 16 * EPS32 * (abs(c[a]) + abs(p0[a]) + pxm * abs(du[a]) + pym * abs(dv[a]))
        Dl[:, a] = base + np.minimum(u0, u1) + np.minimum(v0, v1) - ulp
        Dh[:, a] = base + np.maximum(u0, u1) + np.maximum(v0, v1) + ulp
        Dl1[:, a], Dh1[:, a] = Dl[:, a] + ulp / 2, Dh[:, a] - ulp / 2
    scale = np.maximum(np.abs(Dl), np.abs(Dh)).max(axis=1)
    Dl -= 2 * 1.1e-5 * scale[:, None]
    Dh += 2 * 1.1e-5 * scale[:, None]
    # the undoubled intervals, for the slack's |1/D| term alone (see imax below)
    Dl1, Dh1 = Dl1 + 0.0, Dh1 + 0.0
    scale1 = np.maximum(np.abs(Dl1), np.abs(Dh1)).max(axis=1)
    Dl1 -= 1.1e-5 * scale1[:, None]
    Dh1 += 1.1e-5 * scale1[:, None]
    usable = (scale > 0) & (scale < 1e30)
    mn, mx = bx[:, :3], bx[:, 3:]
    with np.errstate(all="ignore"):
        s3 = np.abs(mn) + np.abs(mx) + np.abs(c)[None, :]
        tol = 2e-4 * s3 + 1e-30
        inside = ((c[None, :] >= mn - tol) & (c[None, :] <= mx + tol)).all(axis=1)
        mag = np.fmax.reduce(s3, axis=1)
        sorted_ = (mn <= mx).all(axis=1)
        skip = ~(usable & ~inside & sorted_ & (mag < 1e30))
        entry_min = np.full(n, -np.inf)
        exit_max = np.full(n, np.inf)
        imax = np.zeros(n)
        for a in range(3):
            use = (Dl[:, a] > 2e-6 * scale) | (Dh[:, a] < -2e-6 * scale)
            iDl, iDh = 1.0 / Dl[:, a], 1.0 / Dh[:, a]
            nA, xA = mn[:, a] - c[a], mx[:, a] - c[a]
            pos = Dl[:, a] > 0
            ne, nx = np.where(pos, nA, xA), np.where(pos, xA, nA)
            e = np.minimum(ne * iDl, ne * iDh)
            f = np.maximum(nx * iDl, nx * iDh)
            entry_min = np.where(use, np.fmax(entry_min, e), entry_min)
            exit_max = np.where(use, np.fmin(exit_max, f), exit_max)
            imax = np.where(use, np.maximum(imax, np.maximum(np.abs(iDl), np.abs(iDh))), imax)
            # The slack term 1e-4 * mag * max |1/D| runs over the axes in use, and doubling the
            # margins takes an axis whose interval nearly reaches 0 out of use: the largest |1/D|
            # of all, gone from the model's slack but not from the builds'.  So the model's max
            # also covers every axis the undoubled rule uses, at the undoubled interval's ends.
            use1 = (Dl1[:, a] > 1e-6 * scale1) | (Dh1[:, a] < -1e-6 * scale1)
            imax = np.where(use1, np.maximum(imax, np.maximum(np.abs(1.0 / Dl1[:, a]), np.abs(1.0 / Dh1[:, a]))), imax)
        abs_slack = 2e-4 * mag * imax + 1e-30
        nan = np.isnan(exit_max) | np.isnan(entry_min) | ~(abs_slack < 1e30)
        behind = exit_max < -2e-4 * np.abs(exit_max) - abs_slack
        apart = entry_min - exit_max > 2e-4 * (np.abs(entry_min) + np.abs(exit_max)) + abs_slack
    return ~skip & ~nan & (behind | apart)


# ---- the sound-side reference -------------------------------------------------------------
def tile_rays(cam, rect):
    """The (m, 6) rays of the rectangle's pixels under TABLE16 (rt.camera_rays on the host)."""
    x0, x1, y0, y1 = rect
    rays, _ = rt.camera_rays(cam, spp=16, jitter=TABLE16, row0=y0, rows=y1 - y0 + 1)
    rays = rays.reshape(y1 - y0 + 1, cam.pixel_width, 16, 6)[:, x0:x1 + 1]
    return np.ascontiguousarray(rays.reshape(-1, 6))


def any_ray_passes(rays, boxes):
    """Per box: some ray passes ref_aabb(ray, box, [1e-4, FLT_MAX])."""
    m, n = rays.shape[0], boxes.shape[0]
    out = np.zeros(n, bool)
    step = max(1, 150000 // m)
    for i in range(0, n, step):
        bb = boxes[i:i + step]
        k = bb.shape[0]
        tmm = np.empty((k * m, 2), F32)
        tmm[:, 0], tmm[:, 1] = TMIN, FLT_MAX
        ok = ref_aabb(np.tile(rays, (k, 1)), np.repeat(bb, m, axis=0), tmm)
        out[i:i + k] = ok.reshape(k, m).any(axis=1)
    return out


# ---- cameras and rectangles -----------------------------------------------------------------
def _cameras(rng, kind):
    """(camera, scale) pairs of one kind of test_gpu_parity._fuzz_cameras around the box
    [-1, 1]^3 * scale + shift: along an axis (a zero direction component in the centre column /
    row), from inside the box, grazing a face, or free; every transform (the scaled ones scale the
    camera's focal length and sensor with the scene), image size and focal length."""
    kind = TILE_CASES.index(kind)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    k = 0
    for (scale, shift) in TRANSFORMS:
        lo, hi = np.full(3, -scale + shift), np.full(3, scale + shift)
        for (W, H) in IMAGES:
            for focal in FOCALS:
                if kind == 0:
                    dirn = axes[k % 6]
                else:
                    dirn = rng.normal(size=3)
                    dirn /= np.linalg.norm(dirn)
                if kind == 1:  # inside the box
                    pos = lo + rng.uniform(0.2, 0.8, size=3) * (hi - lo)
                    target = pos - dirn * scale
                elif kind == 2:  # grazing: along a face, at its height
                    a = k % 3
                    dirn = np.roll(np.array([1.0, 0.3 * rng.normal(), 0.0]), a)
                    dirn /= np.linalg.norm(dirn)
                    target = (lo + hi) / 2
                    target[(a + 2) % 3] = hi[(a + 2) % 3]
                    pos = target + dirn * scale * 4
                else:
                    t = rng.choice([0.0, 1.0, 0.5, rng.uniform()], size=3)
                    target = lo + t * (hi - lo)
                    pos = target + dirn * scale * 2 * rng.choice([0.05, 0.6, 3.0])
                fwd = target - pos
                up = (0.0, 0.0, 1.0) if abs(fwd[2]) < 0.9 * np.linalg.norm(fwd) else (0.0, 1.0, 0.0)
                yield rt.Camera(tuple(pos), tuple(target), up, float(focal) * scale, 24.0 * scale, W, H), scale
                k += 1


def _rects(rng, W, H, k):
    """Three rectangles for a W x H image: x0 = 0, the last columns, and a free position; the
    shapes cycle through RECTS."""
    out = []
    for j in range(3):
        w, h = RECTS[(k + j) % len(RECTS)]
        w, h = min(w, W), min(h, H)
        if j == 0:
            x0 = 0
        elif j == 1:  # ends in one of the last four columns (1916..1919 of 1920, 3836..3839 of 3840)
            x0 = max(0, W - w - int(rng.integers(0, 4)))
        else:
            x0 = int(rng.integers(0, W - w + 1))
        y0 = int(rng.choice([0, H - h, rng.integers(0, H - h + 1)]))
        out.append((x0, x0 + w - 1, y0, y0 + h - 1))
        if (W, H) == (1, 1):
            break
    return out


# ---- boxes ----------------------------------------------------------------------------------
def _perp(rng, d):
    v = rng.normal(size=3)
    v -= d * (v @ d) / (d @ d)
    return v / np.linalg.norm(v)


def _boxes(rng, cam, rect, rays, n, scale):
    """n boxes for one tile: per band and side, a box whose corner sits off a ray of the tile by
    the band's relative offset, along the outward normal of the tile pyramid's face or edge for a
    boundary ray (outside: no ray reaches it; inside: that ray does) or a free perpendicular; flat
    boxes on one, two and three axes through a ray's point; boxes around and behind the camera;
    inverted, NaN and 2^100 boxes; free boxes."""
    c = rays[0, :3].astype(np.float64)
    d = rays[:, 3:].astype(np.float64)
    dmean = d.mean(axis=0)
    dmean /= np.linalg.norm(dmean)
    # boundary rays: the largest angle from the mean direction (pyramid corners), and per image
    # axis the extreme rays (faces)
    b = cam.basis()
    du, dv = b["pixel_delta_u"].astype(np.float64), b["pixel_delta_v"].astype(np.float64)
    su, sv = d @ du, d @ dv
    boxes = np.zeros((n, 6))
    band = np.full(n, -1, np.int64)
    side = np.zeros(n, np.int64)
    for i in range(n):
        kind = i % 18
        r = int(rng.integers(0, d.shape[0]))
        t = scale * float(rng.choice([0.3, 1.0, 2.0, 5.0]) * rng.uniform(0.5, 1.5))
        size = scale * float(rng.choice([1e-3, 0.1, 1.0]))
        if kind < 12:  # bands
            band[i], side[i] = kind // 2, 1 if kind % 2 == 0 else -1
            how = int(rng.integers(0, 6))
            da = d[r]
            if how == 0:  # a face: the extreme ray along +-u or +-v, the normal pointing away
                s, axis = (su, du) if rng.random() < 0.5 else (sv, dv)
                sgn = 1.0 if rng.random() < 0.5 else -1.0
                da = d[int(np.argmax(sgn * s))]
                nrm = sgn * axis - da * (sgn * axis @ da)
            elif how == 1:  # an edge of the pyramid: the corner ray, the normal away from the mean
                da = d[int(np.argmin(d @ dmean))]
                nrm = da - dmean * (da @ dmean) / (dmean @ dmean)
                nrm = nrm - da * (nrm @ da) if np.linalg.norm(nrm) > 0 else _perp(rng, da)
            elif how <= 3:  # a direction of the padded pyramid between the samples, half of them
                # on its face px = x0 - 1 or x1 + 1 (inside offsets there reach no sample's ray)
                x0, x1, y0, y1 = rect
                px, py = rng.uniform(x0 - 1, x1 + 1), rng.uniform(y0 - 1, y1 + 1)
                sgn = 1.0 if rng.random() < 0.5 else -1.0
                if how == 2:
                    px = x1 + 1 if sgn > 0 else x0 - 1
                da = b["pixel00_loc"].astype(np.float64) + px * du + py * dv - c
                da /= np.linalg.norm(da)
                nrm = sgn * du - da * (sgn * du @ da) if how == 2 else _perp(rng, da)
            else:
                nrm = _perp(rng, da)
            nn = np.linalg.norm(nrm)
            nrm = nrm / nn if nn > 0 else _perp(rng, da)
            q = c + t * da
            corner = q + side[i] * BANDS[band[i]] * t * nrm
            sg = np.where(nrm >= 0, 1.0, -1.0)
            boxes[i, :3], boxes[i, 3:] = np.minimum(corner, corner + sg * size), np.maximum(corner, corner + sg * size)
        elif kind == 12:  # flat on 1, 2 or 3 axes, through a point of a ray or just off it
            q = c + t * d[r] + _perp(rng, d[r]) * t * float(rng.choice([0.0, 1e-6, 1e-3, 1e-1]))
            flat = rng.random(3).argsort() < rng.integers(1, 4)
            h = np.where(flat, 0.0, size)
            boxes[i, :3], boxes[i, 3:] = q - h, q + h
        elif kind == 13:  # around the camera, or just beside it
            off = _perp(rng, dmean) * size * float(rng.choice([0.0, 0.5, 0.9999, 1.0001, 1.5]))
            boxes[i, :3], boxes[i, 3:] = c + off - size, c + off + size
        elif kind == 14:  # behind the camera
            q = c - t * d[r]
            boxes[i, :3], boxes[i, 3:] = q - size, q + size * float(rng.choice([1.0, 0.0]))
        elif kind == 15:  # inverted on an axis, or a NaN coordinate
            q = c + t * d[r]
            boxes[i, :3], boxes[i, 3:] = q - size, q + size
            a = int(rng.integers(0, 3))
            if rng.random() < 0.5:
                boxes[i, a], boxes[i, 3 + a] = boxes[i, 3 + a], boxes[i, a]
            else:
                boxes[i, int(rng.integers(0, 6))] = np.nan
        elif kind == 16:  # a coordinate of 2^100: never culled
            q = c + t * d[r] + _perp(rng, d[r]) * t * float(rng.choice([0.0, 0.5, 3.0]))
            boxes[i, :3], boxes[i, 3:] = q - size, q + size
            a = int(rng.integers(0, 3))
            if rng.random() < 0.5:
                boxes[i, 3 + a] = 2.0 ** 100
            else:
                boxes[i, a] = -2.0 ** 100
        else:  # free
            q = c + t * (dmean + rng.normal(size=3) * float(rng.choice([0.01, 0.3, 2.0])))
            h = np.abs(rng.normal(size=3)) * size
            boxes[i, :3], boxes[i, 3:] = q - h, q + h
    return np.ascontiguousarray(boxes, F32), band, side


@lru_cache(maxsize=None)
def tile_case(name: str) -> tuple:
    rng = np.random.default_rng([31, TILE_CASES.index(name)])
    groups = []
    for k, (cam, scale) in enumerate(_cameras(rng, name)):
        for rect in _rects(rng, cam.pixel_width, cam.pixel_height, k):
            rays = tile_rays(cam, rect)
            nb = BOXES_PER_GROUP if rays.shape[0] <= 256 else BOXES_PER_GROUP // 2
            boxes, band, side = _boxes(rng, cam, rect, rays, nb, scale)
            tiles = np.ascontiguousarray(np.tile(np.array(rect, np.int32), (nb, 1)))
            g = {"cam": cam, "rect": rect, "tiles": tiles, "boxes": boxes, "band": band, "side": side,
                 "any_pass": any_ray_passes(rays, boxes), "model_cull": model_cull(cam, tiles, boxes)}
            for v in g.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            groups.append(g)
    return tuple(groups)


def gather(groups, key):
    return np.concatenate([g[key] for g in groups])


def run_groups(fn, groups):
    """fn(cam, tiles, boxes) -> (n,) int32 per group, concatenated."""
    return np.concatenate([fn(g["cam"], g["tiles"], g["boxes"]) for g in groups])


def describe(groups, idx, limit=5):
    """The first `limit` items of the flat indices idx: camera basis, rectangle and box as hex floats."""
    sizes = np.cumsum([0] + [g["tiles"].shape[0] for g in groups])
    out = []
    for i in np.asarray(idx)[:limit]:
        gi = int(np.searchsorted(sizes, i, side="right") - 1)
        g, j = groups[gi], int(i - sizes[gi])
        basis = {k: [float(x).hex() for x in v] for k, v in g["cam"].basis().items()}
        out.append("item %d (group %d, %dx%d image): rect %s box %s camera %s" % (
            i, gi, g["cam"].pixel_width, g["cam"].pixel_height, g["rect"],
            [float(x).hex() for x in g["boxes"][j]], basis))
    return "\n".join(out)


def shares(groups, got):
    """Of the all-rays-miss items: the share the build culls and the share the model culls."""
    miss = ~gather(groups, "any_pass")
    return float(got[miss].mean()), float(gather(groups, "model_cull")[miss].mean())


# ---- what both builds must satisfy (the host tests and the GPU tests call these) -------------
def host_fn(cam, tiles, boxes, n=None):
    import ctypes as C

    from raytracinginonesemester_amd import _lib

    n = tiles.shape[0] if n is None else n
    out = np.full(n, -1, np.int32)
    _lib.check(_lib.lib().rt_debug_tile_test_host(C.byref(cam.c), tiles.ctypes.data, boxes.ctypes.data, n, out.ctypes.data))
    return out


def device_fn(cam, tiles, boxes, n=None):
    import ctypes as C

    from raytracinginonesemester_amd import _lib

    n = tiles.shape[0] if n is None else n
    out = np.full(n, -1, np.int32)
    _lib.check(_lib.lib().rt_debug_tile_test_batch(0, C.byref(cam.c), tiles.ctypes.data, boxes.ctypes.data, n,
                                                   out.ctypes.data))
    return out


def check_set(fn, name):
    """Both sides on one set; prints the culled shares (not asserted)."""
    groups = tile_case(name)
    got = run_groups(fn, groups)
    assert np.isin(got, (0, 1)).all()
    any_pass, model = gather(groups, "any_pass"), gather(groups, "model_cull")
    bad = np.flatnonzero(any_pass & (got == 1))
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} items culled although a ray of the tile passes "
                           f"the box\n" + describe(groups, bad))
    bad = np.flatnonzero(model & (got == 0))
    assert bad.size == 0, (f"{name}: {bad.size} of {got.size} items kept although the doubled-margin model "
                           f"culls them\n" + describe(groups, bad))
    dev, mod = shares(groups, got)
    print(f"{name}: {got.size} items in {len(groups)} groups, all-rays-miss {float((~any_pass).mean()):.3f}; "
          f"of those culled: build {dev:.4f}, model {mod:.4f}")
    big = np.abs(gather(groups, "boxes")).max(axis=1) >= 2.0 ** 100
    assert big.any() and not got[big].any()
    return got


def check_short_batches(fn, name="axis"):
    """1, 63 and 65 items of a group (n below the arrays' length: nothing is written past n)."""
    for g in tile_case(name)[:6]:
        reps = -(-65 // g["tiles"].shape[0])
        tiles = np.ascontiguousarray(np.tile(g["tiles"], (reps, 1)))
        boxes = np.ascontiguousarray(np.tile(g["boxes"], (reps, 1)))
        full = fn(g["cam"], tiles, boxes)
        for n in (1, 63, 65):
            assert np.array_equal(fn(g["cam"], tiles, boxes, n), full[:n]), n


# ---- degenerate cameras (tests/camera_cases.py): sound side only -----------------------------
# The tile test takes every ray direction for a positive multiple of D = pixel00 + px du + py dv
# - center; get_ray's direction is that only while 1e-12 <= |D| <= ~1.8e19.
# These sets hold the test, as a frame runs it (behind the camera's class), against the rays of
# cameras outside that range.  No tight side: such a camera is not culled at all.
CAMERA_TILE_CASES = ("fallback", "threshold", "overflow", "nonfinite")


def _camera_boxes(rng, c, n_random=24):
    """The scene's root and the boxes of its first tree levels (what a cut is made of), then boxes
    on all sides of the camera: at distances 0.5 to 4 along the six axes and along random
    directions, sized 0.05 to 1."""
    import camera_cases as cc

    aabbs = np.asarray(cc.scene(c["scene"])["aabbs"], F32).reshape(-1, 6)
    boxes = [aabbs[:31]]
    ctr = c["cam"].basis()["center"].astype(np.float64)
    ctr = np.where(np.isfinite(ctr) & (np.abs(ctr) < 1e6), ctr, 0.0)
    dirs = np.concatenate([np.eye(3), -np.eye(3), rng.normal(size=(n_random - 6, 3))])
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    q = ctr + dirs * rng.choice([0.5, 1.0, 2.0, 4.0], size=(n_random, 1))
    h = rng.choice([0.05, 0.3, 1.0], size=(n_random, 1)) * rng.uniform(0.5, 1.0, size=(n_random, 3))
    boxes.append(np.concatenate([q - h, q + h], axis=1).astype(F32))
    return np.ascontiguousarray(np.concatenate(boxes), F32)


@lru_cache(maxsize=None)
def camera_tile_case(name: str) -> tuple:
    import camera_cases as cc

    rng = np.random.default_rng([33, CAMERA_TILE_CASES.index(name)])
    groups = []
    for cname in cc.names_of(name):
        c = cc.case(cname)
        W, H = c["W"], c["H"]
        rects = {(0, min(7, W - 1), 0, min(7, H - 1)), (max(0, W - 8), W - 1, max(0, H - 8), H - 1),
                 (W // 2, W // 2, H // 2, H // 2), (0, W - 1, 0, 0)}
        for rect in sorted(rects):
            rays = tile_rays(c["cam"], rect)
            boxes = _camera_boxes(rng, c)
            tiles = np.ascontiguousarray(np.tile(np.array(rect, np.int32), (boxes.shape[0], 1)))
            finite = np.isfinite(rays).all(axis=1)
            # a non-finite ray counts as passing every box: every compare of the reference's is false
            any_pass = np.ones(boxes.shape[0], bool) if not finite.all() else any_ray_passes(rays, boxes)
            if not finite.all() and finite.any():
                any_pass |= any_ray_passes(rays[finite], boxes)
            g = {"cam": c["cam"], "case": cname, "rect": rect, "tiles": tiles, "boxes": boxes, "any_pass": any_pass}
            for v in g.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            groups.append(g)
    return tuple(groups)


def check_camera_set(fn, name):
    """Sound side: nothing culled where a ray of the tile passes the box.  Returns the cases with
    an unsound item (empty when the set passes) after printing the counts."""
    groups = camera_tile_case(name)
    got = run_groups(fn, groups)
    assert np.isin(got, (0, 1)).all()
    any_pass = gather(groups, "any_pass")
    bad = any_pass & (got == 1)
    sizes = np.cumsum([0] + [g["tiles"].shape[0] for g in groups])
    bad_cases = sorted({g["case"] for i, g in enumerate(groups) if bad[sizes[i]:sizes[i + 1]].any()})
    print(f"{name}: {got.size} items in {len(groups)} groups, some ray passes {float(any_pass.mean()):.3f}, culled "
          f"{int(got.sum())}, culled although a ray passes {int(bad.sum())} in cases {bad_cases}")
    assert any_pass.any()
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {got.size} items culled although a ray of the tile passes the "
                           f"box, in cases {bad_cases}\n" + describe(groups, np.flatnonzero(bad)))
    return got
