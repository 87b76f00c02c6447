"""The coherence key of a caller ray restated in float32 numpy, and the special rays and boxes of the
ray-sort tests (rt_ray_*), a helper module: no tests here (TEST DATA GENERATOR)."""
from __future__ import annotations

import numpy as np

import ray_batches as rb

F = np.float32
BITS = {"origin": (1, 2, 5, 10), "origin_dir": (1, 2, 5)}
CASES = [(m, b) for m in BITS for b in BITS[m]]


# ---- the key, restated ------------------------------------------------------------------------------
def np_clamp_cell(t, b):
    """q = t >= 0 ? t : 0 (NaN gives 0); q = q <= 2^b - 1 ? q : 2^b - 1; (uint32)q."""
    assert t.dtype == F
    top = F(2 ** b - 1)
    q = np.where(t >= F(0), t, F(0))
    q = np.where(q <= top, q, top)
    assert q.dtype == F
    return q.astype(np.uint32)


def np_keys(rays, box, mode, b):
    """The key of include/rt_mi355x.h in float32 numpy, one operation per operator, left to right."""
    rays = np.ascontiguousarray(rays, F)
    box = np.asarray(box, F).reshape(6)
    scale = F(2 ** b)
    cells = []
    with np.errstate(all="ignore"):
        for k in range(3):
            x, lo, hi = rays[:, k], box[k], box[3 + k]
            cells.append(np_clamp_cell(((x - lo) / (hi - lo)) * scale, b))
        if mode == "origin_dir":
            dx, dy, dz = rays[:, 3], rays[:, 4], rays[:, 5]
            ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
            assert ln.dtype == F
            for d in (dx, dy, dz):
                u = d / ln
                cells.append(np_clamp_cell(((u + F(1.0)) * F(0.5)) * scale, b))
    key = np.zeros(rays.shape[0], np.uint32)
    for j in range(b - 1, -1, -1):
        for c in cells:
            key = (key << np.uint32(1)) | ((c >> np.uint32(j)) & np.uint32(1))
    return key


def half_box(box):
    """A box of half the size about the same centre: the batches' origins (up to two half extents
    out) clamp on both sides of every axis."""
    box = np.asarray(box, F).reshape(6)
    c, h = (box[:3] + box[3:]) * F(0.5), (box[3:] - box[:3]) * F(0.25)
    return np.concatenate([c - h, c + h]).astype(F)


def root_box(name):
    return np.ascontiguousarray(rb.scene_arrays(name)["aabbs"], F).reshape(-1, 6)[0].copy()



INF, NAN = F(np.inf), F(np.nan)
BIG = F(1e30)  # its square overflows float32
SPECIAL_RAYS = np.array([
    [NAN, 0.5, 0.5, 0, 0, 1], [0.5, NAN, NAN, 0, 1, 0], [INF, 0.5, 0.5, 1, 0, 0], [-INF, 0.5, 0.5, 1, 0, 0],
    [0.5, INF, -INF, 0, 0, -1], [-0.0, -0.0, -0.0, -0.0, -0.0, 1], [0.0, 0.0, 0.0, 1, 1, 1], [1.0, 1.0, 1.0, -1, -1, -1],
    [0.25, 0.5, 0.75, 0, 0, 0], [0.25, 0.5, 0.75, -0.0, 0.0, -0.0], [0.5, 0.5, 0.5, BIG, 1, 1], [0.5, 0.5, 0.5, BIG, -BIG, BIG],
    [0.5, 0.5, 0.5, NAN, 1, 0], [0.5, 0.5, 0.5, INF, 0, 0], [0.5, 0.5, 0.5, -INF, INF, 1], [0.5, 0.5, 0.5, 1e-30, 1e-30, 1e-30],
    [0.5, 0.5, 0.5, 1e-42, 0, 0], [2.0, -1.0, 0.999999, 0.6, 0, 0.8], [0.999, 1e-9, 0.5, -0.6, 0.8, 0], [3e38, -3e38, 0.5, 0, 1, 0],
], F)
SPECIAL_BOXES = {
    "unit": [0, 0, 0, 1, 1, 1],
    "flat_x": [0.5, 0, 0, 0.5, 1, 1],        # 0 / 0 on x for x = 0.5, x / 0 elsewhere
    "flat_all": [0.5, 0.5, 0.5, 0.5, 0.5, 0.5],
    "inverted": [1, 1, 1, 0, 0, 0],
    "empty": [INF, INF, INF, -INF, -INF, -INF],  # a scene without triangles
    "nan": [NAN, 0, 0, 1, NAN, 1],
    "huge": [-3e38, -3e38, -3e38, 3e38, 3e38, 3e38],  # hi - lo overflows
}
