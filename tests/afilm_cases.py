"""Cases and restatements for the adaptive film tests (rt_afilm_*, rt_camera_rays_pixels_*;
DESIGN.md §4.22), a helper module: no tests here (TEST DATA GENERATOR).

``Model`` is the numpy restatement of the film: float32 sums by film_cases.pixel_sums' loop, float32
luminance moments, uint32 counts, shade_rays_cases.pixel_sum's division with each pixel's own count,
and the selection rule in float64.  tests/test_afilm_host.py pins the host build (rt_afilm_host)
against it, so the GPU tests may compare the kernels with the host build.  ``oracle_adaptive`` runs
the whole adaptive loop on the CPU from the oracle's per-sample radiance through the host build.
"""
from __future__ import annotations

import numpy as np

import film_cases as fc

F = np.float32
D = np.float64
W_SMALL, H_SMALL = fc.W_SMALL, fc.H_SMALL
COUNTS = (0, 1, 5, 15)           # the per-pixel counts of the ray tests
PIXEL_NONE = 0xFFFFFFFF


def luma(r):
    """(..., 3) float32 -> the sample luminance, float multiplies and adds in the film's order."""
    r = np.ascontiguousarray(r, F)
    y = (F(0.2126) * r[..., 0] + F(0.7152) * r[..., 1]) + F(0.0722) * r[..., 2]
    assert y.dtype == F
    return y


def noisy(count, m1, m2, tol, floor):
    """The criterion in float64 from the float32 accumulators, item for item."""
    n = np.asarray(count).astype(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.asarray(m1, F).astype(D) / n
        d = np.asarray(m2, F).astype(D) / n - mean * mean
        var = (np.where(d > 0.0, d, 0.0) * n) / (n - 1.0)
        lim = D(tol) * np.where(mean > D(floor), mean, D(floor))
        out = var / n > lim * lim
    return np.where(np.asarray(count) < 2, True, out)


def selected(count, m1, m2, min_spp, max_spp, step, tol, floor=1e-3):
    """Indices of the selected pixels, increasing."""
    c = np.asarray(count).astype(np.int64)
    keep = (c + step <= max_spp) & ((c < min_spp) | noisy(count, m1, m2, tol, floor))
    return np.flatnonzero(keep).astype(np.uint32)


class Model:
    """The numpy restatement of an adaptive film of W x H pixels."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.sum = np.zeros((W * H, 3), F)
        self.count = np.zeros(W * H, np.uint32)
        self.m1 = np.zeros(W * H, F)
        self.m2 = np.zeros(W * H, F)

    def add(self, pixels, rad):
        """rad: (m, n, 3) float32 for the m listed pixels (None: all, in order)."""
        rad = np.ascontiguousarray(rad, F)
        m, n, _ = rad.shape
        px = np.arange(self.W * self.H, dtype=np.uint32) if pixels is None else np.asarray(pixels, np.uint32)
        ok = px < self.W * self.H
        px, rad = px[ok], rad[ok]
        assert np.unique(px).size == px.size
        # film_cases.pixel_sums' loop, started from the running sums
        acc = self.sum[px]
        m1, m2 = self.m1[px], self.m2[px]
        for s in range(n):
            acc = acc + rad[:, s, :]
            y = luma(rad[:, s, :])
            m1 = m1 + y
            m2 = m2 + y * y
        assert acc.dtype == F and m1.dtype == F and m2.dtype == F
        self.sum[px], self.m1[px], self.m2[px] = acc, m1, m2
        self.count[px] += np.uint32(n)

    def rgb(self):
        """shade_rays_cases.pixel_sum's division with the pixel's own count; no samples: 0."""
        c = self.count.astype(F).astype(D)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (self.sum.astype(D) / c).astype(F)
        q[self.count == 0] = F(0.0)
        return q.reshape(self.H, self.W, 3)

    def selected(self, min_spp, max_spp, step, tol, floor=1e-3):
        return selected(self.count, self.m1, self.m2, min_spp, max_spp, step, tol, floor)

    def state(self):
        """Copies in rt_afilm_host's layout: (sums, counts, moments)."""
        return (self.sum.reshape(-1).copy(), self.count.copy(),
                np.ascontiguousarray(np.stack([self.m1, self.m2], axis=1)).reshape(-1).copy())


# The adds of the uneven-count tests: (pixel-list kind, nsamples, seed) in order.  "dense" is the
# NULL list, "perm" a shuffled full list, "sparse" 65 shuffled pixels, "none" a sparse list with
# one RT_PIXEL_NONE and one W*H entry (both skipped).
ADDS = (("dense", 2, 11), ("sparse", 1, 12), ("perm", 3, 13), ("sparse", 5, 14), ("none", 16, 15), ("sparse", 17, 16))


def pixel_list(kind, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "dense":
        return None
    if kind == "perm":
        return rng.permutation(W * H).astype(np.uint32)
    px = rng.permutation(W * H)[:min(65, W * H)].astype(np.uint32)
    if kind == "none" and px.size >= 3:
        px[1], px[-1] = PIXEL_NONE, W * H
    return px


def list_radiance(m, n, seed):
    """(m, n, 3) float32 from film_cases.make_radiance's mix of values."""
    return np.ascontiguousarray(fc.make_radiance(m, 1, n, seed)[0])


def random_accumulators(npix, seed, max_count=20):
    """Counts in [0, max_count] and the moments of that many luminances: a third of the pixels
    constant (never noisy), the rest uniform."""
    rng = np.random.default_rng(seed)
    count = rng.integers(0, max_count + 1, npix).astype(np.uint32)
    m1, m2 = np.zeros(npix, F), np.zeros(npix, F)
    const = rng.integers(0, 3, npix) == 0
    base = rng.random(npix, dtype=F)
    for s in range(max_count):
        y = np.where(const, base, rng.random(npix, dtype=F)).astype(F)
        on = count > s
        m1 = np.where(on, m1 + y, m1).astype(F)
        m2 = np.where(on, m2 + y * y, m2).astype(F)
    return count, m1, m2, const


def oracle_adaptive(hs, cam, min_spp, max_spp, step, tol, floor=1e-3, miss=(0, 0, 0)):
    """The adaptive frame at depth 1 on the CPU: per-sample radiance from the oracle's render_g
    (spp = 1 with row s of the frame's jitter table: the pixel of one sample is the sample; at depth 1
    no random number is drawn), fed through the host build of add / select / resolve exactly as
    DeviceScene.render_adaptive feeds the device.  Returns (rgb (H, W, 3), counts (H, W) uint32, P6 bytes (H, W, 3))."""
    import raytracinginonesemester_amd as rt
    from conftest import oracle_camera
    from oracle import pyoracle as orc

    W, H = cam.pixel_width, cam.pixel_height
    oc = oracle_camera(cam)
    table = rt.jittered_samples(max_spp)
    samples = np.stack([orc.render_g(hs.num_triangles, oc, hs.nodes, hs.aabbs, hs.triangles, hs.tri_object_ids,
                                     hs.materials, hs.lights, spp=1, max_depth=1, miss=miss, jitter_tab=table[s:s + 1])
                        for s in range(max_spp)], axis=2).reshape(W * H, max_spp, 3)
    out = rt.afilm_host(W, H, radiance=np.ascontiguousarray(samples[:, :min_spp]), nsamples=min_spp,
                        select=(min_spp, max_spp, step, tol, floor))
    state = out["state"]
    while out["selected"].size:
        px = out["selected"]
        c = state[1][px]
        rad = np.stack([samples[px, c + s] for s in range(step)], axis=1)
        out = rt.afilm_host(W, H, state, np.ascontiguousarray(rad), px, step, select=(min_spp, max_spp, step, tol, floor))
    out = rt.afilm_host(W, H, state, resolve=True)
    return out["rgb"], state[1].reshape(H, W).copy(), out["bytes"]
