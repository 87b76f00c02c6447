"""Radiance frames and references for the film tests (rt_film_*), a helper module: no tests here
(TEST DATA GENERATOR).

``radiance`` makes the random sample tables of tests/test_film_host.py and tests/test_gpu_film.py;
``reference`` is shade_rays_cases.pixel_sum's restatement of render()'s pixel, with the sums beside
it.  tests/test_film_host.py pins the host build (rt_film_pixels_host) against it, so the GPU tests
may compare the kernels with the host build.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import shade_rays_cases as sc

F = np.float32
W_SMALL, H_SMALL = 61, 7          # odd sizes: no span of the image is a multiple of a vector
NS_HOST = (1, 2, 3, 5, 16, 17)
NS_GPU = (1, 2, 3, 4, 5, 16, 17)
# default_rng seeds of the (61, 7, n) tables: the first of 1, 2, ... for which reversing the sample
# order changes at least 16 pixels (n >= 3: two floats add to the same sum in either order);
# found on the CPU, asserted by tests/test_film_host.py
SEEDS = {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 16: 1, 17: 1}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def make_radiance(W, rows, n, seed):
    """(rows, W, n, 3) float32 in [0, 1]: uniform values with exact 0 and 1 (about one sample in 16
    each) and a few subnormals mixed in."""
    rng = np.random.default_rng(seed)
    r = rng.random((rows, W, n, 3), dtype=F)
    kind = rng.integers(0, 64, r.shape)
    r[kind < 4] = F(0.0)
    r[(kind >= 4) & (kind < 8)] = F(1.0)
    sub = kind == 8
    r[sub] = (rng.integers(1, 1 << 23, int(sub.sum())).astype(np.uint32)).view(F)  # subnormal bit patterns
    assert r.dtype == F and r.min() >= 0.0 and r.max() <= 1.0
    return r


@lru_cache(maxsize=None)
def radiance(W, rows, n, seed=None):
    """The shared, read-only table of a shape (seed: SEEDS[n] by default)."""
    r = make_radiance(W, rows, n, SEEDS[n] if seed is None else seed)
    r.setflags(write=False)
    return r


def pixel_sums(r):
    """col = col + sample in sample order in float32 (pixel_sum's loop): (rows, W, 3)."""
    acc = np.zeros(r.shape[:2] + (3,), F)
    for s in range(r.shape[2]):
        acc = acc + r[:, :, s, :]
    assert acc.dtype == F
    return acc


def reference(r):
    """(sums, pixels) of a (rows, W, n, 3) table by shade_rays_cases.pixel_sum's arithmetic."""
    rows, W, n, _ = r.shape
    return pixel_sums(r), sc.pixel_sum(r, rows, W, n)
