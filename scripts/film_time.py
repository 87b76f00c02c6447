"""Time the film kernels (rt_film_add_device, rt_film_resolve_device) at
1920x1080 with n = 1, 4 and 16 samples per pixel, beside rt_ppm_quantize_device on the same frame
in the same process as the streaming yardstick.  Each figure is the HIP-event median of --reps
launches after --warmup; GB/s is the bytes the algorithm moves (computed from the shapes below) over
that time.  The 16-byte aligned radiance takes film_add_vec_kernel, the same table 4 bytes further
film_add_any_kernel.  Every timed film is also checked against the host build on a 64-row band.

    python scripts/film_time.py [--reps 10] [--warmup 3] [--width 1920] [--height 1080]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytracinginonesemester_amd as rt  # noqa: E402
from raytracinginonesemester_amd import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
a = ap.parse_args()
W, H = a.width, a.height
dev = torch.device("cuda", 0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lib = L.lib()


def median_ms(call):
    ms = []
    for _ in range(a.warmup + a.reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[a.warmup:]
    return float(np.median(ms)), float(min(ms))


def row(what, nbytes, call, **more):
    med, lo = median_ms(call)
    print(json.dumps({"what": what, "width": W, "height": H, **more, "bytes": nbytes, "ms_median": round(med, 4),
                      "ms_min": round(lo, 4), "gb_per_s": round(nbytes / med / 1e6, 1)}), flush=True)


px = W * H
film = rt.Film(W, H)
rgb = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
p6 = torch.empty(px * 3 + 16, dtype=torch.uint8, device=dev)  # (room for the output one byte off alignment)
band = min(64, H)
for n in (1, 4, 16):
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    buf = torch.rand(px * n * 3 + 4, dtype=torch.float32, device=dev, generator=gen)
    for off, kernel in ((0, "film_add_vec_kernel"), (1, "film_add_any_kernel")):
        rad = buf[off:off + px * n * 3]
        assert rad.data_ptr() % 16 == 4 * off
        # check first: one add of the frame against the host build on a band
        film.clear()
        L.check(lib.rt_film_add_device(film._h, rad.data_ptr(), 0, H, n, None))
        got = film.resolve(0, band).cpu().numpy()
        _, want = rt.film_pixels_host(rad[:band * W * n * 3].cpu().numpy(), W, band, n)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, kernel)
        # per pixel: 12 n bytes of radiance in, 12 of sums in and 12 out
        row("film_add", px * (12 * n + 24), lambda: L.check(lib.rt_film_add_device(film._h, rad.data_ptr(), 0, H, n, None)),
            n=n, kernel=kernel)
    del buf
    # (the sums keep growing over the timed adds: resolve's time does not depend on their values)
    sums_in = px * 12
    for what, r_ptr, b_ptr, out in (("film_resolve rgb + p6", rgb.data_ptr(), p6.data_ptr(), px * 15),
                                    ("film_resolve rgb", rgb.data_ptr(), None, px * 12),
                                    ("film_resolve p6", None, p6.data_ptr(), px * 3)):
        row(what, sums_in + out, lambda: L.check(lib.rt_film_resolve_device(film._h, 0, H, r_ptr, b_ptr, None)),
            count=film.row_samples(0), kernel="film_resolve_vec_kernel")
    if n == 16:
        row("film_resolve rgb + p6", sums_in + px * 15,
            lambda: L.check(lib.rt_film_resolve_device(film._h, 0, H, rgb.data_ptr(), p6.data_ptr() + 1, None)),
            count=film.row_samples(0), kernel="film_resolve_any_kernel")
# the yardstick: the quantise kernel on the resolved frame, 12 bytes in and 3 out per pixel
L.check(lib.rt_film_resolve_device(film._h, 0, H, rgb.data_ptr(), None, None))
row("rt_ppm_quantize_device", px * 15, lambda: rt.quantize_p6_device(rgb.data_ptr(), W, H, p6.data_ptr()),
    kernel="quantize_vec_kernel<1>")
film.close()
