"""Time adaptive sampling (DeviceScene.render_adaptive, rt_afilm_*, rt_camera_rays_pixels_device;
DESIGN.md §4.22) on the frog scene at 1920x1080, depth 1, min 4 / max 16 / step 4, beside render_rays
at 16 spp on the same scene in the same process.  Whole frames are HIP-event medians of --reps runs
after --warmup on one stream; render_adaptive reads one word per pass, so its figure includes those
waits.  The per-pass figures replay each pass of one adaptive frame: select, the ray generator, the
shading and the add are timed alone on the pass's own pixel list, median of --reps.

    python scripts/afilm_time.py [--reps 20] [--warmup 3] [--width 1920] [--height 1080] [--tol 0.1]
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--tol", type=float, default=0.1)
ap.add_argument("--min", type=int, default=4)
ap.add_argument("--max", type=int, default=16)
ap.add_argument("--step", type=int, default=4)
a = ap.parse_args()
W, H = a.width, a.height
dev = torch.device("cuda", 0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def median_ms(call):
    ms = []
    for _ in range(a.warmup + a.reps):
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms[a.warmup:])), 4)


hs = rt.HostScene.load_json(REPO / "assets" / "scenes" / "frog.json", REPO)
cam = hs.camera(W, H)
ds = rt.DeviceScene.from_host(hs, device=0)
miss = hs.settings["miss_color"]
common = {"width": W, "height": H, "scene": "frog", "max_depth": 1}

rgb, cnt = ds.render_adaptive(cam, a.min, a.max, a.step, a.tol, miss_color=miss)
v, c = torch.unique(cnt, return_counts=True)
hist = dict(zip(v.tolist(), c.tolist()))
samples = int(cnt.sum().item())
print(json.dumps({"what": "count histogram", **common, "min": a.min, "max": a.max, "step": a.step, "tol": a.tol, "hist": hist,
                  "samples": samples, "samples_saved_frac": round(1.0 - samples / (W * H * a.max), 4)}), flush=True)
full = ds.render_rays(cam, a.max, 1, True, miss)
at = cnt == a.max
assert torch.equal(rgb.view(torch.int32)[at], full.view(torch.int32)[at])  # the pixels that went all the way
del full, rgb

print(json.dumps({"what": "render_adaptive", **common, "tol": a.tol,
                  "ms_median": median_ms(lambda: ds.render_adaptive(cam, a.min, a.max, a.step, a.tol, miss_color=miss))}), flush=True)
print(json.dumps({"what": "render_rays", **common, "spp": a.max,
                  "ms_median": median_ms(lambda: ds.render_rays(cam, a.max, 1, True, miss))}), flush=True)
print(json.dumps({"what": "render", **common, "spp": a.max,
                  "ms_median": median_ms(lambda: ds.render(cam, spp=a.max, max_depth=1, miss_color=miss))}), flush=True)

# the passes of one frame, each stage alone
jd = torch.from_numpy(rt.jittered_samples(a.max)).to(dev)
with rt.AdaptiveFilm(W, H) as film:
    pixels, n, k = None, a.min, 0
    while True:
        m = W * H if pixels is None else int(pixels.shape[0])
        rays, seeds = rt.camera_rays_pixels(cam, pixels, film, n, jd, device=0)
        rad = ds.shade_rays(rays, seeds, 1, True, miss)
        row = {"what": "pass", **common, "pass": k, "pixels": m, "nsamples": n,
               "rays_ms": median_ms(lambda: rt.camera_rays_pixels(cam, pixels, film, n, jd, device=0)),
               "shade_ms": median_ms(lambda: ds.shade_rays(rays, seeds, 1, True, miss))}
        with rt.AdaptiveFilm(W, H) as spare:  # (timed adds go to a film of their own: this one's sums stay the frame's)
            row["add_ms"] = median_ms(lambda: spare.add(rad, pixels, n))
        film.add(rad, pixels, n)
        row["select_ms"] = median_ms(lambda: film.select(a.min, a.max, a.step, a.tol))
        row["overhead_ms"] = round(row["rays_ms"] + row["add_ms"] + row["select_ms"], 4)
        print(json.dumps(row), flush=True)
        pixels, m = film.select(a.min, a.max, a.step, a.tol)
        if m == 0:
            break
        n, k = a.step, k + 1
ds.close()
