"""Time the radiance queries (rt_shade_rays) on frog: the c3 camera's rays at
1920x1080x1 spp, made on the host, shaded at depth 1 and at frog.json's own depth 8.  kernel_ms
is the median of --reps launches after --warmup.  Beside them, on the same rays and frame:
rt_trace_rays closest hit (the first segment alone, a lower bound) and the render kernel's time
for that frame at 1 spp (the camera path: wave traversals, tile culling).

    python scripts/shade_rays_time.py [--reps 10] [--warmup 3]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np  # noqa: E402

import raytracinginonesemester_amd as rt  # noqa: E402
from raytracinginonesemester_amd import configs  # noqa: E402

F = np.float32


def camera_rays(basis, W, H, jitter):
    """Camera::get_ray per sample in float32, order (y, x, s); seeds as render() makes them."""
    c, p00, du, dv = (np.asarray(basis[k], F) for k in ("center", "pixel00_loc", "pixel_delta_u", "pixel_delta_v"))
    jit = np.ascontiguousarray(jitter, F).reshape(-1, 2)
    spp = jit.shape[0]
    px = np.broadcast_to(np.arange(W, dtype=F)[None, :, None] + jit[None, None, :, 0], (H, W, spp))
    py = np.broadcast_to(np.arange(H, dtype=F)[:, None, None] + jit[None, None, :, 1], (H, W, spp))
    v = ((p00 + du * px[..., None]) + dv * py[..., None] - c).reshape(-1, 3)
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    d = (v.astype(np.float64) / ln.astype(np.float64)[:, None]).astype(F)
    y, x, s = (a.reshape(-1).astype(np.uint64) for a in np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij"))
    m = np.uint64(0xFFFFFFFF)
    seeds = ((x * np.uint64(73856093)) & m) ^ ((y * np.uint64(19349663)) & m) ^ ((s * np.uint64(83492791)) & m)
    return np.ascontiguousarray(np.hstack([np.broadcast_to(c, d.shape), d]), F), seeds.astype(np.uint32)


def median_ms(call, reps, warmup):
    ms = [call() for _ in range(warmup + reps)][warmup:]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
cfg = configs.G_CONFIGS["c3"]
hs = rt.HostScene.load_json(configs.scene_path(cfg["scene"]), REPO)
W, H = cfg["width"], cfg["height"]
cam = hs.camera(W, H)
miss = hs.settings["miss_color"]
rays, seeds = camera_rays(cam.basis(), W, H, rt.jittered_samples(1))
ds = rt.DeviceScene.from_host(hs, device=0)
n = rays.shape[0]
med, lo = median_ms(lambda: ds.trace_rays(rays, timing=True)[1], a.reps, a.warmup)
idx, _ = ds.trace_rays(rays)
print(json.dumps({"what": "trace_rays closest", "rays": n, "hit_fraction": round(float((idx >= 0).mean()), 4),
                  "kernel_ms_median": med, "kernel_ms_min": lo, "mrays_per_s": round(n / med / 1e3, 1)}), flush=True)
for depth in (1, hs.settings["max_depth"]):
    for flags, variant in ((0, "wide"), (rt.RT_FLAG_BINARY, "binary")):
        kw = dict(max_depth=depth, diffuse_bounce=hs.settings["diffuse_bounce"], miss_color=miss, flags=flags)
        med, lo = median_ms(lambda: ds.shade_rays(rays, seeds, timing=True, **kw)[1], a.reps, a.warmup)
        assert ds.shade_rays_variant() == (rt.RT_RAYS_VARIANT_BINARY if flags else rt.RT_RAYS_VARIANT_WIDE)
        rad = ds.shade_rays(rays, seeds, **kw)

        def frame_ms():
            ds.render(cam, spp=1, max_depth=depth, diffuse_bounce=hs.settings["diffuse_bounce"], miss_color=miss, flags=flags)
            return float(ds.kernel_times(1)[-1])

        fmed, flo = median_ms(frame_ms, a.reps, a.warmup)
        frame = ds.render(cam, spp=1, max_depth=depth, diffuse_bounce=hs.settings["diffuse_bounce"], miss_color=miss, flags=flags)
        print(json.dumps({"what": "shade_rays", "variant": variant, "depth": depth, "rays": n, "kernel_ms_median": med,
                          "kernel_ms_min": lo, "mrays_per_s": round(n / med / 1e3, 1), "render_kernel_ms_median": fmed,
                          "render_kernel_ms_min": flo, "render_kernel": ds.kernel_name(),
                          "equals_frame": bool(np.array_equal(rad.reshape(H, W, 3).view(np.uint32), frame.view(np.uint32)))}),
              flush=True)
ds.close()
