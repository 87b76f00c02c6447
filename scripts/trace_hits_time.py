"""Time the hit-record queries (rt_trace_hits) beside the closest-hit queries
(rt_trace_rays) on the same rays and the same build, frog: 2^22 rays of classes B (random origins
and directions) and C (from the surface toward the light) of tests/ray_batches.py, 64 batches of
65,536 with seeds 1000..1063 as in §4.17, and the c3 camera's rays at 1920x1080x1 spp made by
rt_camera_rays_device.  kernel_ms is the median of --reps launches after --warmup, WIDE and BINARY.
Every row also checks that tri and t of the records are the closest-hit query's.

    python scripts/trace_hits_time.py [--reps 10] [--warmup 3] [--log2 22]
"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ray_batches as rb  # noqa: E402
import raytracinginonesemester_amd as rt  # noqa: E402
from raytracinginonesemester_amd import configs  # noqa: E402


def median_ms(call, reps, warmup):
    ms = [call() for _ in range(warmup + reps)][warmup:]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--log2", type=int, default=22)
a = ap.parse_args()
cfg = configs.G_CONFIGS["c3"]
hs = rt.HostScene.load_json(configs.scene_path(cfg["scene"]), REPO)
ds = rt.DeviceScene.from_host(hs, device=0)
light = np.array(hs.lights[0]["position"], np.float64)
per = 65536
nb = max((1 << a.log2) // per, 1)
batches = {}
for cls in "BC":
    sl = rb.class_slices(4 * per)[cls]
    batches[cls] = np.ascontiguousarray(np.vstack([rb.make_rays(hs.aabbs, hs.triangles, light, 4 * per, 1000 + k)[sl]
                                                   for k in range(nb)]))
cam = hs.camera(cfg["width"], cfg["height"])
dev = torch.device("cuda", 0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def camera_ms():
    e0.record()
    rt.camera_rays(cam, 1, device=0)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


med, lo = median_ms(camera_ms, a.reps, a.warmup)
dev_rays, _ = rt.camera_rays(cam, 1, device=0)
torch.cuda.synchronize(dev)
batches["c3 camera"] = dev_rays.cpu().numpy()
host_rays, _ = rt.camera_rays(cam, 1)
print(json.dumps({"what": "camera_rays device (table upload, two allocations, launch)", "rays": int(dev_rays.shape[0]),
                  "ms_median": med, "ms_min": lo,
                  "equals_host": bool(np.array_equal(batches["c3 camera"].view(np.uint32), host_rays.view(np.uint32)))}),
      flush=True)
for name, rays in batches.items():
    n = rays.shape[0]
    for flags, variant in ((0, "wide"), (rt.RT_FLAG_BINARY, "binary")):
        tm, tlo = median_ms(lambda: ds.trace_rays(rays, flags=flags, timing=True)[1], a.reps, a.warmup)
        hm, hlo = median_ms(lambda: ds.trace_hits(rays, flags=flags, timing=True)[1], a.reps, a.warmup)
        assert ds.trace_hits_variant() == (rt.RT_RAYS_VARIANT_BINARY if flags else rt.RT_RAYS_VARIANT_WIDE)
        idx, t = ds.trace_rays(rays, flags=flags)
        rec = ds.trace_hits(rays, flags=flags)
        print(json.dumps({"what": "trace_hits beside trace_rays", "rays_of": name, "variant": variant, "rays": n,
                          "hit_fraction": round(float((idx >= 0).mean()), 4), "trace_rays_ms_median": tm,
                          "trace_rays_ms_min": tlo, "trace_hits_ms_median": hm, "trace_hits_ms_min": hlo,
                          "added_ms": round(hm - tm, 4), "trace_hits_mrays_per_s": round(n / hm / 1e3, 1),
                          "record_write_gb_per_s": round(64 * n / hm / 1e6, 1),
                          "tri_t_equal": bool(np.array_equal(rec["tri"], idx)
                                              and np.array_equal(rec["t"].view(np.uint32), t.view(np.uint32)))}),
              flush=True)
ds.close()
