"""Time the closest-point query (rt_closest_points_device) on frog: 2^22 points of
classes a (uniform in the root box inflated 1.5 times) and b (on the triangles, moved along the
normal by 0 to 0.1 extents) of tests/closest_point_cases.py, four batches of 2^20 with seeds
1000..1003, WIDE and BINARY.  Device tensors in and out; each figure is the median (and the minimum)
of --reps launches after --warmup, HIP events around the launch.  The closest-hit query
(rt_trace_rays) on 2^22 rays of class A of tests/ray_batches.py runs in the same process, for scale.
Every row carries the mean number of triangles a lane evaluated and checks WIDE's records against
BINARY's.

    python scripts/closest_points_time.py [--reps 10] [--warmup 3] [--log2 22]
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

import closest_point_cases as cp  # noqa: E402
import ray_batches as rb  # noqa: E402
import raytracinginonesemester_amd as rt  # noqa: E402
from raytracinginonesemester_amd import configs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--log2", type=int, default=22)
a = ap.parse_args()
cfg = configs.G_CONFIGS["c3"]
hs = rt.HostScene.load_json(configs.scene_path(cfg["scene"]), REPO)
ds = rt.DeviceScene.from_host(hs, device=0)
arrays = {"P": hs.num_triangles, "nodes": np.ascontiguousarray(hs.nodes).view(np.uint32).reshape(-1, 4),
          "aabbs": np.ascontiguousarray(hs.aabbs, np.float32).reshape(-1, 6),
          "tris": np.ascontiguousarray(hs.triangles, np.float32).reshape(-1, 18)}
light = np.array(hs.lights[0]["position"], np.float64)
total = 1 << a.log2
per = min(total, 1 << 20)
nb = total // per
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
    ms = ms[a.warmup:]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


rays = torch.from_numpy(np.ascontiguousarray(np.vstack(
    [rb.make_rays(hs.aabbs, hs.triangles, light, 4 * per, 1000 + k)[rb.class_slices(4 * per)["A"]] for k in range(nb)]))).to(dev)
scale = {}
for flags, variant in ((0, "wide"), (rt.RT_FLAG_BINARY, "binary")):
    tm, tlo = median_ms(lambda: ds.trace_rays(rays, flags=flags))
    scale[variant] = tm
    print(json.dumps({"what": "closest hit (trace_rays), for scale", "rays_of": "A", "variant": variant, "rays": rays.shape[0],
                      "ms_median": tm, "ms_min": tlo, "mrays_per_s": round(rays.shape[0] / tm / 1e3, 1)}), flush=True)
del rays

for cls in "ab":
    sl = cp.class_slices(4 * per)[cls]
    pts = torch.from_numpy(np.ascontiguousarray(np.vstack(
        [cp.make_points(arrays, 4 * per, 1000 + k)[sl] for k in range(nb)]))).to(dev)
    n = pts.shape[0]
    first = None
    for flags, variant in ((0, "wide"), (rt.RT_FLAG_BINARY, "binary")):
        mm, mlo = median_ms(lambda: ds.closest_points(pts, flags=flags))
        out = ds.closest_points(pts, flags=flags, evals=True)
        assert ds.closest_points_variant() == (rt.RT_RAYS_VARIANT_BINARY if flags else rt.RT_RAYS_VARIANT_WIDE)
        ev = out[6].to(torch.float64)
        rec = torch.stack([out[0], out[1].view(torch.int32), out[5]], dim=1)
        if first is None:
            first = rec
        print(json.dumps({"what": "closest_points", "points_of": cls, "variant": variant, "points": n, "ms_median": mm,
                          "ms_min": mlo, "mpoints_per_s": round(n / mm / 1e3, 1), "times_trace_rays": round(mm / scale[variant], 3),
                          "evals_mean": round(float(ev.mean().item()), 3), "evals_max": int(ev.max().item()),
                          "d2_mean": float(out[1].to(torch.float64).mean().item()),
                          "checks": bool(torch.equal(rec, first)) and bool((out[0] >= 0).all().item())}), flush=True)
        del out, ev, rec
    del pts, first
ds.close()
