"""Time the multi-hit queries (rt_trace_multi_hits) beside the closest-hit query
(rt_trace_rays) on the same rays and the same build, frog: 2^22 rays of classes A (aimed at the
root box, unnormalised directions) and C (from the surface toward the light) of
tests/ray_batches.py, 64 batches of 65,536 with seeds 1000..1063 as in §4.17, at k = 0, 1, 4, 8 and
32, WIDE and BINARY.  Device tensors in and out (k = 32 writes 2 GiB of records); each figure is the
median (and the minimum) of --reps launches after --warmup, HIP events around the launch.  Every
row also checks the counts against k = 0's and the first entry against the closest-hit query.

    python scripts/multi_hit_time.py [--reps 10] [--warmup 3] [--log2 22]
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


for cls in "AC":
    sl = rb.class_slices(4 * per)[cls]
    rays = torch.from_numpy(np.ascontiguousarray(np.vstack(
        [rb.make_rays(hs.aabbs, hs.triangles, light, 4 * per, 1000 + k)[sl] for k in range(nb)]))).to(dev)
    n = rays.shape[0]
    for flags, variant in ((0, "wide"), (rt.RT_FLAG_BINARY, "binary")):
        tm, tlo = median_ms(lambda: ds.trace_rays(rays, flags=flags))
        idx, t = ds.trace_rays(rays, flags=flags)
        count0 = ds.count_hits(rays, flags=flags)
        assert ds.multi_hits_variant() == (rt.RT_RAYS_VARIANT_BINARY if flags else rt.RT_RAYS_VARIANT_WIDE)
        c = count0.cpu().numpy()
        print(json.dumps({"what": "closest hit and hit counts", "rays_of": cls, "variant": variant, "rays": n,
                          "hit_fraction": round(float((idx >= 0).float().mean().item()), 4),
                          "hits_per_ray": round(float(c.mean()), 4), "most_hits": int(c.max()),
                          "rays_with_more_than_2": round(float((c > 2).mean()), 4),
                          "trace_rays_ms_median": tm, "trace_rays_ms_min": tlo}), flush=True)
        for k in (0, 1, 4, 8, 32):
            mm, mlo = median_ms(lambda: ds.trace_multi_hits(rays, k, flags=flags))
            count, tri, tt, _, _ = ds.trace_multi_hits(rays, k, flags=flags)
            ok = bool(torch.equal(count, count0))
            if k > 0:
                hit = idx >= 0
                ok = ok and bool((tt[hit, 0] <= t[hit]).all().item()) and bool(torch.equal(count > 0, hit))
            print(json.dumps({"what": "trace_multi_hits", "rays_of": cls, "variant": variant, "rays": n, "k": k,
                              "ms_median": mm, "ms_min": mlo, "mrays_per_s": round(n / mm / 1e3, 1),
                              "times_trace_rays": round(mm / tm, 3), "record_write_gb_per_s": round(16 * k * n / mm / 1e6, 1),
                              "checks": ok}), flush=True)
            del count, tri, tt
    del rays
ds.close()
