"""Time the staged path (rt_path_*) on frog: the c3 camera's rays at 1920x1080x1
spp, made on the device, at depth 1 and at depth 8: DeviceScene.trace_paths with and without
compaction against rt_shade_rays (device path) on the same rays.  Each figure is the span between
two HIP events around the whole call on torch's current stream (for trace_paths that includes the
host's read of the live count once per depth), the median of --reps after --warmup.  The three
results are first checked bit-equal.

    python scripts/path_stages_time.py [--reps 10] [--warmup 3]
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
from raytracinginonesemester_amd import configs  # noqa: E402


def timed(call, reps, warmup):
    ms = []
    for _ in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = ms[warmup:]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
cfg = configs.G_CONFIGS["c3"]
hs = rt.HostScene.load_json(configs.scene_path(cfg["scene"]), REPO)
W, H = cfg["width"], cfg["height"]
cam = hs.camera(W, H)
miss, diffuse = hs.settings["miss_color"], hs.settings["diffuse_bounce"]
ds = rt.DeviceScene.from_host(hs, device=0)
rays, seeds = rt.camera_rays(cam, 1, device=0)
n = rays.shape[0]
for depth in (1, 8):
    mono = ds.shade_rays(rays, seeds, depth, diffuse, miss)
    live = []

    def counting(hits, r, ids, d):
        live.append(int(ids.shape[0]))
        return None

    results = {"compact": ds.trace_paths(rays, seeds, depth, diffuse, miss, material_fn=counting),
               "no compact": ds.trace_paths(rays, seeds, depth, diffuse, miss, compact=False)}
    torch.cuda.synchronize()
    for k, v in results.items():
        assert torch.equal(v.view(torch.int32), mono.view(torch.int32)), f"trace_paths ({k}) differs from shade_rays at depth {depth}"
    row = {"depth": depth, "rays": n, "live_entries_per_depth": live, "equal": True}
    row["shade_rays_ms"], row["shade_rays_ms_min"] = timed(lambda: ds.shade_rays(rays, seeds, depth, diffuse, miss), a.reps, a.warmup)
    row["staged_compact_ms"], row["staged_compact_ms_min"] = timed(
        lambda: ds.trace_paths(rays, seeds, depth, diffuse, miss), a.reps, a.warmup)
    row["staged_no_compact_ms"], row["staged_no_compact_ms_min"] = timed(
        lambda: ds.trace_paths(rays, seeds, depth, diffuse, miss, compact=False), a.reps, a.warmup)
    print(json.dumps(row), flush=True)
ds.close()
