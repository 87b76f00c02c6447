"""Does sorting caller rays for coherence pay?  Scene frog, one process, one build:

* 2^22 rays of classes B (random origins and directions) and C (from the surface toward the light)
  of tests/ray_batches.py, 64 batches of 65,536 with seeds 1000..1063, exactly as §4.17 builds them;
* the live rays entering depth 2 of trace_paths on the c3 camera's 1920x1080x1 rays (what a staged
  path tracer actually sorts between depths).

Per batch, mode and bits, HIP-event medians of --reps after --warmup, all through the C ABI on
preallocated buffers (no allocation inside a timed span):
  a  rt_ray_sort_device: keys + sort + ray gather,
  b  the query on the sorted rays (rt_trace_hits_device and rt_trace_rays_device, closest),
  c  the scatter of the query's output back to caller order (64 B records; idx and t),
against the same query on the unsorted rays.  Every row also checks that the scattered output is
the unsorted call's, bit for bit.  Lines go to stdout and to --out.

    python scripts/ray_sort_time.py [--reps 10] [--warmup 3] [--log2 22] [--out profiles/r10/ray_sort.jsonl]
"""
import argparse
import ctypes as C
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
from raytracinginonesemester_amd import _lib as L  # noqa: E402
from raytracinginonesemester_amd import configs  # noqa: E402
from raytracinginonesemester_amd.api import SORT_MODES  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--log2", type=int, default=22)
ap.add_argument("--out", default=str(REPO / "profiles" / "r10" / "ray_sort.jsonl"))
a = ap.parse_args()
SWEEP = {"origin": (2, 3, 4, 5, 6, 8, 10), "origin_dir": (1, 2, 3, 4, 5)}

cfg = configs.G_CONFIGS["c3"]
hs = rt.HostScene.load_json(configs.scene_path(cfg["scene"]), REPO)
ds = rt.DeviceScene.from_host(hs, device=0)
lib = L.lib()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev).cuda_stream
light = np.array(hs.lights[0]["position"], np.float64)
per = 65536
nb = max((1 << a.log2) // per, 1)
batches = {}
for cls in "BC":
    sl = rb.class_slices(4 * per)[cls]
    rays = np.ascontiguousarray(np.vstack([rb.make_rays(hs.aabbs, hs.triangles, light, 4 * per, 1000 + k)[sl] for k in range(nb)]))
    batches[cls] = torch.from_numpy(rays).to(dev)
# the rays a staged path tracer holds after its first depth on the c3 camera's frame
cam = hs.camera(cfg["width"], cfg["height"])
cam_rays, cam_seeds = rt.camera_rays(cam, 1, device=0)
state = ds.path_begin(cam_rays.shape[0], cam_seeds)
nxt, alive = ds.path_step(cam_rays, ds.trace_hits(cam_rays), state)
live, _, count = rt.compact_paths(alive, nxt)
batches["c3 depth 2"] = live.contiguous()
box = ds.bounds()
bx = L.AABB(L.Vec3(*box[:3]), L.Vec3(*box[3:]))
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(call):
    def once():
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    ms = [once() for _ in range(a.warmup + a.reps)][a.warmup:]
    return round(float(np.median(ms)), 4)


out_path = Path(a.out)
out_path.parent.mkdir(parents=True, exist_ok=True)
lines = []


def emit(row):
    lines.append(json.dumps(row))
    print(lines[-1], flush=True)


emit({"what": "setup", "scene": cfg["scene"], "build": lib.rt_build_id().decode()[:12], "reps": a.reps, "warmup": a.warmup,
      "box": [float(v) for v in box], "rays": {k: int(v.shape[0]) for k, v in batches.items()},
      "c3_camera_rays": int(cam_rays.shape[0])})
for name, rays in batches.items():
    n = rays.shape[0]
    srt = torch.empty_like(rays)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    scratch = torch.empty(int(lib.rt_ray_sort_scratch_bytes(n, 0, 1)), dtype=torch.uint8, device=dev)
    hits, hits_s, hits_b = (torch.empty((n, 16), dtype=torch.int32, device=dev) for _ in range(3))
    idx, idx_s, idx_b = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
    t, t_s, t_b = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(3))

    def trace_hits(r, h):
        L.check(lib.rt_trace_hits_device(ds.handle, r.data_ptr(), n, 0, h.data_ptr(), stream))

    def trace_rays(r, i, tt):
        L.check(lib.rt_trace_rays_device(ds.handle, L.RT_RAYS_CLOSEST, r.data_ptr(), None, n, 0, i.data_ptr(), tt.data_ptr(), stream))

    base_hits = timed(lambda: trace_hits(rays, hits_b))
    base_rays = timed(lambda: trace_rays(rays, idx_b, t_b))
    emit({"what": "unsorted", "rays_of": name, "rays": n, "hit_fraction": round(float((idx_b >= 0).float().mean()), 4),
          "trace_hits_ms": base_hits, "trace_rays_ms": base_rays})
    for mode, sweep in SWEEP.items():
        m = SORT_MODES[mode]
        for bits in sweep:
            def sort():
                L.check(lib.rt_ray_sort_device(0, rays.data_ptr(), n, m, bits, C.byref(bx), order.data_ptr(), srt.data_ptr(),
                                               scratch.data_ptr(), stream))

            def scatter_hits():
                L.check(lib.rt_scatter_device(0, hits_s.data_ptr(), n, 64, order.data_ptr(), hits.data_ptr(), stream))

            def scatter_rays():
                L.check(lib.rt_scatter_device(0, idx_s.data_ptr(), n, 4, order.data_ptr(), idx.data_ptr(), stream))
                L.check(lib.rt_scatter_device(0, t_s.data_ptr(), n, 4, order.data_ptr(), t.data_ptr(), stream))

            a_ms = timed(sort)
            bh = timed(lambda: trace_hits(srt, hits_s))
            ch = timed(scatter_hits)
            br = timed(lambda: trace_rays(srt, idx_s, t_s))
            cr = timed(scatter_rays)
            same = bool(torch.equal(hits, hits_b) and torch.equal(idx, idx_b) and torch.equal(t.view(torch.int32), t_b.view(torch.int32)))
            emit({"what": "sorted", "rays_of": name, "rays": n, "mode": mode, "bits": bits, "sort_ms": a_ms,
                  "trace_hits_sorted_ms": bh, "scatter_hits_ms": ch, "trace_hits_total_ms": round(a_ms + bh + ch, 4),
                  "trace_hits_unsorted_ms": base_hits, "trace_rays_sorted_ms": br, "scatter_rays_ms": cr,
                  "trace_rays_total_ms": round(a_ms + br + cr, 4), "trace_rays_unsorted_ms": base_rays, "equal": same})
    del srt, order, scratch, hits, hits_s, hits_b, idx, idx_s, idx_b, t, t_s, t_b
out_path.write_text("\n".join(lines) + "\n")
ds.close()
