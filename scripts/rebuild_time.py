"""Time a rebuild of a resident scene (DeviceScene.rebuild) against what it
replaces: a host LBVH build (rt_build_bvh) plus rt_scene_create_refittable of the same deformed
triangles, on the c3 frog and the c5 heightfield; and what a rebuilt tree is worth to a frame
against a tree that was only refitted 1, 10 and 50 wobble steps away from its creation pose.

    python scripts/rebuild_time.py [--reps 20] [--base-reps 3]

Per scene: the deformed vertices (x += 0.05 extent sin(3 y), scripts/refit_time.py's) go through
triangles_from_mesh on the device; after two warm-up calls the rebuild is timed `reps` times, wall
clock around the call (it synchronises) next to the HIP-event time of its span, medians of both,
with the pack's kernel launches and host read-backs (rt_scene_rebuild_counts).  The baseline is
timed `base-reps` times after one warm-up.  Frames: step k moves x by 0.05 extent sin(3 y + 0.7 k);
the render-kernel time of the first frame, and the median of 5, at the configuration's own size,
on the scene rebuilt at step k and on a scene rebuilt at step 0 and refitted to step k.  One JSON line per scene.
"""
import argparse
import json
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import raytracinginonesemester_amd as rt  # noqa: E402
from raytracinginonesemester_amd import configs  # noqa: E402


def median_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--base-reps", type=int, default=3)
ap.add_argument("--configs", default="c3,c5")
a = ap.parse_args()
for cfg in a.configs.split(","):
    g = configs.G_CONFIGS[cfg]
    sp = configs.scene_path(g["scene"])
    hs = rt.HostScene.load_json(sp, REPO if sp.parent == configs.SCENES else sp.parent)
    P = hs.num_triangles
    extent = float(hs.aabbs[0, 3] - hs.aabbs[0, 0])
    dev = torch.device("cuda", 0)
    tidx = torch.from_numpy(hs.indices.view(np.int32)).to(dev)
    tnrm = None if hs.normals is None else torch.from_numpy(hs.normals).to(dev)

    def step_tris(k):
        pos = hs.positions.copy()
        pos[:, 0] += np.float32(0.05 * extent) * np.sin(np.float32(3) * pos[:, 1] + np.float32(0.7 * k))
        return rt.triangles_from_mesh(torch.from_numpy(pos).to(dev), tidx, tnrm)

    tris_dev = step_tris(0)
    tris_host = tris_dev.cpu().numpy()

    def baseline():
        t0 = time.perf_counter()
        nodes, aabbs = rt.build_bvh_triangles(tris_host)
        t1 = time.perf_counter()
        ds = rt.DeviceScene(P, nodes, aabbs, tris_host, hs.tri_object_ids, hs.materials, hs.lights, 0, refittable=True)
        t2 = time.perf_counter()
        ds.close()
        return t1 - t0, t2 - t1

    baseline()
    base = [baseline() for _ in range(a.base_reps)]
    ds = rt.DeviceScene.from_host(hs, refittable=True)
    for _ in range(2):
        ds.rebuild(tris_dev)
    wall, gpu = [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = ds.rebuild(tris_dev, timing=True)
        wall.append(time.perf_counter() - t0)
        gpu.append(ms * 1e-3)
    path, counts = ds.rebuild_path, ds.rebuild_counts
    rt.set_tuning("record_greedy", 1)  # (a knob the device pack does not take: the host path of the same call)
    ds.rebuild(tris_dev)
    wall_host_path = []
    for _ in range(max(a.base_reps, 1)):
        t0 = time.perf_counter()
        ds.rebuild(tris_dev)
        wall_host_path.append(time.perf_counter() - t0)
    assert ds.rebuild_path == rt.RT_REBUILD_HOST
    rt.reset_tuning()

    # frames: rebuilt at step k against refitted from step 0 to step k
    i = hs.info
    W, H = g["width"], g["height"]
    cam = rt.Camera(tuple(i.cam_position), tuple(i.cam_look_at), tuple(i.cam_up), i.focal_length_mm, i.sensor_height_mm, W, H)
    rgb = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)

    def kernel_ms(scene):
        """(the first frame's render-kernel ms after the scene changed, the median of 5 frames)."""
        opts, _jit = scene.make_opts(spp=g["spp"], max_depth=g["max_depth"])
        ts = []
        for _ in range(5):
            scene.render_device(cam, opts, rgb.data_ptr())
            torch.cuda.synchronize()
            ts.append(float(scene.kernel_times(1)[-1]))
        return [round(ts[0], 4), round(float(np.median(ts)), 4)]

    frames = {}
    refit = rt.DeviceScene.from_host(hs, refittable=True)
    refit.rebuild(step_tris(0))  # the same kind of tree under both: the LBVH of step 0
    for k in (0, 1, 10, 50):
        t = step_tris(k)
        ds.rebuild(t)
        refit.refit(t)
        frames[str(k)] = {"rebuilt_first_median_ms": kernel_ms(ds), "refitted_first_median_ms": kernel_ms(refit)}
    print(json.dumps({"config": cfg, "triangles": P, "path": path, "pack_launches": counts[0], "pack_readbacks": counts[1],
                      "rebuild_wall_ms": median_ms(wall), "rebuild_gpu_span_ms": median_ms(gpu),
                      "rebuild_wall_ms_min_max": [round(min(wall) * 1e3, 3), round(max(wall) * 1e3, 3)],
                      "host_path_wall_ms": median_ms(wall_host_path),
                      "baseline_host_build_ms": median_ms([b[0] for b in base]),
                      "baseline_scene_create_ms": median_ms([b[1] for b in base]),
                      "baseline_wall_ms": median_ms([b[0] + b[1] for b in base]),
                      "baseline_wall_ms_min_max": [round(min(b[0] + b[1] for b in base) * 1e3, 1),
                                                   round(max(b[0] + b[1] for b in base) * 1e3, 1)],
                      "frame_kernel_ms_by_step": frames}), flush=True)
    ds.close()
    refit.close()
