"""Time a refit of a resident scene (DeviceScene.refit) against what it replaces:
a host LBVH build (rt_build_bvh) plus rt_scene_create of the same deformed arrays, on the c3 frog
and the c5 heightfield.

    python scripts/refit_time.py [--reps 20] [--base-reps 3]

Per scene: the deformed vertices (x += 0.05 extent sin(3 y)) go through triangles_from_mesh on the
device; after two warm-up calls the refit is timed `reps` times, wall clock around the call (it
synchronises) next to the HIP-event time of its launches, medians of both; the baseline is timed
`base-reps` times after one warm-up.  bytes: what one refit reads and writes (the triangle array
three times: check, leaves, normals; every rewritten record region once, the child boxes it
gathers once more) against rt_scene_device_bytes.  One JSON line per scene.
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

ARRAYS = ["inode", "wnode", "fnode", "qent", "qhdr", "ibox", "leaf", "tnorm", "cut", "cut2", "tri"]


def median_ms(ts):
    return round(float(np.median(ts)) * 1e3, 3)


def refit_bytes(P, lengths):
    """Bytes one refit moves, from the arrays' lengths: reads then writes per pass."""
    n = dict(zip(ARRAYS, lengths))
    tris = 72 * P
    leaves = tris + n["leaf"]                            # gather a triangle, write the whole record
    normals = tris + n["tnorm"] + n["tri"]
    internal = n["inode"] // 4 + 2 * n["ibox"] + n["inode"] * 3 // 4 + n["ibox"]  # refs + child boxes | child boxes + own box
    wide = n["wnode"] // 8 + n["wnode"] + n["wnode"] * 3 // 4  # refs + 4 boxes gathered | 96 of 128 bytes written
    frustum = n["fnode"] // 8 + 2 * (n["fnode"] * 3 // 4)      # refs + boxes gathered | boxes written
    cuts = 2 * (n["cut"] + n["cut2"])
    return tris + leaves + normals + internal + wide + frustum + cuts


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--base-reps", type=int, default=3)
a = ap.parse_args()
for cfg in ("c3", "c5"):
    sp = configs.scene_path(configs.G_CONFIGS[cfg]["scene"])
    hs = rt.HostScene.load_json(sp, REPO if sp.parent == configs.SCENES else sp.parent)
    P = hs.num_triangles
    extent = float(hs.aabbs[0, 3] - hs.aabbs[0, 0])
    pos = hs.positions.copy()
    pos[:, 0] += np.float32(0.05 * extent) * np.sin(np.float32(3) * pos[:, 1])
    dev = torch.device("cuda", 0)
    tpos = torch.from_numpy(pos).to(dev)
    tidx = torch.from_numpy(hs.indices.view(np.int32)).to(dev)
    tnrm = None if hs.normals is None else torch.from_numpy(hs.normals).to(dev)
    tris_dev = rt.triangles_from_mesh(tpos, tidx, tnrm)
    tris_host = tris_dev.cpu().numpy()

    # what a refit replaces: host build + pack + upload + streams and events, of the same arrays
    def rebuild():
        t0 = time.perf_counter()
        nodes, aabbs = rt.build_bvh(pos, hs.indices)
        t1 = time.perf_counter()
        ds = rt.DeviceScene(P, nodes, aabbs, tris_host, hs.tri_object_ids, hs.materials, hs.lights, 0)
        t2 = time.perf_counter()
        ds.close()
        return t1 - t0, t2 - t1

    rebuild()
    base = [rebuild() for _ in range(a.base_reps)]
    ds = rt.DeviceScene.from_host(hs, refittable=True)
    _, dig = ds.digest()
    for _ in range(2):
        ds.refit(tris_dev)
    wall, gpu, wall_host = [], [], []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms = ds.refit(tris_dev, timing=True)
        wall.append(time.perf_counter() - t0)
        gpu.append(ms * 1e-3)
    for _ in range(max(a.reps // 4, 1)):
        t0 = time.perf_counter()
        ds.refit(tris_host)
        wall_host.append(time.perf_counter() - t0)
    moved = refit_bytes(P, [int(x) for x in dig[0::2]])
    print(json.dumps({"config": cfg, "triangles": P, "scene_bytes": ds.device_bytes, "refit_bytes_moved": moved,
                      "refit_wall_ms": median_ms(wall), "refit_gpu_ms": median_ms(gpu),
                      "refit_gpu_ms_min_max": [round(min(gpu) * 1e3, 3), round(max(gpu) * 1e3, 3)],
                      "rebuild_wall_ms_min_max": [round(min(b[0] + b[1] for b in base) * 1e3, 1),
                                                  round(max(b[0] + b[1] for b in base) * 1e3, 1)],
                      "refit_from_host_wall_ms": median_ms(wall_host),
                      "host_build_ms": median_ms([b[0] for b in base]),
                      "scene_create_ms": median_ms([b[1] for b in base]),
                      "rebuild_wall_ms": median_ms([b[0] + b[1] for b in base]),
                      "effective_GBps": round(moved / float(np.median(gpu)) / 1e9, 1)}), flush=True)
    ds.close()
