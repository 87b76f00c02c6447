"""Time the visibility stage of the soft shadows (rt_light_visibility_device) on
frog: the hit records of 2^20 camera rays (1024 x 1024, one sample), the scene's one light at
radius 0.15, S = 1, 8, 32 and 128 shadow rays per hit, at every built group size and at 0 (the
library's choice), WIDE.  Device tensors in and out, HIP events around the call, the median (and
the minimum) of --reps launches after --warmup.

Beside it, what a caller can do without the stage: the same shadow rays materialised in torch by
rt_light_samples_host's recipe (rng_next and the rejection loop on int64 tensors, the disk's basis,
the sample rays of the hits that face the light), traced by trace_rays(mode="occluded", max_t=d)
and reduced to a fraction per hit.  Two figures: the trace and the reduction alone (the rays
already made), and the whole route.  `equal` is the fraction of hits whose fraction has the
stage's bits (torch's float32 division and square root are not specified to round as the
kernels' do, so this is reported, not asserted).

Then a render_rays frame (640 x 360, 4 spp, depth 2) with and without light_shapes.

    python scripts/soft_shadow_time.py [--reps 10] [--warmup 3] [--side 1024]
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--side", type=int, default=1024)
a = ap.parse_args()
RADIUS = 0.15
EPS = 1e-3
hs = rt.HostScene.load_json(configs.scene_path(configs.G_CONFIGS["c3"]["scene"]), REPO)
assert hs.lights.size == 1
ds = rt.DeviceScene.from_host(hs, device=0)
dev = torch.device("cuda", 0)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def median_ms(call, before=None):
    ms = []
    for _ in range(a.warmup + a.reps):
        if before is not None:
            before()
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[a.warmup:]
    return round(float(np.median(ms)), 4), round(float(min(ms)), 4)


cam = hs.camera(a.side, a.side)
rays, seeds = rt.camera_rays(cam, 1, device=0)
n = rays.shape[0]
hits = ds.trace_hits(rays)
f = rt.hit_fields(hits)
hit = f["tri"] >= 0
state = ds.path_begin(n, seeds)
lpos = torch.tensor(np.asarray(hs.lights["position"][0], np.float32), device=dev)


def shape_tensor(S):
    s = np.zeros(1, rt.LIGHT_SHAPE_DTYPE)
    s[0] = (RADIUS, S)
    return ds._shape_tensor(s, "soft_shadow_time")


def reset():
    state.rng.copy_(seeds)


# ---- the materialised route, in torch ------------------------------------------------------------------
def rng_next(s):
    s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
    h = s
    h = (h ^ 61) ^ (h >> 16)
    h = (h * 9) & 0xFFFFFFFF
    h = h ^ (h >> 4)
    h = (h * 0x27D4EB2D) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    return s, h.to(torch.float32) / 4294967296.0


def dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def unit(v):
    return v / torch.sqrt(dot(v, v))[:, None]


def cross(u, v):
    return torch.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                        u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], dim=1)


def materialise(S):
    """(the facing hits' indices, rays (F * S, 6), bounds (F * S,)) by rt_light_samples_host's recipe."""
    p, N = f["p"], unit(f["normal"])
    toC = lpos[None, :] - p
    facing = hit & (torch.clamp_min(dot(N, unit(toC)), 0.0) > 0)
    k = torch.nonzero(facing)[:, 0]
    p, N, toC = p[k], N[k], toC[k]
    distC = torch.sqrt(dot(toC, toC))
    W = (p - lpos[None, :]) / distC[:, None]
    ax = torch.where((W[:, 0].abs() > 0.9)[:, None], torch.tensor([[0.0, 1.0, 0.0]], device=dev),
                     torch.tensor([[1.0, 0.0, 0.0]], device=dev))
    T = unit(cross(ax, W))
    B = cross(W, T)
    origin = p + N * EPS
    s = seeds[k].to(torch.int64) & 0xFFFFFFFF
    out = torch.empty((k.shape[0], S, 6), dtype=torch.float32, device=dev)
    bound = torch.empty((k.shape[0], S), dtype=torch.float32, device=dev)
    for i in range(S):
        x = torch.zeros(k.shape[0], device=dev)
        y = torch.zeros(k.shape[0], device=dev)
        todo = torch.arange(k.shape[0], device=dev)
        while todo.numel():
            st, u = rng_next(s[todo])
            st, v = rng_next(st)
            s[todo] = st
            xx, yy = 2.0 * u - 1.0, 2.0 * v - 1.0
            r2 = xx * xx + yy * yy
            x[todo], y[todo] = xx, yy
            todo = todo[~((r2 > 1e-10) & (r2 <= 1.0))]
        lp = (lpos[None, :] + T * (x * RADIUS)[:, None]) + B * (y * RADIUS)[:, None]
        toL = lp - p
        d = torch.sqrt(dot(toL, toL))
        out[:, i, :3] = origin
        out[:, i, 3:] = toL / d[:, None]
        bound[:, i] = d
    return k, out.view(-1, 6), bound.view(-1)


def trace_and_reduce(k, srays, bound, S):
    occ = ds.trace_rays(srays, mode="occluded", max_t=bound)
    vis = torch.zeros(n, dtype=torch.float32, device=dev)
    vis[k] = (~occ.view(-1, S)).sum(dim=1).to(torch.float32) / float(S)
    return vis


print(json.dumps({"what": "entries", "scene": "frog", "rays": n, "hits": int(hit.sum().item()), "radius": RADIUS,
                  "device": torch.cuda.get_device_name(0)}), flush=True)
for S in (1, 8, 32, 128):
    sh = shape_tensor(S)
    fused = {}
    vis = None
    for g in (0,) + tuple(rt.LIGHT_VIS_GROUPS):
        fused[g] = median_ms(lambda: ds.light_visibility(hits, state, None, sh, lanes_per_entry=g), reset)
        reset()
        v = ds.light_visibility(hits, state, None, sh, lanes_per_entry=g)
        assert vis is None or torch.equal(v, vis)
        vis = v
    k, srays, bound = materialise(S)
    tr = median_ms(lambda: trace_and_reduce(k, srays, bound, S))
    del srays, bound

    def whole():
        kk, r, b = materialise(S)
        return trace_and_reduce(kk, r, b, S)

    wh = median_ms(whole) if S <= 32 else (None, None)  # (the torch loop at S = 128 runs for seconds: once is enough)
    got = whole()
    equal = float((got[hit].view(torch.int32) == vis[:, 0][hit].view(torch.int32)).float().mean().item())
    best = min(rt.LIGHT_VIS_GROUPS, key=lambda g: fused[g][0])
    print(json.dumps({"what": "light_visibility", "S": S, "shadow_rays": int(k.shape[0]) * S,
                      "partly_lit": int(((vis > 0) & (vis < 1)).sum().item()),
                      **{f"g{g}_ms_median": fused[g][0] for g in fused}, **{f"g{g}_ms_min": fused[g][1] for g in fused},
                      "best_group": best, "trace_rays_and_reduce_ms_median": tr[0], "trace_rays_and_reduce_ms_min": tr[1],
                      "materialise_trace_reduce_ms_median": wh[0], "times_faster_than_trace_and_reduce": round(tr[0] / fused[best][0], 3),
                      "equal": round(equal, 6)}), flush=True)
    del got, vis

# ---- a frame ---------------------------------------------------------------------------------------------
fcam = hs.camera(640, 360)
shape = np.zeros(1, rt.LIGHT_SHAPE_DTYPE)
shape[0] = (RADIUS, 8)
plain = median_ms(lambda: ds.render_rays(fcam, 4, 2))
staged = median_ms(lambda: ds.render_rays(fcam, 4, 2, material_fn=lambda h, r, i, d: None))
soft = median_ms(lambda: ds.render_rays(fcam, 4, 2, light_shapes=shape))
print(json.dumps({"what": "render_rays 640x360 spp 4 depth 2", "shade_rays_ms_median": plain[0], "shade_rays_ms_min": plain[1],
                  "staged_point_lights_ms_median": staged[0], "staged_point_lights_ms_min": staged[1],
                  "soft_S8_ms_median": soft[0], "soft_S8_ms_min": soft[1]}), flush=True)
ds.close()
