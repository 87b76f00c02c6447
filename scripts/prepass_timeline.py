"""Where a frame's pre-pass chain runs against the previous render kernel, from a rocprofv3
--kernel-trace CSV of pipelined frames (`profile_frames.py --mode none`, `bench.py`).

    python scripts/prepass_timeline.py <run_kernel_trace.csv> [N] [--json]

For each of the last N render kernels (render_tiles_kernel, or render_pair_kernel: two frames):
the start and end, in us relative to the END of the previous render kernel, of the gate's wait
kernel (__amd_rocclr_streamOpsWait), the cull and the cut launches that ran since the previous
render kernel started, and of the render kernel itself.  Negative: before the previous render
kernel ended (hidden in its tail).  The last line holds the medians and, of the same trace, the
mean duration of every kernel kind, the two gaps of the chain (cull end -> cut start, cut end ->
render start; medians), the hardware queue ids (the trace's Queue_Id) of the render kernels in
launch order, and per kernel kind the queue ids it ran on.
"""
import csv
import json
import sys

import numpy as np

KINDS = (("gate", "streamOpsWait"), ("cull", "tile_cull"), ("cut", "tile_cut"))
args = [x for x in sys.argv[1:] if not x.startswith("--")]
rows = list(csv.DictReader(open(args[0])))
n = int(args[1]) if len(args) > 1 else 20
ks = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "?")) for r in rows),
            key=lambda x: x[0])
ren = [k for k in ks if "render_tiles_kernel" in k[2] or "render_pair_kernel" in k[2]]
out = []
for i in range(max(1, len(ren) - n), len(ren)):
    s, e, _, rq = ren[i]
    ps, pe = ren[i - 1][0], ren[i - 1][1]
    o = {}
    for kind, pat in KINDS:
        mine = [k for k in ks if pat in k[2] and ps <= k[0] <= s]
        if mine:  # the last launch of the kind before this render kernel: this frame's
            o[kind] = [round((mine[-1][0] - pe) / 1e3, 2), round((mine[-1][1] - pe) / 1e3, 2)]
            o.setdefault("queue", {})[kind] = mine[-1][3]
    o["render"] = [round((s - pe) / 1e3, 2), round((e - pe) / 1e3, 2)]
    o.setdefault("queue", {})["render"] = rq
    out.append(o)
med = {}
for kind in [k for k, _ in KINDS] + ["render"]:
    v = np.array([o[kind] for o in out if kind in o], dtype=float)
    if len(v):
        med[kind + "_start_us"] = round(float(np.median(v[:, 0])), 2)
        med[kind + "_end_us"] = round(float(np.median(v[:, 1])), 2)
for name, a, b in (("cull_to_cut_us", "cull", "cut"), ("cut_to_render_us", "cut", "render")):
    v = [o[b][0] - o[a][1] for o in out if a in o and b in o]
    if v:
        med[name] = round(float(np.median(v)), 2)
dur, queues = {}, {}
for s, e, name, q in ks:
    key = name.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0][:60]
    dur.setdefault(key, []).append((e - s) / 1e3)
    queues.setdefault(key, set()).add(q)
summary = {"frames": len(out), "relative_to": "previous render kernel's end", "median": med,
           "mean_kernel_us": {k: [round(float(np.mean(v)), 2), len(v)] for k, v in sorted(dur.items())},
           "render_queue_ids": [o["queue"]["render"] for o in out],
           "queue_ids": {k: sorted(v) for k, v in sorted(queues.items())}}
if "--json" not in sys.argv:
    for o in out:
        print(o)
print(json.dumps(summary))
