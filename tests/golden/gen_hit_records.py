"""Generate tests/golden/hit_records/ from the reference itself (run by hand, never by a test).

    python tests/golden/gen_hit_records.py [--driver oracle/_ref/ref_hit_records]

For each scene of tests/hit_records.py NAMES and for the small lattice scene of tests/tie_scenes.py: the first 64 rays of each class of its 4096-ray batch
go, with the scene's nodes, aabbs and triangles, through tests/native/ref_hit_records.cpp (the
reference's SearchBVH; compile it as its header says), and the HitRecord fields come back as raw
little-endian arrays, stored gzipped; meta.json keeps their sha256 and the commands.
"""
from __future__ import annotations

import argparse
import gzip
import hashlib
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[2]
for p in (REPO, REPO / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))
import hit_records as hr  # noqa: E402
import tie_scenes as ts  # noqa: E402

COMPILE = ("g++ -std=c++17 -O2 -ffp-contract=off -fno-fast-math -w -D__device__= -I$G/include -I$G/src "
           "-I$G/third_party/glm tests/native/ref_hit_records.cpp -x c++ $G/include/bvh.cu $G/include/query.cu "
           "-o oracle/_ref/ref_hit_records   (G = the reference's HW2/HW2/GPUandCPU)")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--driver", default=str(REPO / "oracle" / "_ref" / "ref_hit_records"))
    a = ap.parse_args()
    pick = hr.fixture_pick()
    meta = {"generator": "tests/golden/gen_hit_records.py", "compile": COMPILE,
            "command": "ref_hit_records <indir> <outdir>   (per scene: nodes.bin, aabbs.bin, tris.bin, rays.f32)",
            "rays": f"tests/hit_records.py batch(name)['rays'][fixture_pick()]: the first {hr.PER_CLASS} of each class",
            "fuzz_case": hr.FUZZ_CASE, "fuzz_ray_seed": hr.FUZZ_RAY_SEED, "sha256": {}, "hits": {}}
    for name in hr.NAMES + (ts.HIT_RECORDS_NAME,):
        lattice = name == ts.HIT_RECORDS_NAME  # (its classes V, E, L, R are quarters of the batch as well)
        s = ts.scene("small") if lattice else hr.scene(name)
        rays = np.ascontiguousarray((ts.batch("small") if lattice else hr.batch(name))["rays"][pick], np.float32)
        out = hr.GOLDEN_DIR / name
        out.mkdir(parents=True, exist_ok=True)
        with tempfile.TemporaryDirectory() as td:
            t = Path(td)
            (t / "nodes.bin").write_bytes(np.ascontiguousarray(s["nodes"], np.uint32).tobytes())
            (t / "aabbs.bin").write_bytes(np.ascontiguousarray(s["aabbs"], np.float32).tobytes())
            (t / "tris.bin").write_bytes(np.ascontiguousarray(s["tris"], np.float32).tobytes())
            (t / "rays.f32").write_bytes(rays.tobytes())
            subprocess.run([a.driver, str(t), str(t)], check=True)
            meta["sha256"][name] = {}
            for f in hr.FIXTURE_FILES:
                raw = (t / f).read_bytes()
                meta["sha256"][name][f] = hashlib.sha256(raw).hexdigest()
                with open(out / (f + ".gz"), "wb") as fh, gzip.GzipFile(fileobj=fh, mode="wb", mtime=0) as g:
                    g.write(raw)
            meta["hits"][name] = int(np.frombuffer((t / "hit.u8").read_bytes(), np.uint8).sum())
    (hr.GOLDEN_DIR / "meta.json").write_text(json.dumps(meta, indent=1) + "\n")
    print(json.dumps(meta["hits"]))


if __name__ == "__main__":
    main()
