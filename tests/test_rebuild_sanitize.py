"""The rebuild's host side — rt_build_bvh_triangles, the record weight and the host half of
rt_scene_rebuild's host path (rt::rebuild_pack) — under AddressSanitizer + UndefinedBehaviorSanitizer
as a stand-alone program (CPU only): tests/native/rebuild_main.cpp and the host units
(build.HOST_UNITS: they link without HIP) compiled with -fsanitize=address,undefined
-fno-sanitize-recover=undefined and the binary run directly, as tests/test_refit_sanitize.py does
for the refit.  Nothing is loaded into python and nothing is preloaded.
"""
from __future__ import annotations

import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import REPO

from raytracinginonesemester_amd import build as B

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def test_rebuild_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([B.CXX, *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip(f"{B.CXX} has no AddressSanitizer/UBSan runtime")
    exe = tmp_path / "rebuild_main"
    srcs = [REPO / "tests" / "native" / "rebuild_main.cpp", *(B.CSRC / f"{u}.cpp" for u in B.HOST_UNITS)]
    objs = [tmp_path / (s.stem + ".o") for s in srcs]
    with ThreadPoolExecutor(max_workers=len(srcs)) as ex:  # one compiler process per unit
        for f in [ex.submit(subprocess.run, [B.CXX, "-std=c++17", *B.FP, *SAN, f"-I{REPO / 'include'}", f"-I{B.CSRC}",
                                             "-c", str(s), "-o", str(o)], check=True) for s, o in zip(srcs, objs)]:
            f.result()
    subprocess.run([B.CXX, *SAN, *map(str, objs), "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout
