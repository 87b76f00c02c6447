"""The ray key's host build (csrc/rt_raysort.hpp: rts::ray_key, the float -> uint32 conversion of
its cells, the gather / scatter kernels' small division) under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone program (CPU only): tests/native/raysort_main.cpp
compiled by hipcc with the sanitizers on the host side only (-Xarch_host; the header is shared with
the kernels, so it is compiled as they are) and the binary run directly.  Nothing is loaded into
python and nothing is preloaded; the program makes no HIP call.
"""
from __future__ import annotations

import subprocess

import pytest

from conftest import REPO

from raytracinginonesemester_amd import build as B

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
HOST_SAN = [f for flag in SAN for f in ("-Xarch_host", flag)]


def _hipcc(src, exe):
    return subprocess.run([B.HIPCC, f"--offload-arch={B.ARCH}", "-x", "hip", "-std=c++17", *B.FP, *HOST_SAN,
                           f"-I{REPO / 'include'}", f"-I{B.CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)


def test_ray_key_is_clean_under_asan_and_ubsan(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _hipcc(probe, tmp_path / "probe")
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")]).returncode != 0:
        pytest.skip(f"{B.HIPCC} has no host AddressSanitizer/UBSan runtime")
    exe = tmp_path / "raysort_main"
    r = _hipcc(REPO / "tests" / "native" / "raysort_main.cpp", exe)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " keys, 0 failures" in r.stdout
