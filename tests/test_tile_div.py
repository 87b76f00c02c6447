"""The render kernels' tile-coordinate helper (csrc/rt_tilediv.hpp: tile / tiles_x as a multiply
and a shift, the constants made on the host) against / and % on the CPU: tests/native/
tilediv_main.cpp, a stand-alone program compiled by hipcc as the kernels' header is and run
directly -- with AddressSanitizer + UndefinedBehaviorSanitizer on the host side where hipcc has
their runtime, plain otherwise.  Nothing is loaded into python and the program makes no HIP call.
"""
from __future__ import annotations

import subprocess

from conftest import REPO

from raytracinginonesemester_amd import build as B

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
HOST_SAN = [f for flag in SAN for f in ("-Xarch_host", flag)]


def _hipcc(src, exe, extra):
    return subprocess.run([B.HIPCC, f"--offload-arch={B.ARCH}", "-x", "hip", "-std=c++17", "-O2", *B.FP, *extra,
                           f"-I{REPO / 'include'}", f"-I{B.CSRC}", str(src), "-o", str(exe)], capture_output=True, text=True)


def test_tile_div_matches_division(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = _hipcc(probe, tmp_path / "probe", HOST_SAN)
    san = HOST_SAN if r.returncode == 0 and subprocess.run([str(tmp_path / "probe")]).returncode == 0 else []
    exe = tmp_path / "tilediv_main"
    r = _hipcc(REPO / "tests" / "native" / "tilediv_main.cpp", exe, san)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print(f"tilediv_main built {'with AddressSanitizer + UBSan' if san else 'WITHOUT sanitizers (no host runtime)'}: "
          f"{r.stdout.strip()}")
    checks = int(r.stdout.split()[0])
    assert checks >= 1024 << 20 and " checks, 0 failures" in r.stdout, r.stdout
