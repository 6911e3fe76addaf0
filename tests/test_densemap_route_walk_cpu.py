"""The checked host walk of the route engine (csrc/densemap_route_core.hpp, dm_route_walk: the one body behind loamx_grid_route_trace
and loamx_route3_trace) for both kinds, driven without a device by tests/route_walk_driver.cpp: a hand-made valid field and the four
refused ones, the program built with the address and undefined-behaviour sanitizers on the host side and every output block exactly
as large as the walk may use.  The header of the engine includes the HIP headers, so the program is built with hipcc ($HIPCC, else
/opt/rocm/bin/hipcc; the same compiler the library itself needs) and not with g++ like the other drivers; no device is touched."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_the_walk_of_both_kinds_under_the_sanitizers(tmp_path):
    assert shutil.which(HIPCC), f"this test builds its driver with hipcc and found none at {HIPCC} (set HIPCC)"
    exe = str(tmp_path / "route_walk_driver")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-Xarch_host",
                        "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "route_walk_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("ok "), r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) >= 100
