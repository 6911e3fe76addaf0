"""CPU: the grid descriptor routine both index builds call (loam_velodyne_amd/csrc/grid_fit.hpp — no HIP in it), under UBSan.

tests/grid_fit_driver.cpp holds a literal copy of the loop grid_from_bounds and bb_make_desc used to duplicate and compares the new
routine with it, bit for bit, over 300 000 random bounds and the edges of the region where that loop's arithmetic is defined (every
axis below 2^31 cells, the product below 2^64: cubes of 2 642 245 cells per axis, one axis just under 2^31).  Beyond that region — extents
of 3e6, 1e12, 1e30 m, +-FLT_MAX on one, two and three axes, the (-2^31, -2^31, 4) product that wraps to 0 — it checks what the routine
promises: nx, ny, nz >= 1, ncell == nx * ny * nz <= budget, a cell edge of at least the initial one and the first of cell0 * 1.25^k that
fits.  The driver is built with -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover, so an undefined conversion ends it.
These extremes are looked at here only: no GPU test goes beyond a 1e6 m cube.  The numpy model of tests/submap_index_model.py is held
to the same routine word for word."""
import os
import subprocess

import numpy as np
import pytest

import submap_index_model as sm
from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_fit") / "grid_fit_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "grid_fit_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_equals_the_former_loop_where_it_was_defined_and_keeps_its_promises_elsewhere(driver):
    r = subprocess.run([driver, "check"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK", r.stdout[-2000:]
    rows = {ln.split()[0]: dict(zip(ln.split()[1::2], map(int, ln.split()[2::2]))) for ln in lines[:-1]}
    rnd, edges, beyond = rows["random"], rows["edges"], rows["beyond"]
    assert rnd["total"] == 300000 and rnd["defined"] > 250000 and rnd["defined"] < rnd["total"] and rnd["grew"] > 50000
    assert 0 < edges["defined"] < edges["total"]          # both sides of 2^31 cells per axis and of the 2^64 product
    assert beyond["defined"] == 0 and beyond["total"] >= 40 and beyond["max_steps"] > 300   # (an edge beyond the float range: ~400 steps)


def test_the_header_needs_no_hip(driver):
    src = open(os.path.join(ROOT, "loam_velodyne_amd", "csrc", "grid_fit.hpp")).read()
    assert "hip/" not in src and '#include "' not in src


def _eval(driver, rows):
    text = "".join(" ".join(f"{int(w):08x}" for w in np.array(list(mn) + list(mx) + [cell], np.float32).view(np.uint32)) + f" {budget}\n"
                   for mn, mx, cell, budget in rows)
    out = subprocess.run([driver, "eval"], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(rows)
    return [ln.split() for ln in out]


def test_the_numpy_model_is_the_same_routine(driver):
    rng = np.random.default_rng(7)
    rows = []
    for _ in range(3000):
        o = ((rng.random(3) - 0.5) * 2 * 10.0 ** (rng.random(3) * 6)).astype(np.float32)
        e = np.where(rng.random(3) < 0.1, 0.0, 10.0 ** (-4 + 11 * rng.random(3)))
        mx = np.maximum((o.astype(np.float64) + e).astype(np.float32), o)
        K = int(rng.choice([1, 2, 16, 64, 65, 1024, 4096]))
        rows.append((o, mx, float(rng.choice([1.05, 2.1, 0.25, 16.0])), sm.MAX_CELLS // K))
    big = np.float32(np.finfo(np.float32).max)
    rows += [((0, 0, 0), (3e9, 3e9, 3.5), 1.05, sm.MAX_CELLS), ((-big, -1, -1), (big, 2, 2), 1.05, 4095), ((-big,) * 3, (big,) * 3, 2.1, sm.MAX_CELLS),
             ((0, 0, 0), (1e30, 1e30, 1e30), 1.05, 1), ((-0.0, 0.0, -0.0), (0.0, 0.0, 0.0), 1.05, 1), ((0, 0, 0), (1e6, 1e6, 1e6), 1.05, sm.MAX_CELLS)]
    for (mn, mx, cell, budget), got in zip(rows, _eval(driver, rows)):
        (inv_h, nx, ny, nz, nc), _ = sm.grid_fit(np.array(mn, np.float32), np.array(mx, np.float32), cell, budget)
        want = [f"{int(w):08x}" for w in np.array(list(mn) + [inv_h], np.float32).view(np.uint32)] + [str(nx), str(ny), str(nz), str(nc)]
        assert got == want, (mn, mx, cell, budget)
