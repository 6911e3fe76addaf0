"""CPU: the surfel of a voxel as the device computes it (include/loamx.h, loamx_densemap_freeze_device and what follows it;
loam_velodyne_amd/csrc/densemap_surfel.hpp — the one function k_dm_surfels runs per slot, standard library only).

tests/densemap_surfel_driver.cpp builds that header with the host compiler and -ffp-contract=off, as the library is built, and prints
the output bytes for voxel words from stdin.  They are held, byte for byte, to loamx_densemap_surfel_of in axes 0, which is the
host's dm_surfel: both texts use only correctly rounded operations in the same order, so no tolerance applies.  The word sets are
the designed voxels of tests/densemap_freeze_cases.py and a few thousand random ones.  The 128-bit conversion that the header
writes out is also held to Python's own int -> float, which rounds to nearest, ties to even.

Also: every new symbol declared and exported, the Python methods present, and the refusals that need no device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_freeze_cases as fc
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_freeze_device", "loamx_densemap_freeze_pyramid_device", "loamx_densemap_freeze_history",
               "loamx_densemap_download_frozen", "loamx_densemap_align_from_history", "loamx_densemap_align_many_from_history",
               "loamx_densemap_align_pyramid_from_history")
SOURCES = ["-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "densemap_surfel_driver.cpp")]


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("freeze_device", "freeze_pyramid_device", "freeze_history", "download_frozen", "align_from_history",
                 "align_many_from_history", "align_pyramid_from_history"):
        assert callable(getattr(loamx.DenseMap, name)), name


def test_refusals_without_a_device():
    L = loamx.lib()
    n, cfg, res, best = C.c_uint64(7), loamx.SurfelConfig(), loamx.AlignResult(), C.c_uint32(5)
    keys, rec = (C.c_uint64 * 4)(), (C.c_float * 24)()
    pose = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    calls = ((L.loamx_densemap_freeze_device, (None, C.byref(cfg), None, C.byref(n))),
             (L.loamx_densemap_freeze_pyramid_device, (None, C.byref(cfg), None, None, None)),
             (L.loamx_densemap_freeze_history, (None, C.c_uint64(0), C.c_uint64(1), None, C.byref(cfg), C.byref(n))),
             (L.loamx_densemap_download_frozen, (None, C.c_uint32(0), keys, rec, C.c_uint64(4), C.byref(n))),
             (L.loamx_densemap_align_from_history, (None, C.c_uint64(0), pose, None, C.byref(res))),
             (L.loamx_densemap_align_many_from_history, (None, C.c_uint64(0), pose, C.c_uint32(1), None, C.byref(res), C.byref(best))),
             (L.loamx_densemap_align_pyramid_from_history, (None, C.c_uint64(0), pose, None, C.c_uint32(0), C.byref(res))))
    for fn, args in calls:
        assert fn(*args) == loamx.E_INVALID, fn.__name__
        assert b"NULL" in L.loamx_last_error(), fn.__name__
    assert n.value == 7 and best.value == 5   # nothing written
    # the settings are checked before the handle is looked at for its features: a bad min_points is named
    assert L.loamx_densemap_freeze_device(None, C.byref(loamx.SurfelConfig(min_points=2)), None, None) == loamx.E_INVALID


# ---- densemap_surfel.hpp on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("densemap_surfel") / "densemap_surfel_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror"] + SOURCES + ["-o", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def driver_surfels(exe, cases, leaf):
    """per case (seven 32-bit words: six f32 and the curvature; has) from the driver"""
    text = []
    for c in cases:
        cfg = loamx.SurfelConfig(c["min_points"], c["min_planar_ratio"])
        text.append(" ".join(str(v) for v in [f32_bits(leaf), *c["idx"], cfg.min_points, f32_bits(cfg.min_planar_ratio),
                                              *[int(x) % (1 << 64) for x in c["vals"]], *[int(x) % (1 << 64) for x in c["mom"]]]))
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [([int(w, 16) for w in row[:7]], row[7] == "1") for row in rows]


def library_surfel(c, leaf):
    """the same seven words and `has` from loamx_densemap_surfel_of in axes 0"""
    s = loamx.surfel_of(leaf, c["idx"], c["vals"], c["mom"], axes="loam", min_points=c["min_points"], min_planar_ratio=c["min_planar_ratio"])
    w = s.view(np.uint32)
    return [int(w[k]) for k in (0, 1, 2, 4, 5, 6, 7)], bool(s[4] != 0 or s[5] != 0 or s[6] != 0)


def check(exe, cases, leaf):
    got = driver_surfels(exe, cases, leaf)
    n_has = 0
    for c, g in zip(cases, got):
        assert g == library_surfel(c, leaf), (c["name"], c["idx"], c["vals"], c["mom"])
        n_has += g[1]
    return n_has


def test_designed_point_voxels_byte_for_byte(exe):
    cases = fc.point_cases()
    names = [c["name"] for c in cases]
    for must in ("n == min_points", "n == min_points - 1", "collinear", "coplanar on axis 2, origin in the plane", "tilted plane, high side",
                 "isotropic blob", "symmetric about the origin, V = 0", "a cross, the two smallest equal", "65536 points near the far corner"):
        assert must in names
    n_has = check(exe, cases, fc.LEAF)
    assert 15 <= n_has < len(cases)   # both outcomes occur
    by = {c["name"]: c for c in cases}
    # what the cases were designed for, on the library's side (the driver equals it)
    assert not library_surfel(by["n == min_points - 1"], fc.LEAF)[1] and library_surfel(by["n == min_points"], fc.LEAF)[1]
    assert library_surfel(by["n == 4 with min_points 4"], fc.LEAF)[1] and not library_surfel(by["collinear"], fc.LEAF)[1]
    for name in ("symmetric about the origin, V = 0", "a cross, the two smallest equal, V = 0", "coplanar on axis 1, origin in the plane"):
        c = by[name]
        assert [int(v) for v in c["mom"][6:]] == [0, 0, 0] or name.startswith("coplanar")
        s = loamx.surfel_of(fc.LEAF, c["idx"], c["vals"], c["mom"])
        first = [v for v in s[4:7] if v != 0][0]
        assert first > 0, name   # V . normal == 0: the first non-zero component is positive
    s = loamx.surfel_of(fc.LEAF, by["a cross, the two smallest equal"]["idx"], by["a cross, the two smallest equal"]["vals"],
                        by["a cross, the two smallest equal"]["mom"])
    assert abs(s[4]) == 1.0 and s[5] == 0 and s[6] == 0   # l0 == l1: the tie keeps the index order, the normal is the x axis
    big = by["65536 points near the far corner"]
    assert big["vals"][0] == 65536 and big["vals"][0] * big["mom"][0] > 1 << 71


def test_designed_word_voxels_byte_for_byte(exe):
    cases = fc.word_cases()
    assert check(exe, cases, fc.LEAF) == len(cases)
    assert check(exe, cases, 0.1) == len(cases)   # (a leaf that is no power of two)


def test_random_voxels_byte_for_byte(exe):
    cases = fc.random_cases(4000, seed=31)
    n_has = check(exe, cases, 0.1)
    assert 1000 < n_has < 3900


def test_the_128_bit_conversion_rounds_to_nearest_even(exe):
    rng = np.random.default_rng(5)
    vals = [0, 1, (1 << 53) + 1, (1 << 53) + 3, (1 << 54) + 2, (1 << 54) + 6, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 1 << 64, (1 << 64) + 1,
            (1 << 64) + (1 << 11), (1 << 64) + (1 << 11) + 1, (1 << 64) + (1 << 11) - 1, (1 << 64) + 3 * (1 << 11), (1 << 65) - 1,
            (1 << 75) + (1 << 22), (1 << 75) + (1 << 22) + 1, (1 << 75) + 3 * (1 << 22), (1 << 126) + (1 << 73), (1 << 127) - 1,
            (1 << 127) - (1 << 73), (1 << 100) - 1]
    for bits in range(1, 128):
        for _ in range(20):
            v = int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62) | (int(rng.integers(0, 8)) << 124)
            v = (v >> (127 - bits)) | (1 << (bits - 1))
            vals.append(v)
            vals.append((v >> 11 << 11) | (1 << 10) if bits > 60 else v | 1)   # (halfway patterns of the 64-bit and wider cases)
    vals = [v for v in vals if v < 1 << 127]
    signed = vals + [-v for v in vals]
    text = "".join(f"{1 if v < 0 else 0} {abs(v) >> 64} {abs(v) & ((1 << 64) - 1)}\n" for v in signed)
    r = subprocess.run([exe, "conv"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == ""
    got = [int(ln, 16) for ln in r.stdout.split()]
    want = [struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in signed]   # (Python: correctly rounded, ties to even)
    assert len(got) == len(want) > 5000
    assert got == want
    # the ties do go both ways
    assert float((1 << 53) + 1) == float(1 << 53) and float((1 << 53) + 3) == float((1 << 53) + 4)
    assert float((1 << 64) + (1 << 11)) == float(1 << 64) and float((1 << 64) + 3 * (1 << 11)) == float((1 << 64) + (1 << 13))
