"""CPU: the dense map's second moments and surfels (include/loamx.h, loamx_densemap_enable_moments ...) — every new symbol declared and
exported, the two new structs laid out as a C compiler lays them out, the default configuration, bad arguments refused without a device,
and loamx_densemap_surfel_of (host only) against the model (tests/densemap_moments_model.py: the exact integer scatter, numpy's eigh in
float64) on voxels whose integer words are built directly from chosen offsets q.

Tolerance of the normal and the curvature, 1e-6: the f32 rounding of the output (6e-8) plus the error of two double-precision
eigen-solvers divided by the relative gap l1 - l0 of the voxel, which every compared voxel is required to keep above 1e-6 (so ~1e-9)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_moments_model as mm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_surfel_default_config", "loamx_densemap_surfel_of", "loamx_densemap_enable_moments",
               "loamx_densemap_download_moments", "loamx_densemap_download_surfels", "loamx_densemap_save_pcd_surfels")
LEAF = 0.5
Q = (1 << 20) - 1
TOL = 1e-6


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("enable_moments", "moments", "surfels"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert callable(loamx.surfel_of) and len(loamx.SURFEL_FIELDS) == 8


@pytest.mark.parametrize("c_name,fields,size", [("loamx_densemap_surfel_config", ["min_points", "min_planar_ratio"], None),
                                                ("loamx_surfel", ["x", "y", "z", "intensity", "normal_x", "normal_y", "normal_z", "curvature"], 32)])
def test_struct_layout_matches_c(tmp_path, c_name, fields, size):
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    if size is None:
        assert got[0] == C.sizeof(loamx.SurfelConfig)
        assert got[1:] == [getattr(loamx.SurfelConfig, f).offset for f in fields]
    else:   # eight packed floats: a row of the (n, 8) float32 array of DenseMap.surfels()
        assert got[0] == size and got[1:] == [4 * k for k in range(8)] and fields == list(loamx.SURFEL_FIELDS)


def test_default_configuration():
    L = loamx.lib()
    c = loamx.SurfelConfig()
    assert (c.min_points, c.min_planar_ratio) == (5, np.float32(0.01)) == (mm.DEFAULT_MIN_POINTS, np.float32(mm.DEFAULT_MIN_PLANAR_RATIO))
    c.min_points, c.min_planar_ratio = 77, 0.5
    L.loamx_densemap_surfel_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.min_points, c.min_planar_ratio) == (5, np.float32(0.01))
    c = loamx.SurfelConfig(min_points=3)
    assert (c.min_points, c.min_planar_ratio) == (3, np.float32(0.01))
    L.loamx_densemap_surfel_default_config(None)   # NULL: nothing to fill


def test_bad_arguments_are_refused_without_a_device():
    L = loamx.lib()
    vals, mom = mm.words_of_q([[1, 2, 3], [4, 5, 7], [9, 1, 1], [2, 2, 8], [5, 5, 5]])
    idx, v, m = (C.c_int32 * 3)(0, 0, 0), (C.c_uint64 * 4)(*vals), (C.c_uint64 * 9)(*mom)
    cfg, out = loamx.SurfelConfig(), (C.c_float * 8)()
    leaf = C.c_float(LEAF)
    call = L.loamx_densemap_surfel_of
    assert call(leaf, idx, v, m, C.byref(cfg), 0, out) == loamx.OK
    assert call(leaf, idx, v, m, None, 0, out) == loamx.OK   # NULL settings: the defaults
    for args in ((leaf, None, v, m, C.byref(cfg), 0, out), (leaf, idx, None, m, C.byref(cfg), 0, out),
                 (leaf, idx, v, None, C.byref(cfg), 0, out), (leaf, idx, v, m, C.byref(cfg), 0, None)):
        assert call(*args) == loamx.E_INVALID
        assert b"NULL" in L.loamx_last_error()
    assert call(leaf, idx, v, m, C.byref(loamx.SurfelConfig(min_points=2)), 0, out) == loamx.E_INVALID
    assert b"min_points" in L.loamx_last_error()
    assert call(leaf, idx, v, m, C.byref(loamx.SurfelConfig(min_planar_ratio=-0.5)), 0, out) == loamx.E_INVALID
    assert b"min_planar_ratio" in L.loamx_last_error()
    assert call(leaf, idx, v, m, C.byref(loamx.SurfelConfig(min_planar_ratio=float("nan"))), 0, out) == loamx.E_INVALID
    assert call(leaf, idx, v, m, C.byref(cfg), 2, out) == loamx.E_INVALID
    assert call(C.c_float(0.0), idx, v, m, C.byref(cfg), 0, out) == loamx.E_INVALID
    assert call(leaf, idx, (C.c_uint64 * 4)(0, 0, 0, 0), m, C.byref(cfg), 0, out) == loamx.E_INVALID   # n == 0
    with pytest.raises(loamx.LoamxError):
        loamx.surfel_of(LEAF, (0, 0, 0), vals, mom, min_points=1)
    # the device entry points with a NULL handle
    n, buf = C.c_uint64(0), (C.c_uint64 * 9)()
    assert L.loamx_densemap_enable_moments(None) == loamx.E_INVALID
    assert L.loamx_densemap_download_moments(None, buf, C.c_uint64(1), C.byref(n)) == loamx.E_INVALID
    assert L.loamx_densemap_download_surfels(None, out, C.c_uint64(1), C.byref(n), 0, C.byref(cfg), None) == loamx.E_INVALID
    assert L.loamx_densemap_save_pcd_surfels(None, b"x.pcd", 0, C.byref(cfg), None) == loamx.E_INVALID


def _compare(idx, vals, mom, want_has, **kw):
    """loamx.surfel_of against the model on one voxel, both axes; returns (the library's LOAM-frame record, the model's details)"""
    got0 = None
    for axes in ("loam", "sensor"):
        got = loamx.surfel_of(LEAF, idx, vals, mom, axes=axes, **kw)
        want, info = mm.surfel_of(LEAF, idx, vals, mom, axes=axes, **{k: v for k, v in kw.items() if v is not None})
        assert info["has"] == want_has, info
        assert got[:4].tobytes() == want[:4].tobytes()           # the bytes of the plain export
        if want_has:
            lam = info["lam"]
            assert lam[1] - lam[0] >= 1e-6 * lam[2], lam       # (the gap the tolerance relies on)
            assert np.abs(got[4:7] - want[4:7]).max() <= TOL, (got, want)
            assert abs(float(got[7]) - float(want[7])) <= TOL
            assert abs(float(np.linalg.norm(got[4:7].astype(np.float64))) - 1.0) <= TOL
        else:
            assert not got[4:].any()
        if axes == "loam":
            got0 = got
        else:   # the normal is permuted like the position: x_s = z, y_s = x, z_s = y
            assert got[[0, 1, 2, 4, 5, 6]].tobytes() == got0[[2, 0, 1, 6, 4, 5]].tobytes()
            assert got[3] == got0[3] and got[7] == got0[7]
    return got0, info


def test_too_few_points_have_no_surfel():
    for q in ([[5, 6, 7]], [[5, 6, 7], [900, 10, 20]]):
        vals, mom = mm.words_of_q(q)
        for mp in (None, 3):
            _compare((1, -2, 3), vals, mom, False, min_points=mp)
    # n == min_points is enough, n == min_points - 1 is not
    rng = np.random.default_rng(1)
    q = rng.integers(0, Q + 1, (5, 3))
    _compare((0, 0, 0), *mm.words_of_q(q), True)
    _compare((0, 0, 0), *mm.words_of_q(q[:4]), False)
    _compare((0, 0, 0), *mm.words_of_q(q[:4]), True, min_points=4)
    # every point the same: the scatter's trace is exactly 0
    _compare((0, 0, 0), *mm.words_of_q([[Q, 3, 9]] * 8), False)


def test_collinear_points_have_no_surfel():
    q = [[100 + 1000 * k, 7 + 2000 * k, 90000 + 3000 * k] for k in range(10)]
    _compare((4, 4, -4), *mm.words_of_q(q), False)
    _compare((4, 4, -4), *mm.words_of_q(q[:3]), False, min_points=3)
    q = [[5, 1000 * k * k, 77] for k in range(10)]   # along one axis
    _compare((0, 0, 0), *mm.words_of_q(q), False)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exactly_coplanar_on_an_axis_plane(axis):
    rng = np.random.default_rng(10 + axis)
    q = rng.integers(0, Q + 1, (40, 3))
    q[:, axis] = 123456
    w = np.zeros((40, 3), np.int64)
    w[:, axis] = 2000            # the sensors are on the low side: the normal points down the axis
    got, info = _compare((-3, 0, 2), *mm.words_of_q(q, w), True)
    want = np.zeros(3, np.float32)
    want[axis] = -1.0
    assert np.array_equal(got[4:7], want) and got[7] == 0.0   # exact zeros stay exact
    w[:, axis] = -2000
    got, _ = _compare((-3, 0, 2), *mm.words_of_q(q, w), True)
    assert np.array_equal(got[4:7], -want)
    # V exactly 0, and V inside the plane (the dot product is exactly 0): the first non-zero component is positive
    for wv in (np.zeros((40, 3), np.int64), np.roll(np.array([[0, 5000, -300]] * 40, np.int64), axis, axis=1)):
        assert not wv[:, axis].any()
        got, info = _compare((-3, 0, 2), *mm.words_of_q(q, wv), True)
        assert info["dot"] == 0.0 and np.array_equal(got[4:7], -want)


def test_exactly_coplanar_on_a_tilted_plane():
    # x + 2 y - 2 z = -2000 in the offsets: unit normal (1, 2, -2) / 3
    rng = np.random.default_rng(5)
    a = 2 * rng.integers(0, 200000, 60)
    b = rng.integers(0, 200000, 60)
    q = np.stack([a, b, a // 2 + b + 1000], axis=1)
    assert np.all(q[:, 0] + 2 * q[:, 1] - 2 * q[:, 2] == -2000) and q.max() <= Q
    nrm = np.array([1.0, 2.0, -2.0]) / 3.0
    for side in (1, -1):
        w = np.tile((side * 3000 * nrm).astype(np.int64), (60, 1))
        got, info = _compare((7, -1, 0), *mm.words_of_q(q, w), True)
        assert np.abs(got[4:7] - (-side * nrm)).max() <= TOL   # it faces the sensors
        assert abs(float(got[7])) <= TOL
    # V exactly 0: the first non-zero component positive
    got, info = _compare((7, -1, 0), *mm.words_of_q(q), True)
    assert info["dot"] == 0.0 and got[4] > 0 and np.abs(got[4:7] - nrm).max() <= TOL


def test_an_isotropic_blob():
    rng = np.random.default_rng(3)
    q = rng.integers(0, Q + 1, (500, 3))
    w = rng.integers(-40000, 40000, (500, 3))
    got, info = _compare((0, 0, 0), *mm.words_of_q(q, w), True)
    assert 0.25 < got[7] <= 1.0 / 3.0 + TOL     # no direction stands out
    # with a demanding ratio the same voxel still passes (l1 / l2 is near 1), an elongated one does not
    _compare((0, 0, 0), *mm.words_of_q(q, w), True, min_planar_ratio=0.5)
    q[:, 1] //= 16
    q[:, 2] //= 256
    _compare((0, 0, 0), *mm.words_of_q(q, w), False, min_planar_ratio=0.5)
    _compare((0, 0, 0), *mm.words_of_q(q, w), True, min_planar_ratio=0.0)


def test_the_128_bit_path():
    # 2^24 - 1 points on the corners (Q, 0, 0), (0, Q, 0), (0, 0, Q): n * Mxx is about 2^86, and the plane x + y + z = Q is exact
    n = (1 << 24) - 1
    k = [n // 3 + 5, n // 3 - 1000, n - 2 * (n // 3) + 995]
    assert sum(k) == n
    vals = [n, k[0] * Q, k[1] * Q, k[2] * Q]
    mom = [k[0] * Q * Q, k[1] * Q * Q, k[2] * Q * Q, 0, 0, 0, 3 * n, 5 * n, -2 * n]
    assert max(mom[:3]) < 1 << 64 and n * mom[0] > 1 << 84
    N = mm.scatter_of(vals, mom)
    assert N[0][0] == n * k[0] * Q * Q - (k[0] * Q) ** 2 and N[0][1] == -k[0] * k[1] * Q * Q
    got, info = _compare((1 << 19, -(1 << 19), 0), vals, [m % (1 << 64) for m in mom], True)
    nrm = np.ones(3) / np.sqrt(3.0)
    assert np.abs(got[4:7] + nrm).max() <= TOL and abs(float(got[7])) <= TOL   # V . (1, 1, 1) > 0: the normal is the negative one
    # one of the points moved to a fourth corner, (0, Q, Q): no longer an exact plane
    k2 = [k[0] - 1, k[1] + 1, k[2] + 1]
    vals2 = [n] + [x * Q for x in k2]
    mom2 = [x * Q * Q for x in k2] + [0, 0, Q * Q] + [m % (1 << 64) for m in mom[6:]]
    got2, _ = _compare((0, 0, 0), vals2, mom2, True)
    assert 0 < got2[7] < 1e-6


def test_the_sign_follows_the_viewpoint():
    rng = np.random.default_rng(8)
    q = rng.integers(0, Q + 1, (200, 3))
    q[:, 1] = 500000 + rng.integers(-3000, 3000, 200)   # a thin slab across y
    for v, sign in (((100, 900, -50), -1.0), ((100, -900, -50), 1.0), ((-(1 << 30), -(1 << 30), 0), 1.0)):
        w = np.tile(np.array(v, np.int64), (200, 1))
        got, info = _compare((0, 1, 2), *mm.words_of_q(q, w), True)
        assert info["v"] == [200 * x for x in v]            # (negative sums come back from their two's complement)
        assert np.sign(got[5]) == sign and abs(got[5]) > 0.99
        assert 0 < got[7] < 1e-3


def test_model_covariance_equals_the_float64_covariance():
    rng = np.random.default_rng(12)
    q = rng.integers(0, Q + 1, (300, 3))
    vals, mom = mm.words_of_q(q)
    N = mm.scatter_of(vals, mom)
    C_int = np.array([[float(N[a][b]) for b in range(3)] for a in range(3)]) / float(len(q)) ** 2
    C_f64 = np.cov(q.astype(np.float64).T, bias=True)
    assert np.abs(C_int - C_f64).max() <= 1e-9 * np.abs(C_f64).max()


def test_model_terms_by_hand():
    # leaf 0.5: the point (0.3, -0.2, 1.0) lies in voxel (0, -1, 2) at the offsets (0.6, 0.6, 0) of its edge
    p = np.array([[0.3, -0.2, 1.0, 0]], np.float32)
    o = (1.0, 0.5, -2.0)
    m = mm.MomentsModel(leaf=LEAF)
    m.add(p, o)
    m.add(p, o)
    t = [float(np.float32(c) * np.float32(2.0)) for c in (0.3, -0.2, 1.0)]
    q = [int((x - np.floor(x)) * (1 << 20)) for x in t]
    d = np.float32([0.3, -0.2, 1.0]) - np.float32(o)
    w = [int(np.float32(x) * np.float32(1024.0)) for x in d]   # (int() truncates toward zero)
    assert w[0] < 0 and w[1] < 0 and w[2] == 3072
    assert mm.idx_of(m.keys[0]) == (0, -1, 2)
    want = [2 * q[a] * q[b] for a, b in mm.PAIRS] + [(2 * x) % (1 << 64) for x in w]
    assert m.moments().tolist() == [want]
    assert m.vals.tolist() == [[2] + [2 * x for x in q]]
