"""CPU: the dense global map's C-ABI (loamx_densemap_*, loamx_write_pcd; include/loamx.h) — declared and exported, laid out as a C compiler
lays it out, failing loudly without a GPU; the host-only PCD writer; and the numpy model the GPU tests check the device against
(tests/densemap_model.py), checked here against voxels computed by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_model as dm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_default_config", "loamx_densemap_create", "loamx_densemap_destroy", "loamx_densemap_reset",
               "loamx_densemap_add", "loamx_densemap_add_from_map", "loamx_densemap_add_from_pipeline", "loamx_densemap_get_stats",
               "loamx_densemap_download", "loamx_densemap_save_pcd", "loamx_write_pcd")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays


def test_config_layout_matches_c(tmp_path):
    probe = tmp_path / "probe.c"
    fields = [f for f, _ in loamx.DenseMapConfig._fields_]
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_densemap_config));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_densemap_config, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(loamx.DenseMapConfig)
    assert got[1:] == [getattr(loamx.DenseMapConfig, f).offset for f in fields]


def test_default_config():
    c = loamx.DenseMapConfig()
    c.leaf, c.initial_slots, c.device = 7.0, 3, 5
    loamx.lib().loamx_densemap_default_config(C.byref(c))   # (host only: no device needed)
    assert np.float32(c.leaf) == np.float32(0.1)
    assert (c.min_range, c.max_range, c.max_voxels, c.initial_slots, c.device) == (0.0, 0.0, 0, 1 << 20, 0)


def test_create_fails_without_gpu():
    if loamx.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = loamx.lib()
    L.loamx_densemap_create.restype = C.c_void_p
    assert not L.loamx_densemap_create(None)
    with pytest.raises(loamx.LoamxError) as e:
        loamx.DenseMap()
    assert "no HIP device" in str(e.value)
    # (the error code itself: create returns NULL, the last error names LOAMX_E_NOGPU's message; a call on the class reports it)
    c = loamx.DenseMapConfig()
    L.loamx_densemap_default_config(C.byref(c))
    assert not L.loamx_densemap_create(C.byref(c))
    assert "no HIP device" in L.loamx_last_error().decode()


def _cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-50, 50, (n, 4)).astype(np.float32)
    a[:, 3] = rng.uniform(0, 16, n).astype(np.float32)
    return a


def test_write_pcd_round_trip(tmp_path):
    pts = _cloud(1000)
    for axes in ("loam", "sensor"):
        path = str(tmp_path / f"c_{axes}.pcd")
        loamx.write_pcd(path, pts, axes=axes)
        hdr, body = dm.read_pcd(path)
        assert hdr["VERSION"] == "0.7" and hdr["FIELDS"] == "x y z intensity" and hdr["SIZE"] == "4 4 4 4"
        assert hdr["TYPE"] == "F F F F" and hdr["COUNT"] == "1 1 1 1" and hdr["HEIGHT"] == "1"
        assert hdr["WIDTH"] == "1000" and hdr["POINTS"] == "1000" and hdr["DATA"] == "binary"
        want = pts if axes == "loam" else pts[:, [2, 0, 1, 3]]
        assert np.array_equal(body, want)
    # the PCL layout: 32-byte records, intensity at byte 16
    path = str(tmp_path / "pcl.pcd")
    loamx.write_pcd(path, loamx.to_pcl_layout(pts), axes="loam")
    _, body = dm.read_pcd(path)
    assert np.array_equal(body, pts)
    # empty cloud
    path = str(tmp_path / "empty.pcd")
    loamx.write_pcd(path, np.zeros((0, 4), np.float32))
    hdr, body = dm.read_pcd(path)
    assert hdr["POINTS"] == "0" and body.shape == (0, 4)


def test_write_pcd_rejects_bad_arguments(tmp_path):
    L = loamx.lib()
    pts = _cloud(4)
    c = loamx.cloud_of(pts)
    assert L.loamx_write_pcd(str(tmp_path / "x.pcd").encode(), C.byref(c), 2) == loamx.E_INVALID
    assert L.loamx_write_pcd(str(tmp_path / "no" / "such" / "dir.pcd").encode(), C.byref(c), 0) == loamx.E_INVALID


def _key(ix, iy, iz):
    return (ix + (1 << 20)) | ((iy + (1 << 20)) << 21) | ((iz + (1 << 20)) << 42)


def test_model_boundaries_and_negative_coordinates():
    # leaf 0.5 (inv = 2 exactly): points on voxel boundaries belong to the voxel they start
    pts = np.array([[0.0, 0.0, 0.0, 0], [0.5, 0.0, 0.0, 0], [-0.5, 0.0, 0.0, 0], [1.25, -0.75, 2.0, 0], [-0.25, -0.25, -0.25, 0]], np.float32)
    keys, q, dr, dk = dm.keys_of(pts, (0, 0, 0), 0.5)
    assert (dr, dk) == (0, 0)
    assert keys.tolist() == [_key(0, 0, 0), _key(1, 0, 0), _key(-1, 0, 0), _key(2, -2, 4), _key(-1, -1, -1)]
    h = 1 << 19   # offset one half
    assert q.tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [h, h, 0], [h, h, h]]
    m = dm.Model(leaf=0.5)
    m.add(pts, (0, 0, 0))
    m.add(pts[:2], (0, 0, 0))
    out = m.points()
    # ascending key = ascending (iz, iy, ix)
    want = np.array([[-0.25, -0.25, -0.25, 1], [-0.5, 0, 0, 1], [0, 0, 0, 2], [0.5, 0, 0, 2], [1.25, -0.75, 2.0, 1]], np.float32)
    assert np.array_equal(out, want)
    assert np.array_equal(m.points("sensor"), want[:, [2, 0, 1, 3]])
    assert m.stats() == dict(voxels=5, offered=7, added=7, dropped_range=0, dropped_key=0)


def test_model_key_range_and_clamp():
    leaf = 1.0
    pts = np.array([[float(1 << 20), 0, 0, 0],            # |i| = 2^20: dropped
                    [-float(1 << 20), 0, 0, 0],           # likewise
                    [float((1 << 20) - 1), 0, 0, 0],      # the last voxel inside
                    [-float((1 << 20) - 1), 0, 0, 0],
                    [np.nan, 0, 0, 0],                    # NaN: fails the range test (d2 >= 0 is false)
                    [-1e-9, 0, 0, 0]], np.float32)        # t - floor(t) rounds to 1.0f: q is clamped to 2^20 - 1
    keys, q, dr, dk = dm.keys_of(pts, (0, 0, 0), leaf)
    assert (dr, dk) == (1, 2)
    assert keys.tolist() == [_key((1 << 20) - 1, 0, 0), _key(-(1 << 20) + 1, 0, 0), _key(-1, 0, 0)]
    assert q[2].tolist() == [(1 << 20) - 1, 0, 0]
    f = np.float32(-1e-9) - np.floor(np.float32(-1e-9))
    assert f == np.float32(1.0)   # (why the clamp is there)
    m = dm.Model(leaf=leaf)
    m.add(pts, (0, 0, 0))
    assert m.stats() == dict(voxels=3, offered=6, added=3, dropped_range=1, dropped_key=2)
    rec = m.points()
    assert rec[1, 0] == np.float32(-1.0 + ((1 << 20) - 1) / float(1 << 20)) and rec[1, 3] == 1   # (keys ascending: ix -2^20 + 1, -1, 2^20 - 1)


def test_model_range_filter_and_capacity():
    pts = np.array([[1, 0, 0, 0], [3, 0, 0, 0], [10, 0, 0, 0], [0, 0, 20, 0]], np.float32)
    keys, q, dr, dk = dm.keys_of(pts, (0, 0, 0), 0.1, min_range=2.0, max_range=15.0)
    assert (len(keys), dr, dk) == (2, 2, 0)
    keys, q, dr, dk = dm.keys_of(pts, (9, 0, 0), 0.1, min_range=2.0, max_range=15.0)   # the origin moves: other points kept
    assert (len(keys), dr) == (2, 2)
    m = dm.Model(leaf=0.1, max_voxels=5)
    assert m.add(pts, (0, 0, 0))            # 0 + 4 <= 5
    assert not m.add(pts[:2], (0, 0, 0))    # 4 + 2 > 5: refused, nothing changes
    assert m.stats()["offered"] == 4
    assert m.add(pts[:1], (0, 0, 0))        # 4 + 1 <= 5
