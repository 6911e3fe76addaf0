"""CPU: the dense map's free-space carving (include/loamx.h, loamx_densemap_enable_carving ...) — every new symbol declared and exported,
the two new structs laid out as a C compiler lays them out, the default configurations, bad arguments refused without a device; and the
model the GPU tests check the device against (tests/densemap_carve_model.py), checked here against rays worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_carve_model as cm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_carve_default_config", "loamx_densemap_static_rule_default", "loamx_densemap_rule_is_dynamic",
               "loamx_densemap_enable_carving", "loamx_densemap_get_carve_stats", "loamx_densemap_download_misses",
               "loamx_densemap_download_static", "loamx_densemap_save_pcd_static", "loamx_densemap_prune")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("enable_carving", "carve_stats", "misses", "prune"):
        assert callable(getattr(loamx.DenseMap, name)), name


@pytest.mark.parametrize("c_name,py", [("loamx_densemap_carve_config", "DenseMapCarveConfig"), ("loamx_densemap_static_rule", "StaticRule")])
def test_struct_layout_matches_c(tmp_path, c_name, py):
    struct = getattr(loamx, py)
    fields = [f for f, _ in struct._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(struct)
    assert got[1:] == [getattr(struct, f).offset for f in fields]


def test_header_compiles_as_cxx11(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "loamx.h"\nint main() { loamx_densemap_carve_config c; loamx_densemap_carve_default_config(&c); return 0; }\n')
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(probe)], check=True)


def test_default_configurations():
    L = loamx.lib()
    c = loamx.DenseMapCarveConfig()
    c.max_range, c.ray_stride, c.end_margin, c.max_steps = 7.0, 9, 9, 9
    L.loamx_densemap_carve_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.max_range, c.ray_stride, c.end_margin, c.max_steps) == (0.0, 1, 1, 4096)
    r = loamx.StaticRule()
    assert (r.min_misses, r.num, r.den) == (3, 1, 1) == cm.DEFAULT_RULE
    r = loamx.StaticRule(num=2)
    assert (r.min_misses, r.num, r.den) == (3, 2, 1)
    L.loamx_densemap_carve_default_config(None)   # NULL: nothing to fill
    L.loamx_densemap_static_rule_default(None)


def test_bad_arguments_are_refused_without_a_device():
    L = loamx.lib()
    rule, cfg = loamx.StaticRule(), loamx.DenseMapCarveConfig()
    s, n, removed = (C.c_uint64 * 6)(), C.c_uint64(0), C.c_uint64(0)
    out = np.zeros((4, 4), np.float32)
    cl = loamx.cloud_of(out)
    buf = (C.c_uint32 * 4)()
    assert L.loamx_densemap_enable_carving(None, C.byref(cfg)) == loamx.E_INVALID
    assert L.loamx_densemap_get_carve_stats(None, s) == loamx.E_INVALID
    assert L.loamx_densemap_download_misses(None, buf, C.c_uint64(4), C.byref(n)) == loamx.E_INVALID
    assert L.loamx_densemap_download_static(None, C.byref(cl), 0, C.byref(rule)) == loamx.E_INVALID
    assert L.loamx_densemap_save_pcd_static(None, b"x.pcd", 0, C.byref(rule)) == loamx.E_INVALID
    assert L.loamx_densemap_prune(None, C.byref(rule), C.byref(removed)) == loamx.E_INVALID
    assert b"NULL" in L.loamx_last_error()
    assert L.loamx_densemap_rule_is_dynamic(None, C.c_uint64(1), C.c_uint32(5)) == loamx.E_INVALID
    # den == 0
    bad = loamx.StaticRule(den=0)
    assert L.loamx_densemap_rule_is_dynamic(C.byref(bad), C.c_uint64(1), C.c_uint32(5)) == loamx.E_INVALID
    assert b"den" in L.loamx_last_error()
    with pytest.raises(loamx.LoamxError):
        bad.is_dynamic(1, 5)


def test_rule_equals_the_model():
    rules = [cm.DEFAULT_RULE, (0, 1, 1), (3, 2, 1), (1, 1, 3), (5, 0, 1), (2, 0xffffffff, 0xffffffff)]
    for rule in rules:
        r = loamx.StaticRule(*rule)
        for n in (1, 2, 3, 4, 10, 1 << 33):
            for miss in (0, 1, 2, 3, 4, 5, 11, 0xffffffff):
                assert r.is_dynamic(n, miss) == cm.is_dynamic(rule, n, miss), (rule, n, miss)
    assert not loamx.StaticRule().is_dynamic(3, 3) and loamx.StaticRule().is_dynamic(3, 4) and not loamx.StaticRule().is_dynamic(1, 2)


# ---- the model against rays worked out by hand (leaf 0.5: inv = 2 exactly, cell i spans [0.5 i, 0.5 (i + 1)))

def test_model_axis_aligned_ray():
    cells, n = cm.trace((0.25, 0.25, 0.25), (2.25, 0.25, 0.25), 0.5)
    assert n == 4
    assert cells == [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)]
    assert cm.visited(cells, n, 1) == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    assert cm.visited(cells, n, 0) == cells[:4]   # the end cell is never visited
    # along z, the other two axes never move
    cells, n = cm.trace((0.1, 0.2, 0.3), (0.1, 0.2, 1.3), 0.5)
    assert (cells, n) == ([(0, 0, 0), (0, 0, 1), (0, 0, 2)], 2)


def test_model_negative_direction_across_index_zero():
    cells, n = cm.trace((0.75, 0.25, 0.25), (-0.75, 0.25, 0.25), 0.5)
    assert n == 3
    assert cells == [(1, 0, 0), (0, 0, 0), (-1, 0, 0), (-2, 0, 0)]
    # an oblique one by hand: from (0.25, 0.25) to (-0.6, -0.25), in voxel units (0.5, 0.5) -> (-1.2, -0.5): d = (-1.7, -1.0);
    # tmax_x = (0 - 0.5) / -1.7 = 0.294, tmax_y = (0 - 0.5) / -1.0 = 0.5: x, then y, then x again at 0.294 + 1 / 1.7 = 0.882
    cells, n = cm.trace((0.25, 0.25, 0.1), (-0.6, -0.25, 0.1), 0.5)
    assert n == 3
    assert cells == [(0, 0, 0), (-1, 0, 0), (-1, -1, 0), (-2, -1, 0)]
    # a negative origin, and a negative point exactly on a cell boundary (voxel units -2.0: cell -2)
    cells, n = cm.trace((-0.25, -0.25, -0.25), (-1.0, -0.25, -0.25), 0.5)
    assert (cells, n) == ([(-1, -1, -1), (-2, -1, -1)], 1)


def test_model_exact_diagonal_ties_go_x_y_z():
    # from the centre of cell (0, 0, 0) to the centre of cell (2, 2, 2): every tmax is 1/4, then 3/4 — all ties
    cells, n = cm.trace((0.25, 0.25, 0.25), (1.25, 1.25, 1.25), 0.5)
    assert n == 6
    assert cells == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]
    # and in the negative direction
    cells, n = cm.trace((0.25, 0.25, 0.25), (-0.25, -0.25, -0.25), 0.5)
    assert cells == [(0, 0, 0), (-1, 0, 0), (-1, -1, 0), (-1, -1, -1)]


@pytest.mark.parametrize("end_margin", [0, 1, 2])
def test_model_short_rays(end_margin):
    o = (0.25, 0.25, 0.25)
    # n_steps 0 (the point in the origin's cell), 1, and end_margin + 1: the first ray that visits anything beyond margin 0
    cells, n = cm.trace(o, (0.3, 0.4, 0.1), 0.5)
    assert (cells, n) == ([(0, 0, 0)], 0)
    assert cm.visited(cells, n, end_margin) == []
    cells, n = cm.trace(o, (0.25, 0.75, 0.25), 0.5)
    assert (cells, n) == ([(0, 0, 0), (0, 1, 0)], 1)
    assert cm.visited(cells, n, end_margin) == ([(0, 0, 0)] if end_margin == 0 else [])
    p = (0.25 + 0.5 * (end_margin + 1), 0.25, 0.25)
    cells, n = cm.trace(o, p, 0.5)
    assert n == end_margin + 1
    assert cm.visited(cells, n, end_margin) == [(0, 0, 0)]


def test_model_origin_outside_the_key_range():
    assert cm.trace((float(1 << 20), 0, 0), (1.0, 0, 0), 1.0) == (None, None)
    assert cm.trace((np.nan, 0, 0), (1.0, 0, 0), 1.0) == (None, None)
    cells, n = cm.trace((float((1 << 20) - 1), 0, 0), (float((1 << 20) - 3), 0, 0), 1.0)
    assert n == 2 and cells[0] == ((1 << 20) - 1, 0, 0)


def test_model_occupied_wins_and_statistics():
    leaf = 0.5
    o = (0.25, 0.25, 0.25)
    near = np.array([[1.25, 0.25, 0.25, 0]], np.float32)   # cell (2, 0, 0)
    far = np.array([[3.25, 0.25, 0.25, 0]], np.float32)    # cell (6, 0, 0): its ray crosses (0..4, 0, 0), margin 1 spares (5, 0, 0)
    m = cm.CarveModel(leaf=leaf)
    m.add(np.concatenate([near, far]), o)   # one call: the near voxel is hit by the same call
    assert m.misses().tolist() == [0, 0]
    assert m.carve_stats() == dict(traced=2, skipped_stride=0, skipped_range=0, skipped_steps=0, cells_visited=1 + 5, misses=0)
    m = cm.CarveModel(leaf=leaf)
    m.add(near, o)
    m.add(far, o)                           # two calls: the far ray finds the near voxel with an older stamp
    assert m.misses().tolist() == [1, 0]
    assert m.carve_stats()["misses"] == 1
    for _ in range(3):
        m.add(far, o)
    assert m.misses().tolist() == [4, 0]
    assert m.dynamic_mask().tolist() == [True, False]    # 4 misses >= 3 and 4 > n = 1
    assert len(m.points(static=cm.DEFAULT_RULE)) == 1 and len(m.points()) == 2
    assert m.prune() == 1 and len(m) == 1 and m.misses().tolist() == [0]
    # stride, range and step limits each count on their own
    pts = np.array([[0.25 + 0.5 * k, 0.25, 0.25, 0] for k in range(1, 11)], np.float32)
    m = cm.CarveModel(leaf=leaf, ray_stride=3)
    m.add(pts, o)
    assert (m.carve_stats()["traced"], m.carve_stats()["skipped_stride"]) == (4, 6)   # indices 0, 3, 6, 9
    m = cm.CarveModel(leaf=leaf, max_steps=4)
    m.add(pts, o)
    assert (m.carve_stats()["traced"], m.carve_stats()["skipped_steps"]) == (4, 6)    # n_steps 1..4 traced, 5..10 not
    m = cm.CarveModel(leaf=leaf, carve_max_range=2.0)
    m.add(pts, o)
    assert (m.carve_stats()["traced"], m.carve_stats()["skipped_range"]) == (4, 6)    # distances 0.5 .. 2.0 traced (<=)
