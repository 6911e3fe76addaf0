"""CPU: the dense map's ray casts (include/loamx.h, loamx_densemap_raycast ...) — every new symbol declared and exported, the two new
structs laid out as a C compiler lays them out, the default configuration, bad arguments refused without a device, range_image_ends;
and the model the GPU tests check the device against (tests/densemap_raycast_model.py), checked here against rays worked out by hand."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_carve_model as cm
import densemap_model as dm
import densemap_raycast_model as rm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_raycast_default_config", "loamx_densemap_raycast", "loamx_densemap_raycast_from_map",
               "loamx_densemap_raycast_from_pipeline")
LEAF = 0.5
O = (0.25, 0.25, 0.25)   # the centre of cell (0, 0, 0)


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_ray_hit;" in hdr and "} loamx_densemap_raycast_config;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("raycast", "raycast_from", "raycast_from_pipeline"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert callable(loamx.range_image_ends)


@pytest.mark.parametrize("c_name,py", [("loamx_ray_hit", "RayHit"), ("loamx_densemap_raycast_config", "RaycastConfig")])
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
    if py == "RayHit":
        assert got[0] == 40 == loamx.RAY_DTYPE.itemsize == rm.RAY_DTYPE.itemsize
        assert got[1:] == [loamx.RAY_DTYPE.fields[f][1] for f in fields] == [rm.RAY_DTYPE.fields[f][1] for f in fields]
        assert loamx.RAY_DTYPE == rm.RAY_DTYPE


def test_default_configuration_and_names():
    L = loamx.lib()
    c = loamx.RaycastConfig(9, 9, 9)
    L.loamx_densemap_raycast_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.max_steps, c.skip_steps, c.min_points) == (4096, 0, 1) == tuple(rm.DEFAULTS.values())
    L.loamx_densemap_raycast_default_config(None)   # NULL: nothing to fill
    assert (loamx.RAY_NOT_TRACED, loamx.RAY_MISS, loamx.RAY_HIT, loamx.RAY_HIT_END) == (rm.NOT_TRACED, rm.MISS, rm.HIT, rm.HIT_END) == (0, 1, 2, 3)
    assert loamx.RAY_COUNTS == rm.COUNT_KEYS
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    for k, name in enumerate(("NOT_TRACED", "MISS", "HIT", "HIT_END")):
        assert f"#define LOAMX_RAY_{name} {k}\n" in hdr


def test_null_handles_are_refused_without_a_device():
    L = loamx.lib()
    ends = np.zeros((4, 4), np.float32)
    cl = loamx.cloud_of(ends)
    o = (C.c_float * 3)()
    counts = (C.c_uint64 * 5)()
    assert L.loamx_densemap_raycast(None, C.byref(cl), o, None, None, None, C.c_uint64(0), counts) == loamx.E_INVALID
    assert b"h is NULL" in L.loamx_last_error()
    assert L.loamx_densemap_raycast_from_map(None, None, None, None, None, C.c_uint64(0), counts) == loamx.E_INVALID
    assert L.loamx_densemap_raycast_from_pipeline(None, None, C.c_uint32(0), None, None, None, C.c_uint64(0), counts) == loamx.E_INVALID


# ---- the model against rays worked out by hand (leaf 0.5: inv = 2 exactly, cell i spans [0.5 i, 0.5 (i + 1)))

def pts(*xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return p


def model_of(*xyz):
    m = dm.Model(leaf=LEAF)
    if xyz:
        m.add(pts(*xyz), O)
    return m


def one(model, origin, end, **kw):
    rec, counts = rm.cast(model, pts(end), origin, **kw)
    return rec[0], counts


def test_model_zero_length_ray():
    r, c = one(model_of(), O, O)
    assert (r["status"], r["steps"], r["key"], r["n"]) == (rm.MISS, 1, 0, 0)    # one cell looked up: the origin's own
    assert c == dict(not_traced=0, miss=1, hit=0, hit_end=0, cells=1)
    r, c = one(model_of((0.3, 0.4, 0.1)), O, O)
    assert (r["status"], r["steps"], r["key"], r["n"], r["miss"]) == (rm.HIT_END, 0, cm.key_of((0, 0, 0)), 1, 0)
    assert r["range"] == 0.0 and abs(r["x"] - 0.3) < 1e-6 and abs(r["y"] - 0.4) < 1e-6 and abs(r["z"] - 0.1) < 1e-6    # L2 == 0
    assert c == dict(not_traced=0, miss=0, hit=0, hit_end=1, cells=1)


def test_model_axis_aligned_rays_across_index_zero():
    o, e = (0.75, 0.25, 0.25), (-0.75, 0.25, 0.25)    # cells (1, 0, 0), (0, 0, 0), (-1, 0, 0), (-2, 0, 0)
    r, c = one(model_of((-0.3, 0.3, 0.2)), o, e)       # a voxel in cell (-1, 0, 0)
    assert (r["status"], r["steps"], r["key"]) == (rm.HIT, 2, cm.key_of((-1, 0, 0))) and c["cells"] == 3
    assert abs(r["x"] + 0.3) < 1e-6 and abs(r["range"] - 1.05) < 1e-6    # along -x: the range is the distance in x
    r, c = one(model_of((-0.8, 0.3, 0.2)), o, e)       # in the end cell (-2, 0, 0)
    assert (r["status"], r["steps"], r["key"]) == (rm.HIT_END, 3, cm.key_of((-2, 0, 0))) and c["cells"] == 4
    r, c = one(model_of((-1.2, 0.3, 0.2), (-0.3, 0.7, 0.2)), o, e)    # behind the end, and beside the ray
    assert (r["status"], r["steps"]) == (rm.MISS, 4) and c == dict(not_traced=0, miss=1, hit=0, hit_end=0, cells=4)
    # along -z from a negative cell, the hit in the origin's own cell, behind the origin: a negative range
    r, _ = one(model_of((-0.2, -0.2, -0.05)), (-0.25, -0.25, -0.3), (-0.25, -0.25, -1.3))
    assert (r["status"], r["steps"], r["key"]) == (rm.HIT, 0, cm.key_of((-1, -1, -1))) and abs(r["range"] + 0.25) < 1e-6


def test_model_exact_diagonal_ties_go_x_y_z():
    e = (1.25, 1.25, 1.25)    # cells (0,0,0), (1,0,0), (1,1,0), (1,1,1), (2,1,1), (2,2,1), (2,2,2): every step a tie
    m = model_of((0.3, 0.6, 0.1), (0.3, 0.6, 0.6), (0.6, 0.6, 0.1))    # (0,1,0) and (0,1,1) are not on the walk; (1,1,0) is
    r, c = one(m, O, e)
    assert (r["status"], r["steps"], r["key"]) == (rm.HIT, 2, cm.key_of((1, 1, 0))) and c["cells"] == 3
    r, _ = one(model_of((0.3, 0.6, 0.1), (1.1, 1.2, 1.3)), O, e)
    assert (r["status"], r["steps"], r["key"]) == (rm.HIT_END, 6, cm.key_of((2, 2, 2)))
    assert abs(r["range"] - np.float32((0.85 + 0.95 + 1.05) / np.sqrt(3.0))) < 1e-5


def test_model_skip_steps_and_max_steps():
    e = (2.25, 0.25, 0.25)    # n_steps 4: cells (0..4, 0, 0)
    m = model_of((0.3, 0.3, 0.3), (1.3, 0.3, 0.3), (2.3, 0.3, 0.3))    # voxels in cells 0, 2 and 4
    assert [int(one(m, O, e, skip_steps=s)[0]["steps"]) for s in (0, 1, 2, 3)] == [0, 2, 2, 4]
    r, c = one(m, O, e, skip_steps=4)    # equal to n_steps: only the end cell is looked up
    assert (r["status"], r["steps"], c["cells"]) == (rm.HIT_END, 4, 1)
    r, c = one(m, O, e, skip_steps=5)    # one more: nothing is looked up
    assert (r["status"], r["steps"], r["key"]) == (rm.MISS, 0, 0) and c == dict(not_traced=0, miss=1, hit=0, hit_end=0, cells=0)
    r, c = one(model_of(), O, e, skip_steps=2)
    assert (r["status"], r["steps"]) == (rm.MISS, 3) and c["cells"] == 3    # n_steps + 1 - skip_steps
    r, c = one(m, O, e, max_steps=4)     # n_steps == max_steps: traced
    assert r["status"] == rm.HIT and c["not_traced"] == 0
    r, c = one(m, O, e, max_steps=3)     # one more step than max_steps
    assert r.tobytes() == bytes(40) and c == dict(not_traced=1, miss=0, hit=0, hit_end=0, cells=0)


def test_model_rays_that_are_not_traced():
    m = model_of((0.3, 0.3, 0.3))
    zero = dict(not_traced=1, miss=0, hit=0, hit_end=0, cells=0)
    for end in ((np.nan, 0.25, 0.25), (0.25, np.inf, 0.25), (0.25, 0.25, -np.inf),
                (524288.0, 0.25, 0.25),      # the cell i = 2^20
                (0.25, -524288.0, 0.25),     # i = -2^20
                (0.25, 0.25, -524287.75)):   # floor(-1048575.5) = -2^20 too
        r, c = one(m, O, end, max_steps=65536)
        assert r.tobytes() == bytes(40) and c == zero, end
    for origin in ((524288.0, 0.25, 0.25), (0.25, np.nan, 0.25)):    # an origin outside the key range
        r, c = one(m, origin, (0.3, 0.3, 0.3))
        assert r.tobytes() == bytes(40) and c == zero, origin
    # the last cells inside the key range on either side are fine
    r, c = one(m, (524287.75, 0.25, 0.25), (524286.75, 0.25, 0.25))
    assert (r["status"], r["steps"]) == (rm.MISS, 3)
    r, c = one(m, (-524287.25, 0.25, 0.25), (-524286.25, 0.25, 0.25))
    assert (r["status"], r["steps"]) == (rm.MISS, 3)
    # ... but a ray from one to the other has more steps than any max_steps allows
    r, c = one(m, (-524287.25, 0.25, 0.25), (524287.75, 0.25, 0.25), max_steps=65536)
    assert r["status"] == rm.NOT_TRACED and c == zero


def test_model_min_points_makes_a_voxel_transparent():
    m = model_of((1.3, 0.3, 0.3), (2.3, 0.3, 0.3), (2.4, 0.2, 0.1))    # cell (2, 0, 0) holds one point, cell (4, 0, 0) two
    e = (3.25, 0.25, 0.25)
    r, _ = one(m, O, e)
    assert (r["status"], r["steps"], r["n"]) == (rm.HIT, 2, 1)
    r, c = one(m, O, e, min_points=2)
    assert (r["status"], r["steps"], r["n"], r["key"]) == (rm.HIT, 4, 2, cm.key_of((4, 0, 0))) and c["cells"] == 5
    assert abs(r["x"] - 2.35) < 1e-6 and abs(r["range"] - 2.1) < 1e-6    # the mean of the two points
    r, _ = one(m, O, e, min_points=3)
    assert (r["status"], r["steps"]) == (rm.MISS, 7)


def test_model_a_dynamic_voxel_is_skipped_under_a_rule():
    near, far = pts((1.25, 0.25, 0.25)), pts((3.25, 0.25, 0.25))    # cells (2, 0, 0) and (6, 0, 0)
    m = cm.CarveModel(leaf=LEAF)
    m.add(near, O)
    for _ in range(4):
        m.add(far, O)    # four rays through the near voxel: 4 misses >= 3 and 4 > n = 1
    assert m.misses().tolist() == [4, 0] and m.dynamic_mask().tolist() == [True, False]
    e = (3.75, 0.25, 0.25)
    r, _ = one(m, O, e)
    assert (r["status"], r["steps"], r["n"], r["miss"]) == (rm.HIT, 2, 1, 4)
    r, c = one(m, O, e, rule=cm.DEFAULT_RULE)
    assert (r["status"], r["steps"], r["n"], r["miss"], r["key"]) == (rm.HIT, 6, 4, 0, cm.key_of((6, 0, 0))) and c["cells"] == 7
    r, _ = one(m, O, e, rule=(5, 1, 1))    # a rule that needs five misses leaves the voxel static
    assert (r["status"], r["steps"]) == (rm.HIT, 2)


def test_model_counts_and_the_scene_of_the_gpu_test():
    # the recipe of tests/test_gpu_densemap_raycast.py: 541 voxels, 23 of them dynamic, and at the smallest many-ray case every
    # status at least three times with and without the rule
    S = rm.box_cast_scene()
    m = cm.CarveModel(leaf=S["leaf"])
    for p, o in S["sweeps"]:
        m.add(p, o)
    assert len(m) == 541 and int(m.dynamic_mask().sum()) == 23
    ends = rm.box_rays(65, S["origin"], S["leaf"])
    walks = rm.walks_of(ends, S["origin"], S["leaf"])
    plain, c0 = rm.cast(m, ends, S["origin"], walks=walks)
    ruled, c1 = rm.cast(m, ends, S["origin"], walks=walks, rule=cm.DEFAULT_RULE)
    for c in (c0, c1):
        assert min(c["miss"], c["hit"], c["hit_end"]) >= 3 and c["not_traced"] == 4
    assert not rm.same_records(plain, ruled)
    hand = rm.hand_ends(S["origin"], S["leaf"])
    assert len(hand) == 13 and np.array_equal(ends[:13], hand, equal_nan=True)
    assert plain["status"][9:12].tolist() == [rm.NOT_TRACED] * 3 and plain["status"][12] == rm.NOT_TRACED    # NaN, the two edges, too long


# ---- range_image_ends

def test_range_image_ends():
    el = [-15.0, 0.0, 90.0]
    ends = loamx.range_image_ends(np.eye(3, 4), el, 4, 10.0)
    assert ends.shape == (12, 4) and ends.dtype == np.float32
    assert ends[:, 3].tolist() == [0.0] * 4 + [1.0] * 4 + [2.0] * 4
    want = {4: (0, 0, 10), 5: (10, 0, 0), 6: (0, 0, -10), 7: (-10, 0, 0), 8: (0, 10, 0)}    # forward +z, then towards +x (left); up +y
    for i, d in want.items():
        assert np.allclose(ends[i, :3], d, atol=1e-5), i
    c, s = np.cos(np.deg2rad(15.0)), np.sin(np.deg2rad(15.0))
    assert np.allclose(ends[0, :3], (0, -10 * s, 10 * c), atol=1e-5) and np.allclose(ends[1, :3], (10 * c, -10 * s, 0), atol=1e-5)
    # a pose: a quarter turn about y (z -> x) and a translation
    P = np.array([[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 3.0]])
    ends = loamx.range_image_ends(P, [0.0], 2, 5.0)
    assert ends.shape == (2, 4) and np.allclose(ends[:, :3], [(6, 2, 3), (-4, 2, 3)], atol=1e-5)
    assert loamx.range_image_ends(np.eye(3, 4), np.linspace(-15, 15, 16), 1800, 100.0).shape == (16 * 1800, 4)
