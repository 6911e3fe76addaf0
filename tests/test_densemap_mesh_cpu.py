"""CPU: the dense map's signed distance field and mesh (include/loamx.h, loamx_densemap_tsdf_* and loamx_densemap_mesh) — every new
symbol declared and exported, the two structs laid out as a C compiler lays them out, the defaults, every bound of
loamx_densemap_tsdf_check, loamx_densemap_tsdf_window against its formula, the PLY writer; and properties of the model the GPU tests
check the device against (tests/densemap_mesh_model.py) that do not depend on the device kernels, so that a model and a kernel that
are wrong together still trip: the triangle rule of a tetrahedron against the gradient of a linear field, and the meshes of the two
scenes as surfaces (closed, oriented, of the right genus, where the scene is)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_mesh_model as mm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_tsdf_default_config", "loamx_densemap_tsdf_check", "loamx_densemap_tsdf_window", "loamx_densemap_tsdf_begin",
               "loamx_densemap_tsdf_add", "loamx_densemap_tsdf_add_from_map", "loamx_densemap_tsdf_add_from_pipeline",
               "loamx_densemap_tsdf_add_from_history", "loamx_densemap_tsdf_download", "loamx_densemap_mesh_default_config",
               "loamx_densemap_mesh", "loamx_write_ply", "loamx_densemap_save_ply")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_tsdf_config;" in hdr and "} loamx_densemap_mesh_config;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("tsdf_begin", "tsdf_add", "tsdf_add_from", "tsdf_add_from_pipeline", "tsdf_add_history", "tsdf", "mesh", "save_ply"):
        assert callable(getattr(loamx.DenseMap, name)), name
    for name in ("tsdf_window", "write_ply", "TsdfConfig", "MeshConfig"):
        assert callable(getattr(loamx, name)), name
    assert loamx.TSDF_STATS == mm.TSDF_STATS and loamx.MESH_STATS == mm.MESH_STATS
    assert "W < 2^25" in hdr   # the range in which every later step is exact


def test_struct_layout_matches_c(tmp_path):
    fields = [f for f, _ in loamx.TsdfConfig._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_densemap_tsdf_config));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_densemap_tsdf_config, {f}));\n' for f in fields) +
                     '  printf("%zu %zu %zu\\n", sizeof(loamx_densemap_mesh_config), offsetof(loamx_densemap_mesh_config, min_weight),'
                     ' offsetof(loamx_densemap_mesh_config, axes));\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(loamx.TsdfConfig) == 48
    assert got[1:-3] == [getattr(loamx.TsdfConfig, f).offset for f in fields] and fields == list(mm.DEFAULTS)
    assert got[-3:] == [8, 0, 4] == [C.sizeof(loamx.MeshConfig), loamx.MeshConfig.min_weight.offset, loamx.MeshConfig.axes.offset]


def test_defaults():
    c = loamx.TsdfConfig()
    assert {f: getattr(c, f) for f, _ in c._fields_} == mm.DEFAULTS
    assert mm.DEFAULTS == dict(x0=-64, y0=-64, z0=-64, nx=128, ny=128, nz=128, trunc_leaves=3.0, free_space=0, ray_stride=1,
                               max_steps=4096, min_range=0.0, max_range=0.0)
    loamx.lib().loamx_densemap_tsdf_default_config(None)   # NULL: nothing to fill
    loamx.lib().loamx_densemap_mesh_default_config(None)
    assert c.check() is c and mm.check(mm.DEFAULTS) is None
    m = loamx.MeshConfig()
    loamx.lib().loamx_densemap_mesh_default_config(C.byref(m))
    assert (m.min_weight, m.axes) == (2, 0)


# (field, values accepted at the edge of the bound, values refused just beyond it, fields set beside it)
BOUNDS = [("x0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("y0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("z0", (-2 ** 21, 2 ** 21), (-2 ** 21 - 1, 2 ** 21 + 1), {}),
          ("nx", (2, 1024), (0, 1, 1025), dict(ny=8, nz=8)),
          ("ny", (2, 1024), (0, 1, 1025), dict(nx=8, nz=8)),
          ("nz", (2, 1024), (0, 1, 1025), dict(nx=8, ny=8)),
          ("trunc_leaves", (1.0, 16.0), (0.5, 16.5, float("nan")), {}),
          ("free_space", (0, 1), (2,), {}),
          ("ray_stride", (1, 2 ** 32 - 1), (0,), {}),
          ("max_steps", (1, 65536), (0, 65537), {}),
          ("min_range", (0.0, 5.0), (-1.0, float("inf")), {}),
          ("max_range", (0.0, 7.0), (-1.0, float("inf")), {}),
          ("max_range", (3.0,), (2.5,), dict(min_range=3.0))]


@pytest.mark.parametrize("field,good,bad,beside", BOUNDS, ids=[f"{b[0]}{'_' + '_'.join(b[3]) if b[3] else ''}" for b in BOUNDS])
def test_check_bounds(field, good, bad, beside):
    L = loamx.lib()
    for v in good:
        c = loamx.TsdfConfig(**beside, **{field: v})
        assert L.loamx_densemap_tsdf_check(C.byref(c)) == loamx.OK, (field, v)
        assert mm.check(dict(mm.DEFAULTS, **beside, **{field: v})) is None
    for v in bad:
        c = loamx.TsdfConfig(**beside, **{field: v})
        assert L.loamx_densemap_tsdf_check(C.byref(c)) == loamx.E_INVALID, (field, v)
        assert field.encode() in L.loamx_last_error(), (field, L.loamx_last_error())
        assert mm.check(dict(mm.DEFAULTS, **beside, **{field: v})) == field
        with pytest.raises(loamx.LoamxError):
            c.check()


def test_check_the_product_and_null():
    L = loamx.lib()
    for shape, ok in (((1024, 64, 1024), True), ((1024, 65, 1024), False), ((512, 512, 256), True), ((512, 512, 257), False)):
        c = loamx.TsdfConfig(nx=shape[0], ny=shape[1], nz=shape[2])
        want = dict(mm.DEFAULTS, nx=shape[0], ny=shape[1], nz=shape[2])
        assert (L.loamx_densemap_tsdf_check(C.byref(c)) == loamx.OK) == ok == (mm.check(want) is None), shape
        if not ok:
            assert b"nx * ny * nz" in L.loamx_last_error() and mm.check(want) == "nx * ny * nz"
    assert L.loamx_densemap_tsdf_check(None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    c = loamx.TsdfConfig(nx=0, max_steps=0)   # the first field out of bounds is the one named
    assert L.loamx_densemap_tsdf_check(C.byref(c)) == loamx.E_INVALID and b"nx" in L.loamx_last_error()


@pytest.mark.parametrize("leaf,centre,half", [(0.25, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0)),     # exactly on cell edges: 17 cells
                                              (0.1, (12.34, -0.05, 1.0), (5.0, 3.0, 2.5)),    # a leaf that is no binary fraction
                                              (0.5, (-7.3, 2.2, 0.4), (4.0, 1.0, 0.0)),       # no extent: still two cells
                                              (0.05, (1.3, 0.0, 0.0), (0.2, 0.15, 0.15))])
def test_tsdf_window(leaf, centre, half):
    c = loamx.tsdf_window(leaf, *centre, half, trunc_leaves=2.0)
    for a, (first, count) in enumerate((("x0", "nx"), ("y0", "ny"), ("z0", "nz"))):
        assert (getattr(c, first), getattr(c, count)) == mm.window(leaf, centre[a], half[a]), first
    assert c.trunc_leaves == 2.0 and c.max_steps == 4096 and c.check() is c   # the other fields are left alone
    if leaf == 0.25:
        assert (c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (-8, 17, -8, 17, -8, 17)
    if leaf == 0.5:
        assert (c.z0, c.nz) == (0, 2)
    assert bytes(loamx.tsdf_window(0.5, 1.0, 2.0, 3.0, 4.0)) == bytes(loamx.tsdf_window(0.5, 1.0, 2.0, 3.0, (4.0, 4.0, 4.0)))


def test_tsdf_window_refusals():
    L = loamx.lib()
    c = loamx.TsdfConfig(x0=5, nx=7)
    F3 = C.c_float * 3
    for leaf, centre, half, word in ((0.5, (0, 0, 0), (300.0, 1, 1), b"nx"), (0.5, (0, 0, 0), (1, 256.25, 1), b"ny"),
                                     (0.5, (0, 0, 0), (1, 1, 1e4), b"nz"), (0.5, (2e6, 0, 0), (1, 1, 1), b"x0"),
                                     (0.5, (0, -2e6, 0), (1, 1, 1), b"y0"), (0.5, (0, 0, 2e6), (1, 1, 1), b"z0"),
                                     (0.5, (0, 0, 0), (255.75, 255.75, 255.75), b"nx * ny * nz"), (0.0, (0, 0, 0), (1, 1, 1), b"leaf"),
                                     (0.5, (np.nan, 0, 0), (1, 1, 1), b"centre"), (0.5, (0, 0, 0), (1, -1.0, 1), b"half_extent")):
        assert L.loamx_densemap_tsdf_window(C.c_float(leaf), F3(*centre), F3(*half), C.byref(c)) == loamx.E_INVALID, (centre, half)
        assert word in L.loamx_last_error(), (word, L.loamx_last_error())
        assert (c.x0, c.nx, c.y0, c.ny, c.z0, c.nz) == (5, 7, -64, 128, -64, 128)    # unchanged
    assert L.loamx_densemap_tsdf_window(C.c_float(0.5), F3(), F3(), None) == loamx.E_INVALID
    assert L.loamx_densemap_tsdf_window(C.c_float(0.5), None, F3(), C.byref(c)) == loamx.E_INVALID and b"centre" in L.loamx_last_error()


def test_null_handle_is_refused_without_a_device():
    L = loamx.lib()
    st = (C.c_uint64 * 8)()
    n = C.c_uint64(77)
    cloud = loamx.cloud_of(np.zeros((2, 4), np.float32))
    o = (C.c_float * 3)()
    for rc in (L.loamx_densemap_tsdf_begin(None, None), L.loamx_densemap_tsdf_add(None, C.byref(cloud), o),
               L.loamx_densemap_tsdf_add_from_map(None, None), L.loamx_densemap_tsdf_add_from_pipeline(None, None, 0),
               L.loamx_densemap_tsdf_add_from_history(None, C.c_uint64(0), C.c_uint64(1), None),
               L.loamx_densemap_tsdf_download(None, None, None, st),
               L.loamx_densemap_mesh(None, None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n), C.byref(n), st),
               L.loamx_densemap_save_ply(None, None, b"/nonexistent/x.ply", st)):
        assert rc == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error()
    assert n.value == 77


# ---- the PLY writer, through the binding, against a reader written from the format
def test_ply_round_trip(tmp_path):
    verts, tris, _ = mm.scene_mesh("wall")
    path = str(tmp_path / "wall.ply")
    loamx.write_ply(path, verts, tris)
    v, t = mm.read_ply(path)
    assert v.tobytes() == verts.tobytes() and t.dtype == np.dtype("<i4") and np.array_equal(t, tris.astype(np.int64))
    loamx.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))   # an empty mesh is a header
    v, t = mm.read_ply(path)
    assert len(v) == 0 and len(t) == 0
    L = loamx.lib()
    bad = np.array([[0, 1, 3]], np.uint32)   # an index beyond the vertices
    three = np.zeros((3, 3), np.float32)
    assert L.loamx_write_ply(path.encode(), three.ctypes.data_as(C.c_void_p), C.c_uint64(3), bad.ctypes.data_as(C.c_void_p),
                             C.c_uint64(1)) == loamx.E_INVALID and b"tris" in L.loamx_last_error()
    assert L.loamx_write_ply(None, None, C.c_uint64(0), None, C.c_uint64(0)) == loamx.E_INVALID and b"path" in L.loamx_last_error()
    assert L.loamx_write_ply(path.encode(), None, C.c_uint64(3), None, C.c_uint64(0)) == loamx.E_INVALID and b"verts" in L.loamx_last_error()
    with pytest.raises(loamx.LoamxError):
        loamx.write_ply(str(tmp_path / "no" / "such" / "dir.ply"), verts, tris)


# ---- the triangle rule against geometry: no table, no model of the whole mesh
def test_tetrahedron_rule_faces_the_positive_side():
    """For every tetrahedron of the split and every sign pattern with a crossing, a linear field with that pattern exists (the
    corners are affinely independent); the triangles the rule gives, with vertices interpolated on their edges, must have
    (v1 - v0) x (v2 - v0) along the field's gradient, the positive side, and a quad's two triangles the same."""
    corner_xyz = lambda n: np.array([n & 1, (n >> 1) & 1, n >> 2], np.float64)
    seen = 0
    for t, (a, b, _) in enumerate(mm.ORDERS):
        corner = (0, a, a | b, 7)
        P = np.array([corner_xyz(n) for n in corner])
        # the six tetrahedra fill the cube, each with volume 1/6, and f is the sign of its orientation
        det = np.linalg.det(P[1:] - P[0])
        assert abs(abs(det) - 1.0) < 1e-12 and (det > 0) == (mm.PARITY[t] == 0), (t, det)
        for inside in itertools.product((False, True), repeat=4):
            tris = mm.tet_triangles(list(inside), mm.PARITY[t])
            if sum(inside) in (0, 4):
                assert tris == []
                continue
            phi = np.array([-1.0 if s else 1.5 for s in inside])      # the corner values: inside is negative
            g = np.linalg.solve(np.c_[P, np.ones(4)], phi)[:3]         # the gradient of the linear field through them
            assert len(tris) == (2 if sum(inside) == 2 else 1)
            for tri in tris:
                v = []
                for i, j in tri:
                    assert i < j and inside[i] != inside[j]               # a vertex lies on a crossing edge, named lower corner first
                    s = phi[i] / (phi[i] - phi[j])
                    v.append(P[i] + s * (P[j] - P[i]))
                n = np.cross(v[1] - v[0], v[2] - v[0])
                assert np.linalg.norm(n) > 1e-9 and n @ g > 0.999 * np.linalg.norm(n) * np.linalg.norm(g), (t, inside, tri)
                seen += 1
    assert seen == 6 * (8 * 1 + 6 * 2)


def test_split_is_face_compatible():
    """the diagonals the six tetrahedra put on a cube's faces are the same on opposite faces, so neighbouring cubes agree"""
    diag = {}
    for a, b, _ in mm.ORDERS:
        corner = (0, a, a | b, 7)
        for i, j in itertools.combinations(range(4), 2):
            e = corner[i] ^ corner[j]
            if bin(e).count("1") == 2:   # a face diagonal
                axis = 7 ^ e             # the face's normal axis
                side = bool(corner[i] & axis)
                assert bool(corner[j] & axis) == side
                diag.setdefault((axis, side), set()).add((corner[i] & ~axis, corner[j] & ~axis))
    assert len(diag) == 6 and all(len(v) == 1 for v in diag.values())
    for axis in (1, 2, 4):
        assert diag[axis, False] == diag[axis, True]


# ---- the two scenes as surfaces
def test_sphere_is_a_closed_oriented_sphere():
    S = mm.SPHERE
    t, pts, origin = mm.scene("sphere")
    st = t.stats()
    assert (st["traced"], st["skipped_stride"], st["skipped_filter"], st["skipped_steps"], st["zero_length"]) == (2500, 0, 0, 0, 0)
    assert st["cells_visited"] == int(t.W.sum()) and st["max_weight"] < 2 ** 25
    verts, tris, ms = mm.scene_mesh("sphere")
    und, twice = mm.topology(tris)
    assert set(und.values()) == {2}, "every undirected edge lies in exactly two triangles"
    assert twice == [], "no directed edge occurs twice"
    V, E, Fc = len(verts), len(und), len(tris)
    assert V - E + Fc == 2 and ms["holes"] == 0 and (ms["vertices"], ms["triangles"]) == (V, Fc)
    assert (V, E, Fc) == (1466, 4392, 2928)   # the counts the rule's first prototype gave for this scene
    n = mm.normals(verts, tris)
    centroid = verts.astype(np.float64)[tris.astype(np.int64)].mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", n, np.float64(origin) - centroid) > 0), "every normal faces the sensor"
    r = np.linalg.norm(verts.astype(np.float64), axis=1)
    assert np.all(np.abs(r - S["R"]) < 0.5 * S["leaf"]), (r.min(), r.max())
    # sensor axes: the same surface with (x, y, z) -> (z, x, y), an even permutation: the orientation stays
    vs, ts, _ = mm.scene_mesh("sphere", "sensor")
    assert np.array_equal(ts, tris) and vs.tobytes() == np.ascontiguousarray(verts[:, [2, 0, 1]]).tobytes()


def test_wall_is_a_disc_on_the_plane():
    Wl = mm.WALL
    verts, tris, ms = mm.scene_mesh("wall")
    und, twice = mm.topology(tris)
    assert len(tris) > 100 and set(und.values()) == {1, 2} and twice == []
    assert mm.boundary_loops(und) == 1, "the boundary is one loop"
    assert len(verts) - len(und) + len(tris) == 1     # a disc
    dev = np.abs(verts[:, 0].astype(np.float64) - Wl["x"])
    assert dev.max() < 0.05 * Wl["leaf"], dev.max() / Wl["leaf"]
    assert np.all(mm.normals(verts, tris)[:, 0] < 0), "every normal faces the sensor, at x = 0"
    # the window's lateral faces cut the mesh: its boundary vertices lie on the outermost cell centres
    c = Wl["cfg"]
    lo = (np.array([c["y0"], c["z0"]]) + 0.5) * Wl["leaf"]
    hi = (np.array([c["y0"] + c["ny"], c["z0"] + c["nz"]]) - 0.5) * Wl["leaf"]
    assert np.allclose(verts[:, 1:].min(axis=0), lo, atol=1e-6) and np.allclose(verts[:, 1:].max(axis=0), hi, atol=1e-6)


def test_model_sums_do_not_depend_on_order_or_split():
    S = mm.SPHERE
    t, pts, origin = mm.scene("sphere")
    u = mm.Tsdf(S["leaf"], **S["cfg"])
    u.add(pts[1250:][::-1], origin)
    u.add(pts[:1250][::-1], origin)
    assert u.W.tobytes() == t.W.tobytes() and u.D.tobytes() == t.D.tobytes() and u.stats() == t.stats()
