"""GPU: the dense map's signed distance field and its mesh (include/loamx.h, loamx_densemap_tsdf_* and loamx_densemap_mesh) against
their model (tests/densemap_mesh_model.py).  Every compared quantity is an integer or an f32 with one defined value: the bytes of W,
of D, of the vertices and of the indices equal the model's, no tolerance anywhere.  The scenes are the model's (a sphere of 1.25 m in
a 16^3 window of 0.25 m cells seen from inside by 2,500 rays; a wall seen by 41 x 41), small enough that the model's plain Python
loops take a fraction of a second; tests/test_densemap_mesh_cpu.py holds what makes the model itself trustworthy."""
import ctypes as C

import numpy as np
import pytest

import densemap_mesh_model as mm
import densemap_rebuild_model as rbm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

S = mm.SPHERE


def new_map(leaf=S["leaf"]):
    return loamx.DenseMap(leaf=leaf, initial_slots=1024)


def device_field(d, sweeps, **cfg):
    c = d.tsdf_begin(**cfg)
    for p, o in sweeps:
        assert d.tsdf_add(p, o) == loamx.OK
    return (*d.tsdf(c), c)


def model_field(leaf, sweeps, **cfg):
    t = mm.Tsdf(leaf, **cfg)
    for p, o in sweeps:
        t.add(p, o)
    return t


def explain(W, D, st, t):
    for name, g, w in (("W", W, t.W), ("D", D, t.D)):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"{name}: {g.shape} {g.dtype}, {w.shape} {w.dtype}"
        for z, y, x in np.argwhere(g != w).tolist():
            return f"{name}[z {z}, y {y}, x {x}]: got {g[z, y, x]}, want {w[z, y, x]} ({int((g != w).sum())} cells differ)"
    return f"stats: got {st}, want {t.stats()}"


def check_field(got, t):
    W, D, st = got[:3]
    ok = W.dtype == np.uint32 and D.dtype == np.int64 and W.tobytes() == t.W.tobytes() and D.tobytes() == t.D.tobytes() and st == t.stats()
    assert ok, explain(W, D, st, t)


def check_mesh(d, t, min_weight=2, axes="loam"):
    """the device's mesh of the field that stands against the model's of t; returns the model's"""
    c = t.cfg
    want = mm.mesh(t.W, t.D, t.leaf, c["x0"], c["y0"], c["z0"], min_weight, axes)
    v, tr, st = d.mesh(min_weight=min_weight, axes=axes)
    assert st == want[2], (st, want[2])
    assert v.dtype == np.float32 and tr.dtype == np.uint32 and v.shape == want[0].shape and tr.shape == want[1].shape
    if v.tobytes() != want[0].tobytes():
        i = int(np.argwhere((v.view(np.uint32) != want[0].view(np.uint32)).any(axis=1))[0, 0])
        raise AssertionError(f"vertex {i}: got {v[i].tolist()}, want {want[0][i].tolist()}")
    if tr.tobytes() != want[1].tobytes():
        i = int(np.argwhere((tr != want[1]).any(axis=1))[0, 0])
        raise AssertionError(f"triangle {i}: got {tr[i].tolist()}, want {want[1][i].tolist()}")
    return want


def test_field_bytes_one_call_two_calls_reversed_and_stride():
    t, pts, o = mm.scene("sphere")
    d = new_map()
    check_field(device_field(d, [(pts, o)], **S["cfg"]), t)
    # the same points in two calls, each in reversed order: integer sums do not care
    got = device_field(d, [(pts[1250:][::-1].copy(), o), (pts[:1250][::-1].copy(), o)], **S["cfg"])
    check_field(got, t)
    # ray_stride 3: i counts per call; 834 rays traced, 1,666 left out
    cfg = dict(S["cfg"], ray_stride=3)
    t3 = model_field(S["leaf"], [(pts, o)], **cfg)
    assert (t3.stats()["traced"], t3.stats()["skipped_stride"]) == (834, 1666)
    check_field(device_field(d, [(pts, o)], **cfg), t3)
    d.close()


def test_free_space_with_refused_rays():
    """the whole ray, and max_steps 11: about two thirds of the rays need more steps and are counted, not traced"""
    _, pts, o = mm.scene("sphere")
    cfg = dict(S["cfg"], free_space=1, max_steps=11)
    t = model_field(S["leaf"], [(pts, o)], **cfg)
    st = t.stats()
    assert st["traced"] > 500 and st["skipped_steps"] > 500 and st["traced"] + st["skipped_steps"] == 2500
    d = new_map()
    check_field(device_field(d, [(pts, o)], **cfg), t)
    check_mesh(d, t)
    # a range filter and a point at the origin: filter and zero length are counted
    p2 = np.concatenate([pts[:64], mm.pts4([o]), mm.pts4([[3.0, 0.0, 0.0]])])
    cfg = dict(S["cfg"], max_range=2.0)
    t = model_field(S["leaf"], [(p2, o)], **cfg)
    assert (t.stats()["zero_length"], t.stats()["skipped_filter"], t.stats()["traced"]) == (1, 1, 64)
    check_field(device_field(d, [(p2, o)], **cfg), t)
    d.close()


def test_window_that_cuts_the_sphere():
    full, pts, o = mm.scene("sphere")
    cfg = dict(S["cfg"], nx=9, nz=11)
    t = model_field(S["leaf"], [(pts, o)], **cfg)
    assert 0 < t.stats()["cells_visited"] < full.stats()["cells_visited"]    # cells outside the window were skipped
    d = new_map()
    check_field(device_field(d, [(pts, o)], **cfg), t)
    v, tr, st = check_mesh(d, t)
    assert sum(1 for n in mm.topology(tr)[0].values() if n == 1) > 0 and st["holes"] == 0    # an open surface
    v, tr, st = check_mesh(d, t, min_weight=12)      # and with most cells invalid, tetrahedra that see a crossing but lack a corner
    assert st["holes"] > 100 and st["triangles"] > 0
    d.close()


def test_mesh_bytes_both_axes_count_only_and_capacity():
    t, pts, o = mm.scene("sphere")
    d = new_map()
    check_field(device_field(d, [(pts, o)], **S["cfg"]), t)
    want = check_mesh(d, t)
    assert want[0].tobytes() == mm.scene_mesh("sphere")[0].tobytes() and want[2]["vertices"] == 1466 and want[2]["triangles"] == 2928
    check_mesh(d, t, axes="sensor")
    assert d.mesh(count_only=True) == (1466, 2928, want[2])
    # LOAMX_E_CAPACITY: the counts are written and nothing else is
    L = loamx.lib()
    v, tr = np.full((1466, 3), 7.0, np.float32), np.full((2928, 3), 7, np.uint32)
    st = (C.c_uint64 * 6)(*([9] * 6))
    for cap_v, cap_t in ((1465, 2928), (1466, 2927), (0, 0)):
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        rc = L.loamx_densemap_mesh(d.h, None, v.ctypes.data_as(C.c_void_p), C.c_uint64(cap_v), tr.ctypes.data_as(C.c_void_p), C.c_uint64(cap_t),
                                   C.byref(nv), C.byref(nt), st)
        assert rc == loamx.E_CAPACITY and (nv.value, nt.value) == (1466, 2928)
        assert np.all(v == 7.0) and np.all(tr == 7) and list(st) == [9] * 6
    d.close()


def test_save_ply(tmp_path):
    t, pts, o = mm.scene("wall")
    d = new_map(mm.WALL["leaf"])
    check_field(device_field(d, [(pts, o)], **mm.WALL["cfg"]), t)
    want = check_mesh(d, t)
    path = str(tmp_path / "wall.ply")
    assert d.save_ply(path) == want[2]
    v, tr = mm.read_ply(path)
    assert v.tobytes() == want[0].tobytes() and np.array_equal(tr, want[1].astype(np.int64))
    d.close()


def test_from_history_under_corrections():
    """two logged sweeps, the first under a rotation and a shift, the second under the identity: the replay where the log lies
    equals the host-fed form given loamx_densemap_correct's output, and the model's; the map, its statistics and its log stay"""
    _, pts, o = mm.scene("sphere")
    sweeps = [(pts[:1250].copy(), o), (pts[1250:].copy(), o + np.float32([0.02, 0.0, -0.01]))]
    corr = np.stack([rbm.rigid((0.02, -0.03, 0.05), (0.04, -0.02, 0.03)), np.float64(rbm.IDENTITY)])
    d = new_map()
    d.enable_history(initial_points=1024)
    for p, org in sweeps:
        assert d.add(p, org) == loamx.OK
    before = (d.stats(), d.points().tobytes(), d.history_size(), [(a.tobytes(), b.tobytes()) for a, b in (d.history(0), d.history(1))],
              d.rebuild_stats())
    c = d.tsdf_begin(**S["cfg"])
    assert d.tsdf_add_history(0, 2, corr) == loamx.OK
    replayed = d.tsdf(c)
    moved = [(loamx.correct(corr[k], p), loamx.correct(corr[k], org.reshape(1, 3))[0]) for k, (p, org) in enumerate(sweeps)]
    assert moved[1][0].tobytes() == sweeps[1][0].tobytes()     # the identity rule: the logged bytes
    fed = device_field(d, moved, **S["cfg"])
    assert replayed[0].tobytes() == fed[0].tobytes() and replayed[1].tobytes() == fed[1].tobytes() and replayed[2] == fed[2]
    t = model_field(S["leaf"], mm.corrected(sweeps, list(corr)), **S["cfg"])
    check_field(fed, t)
    assert t.stats()["traced"] == 2500 and t.W.tobytes() != mm.scene("sphere")[0].W.tobytes()    # the correction moved something
    check_mesh(d, t)
    # a window of the log, no corrections, with a stride: i counts per call
    c = d.tsdf_begin(**S["cfg"], ray_stride=7)
    assert d.tsdf_add_history(1, 1) == loamx.OK
    check_field(d.tsdf(c), model_field(S["leaf"], sweeps[1:], **dict(S["cfg"], ray_stride=7)))
    c = d.tsdf_begin(**S["cfg"], ray_stride=7)
    assert d.tsdf_add_history(0, 2) == loamx.OK
    check_field(d.tsdf(c), model_field(S["leaf"], sweeps, **dict(S["cfg"], ray_stride=7)))
    after = (d.stats(), d.points().tobytes(), d.history_size(), [(a.tobytes(), b.tobytes()) for a, b in (d.history(0), d.history(1))],
             d.rebuild_stats())
    assert after == before
    d.close()


def test_edge_shapes():
    _, pts, o = mm.scene("sphere")
    d = new_map()
    # 17 x 9 x 5 = 765 cells: no multiple of the block
    cfg = dict(x0=-3, y0=-6, z0=-8, nx=17, ny=9, nz=5)
    t = model_field(S["leaf"], [(pts, o)], **cfg)
    check_field(device_field(d, [(pts, o)], **cfg), t)
    assert check_mesh(d, t)[2]["triangles"] > 100
    # 2 x 2 x 2: one cube, on the sphere's surface
    cfg = dict(x0=4, y0=0, z0=0, nx=2, ny=2, nz=2)
    t = model_field(S["leaf"], [(pts, o)], **cfg)
    check_field(device_field(d, [(pts, o)], **cfg), t)
    assert check_mesh(d, t)[2] == dict(valid=8, inside=4, tetrahedra=6, holes=0, vertices=9, triangles=8)
    # an empty field
    c = d.tsdf_begin(**cfg)
    W, D, st = d.tsdf(c)
    assert not W.any() and not D.any() and st == dict.fromkeys(mm.TSDF_STATS, 0)
    v, tr, st = d.mesh()
    assert v.shape == (0, 3) and tr.shape == (0, 3) and st == dict.fromkeys(mm.MESH_STATS, 0)
    assert d.mesh(count_only=True) == (0, 0, st)
    d.close()


def test_mesh_across_scan_tiles():
    """96 x 96 x 64 cells are 2,304 blocks of cubes, more than one tile of the chained scan; the wall's cells lie on both sides of
    block 2,048 (record 524,288: rz 56, ry 85), so offsets of the second tile are used"""
    _, pts, o = mm.scene("wall")
    cfg = dict(x0=0, y0=-48, z0=-57, nx=96, ny=96, nz=64)
    t = model_field(mm.WALL["leaf"], [(pts, o)], **cfg)
    rec = np.flatnonzero(t.W.reshape(-1) >= 2)
    assert rec.min() < 2048 * 256 - 96 * 96 and rec.max() > 2048 * 256 + 96 * 96
    d = new_map(mm.WALL["leaf"])
    check_field(device_field(d, [(pts, o)], **cfg), t)
    assert check_mesh(d, t)[2]["triangles"] > 1000
    d.close()


def test_a_cell_with_d_exactly_zero_is_outside():
    """leaf 0.5, tau 1 m, every number a binary fraction.  In each of four rows of cells along x two opposite rays end at x = 1.375,
    0.125 m beyond the centre of cell 2: one from x = -0.75, and one from x = 1.4375 inside cell 2, whose band is cells 2, 1, 0.
    Cell 2 gets q = +128 and -128: W = 2 and D = 0, valid and outside; cells 3 and 4 see the first ray alone and are inside.  The
    surface lies between cells 2 and 3 with t = 0: every vertex is at x = 1.25 exactly, the centre of the zero cell"""
    leaf, cfg = 0.5, dict(x0=-2, y0=0, z0=0, nx=9, ny=2, nz=2, trunc_leaves=2.0)
    sweeps = []
    for y in (0.25, 0.75):
        for z in (0.25, 0.75):
            sweeps.append((mm.pts4([[1.375, y, z]]), np.float32([-0.75, y, z])))
            sweeps.append((mm.pts4([[1.375, y, z]]), np.float32([1.4375, y, z])))
    t = model_field(leaf, sweeps, **cfg)
    rx = 2 - cfg["x0"]
    assert np.all(t.W[:, :, rx] == 2) and np.all(t.D[:, :, rx] == 0) and np.all(t.D[:, :, rx + 1] == -384) and np.all(t.W[:, :, rx + 1] == 1)
    d = new_map(leaf)
    check_field(device_field(d, sweeps, **cfg), t)
    v, tr, st = check_mesh(d, t, min_weight=1)
    assert st["triangles"] >= 2 and st["inside"] == 8 and np.all(v[:, 0] == np.float32(1.25))
    v, tr, st = check_mesh(d, t, min_weight=2)     # cells 3 and 4 are invalid now: no tetrahedron is complete where the signs change
    assert st["triangles"] == 0 and st["inside"] == 0
    d.close()


def test_refusals_leave_the_field_standing():
    t, pts, o = mm.scene("sphere")
    L = loamx.lib()
    d = new_map()
    st8, st6, n = (C.c_uint64 * 8)(), (C.c_uint64 * 6)(), C.c_uint64(0)
    # no field yet
    for rc in (L.loamx_densemap_tsdf_download(d.h, None, None, st8),
               L.loamx_densemap_mesh(d.h, None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n), C.byref(n), st6),
               L.loamx_densemap_tsdf_add_from_history(d.h, C.c_uint64(0), C.c_uint64(1), None)):
        assert rc == loamx.E_INVALID and b"no signed distance field" in L.loamx_last_error()
    got = device_field(d, [(pts, o)], **S["cfg"])
    check_field(got, t)
    c = got[3]
    cloud = loamx.cloud_of(pts)
    o3 = (C.c_float * 3)(*o.tolist())
    bad_cloud = loamx.cloud_of(pts)
    bad_cloud.stride = 6
    v, tr = np.zeros((1466, 3), np.float32), np.zeros((2928, 3), np.uint32)
    vp, tp = v.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p)
    big = C.c_uint64(1 << 20)
    refusals = [
        (lambda: L.loamx_densemap_tsdf_begin(d.h, C.byref(loamx.TsdfConfig(nx=1))), b"nx"),
        (lambda: L.loamx_densemap_tsdf_begin(d.h, C.byref(loamx.TsdfConfig(trunc_leaves=0.5))), b"trunc_leaves"),
        (lambda: L.loamx_densemap_tsdf_begin(d.h, C.byref(loamx.TsdfConfig(nx=1024, ny=1024, nz=65))), b"nx * ny * nz"),
        (lambda: L.loamx_densemap_tsdf_add(d.h, None, o3), b"cloud"),
        (lambda: L.loamx_densemap_tsdf_add(d.h, C.byref(cloud), None), b"origin"),
        (lambda: L.loamx_densemap_tsdf_add(d.h, C.byref(bad_cloud), o3), b"stride"),
        (lambda: L.loamx_densemap_tsdf_add_from_map(d.h, None), b"m is NULL"),
        (lambda: L.loamx_densemap_tsdf_add_from_pipeline(d.h, None, 0), b"p is NULL"),
        (lambda: L.loamx_densemap_tsdf_add_from_history(d.h, C.c_uint64(0), C.c_uint64(1), None), b"history"),
        (lambda: L.loamx_densemap_tsdf_download(d.h, None, None, None), b"stats"),
        (lambda: L.loamx_densemap_mesh(d.h, C.byref(loamx.MeshConfig(0, 0)), vp, big, tp, big, C.byref(n), C.byref(n), st6), b"min_weight"),
        (lambda: L.loamx_densemap_mesh(d.h, C.byref(loamx.MeshConfig(2, 2)), vp, big, tp, big, C.byref(n), C.byref(n), st6), b"axes"),
        (lambda: L.loamx_densemap_mesh(d.h, None, vp, big, None, big, C.byref(n), C.byref(n), st6), b"verts and tris"),
        (lambda: L.loamx_densemap_mesh(d.h, None, None, big, None, big, C.byref(n), C.byref(n), st6), b"cap_v"),
        (lambda: L.loamx_densemap_mesh(d.h, None, vp, big, tp, big, None, C.byref(n), st6), b"n_verts"),
        (lambda: L.loamx_densemap_mesh(d.h, None, vp, big, tp, big, C.byref(n), None, st6), b"n_tris"),
        (lambda: L.loamx_densemap_mesh(d.h, None, vp, big, tp, big, C.byref(n), C.byref(n), None), b"stats"),
        (lambda: L.loamx_densemap_save_ply(d.h, None, None, st6), b"path"),
    ]
    for call, word in refusals:
        assert call() == loamx.E_INVALID, word
        assert word in L.loamx_last_error(), (word, L.loamx_last_error())
    assert not v.any() and not tr.any()
    check_field(d.tsdf(c), t)         # the field of before, byte for byte
    check_mesh(d, t)
    # with history on, a window beyond the log and a correction that is not finite
    h = new_map()
    h.enable_history(initial_points=1024)
    assert h.add(pts[:100], o) == loamx.OK
    check_field(device_field(h, [(pts, o)], **S["cfg"]), t)
    nan = np.full((1, 3, 4), np.nan)
    for call, word in ((lambda: L.loamx_densemap_tsdf_add_from_history(h.h, C.c_uint64(1), C.c_uint64(1), None), b"beyond the log"),
                       (lambda: L.loamx_densemap_tsdf_add_from_history(h.h, C.c_uint64(0), C.c_uint64(2), None), b"beyond the log"),
                       (lambda: L.loamx_densemap_tsdf_add_from_history(h.h, C.c_uint64(0), C.c_uint64(0), None), b"n_calls"),
                       (lambda: L.loamx_densemap_tsdf_add_from_history(h.h, C.c_uint64(0), C.c_uint64(1), nan.ctypes.data_as(C.c_void_p)), b"corrections")):
        assert call() == loamx.E_INVALID and word in L.loamx_last_error(), (word, L.loamx_last_error())
    check_field(h.tsdf(c), t)
    # reset drops the field
    h.reset()
    assert L.loamx_densemap_tsdf_download(h.h, None, None, st8) == loamx.E_INVALID and b"no signed distance field" in L.loamx_last_error()
    h.close()
    d.close()
