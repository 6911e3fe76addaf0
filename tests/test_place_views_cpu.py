"""CPU: the host-only calls around loamx_place_add_views (include/loamx.h: loamx_place_view_default_config, loamx_place_view_rays,
loamx_grid_view_origins, loamx_place_view_pose) bit for bit against the restatements of tests/place_views_model.py, every refusal
listed for them, and the scene of the chain test of tests/test_gpu_place_views.py ranked by the model alone, so that the scene is
known not to be ambiguous before it reaches a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import densemap_model as dm
import place_model as pm
import place_views_model as vm
from loam_velodyne_amd import loamx


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def refused(rc, word):
    msg = loamx.lib().loamx_last_error()
    assert rc == loamx.E_INVALID and word.encode() in msg, (rc, word, msg)


def test_declared_and_wrapped():
    L = loamx.lib()
    for name in ("loamx_place_view_default_config", "loamx_place_view_rays", "loamx_place_add_views", "loamx_grid_view_origins",
                 "loamx_place_view_pose"):
        assert hasattr(L, name), name
    for name in ("PlaceViewConfig", "view_rays", "grid_view_origins", "view_pose", "PLACE_VIEW_CAST", "PLACE_VIEW_VOXELS"):
        assert hasattr(loamx, name), name
    assert hasattr(loamx.PlaceDB, "add_views")
    c = loamx.PlaceViewConfig(9, 9, 9, 9)
    L.loamx_place_view_default_config(C.byref(c))
    assert (c.mode, c.max_steps, c.skip_steps, c.min_points) == (loamx.PLACE_VIEW_CAST, 4096, 0, 1) and C.sizeof(c) == 16
    L.loamx_place_view_default_config(None)    # (ignored, as the other default functions ignore it)
    assert (loamx.PLACE_VIEW_MAX_ORIGINS, loamx.PLACE_VIEW_MAX_RAYS) == (vm.MAX_ORIGINS, vm.MAX_RAYS) == (4096, 65536)
    assert L.loamx_abi_version() == 6


# ---- loamx_place_view_rays ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_az, el, rng", [(360, np.deg2rad(np.linspace(-15, 15, 16)), 80.0), (7, [0.3], 9.0), (1, [-1.2, 0.0, 1.5], 0.37),
                                           (5, [math.pi / 2, -math.pi / 2], 1e6)])
def test_view_rays_bits(n_az, el, rng):
    got, want = loamx.view_rays(n_az, el, rng), vm.view_rays(n_az, el, rng)
    assert got.dtype == np.float32 and got.shape == (len(el) * n_az, 3) and got.tobytes() == want.tobytes()
    # ray (e, a) at e * n_az + a; azimuth 0 looks along +z, a quarter turn along +x; the length is the range
    assert got[0, 0] == 0 and (got[0, 2] > 0 or abs(el[0]) > 1.5)    # (sin 0 = 0; (float)(pi / 2) lies a hair beyond pi / 2)
    ln = np.linalg.norm(got.astype(np.float64), axis=1)
    assert np.allclose(ln, rng, rtol=1e-6)
    if n_az % 4 == 0:
        assert got[n_az // 4, 0] > 0 and abs(got[n_az // 4, 2]) < 1e-5 * rng


def test_view_rays_refusals():
    L = loamx.lib()
    el = np.array([0.1, 0.2], np.float32)
    out = np.full(3 * 2 * 8, 7, np.float32)

    def call(n_az=8, e=el, n_el=2, rng=5.0, o=out):
        return L.loamx_place_view_rays(C.c_uint32(n_az), ptr(e), C.c_uint32(n_el), C.c_float(rng), ptr(o))
    assert call() == loamx.OK and not (out == 7).any()
    out[:] = 7
    refused(call(e=None), "elevations")
    refused(call(o=None), "offsets")
    refused(call(n_az=0), "n_azimuth")
    refused(call(n_el=0), "n_elevations")
    refused(call(n_az=32769, n_el=2), "LOAMX_PLACE_VIEW_MAX_RAYS")
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(call(rng=bad), "range")
    for bad in (np.inf, np.nan):
        refused(call(e=np.array([0.1, bad], np.float32)), "elevations")
    assert (out == 7).all()    # a refused call writes nothing
    big = np.zeros((65536, 3), np.float32)    # the limit itself is allowed
    assert L.loamx_place_view_rays(C.c_uint32(32768), ptr(el), C.c_uint32(2), C.c_float(1.0), ptr(big)) == loamx.OK


# ---- loamx_grid_view_origins ---------------------------------------------------------------------------------------------------------------
def small_grid(nx=7, nz=5, seed=2):
    rng = np.random.default_rng(seed)
    cells = np.zeros((nz, nx), loamx.GRID_CELL)
    cells["cls"] = rng.integers(0, 4, (nz, nx))
    cells["cls"][0, 0] = loamx.GRID_FREE
    cells["clear2"] = rng.integers(0, 9, (nz, nx))
    cells["clear2"][0, 0] = 8
    cells["elevation"] = rng.uniform(-2, 2, (nz, nx)).astype(np.float32)
    cells["ground"] = rng.integers(-5, 5, (nz, nx))
    return cells, loamx.GridConfig(cell_leaves=3, x0=-4, z0=11, nx=nx, nz=nz)


@pytest.mark.parametrize("leaf", [0.5, 0.1, 0.3])
@pytest.mark.parametrize("stride, min_clear2", [(1, 0), (1, 4), (2, 1), (3, 9), (8, 0), (100, 8)])
def test_grid_view_origins_bits(leaf, stride, min_clear2):
    cells, cfg = small_grid()
    want = vm.grid_view_origins(cells, cfg.x0, cfg.z0, cfg.nx, cfg.nz, cfg.cell_leaves, leaf, stride, min_clear2, 1.7)
    got = loamx.grid_view_origins(cells, cfg, leaf, stride, min_clear2, 1.7)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), (got, want)
    if stride > max(cfg.nx, cfg.nz):    # a stride larger than the window looks at cell (0, 0) alone
        assert len(got) == (1 if min_clear2 <= 8 else 0)
    if (stride, min_clear2) == (1, 0):
        assert len(got) == int((cells["cls"] == loamx.GRID_FREE).sum()) >= 3
    # capacity < n: *n is the full count, only `capacity` triples are written, the rest of the buffer is untouched
    if len(want) >= 2:
        L, n = loamx.lib(), C.c_uint64(0)
        buf = np.full((len(want), 3), 7, np.float32)
        rc = L.loamx_grid_view_origins(ptr(cells), C.byref(cfg), C.c_float(leaf), C.c_uint32(stride), C.c_uint32(min_clear2), C.c_float(1.7),
                                       ptr(buf), C.c_uint64(len(want) - 1), C.byref(n))
        assert rc == loamx.OK and n.value == len(want)
        assert buf[:-1].tobytes() == want[:-1].tobytes() and (buf[-1] == 7).all()
        assert loamx.grid_view_origins(cells, cfg, leaf, stride, min_clear2, 1.7, capacity=1).tobytes() == want[:1].tobytes()


def test_grid_view_origins_is_the_route_points_expression():
    cells, cfg = small_grid()
    got = loamx.grid_view_origins(cells, cfg, 0.3, 1, 0, 0.0)
    free = [(rx, rz) for rz in range(cfg.nz) for rx in range(cfg.nx) if cells["cls"][rz, rx] == loamx.GRID_FREE]
    pts = loamx.route_points(cfg, 0.3, np.array(free, np.uint32), cells)
    assert got[:, [0, 2]].tobytes() == pts[:, [0, 2]].tobytes()
    assert got[:, 1].tobytes() == (pts[:, 1] + np.float32(0.0)).tobytes()


def test_grid_view_origins_refusals():
    L = loamx.lib()
    cells, cfg = small_grid()
    n, out = C.c_uint64(99), np.full((40, 3), 7, np.float32)

    def call(c=cells, g=cfg, leaf=0.5, stride=1, mc=0, sh=1.0, o=out, cap=40, cnt=n):
        return L.loamx_grid_view_origins(ptr(c), C.byref(g) if g is not None else None, C.c_float(leaf), C.c_uint32(stride), C.c_uint32(mc),
                                         C.c_float(sh), ptr(o), C.c_uint64(cap), C.byref(cnt) if cnt is not None else None)
    refused(call(c=None), "cells")
    refused(call(g=None), "cfg")
    refused(call(cnt=None), "n is NULL")
    refused(call(o=None), "origins")
    for bad in (0.0, -0.5, np.inf, np.nan):
        refused(call(leaf=bad), "leaf")
    refused(call(stride=0), "stride")
    for bad in (np.inf, np.nan):
        refused(call(sh=bad), "sensor_height")
    refused(call(g=cfg.copy(nx=0)), "nx")
    refused(call(g=cfg.copy(cell_leaves=65)), "cell_leaves")
    assert n.value == 99 and (out == 7).all()    # nothing written by a refused call
    assert call(o=None, cap=0) == loamx.OK and n.value > 0    # counting alone needs no buffer


# ---- loamx_place_view_pose -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 12, 60, 128])
def test_view_pose_bits(S):
    rng = np.random.default_rng(S)
    for shift in sorted({0, 1, S // 4, S // 2, S - 1, 7 % S}):
        v = rng.uniform(-50, 50, 3).astype(np.float32)
        q = rng.uniform(-5, 5, 3).astype(np.float32)
        for qo in (None, q):
            got, want = loamx.view_pose(v, shift, S, qo), vm.view_pose(v, shift, S, qo)
            assert got.dtype == np.float64 and got.shape == (3, 4) and got.tobytes() == want.tobytes(), (shift, got, want)
            R = got[:, :3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.linalg.det(R) > 0
            # the pose takes the query's origin onto the view's
            assert np.allclose(R @ (np.zeros(3) if qo is None else qo.astype(np.float64)) + got[:, 3], v.astype(np.float64), atol=1e-12)
    # the header's yaw convention: R = rot_y(+yaw_hint) turns +z towards +x
    P = loamx.view_pose(np.zeros(3, np.float32), 1, S)
    assert P[0, 2] > 0 and P[2, 0] < 0 and P[0, 2] == math.sin(2.0 * math.pi / S)


def test_view_pose_refusals():
    L = loamx.lib()
    v, out = np.array([1, 2, 3], np.float32), np.full(12, 7.0)

    def call(vo=v, shift=3, S=60, q=None, o=out):
        return L.loamx_place_view_pose(ptr(vo), C.c_uint32(shift), C.c_int(S), ptr(q), ptr(o))
    refused(call(vo=None), "view_origin")
    refused(call(o=None), "pose")
    for S in (3, 129, 0, -1):
        refused(call(S=S), "n_sectors")
    refused(call(shift=60), "shift")
    refused(call(shift=4, S=4), "shift")
    refused(call(vo=np.array([1, np.nan, 3], np.float32)), "view_origin")
    refused(call(q=np.array([np.inf, 0, 0], np.float32)), "query_origin")
    assert (out == 7).all()
    assert call() == loamx.OK and not (out == 7).any()


# ---- the model itself: a composition --------------------------------------------------------------------------------------------------------
def test_model_view_is_cast_then_describe():
    """a view of the model is rm.cast followed by pm.descriptor of the hit positions, and a view from straight below the hand-placed
    voxel has a hit that the sector rule drops"""
    import densemap_raycast_model as rm
    m = dm.Model(leaf=vm.LEAF)
    m.add(vm.ABOVE_POINT, (0, 0, 0))
    assert m.points()[:, :3].tobytes() == vm.ABOVE_POINT[:, :3].tobytes()    # on the lattice: the export is the point
    place = pm.Model(R=8, S=12, max_range=8.0, height_offset=2.0)
    first, st = vm.add_views(m, place, vm.ABOVE_ORIGIN[None], vm.ABOVE_OFFSETS)
    rec, counts = rm.cast(m, vm.ends_of(vm.ABOVE_ORIGIN, vm.ABOVE_OFFSETS), vm.ABOVE_ORIGIN)
    assert (first, len(place)) == (0, 1) and st == dict(entries=1, **counts)
    assert (counts["not_traced"], counts["miss"], counts["hit"] + counts["hit_end"]) == (0, 2, 1)
    used, _, sector, h, _ = pm.cells_of(vm.hit_cloud(rec), vm.ABOVE_ORIGIN, R=8, S=12, max_range=8.0, height_offset=2.0)
    assert sector.tolist() == [-1] and not used.any() and h[0] > 0    # a = b = 0: no sector qualifies
    assert not place.desc[0].any()
    # VOXELS mode sees the same voxel from the side
    place2 = pm.Model(R=8, S=12, max_range=8.0, height_offset=2.0)
    _, st2 = vm.add_views(m, place2, np.array([[9.0, 0.25, 10.25]], np.float32))
    assert st2 == dict(entries=1, not_traced=1, miss=0, hit=0, hit_end=0, cells=0) and np.count_nonzero(place2.desc[0]) == 1


# ---- the chain's scene, ranked by the model alone ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    import densemap_raycast_model as rm
    S = vm.chain_scene()
    m = dm.Model(leaf=S["leaf"])
    for p, o in S["sweeps"]:
        m.add(p, o)
    place = pm.Model(**S["place"], exclude_recent=0)
    first, stats = vm.add_views(m, place, S["origins"], S["offsets"])
    rec, _ = rm.cast(m, vm.ends_of(S["origins"][4], S["offsets"]), S["origins"][4])
    return dict(S=S, map=m, place=place, first=first, stats=stats, hits=vm.hit_cloud(rec))


def test_chain_scene_is_not_ambiguous(chain):
    """The query (the hits seen from origin 4, turned by 7 sectors) ranks entry 4 first with shift 7 in the model.  Distances of
    the model on this scene: first 0.0 (entry 4, shift 7: a turn by whole sectors shifts the columns and changes nothing else),
    second 0.4707 (entry 5, shift 4): margin 0.4707; the other seven entries lie between 0.52 and 0.74."""
    S, place = chain["S"], chain["place"]
    assert chain["first"] == 0 and len(place) == 9 and chain["stats"]["entries"] == 9
    assert chain["stats"]["hit"] + chain["stats"]["hit_end"] > 9 * 400 and len(chain["hits"]) > 400
    assert all(np.count_nonzero(D) >= 20 for D in place.desc)
    q = vm.turned_query(chain["hits"], S["origins"][4], S["turn"], S["place"]["S"])
    res = place.query(q, (0, 0, 0), exclude_recent=0, n_results=9)
    print([(r[0], r[1], float(r[2])) for r in res])
    assert len(res) == 9
    assert (res[0][0], res[0][1]) == (4, S["turn"])
    margin = float(res[1][2]) - float(res[0][2])
    print("margin", margin)
    assert margin > 0.0
    # the pose the match implies lands the query's points back on the hits: the rounding of the query is the only error
    P = vm.view_pose(S["origins"][4], res[0][1], S["place"]["S"])
    back = q[:, :3].astype(np.float64) @ P[:, :3].T + P[:, 3]
    tol = 4.0 * float(np.spacing(np.float32(np.abs(chain["hits"][:, :3]).max())))
    assert np.abs(back - chain["hits"][:, :3].astype(np.float64)).max() <= tol
