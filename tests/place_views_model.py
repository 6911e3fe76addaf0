"""Model of the views a place database describes from a dense map (include/loamx.h, loamx_place_add_views and the host-only calls
around it), exact to the bit.  A composition and nothing else: tests/densemap_model.py (the map and its export),
tests/densemap_raycast_model.py (cast) and tests/place_model.py (descriptor, ring_key) stay the models of their parts; the only
arithmetic added here is end = o + off in f32.  The host-only calls are restated in float64 with the C library's cos / sin
(math.cos, math.sin: numpy's vectorised ones may differ in the last bit).  The checker of tests/test_place_views_cpu.py and
tests/test_gpu_place_views.py, and the builder of the scenes both of them use."""
import math

import numpy as np

import densemap_align_model as am
import densemap_carve_model as cm
import densemap_model as dm
import densemap_raycast_model as rm
import place_model as pm

F = np.float32
CAST, VOXELS = 0, 1
MAX_ORIGINS, MAX_RAYS = 4096, 65536
STAT_KEYS = ("entries", "not_traced", "miss", "hit", "hit_end", "cells")


def ends_of(origin, offsets):
    """(n_rays, 4) f32: end_j = o + off[j], one f32 addition per component"""
    o = np.asarray(origin, F).reshape(3)
    off = np.asarray(offsets, F).reshape(-1, 3)
    out = np.zeros((len(off), 4), F)
    with np.errstate(over="ignore"):
        out[:, :3] = o[None, :] + off
    return out


def hit_cloud(records):
    """(m, 4) f32: x, y, z of the records with status HIT or HIT_END, in ray order"""
    hit = records["status"] >= rm.HIT
    out = np.zeros((int(hit.sum()), 4), F)
    for a, name in enumerate("xyz"):
        out[:, a] = records[name][hit]
    return out


def voxel_cloud(model, min_points=1, rule=None):
    """(m, 4) f32: the exported records of the voxels with n >= min_points that the rule does not call dynamic (VOXELS mode)"""
    miss_of = getattr(model, "miss", {})
    keep = np.array([int(n) >= min_points and not (rule is not None and cm.is_dynamic(rule, int(n), int(miss_of.get(int(k), 0))))
                     for k, n in zip(model.keys.tolist(), model.vals[:, 0].tolist())], bool)
    return dm.export(model.keys[keep], model.vals[keep], model.leaf)


def place_kw(place):
    return dict(R=place.R, S=place.S, max_range=place.max_range, min_range=place.min_range, height_offset=place.height_offset)


def add_views(model, place, origins, offsets=None, mode=None, max_steps=4096, skip_steps=0, min_points=1, rule=None):
    """loamx_place_add_views on a densemap model and a place_model.Model: appends one entry per origin and returns (first_id, stats as
    a dict in the order of STAT_KEYS), or None when max_entries would be passed (nothing changes)"""
    origins = np.asarray(origins, F).reshape(-1, 3)
    mode = (VOXELS if offsets is None else CAST) if mode is None else mode
    assert 1 <= len(origins) <= MAX_ORIGINS and min_points >= 1
    if place.max_entries and len(place) + len(origins) > place.max_entries:
        return None
    stats = dict.fromkeys(STAT_KEYS, 0)
    stats["entries"] = len(origins)
    first = len(place)
    cloud = voxel_cloud(model, min_points, rule) if mode == VOXELS else None
    if mode == VOXELS:
        assert offsets is None
        stats["not_traced"] = len(cloud)
    else:
        assert 1 <= len(offsets) <= MAX_RAYS
    for o in origins:
        if mode == CAST:
            rec, counts = rm.cast(model, ends_of(o, offsets), o, max_steps=max_steps, skip_steps=skip_steps, min_points=min_points, rule=rule)
            cloud = hit_cloud(rec)
            for k in rm.COUNT_KEYS:
                stats[k] += counts[k]
        D = pm.descriptor(cloud, o, **place_kw(place))
        place.desc.append(D)
        place.keys.append(pm.ring_key(D))
    return first, stats


# ---- the host-only calls, restated ------------------------------------------------------------------------------------------------------
def view_rays(n_azimuth, elevations, range_m):
    """loamx_place_view_rays: (n_el * n_az, 3) f32"""
    el = np.asarray(elevations, F).reshape(-1)
    r = float(F(range_m))
    out = np.zeros((len(el) * n_azimuth, 3), F)
    for e in range(len(el)):
        ce, se = math.cos(float(el[e])), math.sin(float(el[e]))
        for a in range(n_azimuth):
            az = 2.0 * math.pi * float(a) / float(n_azimuth)
            out[e * n_azimuth + a] = (F(r * ce * math.sin(az)), F(r * se), F(r * ce * math.cos(az)))
    return out


def grid_view_origins(cells, x0, z0, nx, nz, cell_leaves, leaf, stride, min_clear2, sensor_height):
    """loamx_grid_view_origins: (n, 3) f32, all of them; cells: a structured array with cls, clear2, elevation, (nz, nx) or flat"""
    c = np.asarray(cells).reshape(nz, nx)
    lf, k = np.float64(F(leaf)), np.float64(cell_leaves)
    out = []
    for rz in range(0, nz, stride):
        for rx in range(0, nx, stride):
            r = c[rz, rx]
            if int(r["cls"]) != 1 or int(r["clear2"]) < min_clear2:
                continue
            out.append((F((np.float64(x0) + np.float64(rx) + 0.5) * lf * k), F(r["elevation"]) + F(sensor_height),
                        F((np.float64(z0) + np.float64(rz) + 0.5) * lf * k)))
    return np.array(out, F).reshape(-1, 3)


def view_pose(view_origin, shift, n_sectors, query_origin=None):
    """loamx_place_view_pose: (3, 4) f64"""
    v = np.asarray(view_origin, F).astype(np.float64)
    q = np.zeros(3) if query_origin is None else np.asarray(query_origin, F).astype(np.float64)
    psi = float(shift) * (2.0 * math.pi) / float(n_sectors)
    c, s = math.cos(psi), math.sin(psi)
    return np.array([[c, 0.0, s, v[0] - (c * q[0] + s * q[2])],
                     [0.0, 1.0, 0.0, v[1] - q[1]],
                     [-s, 0.0, c, v[2] - (c * q[2] - s * q[0])]], np.float64)


# ---- the scenes of tests/test_place_views_cpu.py and tests/test_gpu_place_views.py -------------------------------------------------------
LEAF = am.BOX_LEAF
# a hand-placed voxel of one point on the 2^-20-of-a-leaf lattice (its exported position is the point itself), away from the box, and
# the origin straight below it: the hit has a = b = 0 and is dropped by the sector rule
ABOVE_POINT = np.array([[10.25, 1.25, 10.25, 0.0]], F)
ABOVE_ORIGIN = np.array([10.25, 0.25, 10.25], F)
ABOVE_OFFSETS = np.array([[0.0, 2.0, 0.0], [0.0, -2.0, 0.0], [2.0, 0.0, 0.0]], F)


def lidar_offsets(n_rays, range_m=9.0, seed=5):
    """n_rays offsets: the rays of view_rays(n_az, 4 elevations) as far as they go, then random directions of random length (some end
    inside the box, some in a wall, some behind one)"""
    n_az = max(n_rays // 4, 1)
    out = view_rays(n_az, np.deg2rad([-30.0, -10.0, 5.0, 25.0]), range_m)[:n_rays]
    if len(out) < n_rays:
        rng = np.random.default_rng(seed)
        extra = rng.uniform(-6.0, 6.0, (n_rays - len(out), 3)).astype(F)
        out = np.concatenate([out, extra])
    return np.ascontiguousarray(out, F)


def lattice_origins(n, seed=9):
    """n origins inside the box, (n, 3) f32: the first in an empty cell on a cell face in x (x = -0.5: the walk starts on a boundary), the rest random"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(am.BOX_LO + 0.6, am.BOX_HI - 0.6, (n, 3)).astype(F)
    o[0] = (-0.5, -0.25, 0.125)
    return o


def pillars():
    """(points (n, 4) f32, origin): four pillars of distinct heights on the box's floor at places without a symmetry, 300 points each"""
    rng = np.random.default_rng(21)
    spec = [(-2.0, -0.9, 1.0), (-0.6, 0.7, 2.0), (1.1, -0.6, 3.0), (2.3, 0.6, 4.0)]   # x, z, height
    pts = []
    for x, z, h in spec:
        p = np.zeros((300, 4), F)
        p[:, 0] = x + rng.uniform(-0.12, 0.12, 300)
        p[:, 1] = am.BOX_LO[1] + rng.uniform(0.0, h, 300)
        p[:, 2] = z + rng.uniform(-0.12, 0.12, 300)
        pts.append(p)
    return np.concatenate(pts), (0.0, 0.0, 0.0)


CHAIN_TURN = 7                                                     # sectors by which the query's frame is turned
CHAIN_PLACE = dict(R=20, S=60, max_range=8.0, min_range=0.0, height_offset=3.0)
_CHAIN = {}


def chain_scene():
    """dict for the chain test: sweeps (the box's three sweeps and the pillars), leaf, origins (the 3 x 3 lattice, (9, 3) f32),
    offsets (8 x 90 rays of 9 m), place (the database's parameters), turn.  Computed once"""
    if not _CHAIN:
        S = am.box_scene()
        xs, zs = (-1.5, 0.25, 1.75), (-0.75, 0.0, 0.75)
        origins = np.array([(x, -0.75, z) for z in zs for x in xs], F)
        offsets = view_rays(90, np.deg2rad([-40.0, -25.0, -12.0, -4.0, 4.0, 12.0, 25.0, 40.0]), 9.0)
        _CHAIN.update(sweeps=list(S["sweeps"]) + [pillars()], leaf=S["leaf"], origins=origins, offsets=offsets, place=dict(CHAIN_PLACE),
                      turn=CHAIN_TURN)
    return _CHAIN


def turned_query(hits, origin, turn, n_sectors):
    """(m, 4) f32: the hit positions seen from origin in a frame turned by `turn` sectors: R^T (hit - o) in double, rounded once,
    R = rot_y(turn * 2 pi / n_sectors)"""
    R = view_pose(np.zeros(3, F), turn, n_sectors)[:, :3]
    d = np.asarray(hits, F)[:, :3].astype(np.float64) - np.asarray(origin, F).astype(np.float64)
    out = np.zeros((len(d), 4), F)
    out[:, :3] = d @ R      # row-wise R^T d
    return out
