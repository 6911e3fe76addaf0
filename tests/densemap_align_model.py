"""numpy model of the alignment against the dense map's frozen snapshot (include/loamx.h, loamx_densemap_freeze and what follows it).
step(): one linearisation, restating the header's f32 arithmetic with the library's roundings (numpy multiplies and adds f32 arrays one
operation at a time: no fused multiply-add) and its integer sums, exact.  It takes the snapshot as (ascending keys, (m, 6) float32
records), so that whose eigen-solver computed the normals stays out of a comparison of steps.  solve() and align(): the 6x6 solve
(numpy.linalg.eigh instead of the library's Jacobi) and the Gauss-Newton loop in float64.  Built on tests/densemap_model.py and
tests/densemap_moments_model.py, which stay the models of the map and its surfels.  The checker of tests/test_densemap_align_cpu.py
and tests/test_gpu_densemap_align.py."""
import numpy as np

import densemap_model as dm

F = np.float32
IMAX = 1 << dm.QBITS
FAR, OUTSIDE, UNMATCHED, REJECTED, MATCHED = range(5)
DEFAULTS = dict(max_iterations=20, neighbourhood=1, max_residual=0.0, min_matched=50, eps_rot=1e-5, eps_trans=1e-5, degenerate_ratio=1e-4)


def frozen_of(keys, surfels):
    """(keys, (m, 6) float32 records) of a freeze: the voxels (ascending keys, their (n, 8) surfels) that have a normal"""
    keys, surfels = np.asarray(keys, np.uint64), np.asarray(surfels, np.float32).reshape(-1, 8)
    assert len(keys) == len(surfels)
    has = surfels[:, 4:7].any(axis=1)
    return keys[has], np.ascontiguousarray(surfels[has][:, [0, 1, 2, 4, 5, 6]])


def table_slots(count):
    """slots of the snapshot's table: the smallest power of two >= 2 * count and >= 1024"""
    s = 1024
    while s < 2 * count:
        s *= 2
    return s


def rtc_of(R=np.eye(3), t=(0, 0, 0), c=(0, 0, 0)):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64), np.asarray(c, np.float64)]).astype(np.float32)


def _keys_of_cells(cells):
    u = (cells + IMAX).astype(np.uint64)
    return u[:, 0] | (u[:, 1] << np.uint64(dm.KBITS)) | (u[:, 2] << np.uint64(2 * dm.KBITS))


def match(keys, recs, points, rtc, leaf, neighbourhood=1):
    """the per-point part of step(): (cls (n,) with FAR / OUTSIDE / UNMATCHED or -1 for a point that found a surfel, a (n, 3), e (n, 3),
    index (n,) of the chosen record or -1)"""
    keys, recs = np.asarray(keys, np.uint64), np.asarray(recs, np.float32).reshape(-1, 6)
    assert neighbourhood in (0, 1) and np.all(keys[1:] > keys[:-1])
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    rtc = np.asarray(rtc, np.float32)
    R, t, c = rtc[:9].reshape(3, 3), rtc[9:12], rtc[12:15]
    n = len(p)
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        d = p - c
        a = np.stack([(R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1]) + R[k, 2] * d[:, 2] for k in range(3)], axis=1)
        pp = a + t
        near = np.all(np.abs(a) < F(1024.0), axis=1)    # (NaN: not near)
        fi = np.floor(pp * inv)
        inside = np.all(np.abs(fi) < F(IMAX), axis=1)
    cls = np.full(n, -1, np.int64)
    cls[~near] = FAR
    cls[near & ~inside] = OUTSIDE
    act = np.flatnonzero(near & inside)
    ic = fi[act].astype(np.int64)
    found = np.zeros(len(act), bool)
    best = np.zeros(len(act), np.float32)
    e = np.zeros((len(act), 3), np.float32)
    which = np.full(len(act), -1, np.int64)
    rng = (-1, 0, 1) if neighbourhood else (0,)
    for oz in rng:
        for oy in rng:
            for ox in rng:
                cc = ic + np.array([ox, oy, oz], np.int64)
                ok = np.all(np.abs(cc) < IMAX, axis=1)    # a cell outside the key range is skipped
                if not len(keys) or not ok.any():
                    continue
                key = _keys_of_cells(np.where(ok[:, None], cc, 0))
                pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
                hit = ok & (keys[pos] == key)
                ee = pp[act] - recs[pos, :3]
                d2 = (ee[:, 0] * ee[:, 0] + ee[:, 1] * ee[:, 1]) + ee[:, 2] * ee[:, 2]
                better = hit & (~found | (d2 < best))    # strict <: a tie stays with the earlier candidate
                found |= better
                best[better] = d2[better]
                e[better] = ee[better]
                which[better] = pos[better]
    cls[act[~found]] = UNMATCHED
    a_all, e_all, w_all = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.full(n, -1, np.int64)
    a_all[act], e_all[act], w_all[act] = a[act], e, which
    return cls, a_all, e_all, w_all


def step(keys, recs, points, rtc, leaf, neighbourhood=1, max_residual=None):
    """(sums (28,) int64, counts (5,) uint64) of loamx_densemap_align_step; max_residual None: the leaf"""
    recs = np.asarray(recs, np.float32).reshape(-1, 6)
    max_residual = F(leaf if max_residual is None else max_residual)
    assert 0.0 < max_residual <= 16.0
    cls, a, e, which = match(keys, recs, points, rtc, leaf, neighbourhood)
    got = np.flatnonzero(which >= 0)
    a, e, nr = a[got], e[got], recs[which[got], 3:6]
    r = (nr[:, 0] * e[:, 0] + nr[:, 1] * e[:, 1]) + nr[:, 2] * e[:, 2]
    ok = np.abs(r) <= max_residual
    cls[got[ok]] = MATCHED
    cls[got[~ok]] = REJECTED
    a, nr, r = a[ok], nr[ok], r[ok]
    J = [a[:, 1] * nr[:, 2] - a[:, 2] * nr[:, 1], a[:, 2] * nr[:, 0] - a[:, 0] * nr[:, 2], a[:, 0] * nr[:, 1] - a[:, 1] * nr[:, 0],
         nr[:, 0], nr[:, 1], nr[:, 2]]
    terms = [(J[k] * J[l]) * F(65536.0) for k in range(6) for l in range(k, 6)]
    terms += [(J[k] * r) * F(16777216.0) for k in range(6)] + [(r * r) * F(16777216.0)]
    assert all(t.dtype == np.float32 for t in terms)
    sums = np.array([int(np.rint(t).astype(np.int64).sum()) for t in terms], np.int64)    # (rint: to nearest, ties to even, as rintf)
    counts = np.array([(cls == k).sum() for k in range(5)], np.uint64)
    assert int(counts.sum()) == len(cls)
    return sums, counts


def system_of(sums):
    """(H (6, 6), g (6,), sum of r^2) in float64"""
    s = np.asarray(sums, np.int64).astype(np.float64)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = s[:21] / 65536.0
    H = H + np.triu(H, 1).T
    return H, s[21:27] / 16777216.0, s[27] / 16777216.0


def solve(sums, degenerate_ratio=1e-4):
    """(x (6,) float64, dropped) of loamx_densemap_align_solve"""
    H, g, _ = system_of(sums)
    lam, V = np.linalg.eigh(H)
    keep = (lam > 0.0) & (lam > float(F(degenerate_ratio)) * max(lam.max(), 0.0))
    x = np.zeros(6)
    for k in np.flatnonzero(keep):
        x -= V[:, k] * ((V[:, k] @ g) / lam[k])
    return x, int((~keep).sum())


def exp_so3(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    A = 1.0 - th * th / 6.0 if th < 1e-4 else np.sin(th) / th
    B = 0.5 - th * th / 24.0 if th < 1e-4 else (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + A * K + B * (K @ K)


def align(keys, recs, points, pose_in, leaf, centre=None, **cfg):
    """loamx_densemap_align: dict(pose (3, 4), iterations, degenerate_dims, status, rms, counts)"""
    cfg = dict(DEFAULTS, **cfg)
    P = np.asarray(pose_in, np.float64).reshape(3, 4)
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float32).astype(np.float64)
    R, t = P[:, :3].copy(), P[:, :3] @ c + P[:, 3]
    max_residual = cfg["max_residual"] if cfg["max_residual"] != 0 else leaf
    out = dict(pose=P.copy(), iterations=0, degenerate_dims=0, status=1, rms=0.0, counts=None)
    for it in range(cfg["max_iterations"]):
        sums, counts = step(keys, recs, points, rtc_of(R, t, c), leaf, cfg["neighbourhood"], max_residual)
        matched = int(counts[MATCHED])
        out.update(iterations=it + 1, counts=counts, rms=float(np.sqrt(system_of(sums)[2] / matched)) if matched else 0.0)
        if matched < cfg["min_matched"]:
            out["status"] = 2
            break
        x, out["degenerate_dims"] = solve(sums, cfg["degenerate_ratio"])
        R, t = exp_so3(x[:3]) @ R, t + x[3:]
        out["pose"] = np.concatenate([R, (t - R @ c)[:, None]], axis=1)
        if np.linalg.norm(x[:3]) < float(F(cfg["eps_rot"])) and np.linalg.norm(x[3:]) < float(F(cfg["eps_trans"])):
            out["status"] = 0
            break
    return out


def pose_error(pose, truth):
    """(rotation angle in rad, translation distance) between two 3x4 poses"""
    A, B = np.asarray(pose, np.float64).reshape(3, 4), np.asarray(truth, np.float64).reshape(3, 4)
    dR = A[:, :3] @ B[:, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(A[:, 3] - B[:, 3]))


# ---- scenes -------------------------------------------------------------------------------------------------------------------------
BOX_LO, BOX_HI = np.array([-2.9, -2.3, -1.6]), np.array([3.1, 2.7, 1.4])    # 6 x 5 x 3 m, no wall on a cell face
BOX_LEAF = 0.5


def box_points(rng, n, sigma=0.01):
    """n points on the inside of the box's six faces, area-weighted, with noise sigma across the face; (n, 4) float32, map frame"""
    ext = BOX_HI - BOX_LO
    area = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, n, p=area / area.sum())
    p = BOX_LO + rng.uniform(0.0, 1.0, (n, 3)) * ext
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, BOX_LO[ax], BOX_HI[ax]) + rng.normal(0.0, sigma, n)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = p
    return out


def box_scene(seed=7, case=0):
    """dict: sweeps = three (points, origin) of 4000 map-frame points each; cloud = a fourth sweep of 4000 points in its sensor frame;
    truth = its pose (3, 4); start = the pose the alignment starts from, 0.02-0.1 rad and 0.1-0.4 m off (case picks the offset)"""
    rng = np.random.default_rng(seed)
    origins = [(0.4, -0.3, 0.1), (-1.2, 0.8, -0.4), (1.5, 0.6, 0.3)]
    sweeps = [(box_points(rng, 4000), o) for o in origins]
    Rt = exp_so3([0.05, -0.12, 0.3])
    tt = np.array([0.3, 0.5, -0.2])
    q = box_points(rng, 4000)
    cloud = np.zeros((4000, 4), np.float32)
    cloud[:, :3] = (q[:, :3].astype(np.float64) - tt) @ Rt    # R^T (q - t), row-wise
    truth = np.concatenate([Rt, tt[:, None]], axis=1)
    off_rot = ([0.02, 0.0, 0.0], [0.03, -0.05, 0.04], [-0.06, 0.05, 0.06])[case]
    off_t = ([0.1, 0.0, 0.0], [-0.15, 0.1, 0.1], [0.25, -0.25, 0.18])[case]
    Rs = exp_so3(off_rot) @ Rt
    start = np.concatenate([Rs, (tt + np.array(off_t))[:, None]], axis=1)
    return dict(sweeps=sweeps, cloud=cloud, truth=truth, start=start, leaf=BOX_LEAF)


def lattice_plane(z=0.0, x0=-4.0, nx=64):
    """the exact plane: nx x 64 points at spacing 0.125 on the plane z, x from x0, y from -4; with the leaf 0.5 every voxel holds 16
    points at the offsets 0, 1/4, 1/2, 3/4: mean = the cell's low corner + 0.1875, normal exactly (0, 0, 1) seen from above"""
    x = x0 + 0.125 * np.arange(nx)
    y = -4.0 + 0.125 * np.arange(64)
    out = np.zeros((nx * 64, 4), np.float32)
    out[:, 0] = np.repeat(x, 64)
    out[:, 1] = np.tile(y, nx)
    out[:, 2] = z
    return out


PLANE_ORIGIN = (0.3, 0.2, 2.0)
