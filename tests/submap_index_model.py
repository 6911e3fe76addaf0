"""The sub-map grid index (csrc/submap_index.hip, grid_fit.hpp) stated directly in numpy float32 — what a build must produce, word for
word: the bounds through the order-preserving encoding (so -0.0 sorts below +0.0, as the integer atomics see it), the descriptor
loop of grid_fit.hpp, a point's cell as floor((x - o) * inv_h) clamped (a subtraction, then a multiplication: nothing to contract),
the cell table as the exclusive scan of the cell counts, and the packed .w of a sorted point.  Plus the analysis the case tests use:
which set-up path a build takes, how far its grids grow, what its waves look like to wave_runs and cloud_bounds_update."""
import numpy as np

F = np.float32
MAX_CELLS = 16 * 1024 * 1024 - 2048      # LX_MAX_CELLS
FUSE_MAXK = 64                           # BB_FUSE_MAXK: up to here the set-up is folded into the count
SETUP_ROUND = 1024                       # k_bb_setup: clouds per round of its one workgroup
SINGLE, PACK_RING, FOLD_BOUNDS = 1, 2, 4
DESC = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("inv_h", "<f4"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"),
                 ("ncell", "<u4"), ("cell_base", "<u4"), ("pt_base", "<u4")])


def enc_f32(x):
    u = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec_f32(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(F)


def bounds(xyz):
    """(mn[3], mx[3]) of a non-empty cloud as the accumulators hold them"""
    e = enc_f32(xyz)
    return dec_f32(e.min(axis=0)), dec_f32(e.max(axis=0))


def grid_fit(mn, mx, cell0, budget):
    """grid_fit.hpp -> ((inv_h, nx, ny, nz, ncell), growth steps)"""
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    h, steps = F(cell0), 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        while True:
            inv_h = F(1.0) / h
            if not inv_h > 0:
                return (F(0), 1, 1, 1, 1), steps
            q = np.floor((mx - mn) * inv_h)
            if np.all((q >= 0) & (q < F(2147483648.0))):
                nx, ny, nz = (int(v) + 1 for v in q)
                if nx * ny * nz <= budget:
                    return (inv_h, nx, ny, nz, nx * ny * nz), steps
            h = F(h * F(1.25))
            steps += 1


def budget_of(K, single=False):
    return MAX_CELLS if single else MAX_CELLS // K


def descriptors(pts, off, cell0, single=False):
    """-> (DESC[K], growth steps per cloud); an empty cloud owns one cell of a unit grid at the origin"""
    off = np.asarray(off, np.int64)
    K = len(off) - 1
    d, steps, base = np.zeros(K, DESC), np.zeros(K, np.int64), 0
    for c in range(K):
        a, b = off[c], off[c + 1]
        d[c]["pt_base"], d[c]["cell_base"] = a, base
        if a == b:
            d[c]["inv_h"], d[c]["nx"], d[c]["ny"], d[c]["nz"], d[c]["ncell"] = 1.0, 1, 1, 1, 1
        else:
            mn, mx = bounds(pts[a:b, :3])
            (inv_h, nx, ny, nz, nc), steps[c] = grid_fit(mn, mx, cell0, budget_of(K, single))
            d[c]["ox"], d[c]["oy"], d[c]["oz"], d[c]["inv_h"] = mn[0], mn[1], mn[2], inv_h
            d[c]["nx"], d[c]["ny"], d[c]["nz"], d[c]["ncell"] = nx, ny, nz, nc
        base += int(d[c]["ncell"])
    return d, steps


def cloud_of(off, n):
    """cloud of every point index: the last cloud whose offset is <= i (the kernels' binary search; empty clouds own nothing)"""
    return np.searchsorted(np.asarray(off, np.int64), np.arange(n), side="right") - 1


def cell_xyz(d, xyz):
    """integer cell coordinates of points under ONE descriptor record"""
    o = np.array([d["ox"], d["oy"], d["oz"]], F)
    q = np.floor((np.asarray(xyz, F) - o) * F(d["inv_h"]))
    hi = np.array([d["nx"], d["ny"], d["nz"]], np.int64) - 1
    return np.clip(np.nan_to_num(q, nan=0.0), 0, hi.astype(F)).astype(np.int64).clip(0, hi)


def cells(pts, off, desc):
    """global table entry (cell_base + linear cell) of every point"""
    n = len(pts)
    out, cl = np.zeros(n, np.int64), cloud_of(off, n)
    for c in np.unique(cl):
        m = cl == c
        d = desc[c]
        ijk = cell_xyz(d, pts[m, :3])
        out[m] = int(d["cell_base"]) + (ijk[:, 2] * int(d["ny"]) + ijk[:, 1]) * int(d["nx"]) + ijk[:, 0]
    return out


def packed_w(pts, off, pack_ring):
    """.w word of every input point once sorted: its index inside its cloud, under pack_ring with (int)w in the top byte (255: no ring)"""
    n = len(pts)
    off = np.asarray(off, np.int64)
    li = np.arange(n) - off[cloud_of(off, n)] if n else np.zeros(0, np.int64)
    if not pack_ring:
        return li.astype(np.uint32)
    ring = np.trunc(pts[:, 3].astype(np.float64)).astype(np.int64)
    ok = (li <= 0xffffff) & (ring >= 0) & (ring < 255)
    return np.where(ok, (ring << 24) | li, 0xff000000 | (li & 0xffffff)).astype(np.uint32)


def build(pts, off, cell0=1.05, flags=0):
    """-> dict(desc, steps, cell (table entry of every input point), table (total cells + 1), w (packed .w of every input point))"""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 4)
    desc, steps = descriptors(pts, off, cell0, bool(flags & SINGLE))
    cell = cells(pts, off, desc)
    total = int(desc[-1]["cell_base"]) + int(desc[-1]["ncell"])
    table = np.zeros(total + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=total), out=table[1:])
    return dict(desc=desc, steps=steps, cell=cell, table=table.astype(np.uint32), w=packed_w(pts, off, bool(flags & PACK_RING)))


# ---- analysis: which paths a build takes ------------------------------------------------------------------------------------------
def setup_path(off, flags=0):
    """'single' | 'fused' (K <= 64 and points) | 'unfused' (k_bb_setup) | 'unfused2' (k_bb_setup goes round its loop more than once)"""
    K, n = len(off) - 1, int(off[-1])
    if flags & SINGLE:
        return "single"
    if n > 0 and K <= FUSE_MAXK:
        return "fused"
    return "unfused2" if K > SETUP_ROUND else "unfused"


def wave_facts(cell, off):
    """what wave_runs and cloud_bounds_update meet: point i is lane i % 64 of wave i // 64, four waves to a workgroup"""
    n = len(cell)
    cl = cloud_of(off, n)
    f = dict(tail_lanes=n % 64, waves=(n + 63) // 64, cut_at_wave_end=0, run_across_waves=0, mixed_waves=0, max_clouds_in_workgroup=0,
             same_cloud_waves_in_workgroup=0, longest_run=0, boundaries_inside_a_wave=0)
    if n == 0:
        return f
    edge = np.arange(64, n, 64)
    f["cut_at_wave_end"] = int((cell[edge] != cell[edge - 1]).sum())
    f["run_across_waves"] = int((cell[edge] == cell[edge - 1]).sum())
    change = np.flatnonzero(np.diff(cell) != 0) + 1
    f["longest_run"] = int(np.diff(np.concatenate([[0], change, [n]])).max())
    for g in range(0, n, 256):
        whole = []
        for w in range(g, min(g + 256, n), 64):
            u = np.unique(cl[w:w + 64])
            if len(u) > 1:
                f["mixed_waves"] += 1
                f["boundaries_inside_a_wave"] = max(f["boundaries_inside_a_wave"], len(u) - 1)
            else:
                whole.append(int(u[0]))
        f["max_clouds_in_workgroup"] = max(f["max_clouds_in_workgroup"], len(np.unique(cl[g:g + 256])))
        f["same_cloud_waves_in_workgroup"] = max(f["same_cloud_waves_in_workgroup"], max([whole.count(c) for c in whole], default=0))
    return f


def neighbourhood_violations(pts, off, desc, cell0, queries_per_cloud=64, seed=0):
    """brute force: points of a cloud within cell0 * sqrt(0.9999) of a query (float64 distance) that do NOT lie in the 27 cells around the
    query's cell — the property both searches rest on.  Queries: points of the cloud and points between them."""
    rng = np.random.default_rng(seed)
    gate2 = float(cell0) ** 2 * 0.9999
    bad = []
    off = np.asarray(off, np.int64)
    clouds = [c for c in range(len(off) - 1) if off[c + 1] > off[c]]
    if len(clouds) > 48:
        clouds = [clouds[i] for i in sorted(rng.choice(len(clouds), 48, replace=False))]
    for c in clouds:
        P = pts[off[c]:off[c + 1], :3]
        pick = rng.choice(len(P), min(len(P), queries_per_cloud), replace=False)
        Q = np.concatenate([P[pick], ((P[pick].astype(np.float64) + P[rng.permutation(pick)]) / 2).astype(F)])
        cq, cp = cell_xyz(desc[c], Q), cell_xyz(desc[c], P)
        d2 = ((Q[:, None, :].astype(np.float64) - P[None, :, :].astype(np.float64)) ** 2).sum(axis=2)
        far = (np.abs(cq[:, None, :] - cp[None, :, :]) > 1).any(axis=2)
        for qi, pi in zip(*np.nonzero((d2 < gate2) & far)):
            bad.append((c, Q[qi].tolist(), P[pi].tolist()))
    return bad
