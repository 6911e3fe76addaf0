"""numpy / Python model of the dense map's signed distance field and its mesh (include/loamx.h, loamx_densemap_tsdf_* and
loamx_densemap_mesh), exact to the bit, written from the header's text: the per-ray arithmetic in f32 scalars with the library's
roundings (no fused multiply-add, correctly rounded / and sqrt), the walk ported from tests/densemap_carve_model.py, integer sums
per cell, marching tetrahedra in plain Python over the cubes that can hold a triangle, vertices in f64 with one f32 rounding.  The
checker of tests/test_densemap_mesh_cpu.py and tests/test_gpu_densemap_mesh.py; the scenes the two share are at the end."""
import numpy as np

import densemap_carve_model as cm
import densemap_rebuild_model as rbm

F = np.float32
DEFAULTS = dict(x0=-64, y0=-64, z0=-64, nx=128, ny=128, nz=128, trunc_leaves=3.0, free_space=0, ray_stride=1, max_steps=4096,
                min_range=0.0, max_range=0.0)
TSDF_STATS = ("traced", "skipped_stride", "skipped_filter", "skipped_steps", "zero_length", "cells_visited", "cells_set", "max_weight")
MESH_STATS = ("valid", "inside", "tetrahedra", "holes", "vertices", "triangles")
ORDERS = ((1, 2, 4), (1, 4, 2), (2, 1, 4), (2, 4, 1), (4, 1, 2), (4, 2, 1))
PARITY = (0, 1, 1, 0, 0, 1)


def check(c):
    """the name of the first field out of its bounds, None when the configuration is valid (loamx_densemap_tsdf_check)"""
    for f in ("x0", "y0", "z0"):
        if not -2 ** 21 <= c[f] <= 2 ** 21:
            return f
    for f in ("nx", "ny", "nz"):
        if not 2 <= c[f] <= 1024:
            return f
    if c["nx"] * c["ny"] * c["nz"] > 2 ** 26:
        return "nx * ny * nz"
    if not 1.0 <= c["trunc_leaves"] <= 16.0:
        return "trunc_leaves"
    if c["free_space"] not in (0, 1):
        return "free_space"
    if c["ray_stride"] < 1:
        return "ray_stride"
    if not 1 <= c["max_steps"] <= 65536:
        return "max_steps"
    if not (c["min_range"] >= 0 and np.isfinite(c["min_range"])):
        return "min_range"
    if not (c["max_range"] >= 0 and np.isfinite(c["max_range"]) and (c["max_range"] == 0 or c["max_range"] >= c["min_range"])):
        return "max_range"
    return None


def window(leaf, centre, half):
    """(first, count) of one axis of loamx_densemap_tsdf_window, in double"""
    e = np.float64(F(leaf))
    lo = np.floor((np.float64(F(centre)) - np.float64(F(half))) / e)
    hi = np.floor((np.float64(F(centre)) + np.float64(F(half))) / e)
    return int(lo), int(max(hi - lo + 1, 2))


def walk(s, e, leaf):
    """carving's walk (densemap_carve_model.trace) from s to e: (cells k = 0 .. n_steps, n_steps), or (None, None) when the start
    cell fails the key rule"""
    return cm.trace(s, e, leaf)


class Tsdf:
    """the field of one loamx_densemap_tsdf_begin: W (uint32) and D (int64) as (nz, ny, nx) arrays, and the eight statistics"""

    def __init__(self, leaf, **cfg):
        self.leaf = F(leaf)
        self.cfg = dict(DEFAULTS, **cfg)
        assert check(self.cfg) is None, check(self.cfg)
        c = self.cfg
        self.W = np.zeros((c["nz"], c["ny"], c["nx"]), np.uint32)
        self.D = np.zeros((c["nz"], c["ny"], c["nx"]), np.int64)
        self.st = dict.fromkeys(TSDF_STATS[:6], 0)

    def add(self, points, origin):
        c, leaf, st = self.cfg, self.leaf, self.st
        pts = np.asarray(points, np.float32)
        o = np.asarray(origin, np.float32)
        keep, d2s = cm.added_mask(pts, o, leaf, c["min_range"], c["max_range"])
        tau = F(c["trunc_leaves"]) * leaf
        for i in range(len(pts)):
            if i % c["ray_stride"] != 0:
                st["skipped_stride"] += 1
                continue
            if not keep[i]:
                st["skipped_filter"] += 1
                continue
            p = pts[i, :3]
            ln = np.sqrt(d2s[i])
            if ln == 0:
                st["zero_length"] += 1
                continue
            d = p - o
            u = d / ln
            back = ln if c["free_space"] else min(tau, ln)
            with np.errstate(invalid="ignore", over="ignore"):
                s, e = p - u * back, p + u * tau
            cells, n_steps = walk(s, e, leaf)
            if cells is None or n_steps > c["max_steps"]:
                st["skipped_steps"] += 1
                continue
            st["traced"] += 1
            for cell in cells:
                rx, ry, rz = cell[0] - c["x0"], cell[1] - c["y0"], cell[2] - c["z0"]
                if not (0 <= rx < c["nx"] and 0 <= ry < c["ny"] and 0 <= rz < c["nz"]):
                    continue
                m = [(F(cell[a]) + F(0.5)) * leaf for a in range(3)]
                sd = ((p[0] - m[0]) * u[0] + (p[1] - m[1]) * u[1]) + (p[2] - m[2]) * u[2]
                r = min(max(sd / tau, F(-1)), F(1))
                q = int(np.rint(F(r) * F(1024)))
                self.W[rz, ry, rx] += 1
                self.D[rz, ry, rx] += q
                st["cells_visited"] += 1

    def stats(self):
        return dict(self.st, cells_set=int((self.W > 0).sum()), max_weight=int(self.W.max()))


def tet_triangles(inside, f):
    """the triangles of a processed tetrahedron: inside = four booleans by position, f its parity; a list of triangles, each three
    (i, j) position pairs with i < j, the edges its vertices lie on"""
    E = lambda i, j: (min(i, j), max(i, j))
    k = sum(inside)
    if k in (0, 4):
        return []
    if k in (1, 3):
        a = inside.index(k == 1)
        o = [i for i in range(4) if i != a]
        t = [E(a, o[0]), E(a, o[1]), E(a, o[2])]
        if (f + a + (k == 3)) % 2:
            t[1], t[2] = t[2], t[1]
        return [t]
    (a, b), (c, d) = [i for i in range(4) if inside[i]], [i for i in range(4) if not inside[i]]
    seq = (a, b, c, d)
    inv = sum(seq[i] > seq[j] for i in range(4) for j in range(i + 1, 4))
    q = [E(a, c), E(a, d), E(b, d), E(b, c)]
    if (f + inv) % 2:
        q = q[::-1]
    return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]


def mesh(W, D, leaf, x0, y0, z0, min_weight=2, axes="loam"):
    """(verts (V, 3) float32, tris (T, 3) uint32, stats) of loamx_densemap_mesh over the planes W, D ((nz, ny, nx))"""
    nz, ny, nx = W.shape
    valid = W >= min_weight
    inside = valid & (D < 0)
    rec = lambda x, y, z: (z * ny + y) * nx + x
    edges = {}     # (owner's record, e) -> (cell A, cell B)
    tri_keys = []  # per triangle three (owner's record, e)
    n_tet = n_hole = 0
    # only a cube with a valid corner can hold a processed tetrahedron or a hole
    cand = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for n in range(8):
        cand |= valid[(n >> 2):nz - 1 + (n >> 2), ((n >> 1) & 1):ny - 1 + ((n >> 1) & 1), (n & 1):nx - 1 + (n & 1)]
    for z, y, x in np.argwhere(cand).tolist():   # ascending (z, y, x) = ascending record
        cell = [(x + (n & 1), y + ((n >> 1) & 1), z + (n >> 2)) for n in range(8)]
        v8 = [bool(valid[c[2], c[1], c[0]]) for c in cell]
        i8 = [bool(inside[c[2], c[1], c[0]]) for c in cell]
        for t, (a, b, _) in enumerate(ORDERS):
            corner = (0, a, a | b, 7)
            v4 = [v8[n] for n in corner]
            i4 = [i8[n] for n in corner]
            if not all(v4):
                signs = {i4[k] for k in range(4) if v4[k]}
                n_hole += len(signs) == 2
                continue
            n_tet += 1
            for tri in tet_triangles(i4, PARITY[t]):
                keys = []
                for i, j in tri:
                    ca, cb = corner[i], corner[j]
                    key = (rec(*cell[ca]), (cb ^ ca) - 1)
                    edges[key] = (cell[ca], cell[cb])
                    keys.append(key)
                tri_keys.append(keys)
    order = sorted(edges)
    index = {k: n for n, k in enumerate(order)}
    lf = np.float64(F(leaf))
    first = (x0, y0, z0)
    verts = np.zeros((len(order), 3), np.float32)
    for n, key in enumerate(order):
        A, B = edges[key]
        da, wa = int(D[A[2], A[1], A[0]]), int(W[A[2], A[1], A[0]])
        db, wb = int(D[B[2], B[1], B[0]]), int(W[B[2], B[1], B[0]])
        N = da * wb
        M = N - db * wa
        assert abs(N) < 2 ** 63 and abs(M) < 2 ** 63 and M != 0
        t = np.float64(N) / np.float64(M)
        for a in range(3):
            ma = (np.float64(first[a] + A[a]) + 0.5) * lf
            mb = (np.float64(first[a] + B[a]) + 0.5) * lf
            verts[n, a] = F(ma + t * (mb - ma))
    if axes == "sensor":
        verts = verts[:, [2, 0, 1]].copy()
    tris = np.array([[index[k] for k in keys] for keys in tri_keys], np.uint32).reshape(-1, 3)
    st = dict(valid=int(valid.sum()), inside=int(inside.sum()), tetrahedra=n_tet, holes=n_hole, vertices=len(verts), triangles=len(tris))
    return verts, tris, st


def read_ply(path):
    """(verts (V, 3) float32, tris (T, 3) int32) of a binary little-endian PLY file as loamx_write_ply writes it"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nt = int([l for l in lines if l.startswith("element face")][0].split()[2])
    assert [l for l in lines if l.startswith("property")] == ["property float x", "property float y", "property float z",
                                                               "property list uchar int vertex_indices"]
    verts = np.frombuffer(raw, "<f4", 3 * nv, end).reshape(nv, 3)
    faces = np.frombuffer(raw, np.dtype([("n", "u1"), ("i", "<i4", 3)]), nt, end + 12 * nv)
    assert len(raw) == end + 12 * nv + 13 * nt and np.all(faces["n"] == 3)
    return verts, faces["i"]


# ---- topology of an indexed mesh

def topology(tris):
    """(undirected edge -> number of triangles, the directed edges that occur more than once)"""
    und, seen, twice = {}, set(), []
    for t in np.asarray(tris).tolist():
        for i in range(3):
            a, b = t[i], t[(i + 1) % 3]
            und[(min(a, b), max(a, b))] = und.get((min(a, b), max(a, b)), 0) + 1
            if (a, b) in seen:
                twice.append((a, b))
            seen.add((a, b))
    return und, twice


def boundary_loops(und):
    """the number of closed loops the boundary edges (those in one triangle) form, None when they form no loops"""
    nb = {}
    for (a, b), n in und.items():
        if n == 1:
            nb.setdefault(a, []).append(b)
            nb.setdefault(b, []).append(a)
    if any(len(v) != 2 for v in nb.values()):
        return None
    loops, left = 0, set(nb)
    while left:
        loops += 1
        stack = [left.pop()]
        while stack:
            for w in nb[stack.pop()]:
                if w in left:
                    left.remove(w)
                    stack.append(w)
    return loops


def normals(verts, tris):
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


# ---- the scenes that the CPU and the GPU tests share

def pts4(xyz):
    p = np.zeros((len(xyz), 4), np.float32)
    p[:, :3] = xyz
    return p


SPHERE = dict(leaf=0.25, R=1.25, origin=(0.07, 0.03, -0.05), cfg=dict(x0=-8, y0=-8, z0=-8, nx=16, ny=16, nz=16, trunc_leaves=3.0))


def sphere_points(n=2500, R=SPHERE["R"]):
    """n Fibonacci-sphere directions from the scene's origin, each ending on the sphere of radius R about (0, 0, 0)"""
    o = np.float64(SPHERE["origin"])
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    b = d @ o
    t = -b + np.sqrt(b * b - (o @ o - R * R))
    return pts4(o + d * t[:, None])


# The wall x = 1.3 m seen from the origin.  The distance a ray adds to a cell is the projective one, (p - m) . u: with p - m =
# (dx, ey, ez) and u ~ (1, (m_y + ey) / range, (m_z + ez) / range) its mean over the rays through a cell is dx + (var(ey) + var(ez)) /
# range + (mean(ey) m_y + mean(ez) m_z) / range.  The variance term, leaf^2 / (6 range) for rays that cover the cell evenly, shifts
# the zero crossing by leaf / (6 range) leaves; the mean term vanishes only where the rays cover a cell symmetrically, so the window
# lies inside the rays' footprint (0.3 m * 1.15 / 1.3 = 0.265 m at the near end of the band, the window's cells reach 0.2 m).
# leaf 0.05 m: 0.05 / 7.8 = 0.0064 leaves, an eighth of the 0.05 leaves the test allows; 41 rays over 0.6 m are 3.3 per cell and axis.
WALL = dict(leaf=0.05, x=1.3, origin=(0.0, 0.0, 0.0), cfg=dict(x0=22, y0=-3, z0=-4, nx=8, ny=7, nz=7, trunc_leaves=3.0))


def wall_points(n=41, half=0.3):
    """n x n rays from the origin that end on the plane x = 1.3, y and z in [-half, half]"""
    g = np.linspace(-half, half, n)
    y, z = np.meshgrid(g, g, indexing="ij")
    return pts4(np.stack([np.full(y.size, WALL["x"]), y.ravel(), z.ravel()], axis=1))


_cache = {}


def scene(name):
    """(Tsdf, points, origin) of "sphere" or "wall", integrated once and shared: do not change what comes back"""
    if name not in _cache:
        S, pts = (SPHERE, sphere_points()) if name == "sphere" else (WALL, wall_points())
        t = Tsdf(S["leaf"], **S["cfg"])
        t.add(pts, S["origin"])
        _cache[name] = (t, pts, np.float32(S["origin"]))
    return _cache[name]


def scene_mesh(name, axes="loam"):
    key = (name, "mesh", axes)
    if key not in _cache:
        t = scene(name)[0]
        _cache[key] = mesh(t.W, t.D, t.leaf, t.cfg["x0"], t.cfg["y0"], t.cfg["z0"], 2, axes)
    return _cache[key]


def corrected(sweeps, corrections):
    """the sweeps moved as the history form moves them (densemap_rebuild_model.corrected_sweeps)"""
    return rbm.corrected_sweeps(sweeps, corrections)
