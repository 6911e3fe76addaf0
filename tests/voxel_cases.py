"""Edge-shape cases for the segmented voxel grid (csrc/voxel.hip through loamx_voxel_probe), their reference and their analysis.

A case is plain data: points, segments (contiguous `seg_off` OR one `seg_ids` entry per point), an optional mask, the two leaves —
plus `claims`: what the generator built the case FOR (key bits, pass-through segments, runs across tile ends).  analyse() recomputes
those facts from the points in numpy int64, the way the kernels derive them (floor(p * (1/leaf)) in float32), and
tests/test_voxel_cases_cpu.py holds every case to its claims: a generator cannot silently miss the edge it was written for.

reference(): pcl::VoxelGrid per segment through the oracle — every segment's valid points in input order, the leaf by the segment's
parity, results back to back, out_off the running count.
"""
import numpy as np

TILE = 2048           # elements per tile of k_vox_ds / k_vox_ds_seg
SEG_KERNEL_MAX = 256  # contiguous, unmasked input of at most this many segments goes to k_vox_ds_seg
INT_MAX = 2**31 - 1


def bits(v: int) -> int:
    return int(v).bit_length()


class Case:
    def __init__(self, name, pts, nseg, leaf_even, leaf_odd=None, seg_off=None, seg_ids=None, valid=None, **claims):
        self.name = name
        self.pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        self.n = len(self.pts)
        self.nseg = int(nseg)
        self.leaf_even = float(leaf_even)
        self.leaf_odd = float(leaf_even if leaf_odd is None else leaf_odd)
        assert (seg_off is None) != (seg_ids is None)
        self.seg_off = None if seg_off is None else np.asarray(seg_off, np.uint32)
        self.seg_ids = None if seg_ids is None else np.asarray(seg_ids, np.uint32)
        self.valid = None if valid is None else np.asarray(valid, np.uint8)
        assert self.seg_off is None or (len(self.seg_off) == self.nseg + 1 and self.seg_off[0] == 0 and self.seg_off[-1] == self.n
                                        and np.all(np.diff(self.seg_off.astype(np.int64)) >= 0))
        assert self.seg_ids is None or (len(self.seg_ids) == self.n and (self.n == 0 or int(self.seg_ids.max()) < self.nseg))
        assert self.valid is None or len(self.valid) == self.n
        # claims: B (key bits of the largest linear voxel index among the filtered segments), passthrough (sorted segment list),
        # optionally cross / ends_on_tile / starts_on_tile / head_last_of_tile (see analyse)
        self.claims = claims
        assert "B" in claims and "passthrough" in claims, name

    def __repr__(self):
        return self.name

    @property
    def contiguous_unmasked(self):
        return self.seg_off is not None and self.valid is None

    @property
    def seg_kernel(self):
        """sort_reduce's dispatch: contiguous segments, no mask, <= 256 segments -> k_vox_ds_seg (unless LOAMX_VDS_GLOBAL)"""
        return self.contiguous_unmasked and self.nseg <= SEG_KERNEL_MAX and self.n > 0

    def seg_of_point(self):
        if self.seg_ids is not None:
            return self.seg_ids.astype(np.int64)
        return np.repeat(np.arange(self.nseg, dtype=np.int64), np.diff(self.seg_off.astype(np.int64)))

    def valid_mask(self):
        return np.ones(self.n, bool) if self.valid is None else self.valid != 0

    def settings(self):
        """the environments a case runs under: default, one workgroup walking every tile, and — contiguous unmasked input — the general kernel"""
        s = [{}, {"LOAMX_VDS_WGS": "1"}]
        if self.contiguous_unmasked:
            s.append({"LOAMX_VDS_GLOBAL": "1"})
        return s


def reference(orc, case):
    seg, ok = case.seg_of_point(), case.valid_mask()
    order = np.argsort(seg, kind="stable")
    order = order[ok[order]]
    counts = np.bincount(seg[order], minlength=case.nseg)
    starts = np.concatenate([[0], np.cumsum(counts)])
    out, out_off = [], np.zeros(case.nseg + 1, np.uint32)
    for s in range(case.nseg):
        if counts[s]:
            p = case.pts[order[starts[s]:starts[s + 1]]]
            r = orc.voxel_grid(p, case.leaf_odd if s & 1 else case.leaf_even)
            out.append(r)
            out_off[s + 1] = out_off[s] + len(r)
        else:
            out_off[s + 1] = out_off[s]
    return (np.concatenate(out) if out else np.zeros((0, 4), np.float32)), out_off


def _runs(keys_sorted):
    """[start, end) of the runs of equal rows"""
    m = len(keys_sorted)
    if m == 0:
        return np.zeros((0, 2), np.int64)
    head = np.ones(m, bool)
    head[1:] = np.any(keys_sorted[1:] != keys_sorted[:-1], axis=1)
    st = np.flatnonzero(head)
    return np.stack([st, np.concatenate([st[1:], [m]])], axis=1)


def _tile_facts(runs, base=None):
    """runs: [start, end) in sorted positions; base: per run, the position its tiles are counted from (segment start in the
    segmented kernel's layout, 0 in the general one)"""
    f = dict(cross=[], ends_on_tile=[], starts_on_tile=[], head_last_of_tile=[])
    for k, (a, b) in enumerate(runs):
        o = 0 if base is None else int(base[k])
        a, b = int(a) - o, int(b) - o
        for t in range(a // TILE + 1, (b - 1) // TILE + 1):   # tile ends strictly inside the run
            f["cross"].append((t * TILE, a, b))
        if b % TILE == 0:
            f["ends_on_tile"].append((a, b))
        if a % TILE == 0 and a > 0:
            f["starts_on_tile"].append((a, b))
        if a % TILE == TILE - 1 and b - a > 1:
            f["head_last_of_tile"].append((a, b))
    return f


def analyse(case):
    """the facts the kernels derive from a case, in numpy int64"""
    seg, ok = case.seg_of_point(), case.valid_mask()
    leaf = np.where(seg & 1, np.float32(case.leaf_odd), np.float32(case.leaf_even)).astype(np.float32)
    inv = (np.float32(1.0) / leaf).astype(np.float32)
    scaled = (case.pts[:, :3] * inv[:, None]).astype(np.float32)
    ijk = np.floor(scaled).astype(np.int64)
    res = dict(max_scaled=float(np.abs(scaled[ok]).max()) if ok.any() else 0.0, max_extent=0, passthrough=[], B=0, B_general=0, B_seg=0)
    lin = np.zeros(case.n, np.int64)
    top_f = top_g = top_s = 0
    vi = np.flatnonzero(ok)
    by_seg = vi[np.argsort(seg[vi], kind="stable")]   # the valid points, grouped by segment, input order inside
    if len(by_seg):
        ss = seg[by_seg]
        starts = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
        counts = np.diff(np.concatenate([starts, [len(ss)]]))
        mn, mx = np.minimum.reduceat(ijk[by_seg], starts), np.maximum.reduceat(ijk[by_seg], starts)
        d = mx - mn + 1
        res["max_extent"] = int(d.max())
        prod = d[:, 0].astype(object) * d[:, 1].astype(object) * d[:, 2].astype(object)   # (Python integers: up to 2^72)
        through = np.array([v > INT_MAX for v in prod], bool)
        k = np.repeat(np.arange(len(starts)), counts)
        r = ijk[by_seg] - mn[k]
        with np.errstate(over="ignore"):
            flt = r[:, 0] + r[:, 1] * d[k, 0] + r[:, 2] * d[k, 0] * d[k, 1]
        # PCL copies a segment of more than INT_MAX voxels through; the kernels give each of its points a key of its own
        own = by_seg if case.seg_ids is not None else by_seg - case.seg_off.astype(np.int64)[ss]
        lin[by_seg] = np.where(through[k], own, flt)
        res["passthrough"] = [int(v) for v in ss[starts][through]]
        if (~through).any():
            top_f = max(int(v) for v in prod[~through]) - 1
        if through.any():
            top_g, top_s = case.n, int(counts[through].max())
    res["B"] = bits(top_f)
    res["B_general"] = bits(max(top_f, top_g))
    res["B_seg"] = bits(max(top_f, top_s))
    res["passes_general"] = max(1, -(-(res["B_general"] + bits(case.nseg)) // 8))
    res["passes_seg"] = max(1, -(-res["B_seg"] // 9))
    order = np.lexsort((lin, seg))   # stable: equal keys stay in input order
    order = order[ok[order]]
    keys = np.stack([seg[order], lin[order]], axis=1)
    runs = _runs(keys)
    res["order"], res["runs"], res["run_seg"] = order, runs, keys[runs[:, 0], 0] if len(runs) else np.zeros(0, np.int64)
    res["general"] = _tile_facts(runs)
    if case.seg_kernel:
        res["seg"] = _tile_facts(runs, base=case.seg_off.astype(np.int64)[keys[runs[:, 0], 0]])
    return res


def model(case):
    """what the kernels are DESIGNED to compute, from analyse(): per run of equal (segment, voxel index) in stably sorted order, the
    float32 sums accumulated from 0 in input order, divided by the count — the specification a device mismatch is measured against
    (tests/test_voxel_cases_cpu.py holds it to the oracle on every case, -0.0 in a pass-through segment excepted: see voxel.hpp)"""
    a = analyse(case)
    out = np.zeros((len(a["runs"]), 4), np.float32)
    zero = np.zeros((1, 4), np.float32)
    for k, (b, e) in enumerate(a["runs"]):
        out[k] = np.cumsum(np.concatenate([zero, case.pts[a["order"][b:e]]]), axis=0, dtype=np.float32)[-1] / np.float32(e - b)
    out_off = np.concatenate([[0], np.cumsum(np.bincount(a["run_seg"], minlength=case.nseg))]).astype(np.uint32)
    return out, out_off


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def _intensity(rng, n):
    """mixed magnitudes: a float sum of these depends on the order"""
    return (rng.random(n) * 10.0 ** rng.integers(-3, 5, n)).astype(np.float32)


def box_points(rng, n, dims, leaf, origin=(0, 0, 0), per_voxel=3):
    """n points in a box of dims voxels whose min corner is voxel `origin`: the first two points sit in the two extreme corners (so
    the box — and with it the key width — is exactly dims), the rest fall about per_voxel to a voxel, in shuffled order.  Points
    keep clear of the voxel faces (0.25 .. 0.75 of the leaf), so the float product p * (1/leaf) cannot round across one."""
    dims = np.asarray(dims, np.int64)
    nvox = max(1, min(int(np.prod(dims.astype(object))), -(-n // per_voxel)))
    vox = np.stack([rng.integers(0, d, nvox) for d in dims], axis=1)
    v = vox[rng.integers(0, nvox, n)]
    if n >= 1:
        v[0] = 0
    if n >= 2:
        v[1] = dims - 1
    p = np.zeros((n, 4), np.float32)
    leaf = np.broadcast_to(np.asarray(leaf, np.float64), (n,))   # (one leaf, or one per point)
    p[:, :3] = ((v + np.asarray(origin, np.int64) + 0.25 + 0.5 * rng.random((n, 3))) * leaf[:, None]).astype(np.float32)
    p[:, 3] = _intensity(rng, n)
    return p


def _key_bits(dims):
    return bits(int(dims[0]) * int(dims[1]) * int(dims[2]) - 1)


def _with_corners_in(rng, n, nseg, dims, leaf, origin, seg, full_seg, valid=None, leaf_odd=None):
    """box points for a given per-point segment array, every point scaled by its own segment's leaf (no segment's box exceeds dims):
    two valid points of segment full_seg sit in the box's extreme corners, so the batch's key width is exactly that of dims"""
    seg = np.asarray(seg, np.int64)
    lf = np.where(seg & 1, leaf if leaf_odd is None else leaf_odd, leaf)
    cand = np.flatnonzero((seg == full_seg) & (np.ones(n, bool) if valid is None else np.asarray(valid) != 0))
    assert len(cand) >= 2, "the segment that spans the box needs two valid points"
    order = np.concatenate([cand[:2], np.setdiff1d(np.arange(n), cand[:2])])   # box_points puts the corners first
    p = np.zeros((n, 4), np.float32)
    p[order] = box_points(rng, n, dims, lf[order], origin)
    return p


def _lengths(rng, n, nseg, empty=()):
    """nseg segment lengths adding up to n; the segments listed in `empty` get none"""
    live = np.array([s for s in range(nseg) if s not in set(empty)], np.int64)
    assert len(live) >= 1
    cnt = np.zeros(nseg, np.int64)
    if n >= len(live):
        cnt[live] = 1
        np.add.at(cnt, live[rng.integers(0, len(live), n - len(live))], 1)
    else:
        np.add.at(cnt, live[rng.integers(0, len(live), n)], 1)
    return cnt


def _off(cnt):
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


# ---- families ------------------------------------------------------------------------------------------------------------------

TILE_EDGE_N = (1, 2, 255, 256, 2047, 2048, 2049, 4096, 6149)


def tile_edge_cases():
    out = []
    for n in TILE_EDGE_N:
        rng = np.random.default_rng(1000 + n)
        dims = (16, 8, 8) if n >= 2 else (1, 1, 1)
        out.append(Case(f"tile_single_n{n}", box_points(rng, n, dims, 0.5, (-8, -4, -4)), 1, 0.5, seg_off=[0, n],
                        B=_key_bits(dims), passthrough=[]))
    for name, off in [("b2047", [0, 2047, 4094, 4871]), ("b2048", [0, 2048, 4096, 4873]), ("b2049", [0, 2049, 4098, 4875]),
                      ("thin", [0, 2047, 2048, 4097])]:
        rng = np.random.default_rng(1100 + off[1] + off[2])
        n, dims = off[-1], (16, 8, 8)
        seg = np.repeat(np.arange(3), np.diff(off))
        p = _with_corners_in(rng, n, 3, dims, 0.5, (-8, -4, -4), seg, 0)
        out.append(Case(f"tile_three_{name}", p, 3, 0.5, seg_off=off, B=_key_bits(dims), passthrough=[]))
    return out


def _row_of_runs(rng, counts, leaf=1.0):
    """one row of voxels along x: voxel k holds counts[k] points; the input order is shuffled, so the sort has work to do while a
    voxel's points keep an order of their own.  Coordinates and intensities of mixed magnitudes: the float sums depend on the order."""
    counts = np.asarray(counts, np.int64)
    vx = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    n = len(vx)
    vx = vx[rng.permutation(n)]
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = ((vx + 0.25 + 0.5 * rng.random(n) * 10.0 ** -rng.integers(0, 4, n)) * leaf).astype(np.float32)
    p[:, 1] = ((0.25 + 0.5 * rng.random(n)) * leaf * 10.0 ** -rng.integers(0, 6, n)).astype(np.float32)
    p[:, 2] = ((0.25 + 0.5 * rng.random(n)) * leaf).astype(np.float32)
    p[:, 3] = _intensity(rng, n)
    return p


def _fill(total, small=3):
    """voxel counts of `small` (the last one shorter) adding up to total"""
    c = [small] * (total // small)
    if total % small:
        c.append(total % small)
    return c


def run_cases():
    out = []
    # one voxel of 5000 points at sorted positions [1000, 6000): tiles 0, 1 and 2
    counts = _fill(1000) + [5000] + _fill(140)
    facts = dict(cross=[(2048, 1000, 6000), (4096, 1000, 6000)], ends_on_tile=[], starts_on_tile=[], head_last_of_tile=[])
    # a run that ends on a tile's last element, the next one starting on a tile's first; a run whose head is a tile's last element
    counts2 = _fill(2040) + [8, 10] + _fill(4095 - 2058) + [6] + _fill(900)
    facts2 = dict(cross=[(4096, 4095, 4101)], ends_on_tile=[(2040, 2048)], starts_on_tile=[(2048, 2058)], head_last_of_tile=[(4095, 4101)])
    for name, cnt, f, seed in (("run_5000_over_three_tiles", counts, facts, 21), ("run_tile_edges", counts2, facts2, 22)):
        rng = np.random.default_rng(seed)
        p = _row_of_runs(rng, cnt)
        n = len(p)
        out.append(Case(name, p, 1, 1.0, seg_off=[0, n], B=bits(len(cnt) - 1), passthrough=[], **f))
        # the same run structure where the map uses it: scattered ids and a mask (ignored slots sort behind everything, so the
        # positions of the valid elements — and the facts above — are the same)
        extra = _row_of_runs(rng, _fill(600))
        extra[:, 0] += 5.0
        at = np.sort(rng.choice(n + 600, 600, replace=False))
        q = np.zeros((n + 600, 4), np.float32)
        valid = np.ones(n + 600, np.uint8)
        valid[at] = 0
        q[valid != 0] = p
        q[at] = extra
        out.append(Case(name + "_masked_ids", q, 1, 1.0, seg_ids=np.zeros(n + 600, np.uint32), valid=valid, B=bits(len(cnt) - 1),
                        passthrough=[], **f))
    return out


KEY_BITS = (0, 1, 7, 8, 9, 10, 16, 17, 18, 19, 24, 25, 27, 28, 30, 31)
KEY_NSEG = (1, 300, 5000)


def dims_for_bits(B):
    """extents spread over the three axes whose largest linear index needs exactly B bits"""
    if B == 31:
        return (2**11, 2**10, 2**10 - 1)   # 2^31 - 2^21 voxels: the widest box PCL still filters
    a = (B + 2) // 3
    b = (B - a + 1) // 2
    return (2**a, 2**b, 2**(B - a - b))


def key_width_cases(B):
    dims = dims_for_bits(B)
    assert _key_bits(dims) == B
    origin = tuple(-(d // 2) for d in dims)
    rng = np.random.default_rng(300 + B)
    n = 3001
    out = [Case(f"bits{B}_contiguous", box_points(rng, n, dims, 0.5, origin), 1, 0.5, seg_off=[0, n], B=B, passthrough=[])]
    for nseg in KEY_NSEG:
        n = 3001 if nseg < 5000 else 7001
        seg = rng.integers(0, nseg, n)
        full = nseg // 2
        seg[:2] = full
        p = _with_corners_in(rng, n, nseg, dims, 0.5, origin, seg, full)
        out.append(Case(f"bits{B}_ids_nseg{nseg}", p, nseg, 0.5, seg_ids=seg, B=B, passthrough=[]))
    return out


def passthrough_cases():
    out = []
    rng = np.random.default_rng(41)
    n = 2500
    # 2^31 voxels: one more than INT_MAX -> copied through (dims_for_bits(31), one layer less, is filtered: key_width_cases(31))
    big = (2**11, 2**10, 2**10)
    out.append(Case("pass_2^31", box_points(rng, n, big, 0.5, (-1024, -512, -512)), 1, 0.5, seg_off=[0, n], B=0, passthrough=[0]))
    # dx * dy alone overflows 32 bits
    flat = (2**16, 2**16, 1)
    out.append(Case("pass_dxdy_2^32", box_points(rng, n, flat, 0.5, (-2**15, -2**15, 0)), 1, 0.5, seg_off=[0, n], B=0, passthrough=[0]))
    # a pass-through segment between ordinary ones, contiguous and scattered + masked
    small = (16, 8, 8)
    off = np.array([0, 2100, 4500, 7000], np.uint32)
    parts = [box_points(rng, 2100, small, 0.5, (-8, -4, -4)), box_points(rng, 2400, big, 0.5, (-1024, -512, -512)),
             box_points(rng, 2500, small, 0.5, (0, 0, 0))]
    p = np.concatenate(parts)
    out.append(Case("pass_between_ordinary", p, 3, 0.5, seg_off=off, B=_key_bits(small), passthrough=[1]))
    seg = np.repeat(np.arange(3), np.diff(off))
    perm = rng.permutation(len(p))
    valid = (rng.random(len(p)) > 0.2).astype(np.uint8)
    corners = np.isin(perm, [0, 1, 2100, 2101, 4500, 4501])   # every segment's two corner points stay valid
    valid[corners] = 1
    out.append(Case("pass_between_ordinary_masked_ids", p[perm], 3, 0.5, seg_ids=seg[perm], valid=valid, B=_key_bits(small), passthrough=[1]))
    return out


def _face_points(rng, n, leaf, lim=60.0):
    """coordinates in [-lim, lim]: most exactly on a face k * leaf (k negative and positive), some zeros of both signs, +-1e-30,
    the rest anywhere; the first two points are the corners (-lim, -lim, -lim) and (lim, lim, lim)"""
    kmax = int(round(lim / leaf))
    k = rng.integers(-kmax, kmax + 1, (n, 3))
    k = k[rng.integers(0, max(1, n // 3), n)]   # about three points per face corner
    xyz = (k.astype(np.float32) * np.float32(leaf)).astype(np.float32)
    kind = rng.integers(0, 10, (n, 3))
    xyz = np.where(kind == 0, np.float32(-0.0), xyz)
    xyz = np.where(kind == 1, np.float32(0.0), xyz)
    xyz = np.where(kind == 2, np.float32(1e-30), xyz)
    xyz = np.where(kind == 3, np.float32(-1e-30), xyz)
    xyz = np.where(kind == 4, (rng.random((n, 3)) * 2 * lim - lim).astype(np.float32), xyz).astype(np.float32)
    xyz[0], xyz[1] = -lim, lim
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = xyz
    p[:, 3] = _intensity(rng, n)
    return p


def face_cases():
    out = []
    for name, le, lo, Be in (("dyadic", 0.25, 0.5, bits(481**3 - 1)), ("fifths", 0.2, 0.4, bits(601**3 - 1))):
        rng = np.random.default_rng(50 + len(name))
        n = 4000
        p = _face_points(rng, n, le)
        out.append(Case(f"faces_{name}_single", p, 1, le, lo, seg_off=[0, n], B=Be, passthrough=[]))
        # even / odd segments with different leaves
        off = np.array([0, 1300, 2700, 2700, 4000], np.uint32)
        q = np.concatenate([_face_points(rng, 1300, le), _face_points(rng, 1400, lo), _face_points(rng, 1300, le)])
        out.append(Case(f"faces_{name}_even_odd", q, 4, le, lo, seg_off=off, B=Be, passthrough=[]))
        seg = np.repeat(np.arange(4), np.diff(off))
        perm = rng.permutation(n)
        out.append(Case(f"faces_{name}_even_odd_ids", q[perm], 4, le, lo, seg_ids=seg[perm], B=Be, passthrough=[]))
    return out


SEGMENT_NSEG = (1, 2, 3, 255, 256, 257, 300, 5000)


def _empties(nseg):
    """first, last, one in the middle and several in a row — as far as the segment count has room for them"""
    if nseg == 1:
        return ()
    if nseg == 2:
        return (0,)
    if nseg == 3:
        return (0, 2)
    mid = nseg // 2
    return (0, nseg - 1, mid // 2, mid, mid + 1, mid + 2)


def segment_cases(nseg):
    out = []
    dims, origin, leaf = (32, 16, 8), (-16, -8, -4), 0.5
    n = 6000 if nseg < 5000 else 9000
    for tag, empty in (("full", ()), ("empties", _empties(nseg))):
        if tag == "empties" and not empty:
            continue
        rng = np.random.default_rng(600 + nseg + len(empty))
        cnt = _lengths(rng, n, nseg, empty)
        full = int(np.argmax(cnt))
        seg = np.repeat(np.arange(nseg), cnt)
        p = _with_corners_in(rng, n, nseg, dims, leaf, origin, seg, full, leaf_odd=2 * leaf)
        # contiguous ranges: k_vox_ds_seg up to 256 segments, the general kernel with a search for the segment beyond
        out.append(Case(f"seg{nseg}_{tag}_contiguous", p, nseg, leaf, 2 * leaf, seg_off=_off(cnt), B=_key_bits(dims), passthrough=[]))
        # the same points as grouped ids: a workgroup of k_vox_ijk has a lead segment
        out.append(Case(f"seg{nseg}_{tag}_ids_grouped", p, nseg, leaf, 2 * leaf, seg_ids=seg, B=_key_bits(dims), passthrough=[]))
        # interleaved point by point: every wave straddles segments
        live = np.array([s for s in range(nseg) if s not in set(empty)])
        segi = live[np.arange(n) % len(live)]
        full = int(live[0])
        pi = _with_corners_in(rng, n, nseg, dims, leaf, origin, segi, full, leaf_odd=2 * leaf)
        out.append(Case(f"seg{nseg}_{tag}_ids_interleaved", pi, nseg, leaf, 2 * leaf, seg_ids=segi, B=_key_bits(dims), passthrough=[]))
    return out


def mask_cases():
    out = []
    dims, origin, leaf = (32, 16, 8), (-16, -8, -4), 0.5
    B = _key_bits(dims)
    n, nseg = 5000, 5
    rng = np.random.default_rng(71)
    cnt = _lengths(rng, n, nseg)
    off = _off(cnt)
    seg = np.repeat(np.arange(nseg), cnt)

    def both(name, valid, full, Bc=B):
        valid = np.asarray(valid, np.uint8)
        if valid.any():
            p = _with_corners_in(rng, n, nseg, dims, leaf, origin, seg, full, valid)
        else:
            p = box_points(rng, n, dims, leaf, origin)
        out.append(Case(f"mask_{name}_contiguous", p, nseg, leaf, seg_off=off, valid=valid, B=Bc, passthrough=[]))
        perm = rng.permutation(n)
        out.append(Case(f"mask_{name}_ids", p[perm], nseg, leaf, seg_ids=seg[perm], valid=valid[perm], B=Bc, passthrough=[]))

    v = (rng.random(n) >= 0.3).astype(np.uint8)
    both("30pc", v, 2)
    v = np.ones(n, np.uint8)
    v[0] = v[-1] = 0
    both("first_last", v, 2)
    v = np.ones(n, np.uint8)
    v[seg == 1] = 0
    both("whole_segment", v, 2)
    v = (rng.random(n) >= 0.3).astype(np.uint8)
    v[0] = v[-1] = 0
    v[seg == 3] = 0
    both("mixed", v, 2)
    both("all_invalid", np.zeros(n, np.uint8), 2, Bc=0)
    # n = 0: with and without a mask, contiguous and scattered
    e = np.zeros((0, 4), np.float32)
    out.append(Case("mask_n0_contiguous", e, 3, leaf, seg_off=[0, 0, 0, 0], B=0, passthrough=[]))
    out.append(Case("mask_n0_ids_masked", e, 3, leaf, seg_ids=np.zeros(0, np.uint32), valid=np.zeros(0, np.uint8), B=0, passthrough=[]))
    return out


def reuse_sequence():
    """one fixed sequence on the process's pipeline: large general, small segmented, the same large general again, n = 0, 5000
    segments, one segment"""
    dims, origin, leaf = (64, 32, 16), (-32, -16, -8), 0.4
    B = _key_bits(dims)
    rng = np.random.default_rng(81)
    n, nseg = 20000, 126
    seg = rng.integers(0, nseg, n)
    valid = (rng.random(n) >= 0.1).astype(np.uint8)
    seg[:2], valid[:2] = 7, 1
    large = Case("reuse_large_general", _with_corners_in(rng, n, nseg, dims, leaf, origin, seg, 7, valid), nseg, leaf, seg_ids=seg,
                 valid=valid, B=B, passthrough=[])
    cnt = np.array([1000, 1500, 500])
    segc = np.repeat(np.arange(3), cnt)
    small = Case("reuse_small_segmented", _with_corners_in(rng, 3000, 3, dims, leaf, origin, segc, 1), 3, leaf, seg_off=_off(cnt),
                 B=B, passthrough=[])
    empty = Case("reuse_n0", np.zeros((0, 4), np.float32), 126, leaf, seg_ids=np.zeros(0, np.uint32), valid=np.zeros(0, np.uint8),
                 B=0, passthrough=[])
    n5 = 9000
    seg5 = rng.integers(0, 5000, n5)
    seg5[:2] = 2500
    many = Case("reuse_nseg5000", _with_corners_in(rng, n5, 5000, dims, leaf, origin, seg5, 2500), 5000, leaf, seg_ids=seg5, B=B,
                passthrough=[])
    one = Case("reuse_nseg1", box_points(rng, 2500, dims, leaf, origin), 1, leaf, seg_ids=np.zeros(2500, np.uint32), B=B, passthrough=[])
    return [large, small, large, empty, many, one]


def all_cases():
    out = tile_edge_cases() + run_cases()
    for B in KEY_BITS:
        out += key_width_cases(B)
    out += passthrough_cases() + face_cases()
    for nseg in SEGMENT_NSEG:
        out += segment_cases(nseg)
    out += mask_cases() + reuse_sequence()
    return out
