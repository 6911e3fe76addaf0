"""Edge-shape cases for the per-ring less-flat voxel grid (csrc/features.hip: k_feat_lf_voxel, and the generic VoxelPipeline
behind it for rings of more than 4096 points), their model and their analysis.

The handle on the kernel is the public ScanRegistration.process: with surface_curvature_threshold = 3e38 (huge, finite) no point is
ever a corner, and flat picks keep a label <= less flat, so EVERY point of every feature region is a less-flat candidate.  With
n_feature_regions = 1 the one region of a ring of `len` points is [cr, len - cr - 2]: the ring contributes p[cr : len - cr - 1] in
order (len >= 2 * cr + 3; a shorter ring contributes nothing).  With more regions, regions of one point are skipped
(oracle/oracle_features.hpp: `if (ep <= sp) continue`), so candidates() restates the region formula instead of assuming the slice.
Two consequences: a ring cannot have ONE candidate, and a ring of 4096 points has at most 4096 - 2 * cr - 1 of them.

A case is plain data: a list of rings (float32 (len, 4), intensity = ring + fraction as real sweeps have), leaf, cr, nreg — plus
`claims`, what the case was written FOR.  analyse() recomputes those facts per ring in numpy the way the kernel derives them
(float32 floor(p * (1/leaf)), int64 products) and tests/test_lfvoxel_cases_cpu.py holds every case to its claims.

Where a ring is built from a body of chosen candidates (n_feature_regions = 1), `cr` pad points in front and `cr + 1` behind copy the
first body point; they are never candidates.

Every case keeps |p / leaf| < 2^23.  The oracle subtracts the box corner in float as PCL does (floor(p * inv) - (float)min_b), the
kernel in integers; the two agree only while the quotients and their differences are exactly representable in float32, and below
2^23 the half-integer coordinates the wide boxes use are exact too.  With extents below 2^24 an axis alone never exceeds INT_MAX, so
the kernel's `dx > INT_MAX` and `dy > INT_MAX` guards are unreachable here; and `dz > INT_MAX / (dx * dy) + 1` implies
dx * dy * dz > INT_MAX in exact arithmetic, so that guard never decides alone — the `tall` pair sits on both sides of it with a
small dx * dy, which is as close as a case can come.  No pass-through case holds a -0.0: the kernel's (0 + x) / 1 turns it into
+0.0 where PCL copies it (the difference csrc/voxel.hpp documents)."""
import numpy as np

INT_MAX = 2**31 - 1
LFV_MAX = 4096        # rings up to this length: k_feat_lf_voxel; one longer ring sends every ring to the generic VoxelPipeline
LFV_THREADS = 1024    # a step of the kernel's head scan, and the divisor of per_wave
STEPS = (1024, 2048, 3072)
GUARDS = ("dx", "dy", "dxdy", "dz", "dxdydz")   # the kernel's pass-through conditions, in its order
THRESHOLD = 3e38


def candidates(length, cr, nreg):
    """ring-relative indices of the less-flat candidates of a ring of `length` points, in output order: the region bounds of
    oracle/oracle_features.hpp (e0 is the ring's LAST index; regions of a single point are skipped)"""
    e0 = length - 1
    if e0 <= 2 * cr:
        return np.zeros(0, np.int64)
    out = []
    for j in range(nreg):
        sp = (cr * (nreg - j) + (e0 - cr) * j) // nreg
        ep = (cr * (nreg - 1 - j) + (e0 - cr) * (j + 1)) // nreg - 1
        if ep <= sp:
            continue
        out.append(np.arange(sp, ep + 1, dtype=np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


class Case:
    def __init__(self, name, rings, leaf, cr=5, nreg=1, **claims):
        self.name, self.leaf, self.cr, self.nreg, self.claims = name, float(leaf), int(cr), int(nreg), claims
        self.rings = [np.ascontiguousarray(r, np.float32).reshape(-1, 4) for r in rings]

    def __repr__(self):
        return self.name

    def cloud(self):
        return np.concatenate(self.rings) if self.rings else np.zeros((0, 4), np.float32)

    def sizes(self):
        return [len(r) for r in self.rings]

    def ring_candidates(self, r):
        return self.rings[r][candidates(len(self.rings[r]), self.cr, self.nreg)]

    def device_config(self):
        return dict(n_feature_regions=self.nreg, curvature_region=self.cr, less_flat_filter_size=self.leaf,
                    surface_curvature_threshold=THRESHOLD)

    def oracle_config(self):
        return dict(nFeatureRegions=self.nreg, curvatureRegion=self.cr, lessFlatFilterSize=self.leaf,
                    surfaceCurvatureThreshold=THRESHOLD)


def reference(orc, case):
    """pcl::VoxelGrid through the oracle on every ring's candidates in order, results back to back; (cloud, per-ring offsets)"""
    out, off = [], np.zeros(len(case.rings) + 1, np.int64)
    for r in range(len(case.rings)):
        c = case.ring_candidates(r)
        g = orc.voxel_grid(c, case.leaf) if len(c) else np.zeros((0, 4), np.float32)
        out.append(g)
        off[r + 1] = off[r] + len(g)
    return (np.concatenate(out) if out else np.zeros((0, 4), np.float32)), off


_REF = {}


def cached_reference(orc, case):
    """reference(), computed once per case name (the generators are deterministic) and handed out read-only"""
    if case.name not in _REF:
        out, off = reference(orc, case)
        out.flags.writeable = off.flags.writeable = False
        _REF[case.name] = (out, off)
    return _REF[case.name]


def _keys(c, leaf):
    """(ijk int64, dims, product as a Python integer) of the candidates c, as the kernel derives them"""
    inv = np.float32(1.0) / np.float32(leaf)
    scaled = (c[:, :3] * inv).astype(np.float32)
    ijk = np.floor(scaled).astype(np.int64)
    dims = ijk.max(axis=0) - ijk.min(axis=0) + 1
    return scaled, ijk, dims, int(dims[0]) * int(dims[1]) * int(dims[2])


def _fsum_rows(p, reverse=False):
    """float32 sums of the rows of p accumulated from 0 in order (or in reversed order)"""
    q = p[::-1] if reverse else p
    return np.cumsum(np.concatenate([np.zeros((1, p.shape[1]), np.float32), q]), axis=0, dtype=np.float32)[-1]


def _run_bounds(k_sorted):
    head = np.ones(len(k_sorted), bool)
    head[1:] = k_sorted[1:] != k_sorted[:-1]
    st = np.flatnonzero(head)
    return st, np.concatenate([st[1:], [len(k_sorted)]])


def analyse_ring(c, leaf):
    """the facts k_feat_lf_voxel derives from one ring's candidates c (m, 4)"""
    m = len(c)
    f = dict(m=m, per_wave=-(-m // LFV_THREADS) * 64, dims=[0, 0, 0], passthrough=False, guards=(), bits=0, passes=0, voxels=0,
             longest_run=0, straddles=[], heads_at=[], ends_at=[], digits=[], order_sensitive=0, max_scaled=0.0, negative=False,
             on_faces=0)
    if m == 0:
        return f
    scaled, ijk, dims, prod = _keys(c, leaf)
    dx, dy, dz = (int(v) for v in dims)
    fired = (dx > INT_MAX, dy > INT_MAX, dx * dy > INT_MAX, dz > INT_MAX // (dx * dy) + 1, prod > INT_MAX)
    f.update(dims=[dx, dy, dz], passthrough=any(fired), guards=tuple(g for g, on in zip(GUARDS, fired) if on),
             max_scaled=float(np.abs(scaled).max()), negative=bool((ijk < 0).any()),
             on_faces=int((scaled == np.floor(scaled)).any(axis=1).sum()))
    if f["passthrough"]:
        lin = np.arange(m, dtype=np.int64)   # a key of its own per point; nothing is sorted
    else:
        r = ijk - ijk.min(axis=0)
        lin = r[:, 0] + r[:, 1] * dx + r[:, 2] * dx * dy
        if m > 1:
            f["bits"] = (prod - 1).bit_length()
            f["passes"] = -(-f["bits"] // 8)
    order = np.argsort(lin, kind="stable")
    st, en = _run_bounds(lin[order])
    f.update(order=order, lin=lin, run_start=st, run_end=en, voxels=len(st), longest_run=int((en - st).max()))
    f["straddles"] = [s for s in STEPS if np.any((st < s) & (en > s))]
    f["heads_at"] = [s - 1 for s in STEPS if np.any(st == s - 1)]
    f["ends_at"] = [s for s in STEPS if np.any(en == s)]
    for ps in range(f["passes"]):
        h = np.bincount((lin >> (8 * ps)) & 255, minlength=256)
        f["digits"].append((int((h > 0).sum()), int(h.max())))
    if not f["passthrough"]:
        for a, b in zip(st, en):
            if b - a > 1:
                p = c[order[a:b]]
                f["order_sensitive"] += int(not np.array_equal(_fsum_rows(p).view(np.uint32), _fsum_rows(p, True).view(np.uint32)))
    return f


def analyse(case):
    """analyse_ring for every ring of the case"""
    return [analyse_ring(case.ring_candidates(r), case.leaf) for r in range(len(case.rings))]


def model(case, reverse=False, unstable=False, passthrough=True):
    """what the kernel is DESIGNED to compute: per ring, the candidates keyed by PCL's linear voxel index, sorted stably, every voxel
    the float32 sum from 0 in input order over the count; a ring of more than INT_MAX voxels copied through.  The three switches
    build the wrong models the CPU test must be able to tell from the oracle: sums in reversed order, an unstable sort (by key, then
    by coordinate), no pass-through."""
    out = []
    for r in range(len(case.rings)):
        c = case.ring_candidates(r)
        if len(c) == 0:
            continue
        _, ijk, dims, prod = _keys(c, case.leaf)
        if passthrough and prod > INT_MAX:
            out.append(c.copy())
            continue
        rel = ijk - ijk.min(axis=0)
        lin = rel[:, 0] + rel[:, 1] * int(dims[0]) + rel[:, 2] * int(dims[0]) * int(dims[1])
        order = np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0], lin)) if unstable else np.argsort(lin, kind="stable")
        st, en = _run_bounds(lin[order])
        g = np.zeros((len(st), 4), np.float32)
        for k, (a, b) in enumerate(zip(st, en)):
            g[k] = _fsum_rows(c[order[a:b]], reverse) / np.float32(b - a)
        out.append(g)
    return np.concatenate(out) if out else np.zeros((0, 4), np.float32)


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def _stamp(xyz, ring):
    """(n, 3) -> (n, 4) with intensity = ring + fraction of the sweep"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = xyz
    p[:, 3] = (ring + 0.1 * np.arange(n) / 8192.0).astype(np.float32)
    return p


def ring_of(body, cr, ring=0, extra_back=0):
    """a ring whose candidates (n_feature_regions = 1) are exactly `body` (+ extra_back copies of its first point behind it); the
    pad points copy the first body point whole, intensity included"""
    body = _stamp(body, ring)
    assert len(body) >= 2
    return np.concatenate([np.repeat(body[:1], cr, 0), body, np.repeat(body[:1], cr + 1 + extra_back, 0)])


def _cells(rng, cells, leaf, jitter=True):
    """points inside the given integer voxels: at the voxel's middle, or anywhere in its middle half (clear of the faces)"""
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    f = 0.25 + 0.5 * rng.random(cells.shape) if jitter else 0.5
    return ((cells + f) * leaf).astype(np.float32)


def _box(rng, n, dims, leaf=1.0, origin=(0, 0, 0), per_voxel=1, jitter=True):
    """n points in a box of dims voxels at voxel `origin`: the first two in its extreme corners (each alone in its voxel), the
    rest about per_voxel to a voxel, in shuffled order"""
    dims, origin = np.asarray(dims, np.int64), np.asarray(origin, np.int64)
    nvox = max(1, (n - 2) // per_voxel)
    vox = np.stack([rng.integers(0, d, nvox) for d in dims], axis=1)
    assert dims[0] > 2
    vox[np.all(vox == 0, axis=1) | np.all(vox == dims - 1, axis=1), 0] = 1   # (off the two corners)
    v = vox[rng.integers(0, nvox, n)]
    v[0], v[1] = 0, dims - 1
    return _cells(rng, v + origin, leaf, jitter)


def _spread(rng, n, lo, hi):
    """n points anywhere in the box [lo, hi) (per-axis bounds), as a sweep's are: the first two 1 cm (at most) inside its two
    extreme corners, so the box is the whole of it; voxel faces are not avoided"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = lo + (hi - lo) * rng.random((n, 3))
    inset = 0.01 * np.minimum(hi - lo, 1.0)
    p[0], p[1] = lo + inset, hi - inset
    return p.astype(np.float32)


def _row_of_runs(rng, counts, leaf=1.0, shuffle=True):
    """one row of voxels along x: voxel k holds counts[k] points of mixed magnitudes (their float sums depend on the order), the
    input order shuffled"""
    counts = np.asarray(counts, np.int64)
    vx = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
    n = len(vx)
    if shuffle:
        vx = vx[rng.permutation(n)]
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = ((vx + 0.25 + 0.5 * rng.random(n) * 10.0 ** -rng.integers(0, 4, n)) * leaf).astype(np.float32)
    p[:, 1] = ((0.25 + 0.5 * rng.random(n)) * leaf * 10.0 ** -rng.integers(0, 6, n)).astype(np.float32)
    p[:, 2] = ((0.25 + 0.5 * rng.random(n)) * leaf).astype(np.float32)
    return p


def _fill(total, small=3):
    c = [small] * (total // small)
    if total % small:
        c.append(total % small)
    return c


BIG = (2047, 1024, 1024)   # 2^31 - 2^20 voxels: the widest such box PCL still filters


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def passthrough_cases():
    out = []
    rng = np.random.default_rng(11)
    # 2^31 voxels, half-integer coordinates: only the product of all three extents exceeds INT_MAX
    v = np.stack([rng.integers(0, d, 502) for d in (2048, 1024, 1024)], axis=1)
    v[0], v[1] = 0, (2047, 1023, 1023)
    out.append(Case("2^31 voxels", [ring_of(_cells(rng, v, 1.0, jitter=False), 5)], 1.0, dims=[2048, 1024, 1024], passthrough=True,
                    guards=("dxdydz",), m=502))
    # one layer of x less: the last product below the limit
    out.append(Case("2^31 - 2^20 voxels", [ring_of(_box(rng, 3000, BIG, per_voxel=3), 5)], 1.0, dims=list(BIG), passthrough=False,
                    bits=31, passes=4, m=3000))
    # dx * dy alone is 2^31
    v = np.stack([rng.integers(0, 65536, 600), rng.integers(0, 32768, 600), np.zeros(600, np.int64)], axis=1)
    v[0], v[1] = 0, (65535, 32767, 0)
    out.append(Case("sheet", [ring_of(_cells(rng, v, 1.0, jitter=False), 5)], 1.0, dims=[65536, 32768, 1], passthrough=True,
                    guards=("dxdy", "dxdydz"), m=600))
    # dx * dy = 1024 and dz one more than INT_MAX / 1024 + 1: the dz guard fires (and with it, necessarily, the product)
    for name, dz, through in (("tall", 2097153, True), ("tall, one below the dz guard", 2097151, False)):
        v = np.stack([rng.integers(0, 32, 700), rng.integers(0, 32, 700), rng.integers(0, dz, 700)], axis=1)
        v[0], v[1] = 0, (31, 31, dz - 1)
        claims = dict(guards=("dz", "dxdydz")) if through else dict(bits=31, passes=4)
        out.append(Case(name, [ring_of(_cells(rng, v, 1.0, jitter=False), 5)], 1.0, dims=[32, 32, dz], passthrough=through, m=700, **claims))
    return out


def pass_count_cases():
    out = []
    rng = np.random.default_rng(12)
    body = (0.01 + 0.18 * rng.random((1500, 3))).astype(np.float32)
    out.append(Case("one voxel", [ring_of(body, 5)], 0.2, dims=[1, 1, 1], passthrough=False, bits=0, passes=0, m=1500, voxels=1,
                    longest_run=1500, straddles=[1024], per_wave=128, min_order_sensitive=1))
    out.append(Case("1 pass", [ring_of(_spread(rng, 1025, (0, 0, 0), (1.2, 1.2, 1.2)), 5)], 0.2, dims=[6, 6, 6], passthrough=False,
                    bits=8, passes=1, m=1025, per_wave=128, min_order_sensitive=100))
    out.append(Case("2 passes", [ring_of(_spread(rng, 2049, (-3, -3, -3), (3, 3, 3)), 5)], 0.2, dims=[30, 30, 30], passthrough=False,
                    bits=15, passes=2, m=2049, per_wave=192))
    out.append(Case("3 passes", [ring_of(_spread(rng, 3073, (-20, -2, -20), (20, 2, 20)), 5)], 0.2, dims=[200, 20, 200], passthrough=False,
                    bits=20, passes=3, m=3073, per_wave=256))
    # 12 voxels of 340 jittered points each behind the low corner, 11 single voxels and the high corner in the top layer:
    # the dense runs sit at sorted positions 1 + 340 k, so one of them lies across each of 1024, 2048 and 3072
    dense = np.stack([rng.integers(1, 2046, 12), rng.integers(0, 1024, 12), np.sort(rng.choice(1000, 12, replace=False))], axis=1)
    single = np.stack([np.arange(11) * 7, rng.integers(0, 1024, 11), np.full(11, 1023)], axis=1)
    v = np.concatenate([np.repeat(dense, 340, 0), single])
    v = v[rng.permutation(len(v))]
    v = np.concatenate([[[0, 0, 0], [2046, 1023, 1023]], v])
    assert len(v) == 4093
    out.append(Case("4 passes, dense runs", [ring_of(_cells(rng, v, 1.0), 1)], 1.0, cr=1, dims=list(BIG), passthrough=False, bits=31,
                    passes=4, m=4093, per_wave=256, longest_run=340, straddles=[1024, 2048, 3072], ring_len=4096,
                    min_order_sensitive=12))
    return out


def face_cases():
    rng = np.random.default_rng(13)
    k = rng.integers(-8, 9, (2000, 3))
    k = k[rng.integers(0, 700, 2000)]   # about three points per lattice node
    p = (k * 0.25).astype(np.float32)
    kind = rng.integers(0, 12, (2000, 3))
    p = np.where(kind == 0, np.float32(-0.0), p)
    p = np.where(kind == 1, np.float32(-1e-7), p)
    p = np.where(kind == 2, np.float32(1e-7), p).astype(np.float32)
    p[0], p[1] = -2.0, 2.0
    return [Case("faces", [ring_of(p, 5)], 0.25, dims=[17, 17, 17], passthrough=False, bits=13, passes=2, m=2000, negative=True,
                 min_on_faces=1500)]


def count_cases():
    out = []
    for cr in (5, 1):
        # two equal candidates; two distinct ones in one voxel; two in two voxels, the later voxel first
        a = np.array([[0.31, 0.52, 0.73], [0.31, 0.52, 0.73]], np.float32)
        b = np.array([[0.31, 0.52, 0.73], [0.3300001, 0.5900001, 0.7900001]], np.float32)
        c = np.array([[5.31, 0.52, 0.73], [-4.3, 0.52, 0.73]], np.float32)
        out.append(Case(f"m = 2, cr {cr}", [ring_of(x, cr, r) for r, x in enumerate((a, b, c))], 0.2, cr=cr, per_ring_m=[2, 2, 2],
                        per_ring_voxels=[1, 1, 2], per_ring_passes=[0, 0, 1], ring_len=2 * cr + 3, passthrough=False))
    rng = np.random.default_rng(14)
    out.append(Case("m = 1024", [ring_of(_spread(rng, 1024, (-6, -1, -6), (6, 1, 6)), 5)], 0.2, dims=[60, 10, 60], passthrough=False,
                    bits=16, passes=2, m=1024, per_wave=64))
    return out


def digit_cases():
    out = []
    rng = np.random.default_rng(15)
    # voxels 0, 256, ..., 65280 along x: every key has the low byte 0, the second byte takes all 256 values
    vx = np.repeat(np.arange(256) * 256, 8)[rng.permutation(2048)][:2000]
    vx[0], vx[1] = 0, 65280
    v = np.stack([vx, np.zeros(2000, np.int64), np.zeros(2000, np.int64)], axis=1)
    out.append(Case("one digit", [ring_of(_cells(rng, v, 1.0), 5)], 1.0, dims=[65281, 1, 1], passthrough=False, bits=16, passes=2, m=2000,
                    digits=[(1, 2000), (256, None)]))
    vx = np.repeat(np.arange(256), 5)[rng.permutation(1280)]
    v = np.stack([vx, np.zeros(1280, np.int64), np.zeros(1280, np.int64)], axis=1)
    out.append(Case("256 digits", [ring_of(_cells(rng, v, 1.0), 5)], 1.0, dims=[256, 1, 1], passthrough=False, bits=8, passes=1, m=1280,
                    digits=[(256, 5)], per_wave=128))
    return out


def step_edge_cases():
    """built from the sorted order: runs [1020, 1023) [1023, 1030) — a head on a step's last position whose run goes on into the
    next step; [2040, 2048) [2048, 2058) — an end and a head exactly on the boundary; [3071, 3072) — a head on the last position
    that is also the end"""
    rng = np.random.default_rng(16)
    counts = _fill(1020) + [3, 7] + _fill(2040 - 1030) + [8, 10] + _fill(3071 - 2058) + [1, 8] + _fill(100)
    body = _row_of_runs(rng, counts)
    return [Case("head at 1023", [ring_of(body, 5)], 1.0, dims=[len(counts), 1, 1], passthrough=False, m=sum(counts), passes=2,
                 heads_at=[1023, 3071], ends_at=[2048, 3072], straddles=[1024], per_wave=256)]


MIXED_LENGTHS = lambda cr: [4096, 3, 4, 2, 0, 1026, 1025, 5, 700, 2 * cr + 3]


def _mixed_rings(cr, lengths):
    rng = np.random.default_rng(17)
    boxes = {4096: ((-20, -2, -20), (20, 2, 20)), 1026: ((0, 0, 0), (1.2, 1.2, 1.2)), 1025: ((-3, -3, -3), (3, 3, 3)),
             700: ((-30, -1, 5), (30, 3, 60))}
    rings = []
    for r, L in enumerate(lengths):
        if L >= 2 * cr + 3:
            lo, hi = boxes.get(min(L, 4096), ((1, 1, 1), (1.1, 1.1, 1.1)))
            rings.append(ring_of(_spread(rng, min(L, 4096) - 2 * cr - 1, lo, hi), cr, r, extra_back=L - min(L, 4096)))
        else:   # too short for a region: any points
            rings.append(_stamp(rng.random((L, 3)) * 10 - 5, r))
    return rings


def mixed_batch_case(cr=5, longest=4096):
    """rings of 0, 2, ~1000 and ~4090 candidates in one launch, sized by the longest; longest = 4097 (one more pad point behind
    the first ring) sends every ring through the generic VoxelPipeline instead"""
    lengths = MIXED_LENGTHS(cr)
    lengths[0] = longest
    m = [max(0, L - 2 * cr - 1) if L >= 2 * cr + 3 else 0 for L in lengths]
    return Case("mixed batch" if longest == 4096 else f"mixed batch, longest ring {longest}", _mixed_rings(cr, lengths), 0.2, cr=cr,
                per_ring_m=m, ring_lens=lengths, passthrough=False)


def region_cases():
    out = []
    for nreg in (6, 13):
        cr = 5
        rng = np.random.default_rng(18 + nreg)
        lengths = [300, 12, 13, 40, nreg * cr + 2 * cr + 1, 2 * cr + 1 + nreg + nreg // 2]   # (the last: regions of one and two points)
        rings = [_stamp(_spread(rng, L, (-4, -1, -4), (4, 1, 4)), r) for r, L in enumerate(lengths)]
        out.append(Case(f"regions, {nreg}", rings, 0.2, cr=cr, nreg=nreg, ring_lens=lengths, passthrough=False))
    return out


def dispatch_pair():
    """the `3 passes` box in a ring of 4096 points (k_feat_lf_voxel) and the same ring with one more pad point behind (4097: the
    generic VoxelPipeline).  The extra pad point is one more candidate — a second copy of the first body point, which is alone in
    its voxel (the box's low corner): (0 + a + a) / 2 == a / 1 exactly, so both rings have the same less-flat cloud."""
    rng = np.random.default_rng(19)
    body = _spread(rng, 4096 - 11, (-20, -2, -20), (20, 2, 20))
    mk = lambda extra: Case(f"3 passes, ring of {4096 + extra}", [ring_of(body, 5, extra_back=extra)], 0.2, dims=[200, 20, 200],
                            passthrough=False, bits=20, passes=3, m=4085 + extra, ring_len=4096 + extra)
    return mk(0), mk(1)


def all_cases():
    return (passthrough_cases() + pass_count_cases() + face_cases() + count_cases() + digit_cases() + step_edge_cases()
            + [mixed_batch_case()] + region_cases())


def by_name(name, cases=None):
    return [c for c in (all_cases() if cases is None else cases) if c.name == name][0]


REUSE_ORDER = ("4 passes, dense runs", "m = 2, cr 5", "2^31 voxels", "one voxel", "mixed batch", "4 passes, dense runs")
