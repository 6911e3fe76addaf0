"""Edge-shape cases for the sub-map grid index (csrc/submap_index.hip through loamx_index_probe): the smallest shapes that reach each
path of the two builds.  Every case states what it is meant to reach in `claims`; tests/test_index_cases_cpu.py proves each claim from
the model (tests/submap_index_model.py), tests/test_gpu_index_probe.py runs the cases on the device.

claims (all optional but `path`):
  path             'single' | 'fused' | 'unfused' | 'unfused2' (k_bb_setup's second round of 1024 clouds)
  grows            growth steps of the coarsest cloud (h *= 1.25f); absent = 0
  tail_lanes       active lanes of the last wave
  cut_at_wave_end  a cell run ends exactly at lane 63 (the next one starts at lane 0)
  run_across_waves a cell run goes on across a wave boundary
  longest_run      at least this many consecutive points in one cell
  mixed_wave       with FOLD_BOUNDS: a wave holds points of more than one cloud
  boundaries_in_wave  at least this many cloud boundaries inside one wave
  clouds_in_wg     at least this many clouds inside one workgroup of 256
  dedup            two whole waves of one cloud in one workgroup (combined by the first of them)
  empties          indices of the empty clouds
  bbox_capped      more points than the bounding-box launch has threads (grid-stride loop taken)
  integer_extent   (mx - mn) * inv_h is an exact integer on some axis (the maximum sits on a cell face)
  zeros            -0.0 and +0.0 both present on an axis (the minimum is -0.0)
  negative         negative coordinates
  rings            the ring bytes expected among the sorted points
A cloud of more than 2^24 points (pack_ring's other fallback) is left out: too large for a test of a few seconds."""
import numpy as np

import submap_index_model as sm

F = np.float32
SINGLE, PACK_RING, FOLD = sm.SINGLE, sm.PACK_RING, sm.FOLD_BOUNDS


class Case:
    def __init__(self, name, pts, off, cell=1.05, flags=0, **claims):
        self.name, self.cell, self.flags, self.claims = name, cell, flags, claims
        self.pts = np.ascontiguousarray(pts, F).reshape(-1, 4)
        self.off = np.asarray(off, np.uint32)
        assert self.off[0] == 0 and self.off[-1] == len(self.pts) and (np.diff(self.off.astype(np.int64)) >= 0).all()
        self.pts.setflags(write=False)

    @property
    def n(self):
        return len(self.pts)

    @property
    def K(self):
        return len(self.off) - 1

    def folded(self):
        return Case(self.name + "_fold", self.pts, self.off, self.cell, self.flags | FOLD, **self.claims)

    def __repr__(self):
        return self.name


def _rng(name):
    return np.random.default_rng(abs(hash_name(name)))


def hash_name(s):
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) & 0xffffffff
    return h


def path_points(rng, n, start=(0, 0, 0), step=0.08, noise=0.02, rings=16):
    """points in scan order: a slow drift, so that neighbouring points mostly share a cell; .w = a ring id"""
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    t = np.arange(n)[:, None] * step
    p = np.asarray(start, np.float64) + t * d + rng.normal(scale=noise, size=(n, 3))
    w = (np.arange(n) * rings // max(n, 1)).astype(np.float64)
    return np.column_stack([p, w]).astype(F)


def box_points(rng, n, lo, ext, w=0.0):
    p = np.asarray(lo, np.float64) + rng.random((n, 3)) * np.asarray(ext, np.float64)
    return np.column_stack([p, np.full(n, w)]).astype(F)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 63, 64, 65, 255, 256, 257)


def size_cases():
    out = []
    for n in SIZES:
        p = path_points(_rng(f"size{n}"), n, start=(-3, 2, -1))
        out.append(Case(f"single_n{n}", p, [0, n], 1.05, SINGLE, path="single", tail_lanes=n % 64, negative=True))
        out.append(Case(f"batch_n{n}", p, [0, n], 2.1, PACK_RING, path="fused", tail_lanes=n % 64, negative=True))
    p = path_points(_rng("single32769"), 32769, step=0.004)
    out.append(Case("single_n32769", p, [0, 32769], 1.05, SINGLE, path="single", tail_lanes=1, bbox_capped=True, run_across_waves=True))
    p = np.concatenate([path_points(_rng("b8193"), 8193, step=0.01), path_points(_rng("b100"), 100, start=(50, 0, 0))])
    out.append(Case("batch_cloud8193", p, [0, 8193, 8293], 2.1, PACK_RING, path="fused", bbox_capped=True, mixed_wave=True))
    return out


# ---- cell patterns ----------------------------------------------------------------------------------------------------------------
def _cells_along_x(cell_ids, rng, h=1.05):
    """points whose cell along x is cell_ids[i] (grid origin pinned by a first point at 0): x = (id + 0.5) * h"""
    n = len(cell_ids)
    p = np.zeros((n, 4))
    p[:, 0] = (np.asarray(cell_ids) + 0.5) * h
    p[:, 1:3] = rng.random((n, 2)) * 0.5
    p[0, :3] = 0.0
    return p.astype(F)


def pattern_cases():
    out = []
    same = np.tile(np.array([[1.5, -2.25, 0.75, 3.0]], F), (300, 1))
    out.append(Case("single_identical300", same, [0, 300], 1.05, SINGLE, path="single", longest_run=300, run_across_waves=True, tail_lanes=44))
    out.append(Case("batch_identical300", same, [0, 300], 2.1, PACK_RING, path="fused", longest_run=300, run_across_waves=True, tail_lanes=44))
    r = _rng("onecell")
    one = box_points(r, 1000, (4, 4, 4), (1.0, 1.0, 1.0))
    out.append(Case("single_onecell1000", one, [0, 1000], 1.05, SINGLE, path="single", longest_run=1000, run_across_waves=True))
    out.append(Case("batch_onecell1000_of3", np.concatenate([path_points(r, 70), one, path_points(r, 70, start=(9, 9, 9))]), [0, 70, 1070, 1140], 1.05, 0,
                    path="fused", longest_run=1000, run_across_waves=True))
    alt = _cells_along_x(np.arange(512) % 2, r)
    out.append(Case("single_two_cells_alternating", alt, [0, 512], 1.05, SINGLE, path="single", longest_run=1, cut_at_wave_end=True))
    out.append(Case("batch_two_cells_alternating", alt, [0, 512], 1.05, PACK_RING, path="fused", longest_run=1, cut_at_wave_end=True))
    ids64 = np.arange(64 * 5) // 64
    out.append(Case("single_runs_cut_at_lane63", _cells_along_x(ids64, r), [0, 320], 1.05, SINGLE, path="single", longest_run=64, cut_at_wave_end=True, tail_lanes=0))
    ids63 = np.concatenate([[0], 1 + np.arange(64 * 5 + 20) // 63])   # runs of 63: their ends walk through every lane
    out.append(Case("single_runs_of_63", _cells_along_x(ids63, r), [0, len(ids63)], 1.05, SINGLE, path="single", longest_run=63, run_across_waves=True))
    for tail in (1, 63):
        n = 64 * 4 + tail
        ids = np.arange(n) // 32
        out.append(Case(f"single_tail{tail}", _cells_along_x(ids, r), [0, n], 1.05, SINGLE, path="single", tail_lanes=tail, cut_at_wave_end=True))
        out.append(Case(f"batch_tail{tail}", _cells_along_x(ids, r, 2.1), [0, n], 2.1, 0, path="fused", tail_lanes=tail, cut_at_wave_end=True))
    big = np.concatenate([np.zeros(10, int), np.full(600, 3), np.arange(100) % 5])
    out.append(Case("single_cell_over_a_workgroup", _cells_along_x(big, r), [0, 710], 1.05, SINGLE, path="single", longest_run=600, run_across_waves=True))
    return out


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def geometry_cases():
    out = []
    r = _rng("geom")
    for h in (0.25, 0.5, 2.0):   # dyadic edges: (x - o) * inv_h is exact, lattice points sit ON the cell faces, the maximum on the far corner
        g = np.stack(np.meshgrid(np.arange(7), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * h + np.array([-3 * h, 1.0, -2.0])
        p = np.column_stack([g, np.arange(len(g)) % 16]).astype(F)
        p = p[r.permutation(len(p))]
        out.append(Case(f"batch_faces_h{h}", p, [0, len(p)], h, PACK_RING, path="fused", integer_extent=True, negative=True))
        out.append(Case(f"batch_faces_h{h}_two_clouds", np.concatenate([p, p + F(100.0)]), [0, len(p), 2 * len(p)], h, 0, path="fused", integer_extent=True))
    k = np.arange(0, 40, dtype=F)
    lat = np.column_stack([k * F(1.05), (k % 7) * F(1.05), (k % 3) * F(1.05), np.zeros(40, F)]).astype(F)   # multiples of float32(1.05): quotients at or just under integers
    out.append(Case("single_faces_105", lat, [0, 40], 1.05, SINGLE, path="single"))
    out.append(Case("batch_faces_21", np.column_stack([k * F(2.1), (k % 7) * F(2.1), (k % 3) * F(2.1), np.zeros(40, F)]).astype(F), [0, 40], 2.1, 0, path="fused"))
    z = box_points(r, 200, (-0.0, -0.0, -0.0), (3, 3, 3))
    z[0, :3] = (-0.0, 0.0, -0.0)
    z[1, :3] = (0.0, -0.0, 0.0)
    z[2, :3] = (0.0, 0.0, 0.0)
    out.append(Case("single_signed_zeros", z, [0, 200], 1.05, SINGLE, path="single", zeros=True))
    out.append(Case("batch_signed_zeros", np.concatenate([z, z[::-1]]), [0, 200, 400], 2.1, 0, path="fused", zeros=True))
    neg = box_points(r, 300, (-500, -80, -30), (40, 30, 6), w=7)
    out.append(Case("single_negative", neg, [0, 300], 1.05, SINGLE, path="single", negative=True))
    out.append(Case("batch_negative", neg, [0, 100, 300], 2.1, PACK_RING, path="fused", negative=True))
    return out


# ---- growth ---------------------------------------------------------------------------------------------------------------------
def _corners(lo, ext):
    lo, ext = np.asarray(lo, np.float64), np.asarray(ext, np.float64)
    return np.column_stack([np.array([lo, lo + ext]), np.zeros(2)]).astype(F)


def _clouds(rng, K, ext, per=6, spread=400.0, w=0.0):
    """K clouds of `per` points each, every cloud spanning exactly `ext` (its two corners come first)"""
    parts = []
    for c in range(K):
        lo = (rng.random(3) - 0.5) * spread
        parts.append(np.concatenate([_corners(lo, (ext,) * 3), box_points(rng, per - 2, lo, (ext,) * 3, w)]))
    return np.concatenate(parts), _offsets([per] * K)


def growth_cases():
    out = []
    r = _rng("growth")
    cube = np.concatenate([_corners((-1500, -1500, -1500), (3000,) * 3), box_points(r, 298, (-1500,) * 3, (3000,) * 3)])
    out.append(Case("single_cube3000", cube, [0, 300], 1.05, SINGLE, path="single", grows=11, negative=True))
    slab = np.concatenate([_corners((0, 0, 0), (5000, 5000, 1)), box_points(r, 298, (0, 0, 0), (5000, 5000, 1))])
    out.append(Case("single_slab5000", slab, [0, 300], 1.05, SINGLE, path="single", grows=1))
    p, off = _clouds(r, 64, 100.0)
    out.append(Case("batch_K64_100m", p, off, 1.05, 0, path="fused", grows=2))
    p, off = _clouds(r, 65, 100.0)
    out.append(Case("batch_K65_100m", p, off, 1.05, 0, path="unfused", grows=2))
    p, off = _clouds(r, 4096, 20.0, per=3)
    out.append(Case("batch_K4096_20m", p, off, 1.05, 0, path="unfused2", grows=2))
    mega = np.concatenate([_corners((0, 0, 0), (1e6,) * 3), box_points(r, 198, (0, 0, 0), (1e6,) * 3)])   # the largest extent any GPU test uses
    out.append(Case("single_cube1e6", mega, [0, 200], 1.05, SINGLE, path="single", grows=37))
    out.append(Case("batch_cube1e6_of2", np.concatenate([mega, path_points(r, 50)]), [0, 200, 250], 2.1, 0, path="fused", grows=35))
    return out


# ---- K ----------------------------------------------------------------------------------------------------------------------------
KS = (1, 2, 16, 64, 65, 1024, 1025, 4096)


def k_cases(K):
    out = []
    for cell in (1.05, 2.1):
        r = _rng(f"K{K}_{cell}")
        lens = r.integers(0 if K > 2 else 1, 10, K)
        parts = [box_points(r, int(m), (r.random(3) - 0.5) * 200, (5, 5, 5), w=c % 64) for c, m in enumerate(lens)]
        path = "fused" if K <= 64 else ("unfused2" if K > 1024 else "unfused")
        out.append(Case(f"K{K}_cell{cell}", np.concatenate(parts), _offsets(lens), cell, PACK_RING if cell == 2.1 else 0, path=path,
                        empties=[int(c) for c in np.flatnonzero(lens == 0)], mixed_wave=K > 1, clouds_in_wg=min(K, 12), negative=True))
    return out


# ---- empty clouds and boundaries ----------------------------------------------------------------------------------------------------
def empty_cases():
    out = []
    r = _rng("empty")

    def make(name, lens, cell=2.1, flags=PACK_RING, **claims):
        parts = [path_points(r, int(m), start=(r.random(3) - 0.5) * 60) for m in lens]
        p = np.concatenate(parts) if sum(lens) else np.zeros((0, 4), F)
        K = len(lens)
        path = ("fused" if K <= 64 else ("unfused2" if K > 1024 else "unfused")) if sum(lens) else ("unfused2" if K > 1024 else "unfused")
        return Case(name, p, _offsets(lens), cell, flags, path=path, empties=[i for i, m in enumerate(lens) if m == 0], **claims)
    out.append(make("empty_first", [0, 70, 5, 130]))
    out.append(make("empty_middle", [70, 0, 5, 130]))
    out.append(make("empty_last", [70, 5, 130, 0]))
    out.append(make("empty_row", [0, 0, 70, 0, 0, 0, 5, 130, 0, 0], mixed_wave=True))
    out.append(make("empty_all_K1", [0]))
    out.append(make("empty_all_K3", [0, 0, 0], 1.05, 0))
    out.append(make("empty_all_K70", [0] * 70))
    out.append(make("empty_all_K1030", [0] * 1030))
    out.append(make("empty_most_K70", [0] * 30 + [9] + [0] * 38 + [4]))
    out.append(make("one_point_clouds_K20", [1] * 20, mixed_wave=True, boundaries_in_wave=19, clouds_in_wg=20))
    out.append(make("one_point_clouds_K300", [1] * 300, mixed_wave=True, boundaries_in_wave=63, clouds_in_wg=256))
    out.append(make("short_clouds_K40", list(r.integers(1, 30, 40)), mixed_wave=True, boundaries_in_wave=2, clouds_in_wg=8))
    out.append(make("boundaries_at_64_256", [64, 64, 128, 256, 256, 192, 64, 512, 64], dedup=True, clouds_in_wg=3))
    out.append(make("boundaries_off_by_one", [63, 65, 127, 257, 255, 193], mixed_wave=True, dedup=True))
    return out


# ---- rings ----------------------------------------------------------------------------------------------------------------------------
RING_VALUES = (0.0, 254.0, 255.0, 300.0, -1.0, 3.7)
RING_BYTES = (0, 254, 255, 255, 255, 3)


def ring_cases():
    r = _rng("rings")
    p = path_points(r, 180)
    p[:, 3] = np.array(RING_VALUES, F)[np.arange(180) % 6]
    return [Case("rings_packed", p, [0, 100, 180], 2.1, PACK_RING, path="fused", rings=sorted(set(RING_BYTES))),
            Case("rings_not_packed", p, [0, 100, 180], 2.1, 0, path="fused")]


# ---- sequences on the one object ------------------------------------------------------------------------------------------------------
def sequences():
    """name -> list of cases run one after another on the process's index objects"""
    by = {c.name: c for c in all_cases()}
    r = _rng("seq")
    wide = Case("seq_wide_box", np.concatenate([_corners((-200, -200, -20), (400, 400, 40)), box_points(r, 2000, (-200, -200, -20), (400, 400, 40))]), [0, 2002], 1.05, SINGLE,
                path="single", grows=2)
    narrow = Case("seq_narrow_box", box_points(r, 500, (10, 10, 0), (3, 3, 3)), [0, 500], 1.05, SINGLE, path="single")
    wide_b = Case("seq_wide_batch", wide.pts, [0, 1000, 2002], 2.1, PACK_RING, path="fused")
    narrow_b = Case("seq_narrow_batch", narrow.pts, [0, 200, 500], 2.1, PACK_RING, path="fused")
    return {
        "large_then_small": [by["single_n32769"], by["single_n2"], by["single_n257"], by["batch_cloud8193"], by["batch_n1"], by["batch_n257"]],
        "wide_then_narrow": [wide, narrow, wide, wide_b, narrow_b, wide_b.folded(), narrow_b.folded()],
        "K_64_65_4096_2": [by["K64_cell2.1"], by["K65_cell2.1"], by["K4096_cell2.1"], by["K2_cell2.1"], by["K4096_cell1.05"].folded(), by["K2_cell1.05"].folded()],
        "fused_unfused_alternating": [by["K16_cell1.05"], by["K65_cell1.05"], by["K16_cell1.05"].folded(), by["K1025_cell1.05"].folded(), by["K64_cell2.1"], by["empty_most_K70"]],
        "all_empty_between": [by["empty_row"], by["empty_all_K3"], by["empty_row"].folded(), by["empty_all_K70"].folded(), by["empty_row"], by["empty_all_K1030"],
                              by["one_point_clouds_K300"]],
        "folded_unfolded_alternating": [by["single_n257"].folded(), by["single_n257"], by["single_negative"].folded(), by["single_signed_zeros"],
                                        by["boundaries_off_by_one"].folded(), by["boundaries_off_by_one"], by["short_clouds_K40"].folded(), by["short_clouds_K40"]],
    }


def fold_cases():
    """FOLD_BOUNDS over the size, boundary and empty-cloud cases"""
    return [c.folded() for c in size_cases() + empty_cases() + [k for K in KS for k in k_cases(K)]]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = size_cases() + pattern_cases() + geometry_cases() + growth_cases() + [c for K in KS for c in k_cases(K)] + empty_cases() + ring_cases()
        _ALL = _ALL + [c.folded() for c in _ALL if c.name in {f.name[:-5] for f in fold_cases()}]
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def group(prefixes, folded=None):
    return [c for c in all_cases() if c.name.startswith(tuple(prefixes)) and (folded is None or folded == bool(c.flags & FOLD))]
