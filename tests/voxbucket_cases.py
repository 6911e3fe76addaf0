"""Edge-shape cases for the bucketed voxel grid (csrc/voxbucket.hip through loamx_voxbucket_probe).

A case is plain data — points, contiguous segments, one pose per sweep (two segments), the two leaves, the probe's flags — plus
`claims`: what the generator built the case FOR.  facts() recomputes them from the model's result (tests/voxbucket_model.py) and
tests/test_voxbucket_cases_cpu.py holds every case to its claims: a generator cannot silently miss the edge it was written for.

Cases are built on demand and kept (get(name)): the largest hold a million points, and collecting the tests must not build them.

Claims (every case states `reasons`, the set of give-up reasons the device can raise for it — empty: the run succeeds):
  cnt            the exact per-bucket point counts                       buckets     the run's bucket count
  nbuckets       per segment                                             pos_bits    per segment
  counts         bucket sizes that must occur                            passes      the set of sort-pass counts over non-empty buckets
  collide        some workgroup of 256 consecutive positions touches two buckets equal mod 256 (the `direct` branch of k_vb_stack)
  straddle       the boundaries between two segments of at least two buckets each; straddle_inside: those inside a workgroup
  has_passes     pass counts that must occur
  runs           subset of {"start7", "end8", "span"}: a voxel run of more than one point starting at sorted element 8k + 7 of its
                 bucket, one ending at 8k, one longer than 16 elements (it spans several threads)
  one_voxel      a bucket that is one voxel of this many points         moved       the round trip moves some point to another voxel
  zero_sign      a mean that starts from the first point instead of 0 gives other words
  plan_bad       the segments k_vb_plan itself gives up                  dup         duplicate splitters inside a segment
Large shuffled segments overflow some bucket with real probability (k_vb_plan sees 512 evenly spaced positions), so large cases
plant the exact voxel-order quantiles at the sampled positions t * ns / 512 and shuffle the rest; "no bucket above VB_CAP" is then
part of `reasons == {}` and proved from the model.
"""
import functools

import numpy as np

import voxbucket_model as vm
import voxel_cases as vc

SRC_POINTERS = 1


class Case:
    def __init__(self, name, pts, seg_off, leaf_even=0.5, leaf_odd=None, poses=None, flags=0, **claims):
        self.name = name
        self.pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        self.n = len(self.pts)
        self.seg_off = np.asarray(seg_off, np.uint32)
        self.nseg = len(self.seg_off) - 1
        self.leaf_even = float(leaf_even)
        self.leaf_odd = float(leaf_even if leaf_odd is None else leaf_odd)
        nsweep = (self.nseg + 1) // 2
        self.poses = np.tile(vm.IDENTITY, (nsweep, 1)) if poses is None else np.ascontiguousarray(poses, np.float32).reshape(nsweep, 12)
        self.flags = int(flags)
        assert self.seg_off[0] == 0 and self.seg_off[-1] == self.n and np.all(np.diff(self.seg_off.astype(np.int64)) >= 0)
        assert "reasons" in claims, name
        self.claims = claims
        self._model = None

    def __repr__(self):
        return self.name

    def model(self):
        """the model's result, computed once and shared by every test that needs it (nobody writes to it)"""
        if self._model is None:
            self._model = vm.run(self.pts, self.seg_off, self.poses, self.leaf_even, self.leaf_odd)
        return self._model

    def voxel_case(self, pts):
        """the same segments and leaves over other points (the model's or the device's stack) as a voxel_cases.Case: what reference() takes"""
        return vc.Case(self.name, pts, self.nseg, self.leaf_even, self.leaf_odd, seg_off=self.seg_off, B=0, passthrough=[])


def facts(case, R):
    """what the claims are about, from the model's result"""
    f = dict(reasons=set(R.reasons), buckets=R.buckets, nbuckets=[int(v) for v in R.segs["nbuckets"]], pos_bits=[int(v) for v in R.segs["pos_bits"]],
             cnt=[int(v) for v in R.cnt], plan_bad=[int(s) for s in np.flatnonzero(R.plan_bad)])
    f["collide"] = len(vm.workgroup_collisions(R)) > 0
    off = case.seg_off.astype(np.int64)
    nbk = np.maximum(1, -(-np.diff(off) // vm.VB_T))
    live = np.flatnonzero(np.diff(off) > 0)
    pairs = [(a, b) for a, b in zip(live[:-1], live[1:]) if nbk[a] >= 2 and nbk[b] >= 2]
    f["straddle"] = [int(off[b]) for a, b in pairs]
    f["straddle_inside"] = [int(off[b]) for a, b in pairs if off[b] % 256]
    f["dup"] = any(len(np.unique(R.lo[b0 + 1:b0 + k])) < k - 1 for b0, k in zip(R.segs["bucket0"].astype(int), R.segs["nbuckets"].astype(int)) if k > 2)
    f["passes"] = {int(-(-b // 8)) for b in R.bucket_bits if b}
    raw, _ = vm.voxels(case.pts[:, :3], (np.float32(1.0) / np.array([case.leaf_even, case.leaf_odd], np.float32))[R.seg & 1])
    f["moved"] = bool(((raw != R.voxel).any(axis=1) & (R.bucket >= 0)).any())
    f["runs"], f["one_voxel"] = set(), []
    if not R.gave_up:
        b = np.searchsorted(R.bucket_start, R.run_start, side="right") - 1
        a = R.run_start - R.bucket_start[b]
        e = a + R.run_count
        if ((a % 8 == 7) & (R.run_count > 1)).any():
            f["runs"].add("start7")
        if ((e % 8 == 0) & (R.run_count > 1)).any():
            f["runs"].add("end8")
        if (R.run_count > 16).any():
            f["runs"].add("span")
        f["one_voxel"] = [int(c) for c, bb in zip(R.run_count, b) if c == R.cnt[bb]]
        other = vm.run(case.pts, case.seg_off, case.poses, case.leaf_even, case.leaf_odd, from_first=True)
        f["zero_sign"] = not np.array_equal(other.out.view(np.uint32), R.out.view(np.uint32))
    return f


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def _plant(rng, p, key):
    """reorder the points of one segment: the exact voxel-order quantiles go to the positions k_vb_plan samples, the rest is shuffled"""
    ns = len(p)
    t = np.arange(vm.VB_SAMPLE, dtype=np.int64)
    at = (t * ns) // vm.VB_SAMPLE
    pick = np.argsort(key, kind="stable")[at]
    out = np.empty_like(p)
    out[at] = p[pick]
    rest = np.ones(ns, bool)
    rest[pick] = False
    free = np.ones(ns, bool)
    free[at] = False
    out[free] = p[rng.permutation(np.flatnonzero(rest))]
    return out


def _keys(p, leaf):
    v, ok = vm.voxels(p[:, :3], np.full(len(p), np.float32(1.0) / np.float32(leaf), np.float32))
    assert ok.all()
    return vm.keys_u64(v)


def planted_segment(rng, ns, dims, leaf=0.5, origin=None):
    origin = tuple(-(d // 2) for d in dims) if origin is None else origin
    p = vc.box_points(rng, ns, dims, leaf, origin)
    return _plant(rng, p, _keys(p, leaf))


def planted_row(rng, buckets):
    """one segment along a row of voxels (leaf 1): buckets[k] lists the point counts of bucket k's voxels ([] = an empty bucket: a
    duplicate splitter).  The sampled positions get points chosen so that splitter k is the first voxel of bucket k (of the next
    non-empty one behind an empty bucket); the ranks between two splitters sit on a first voxel of at least 200 points.  A bucket of
    one point must be followed by an empty or a large one, and an empty one by a large one — asserted."""
    counts = [c for b in buckets for c in b]
    first = np.concatenate([[0], np.cumsum([len(b) for b in buckets])])[:-1]   # first voxel of every bucket
    nb, ns = len(buckets), int(sum(counts))
    assert nb == -(-ns // vm.VB_T) and nb >= 2 and buckets[0] and buckets[-1]
    big = lambda k: bool(buckets[k]) and buckets[k][0] >= 200
    nxt = lambda k: next(j for j in range(k, nb) if buckets[j])
    samp = np.zeros(vm.VB_SAMPLE, np.int64)
    for r in range(vm.VB_SAMPLE):
        k = max(j for j in range(nb) if (j * vm.VB_SAMPLE) // nb <= r)
        if r == (k * vm.VB_SAMPLE) // nb:
            samp[r] = first[nxt(k)]
        else:
            samp[r] = first[k] if big(k) else first[next(j for j in range(k + 1, nb) if big(j))]
    p = vc._row_of_runs(rng, counts)
    vox = np.floor(p[:, 0]).astype(np.int64)
    assert np.array_equal(np.bincount(vox, minlength=len(counts)), counts)
    need = np.bincount(samp, minlength=len(counts))
    assert np.all(need <= np.asarray(counts)) and np.all(np.diff(samp) >= 0)
    rank_in_voxel = np.zeros(ns, np.int64)
    order = np.argsort(vox, kind="stable")
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    rank_in_voxel[order] = np.arange(ns) - start[vox[order]]
    is_sample = rank_in_voxel < need[vox]
    at = (np.arange(vm.VB_SAMPLE, dtype=np.int64) * ns) // vm.VB_SAMPLE
    out = np.empty_like(p)
    free = np.ones(ns, bool)
    free[at] = False
    out[at] = p[rng.permutation(np.flatnonzero(is_sample))]
    out[free] = p[~is_sample]
    return out


def _poses(*six):
    return np.stack([vm.pose_words(*s) for s in six])


def _segments(rng, name, cnt, dims=(32, 16, 8), origin=(-16, -8, -4), leaf=0.5, **kw):
    """box points for given segment lengths, leaves 0.5 / 1.0 by parity"""
    cnt = np.asarray(cnt, np.int64)
    nseg, n = len(cnt), int(cnt.sum())
    seg = np.repeat(np.arange(nseg), cnt)
    p = vc._with_corners_in(rng, n, nseg, dims, leaf, origin, seg, int(np.argmax(cnt)), leaf_odd=2 * leaf)
    return Case(name, p, vc._off(cnt), leaf, 2 * leaf, **kw)


# ---- families ------------------------------------------------------------------------------------------------------------------

BUILDERS = {}


def _case(fn):
    BUILDERS[fn.__name__] = fn
    return fn


def _family(names):
    def deco(fn):
        for k in names:
            BUILDERS[f"{fn.__name__}_{k}"] = functools.partial(fn, k)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def get(name):
    c = BUILDERS[name]()
    c.name = name
    return c


SIZES = (1, 2, 511, 512, 513, 2047, 2048, 2049, 4096, 4097)


@_family(SIZES)
def ns(n):
    """one segment of n points: pos_bits at 1, 2, 2^k, 2^k + 1; one bucket up to 2048, then two, three"""
    rng = np.random.default_rng(2000 + n)
    dims = (16, 8, 8) if n >= 2 else (1, 1, 1)
    return Case("", vc.box_points(rng, n, dims, 0.5, (-8, -4, -4)), [0, n], reasons=set(), nbuckets=[max(1, -(-n // 2048))],
                pos_bits=[max(1, (n - 1).bit_length())])


LARGE = {131072: (64, (64, 64, 16)), 131073: (65, (64, 64, 16)), 524289: (257, (128, 64, 32)), 1048576: (512, (128, 128, 32))}


@_family(LARGE)
def large(n):
    """planted quantiles: 64 buckets search the LDS copy of the splitters, 65 global memory; 257 buckets in shuffled order meet in the
    slot table (buckets 0 and 256); 512 buckets are the most a segment may have, each one sample gap"""
    nb, dims = LARGE[n]
    rng = np.random.default_rng(n)
    claims = dict(reasons=set(), nbuckets=[nb], pos_bits=[(n - 1).bit_length()])
    if nb >= 257:
        claims["collide"] = True
    return Case("", planted_segment(rng, n, dims), [0, n], **claims)


@_case
def large_1048577():
    """513 buckets: reason 1 from the plan, which leaves the segment without buckets — so every point raises reason 0 in k_vb_stack"""
    p = get("large_1048576").pts
    return Case("", np.concatenate([p, p[:1]]), [0, len(p) + 1], reasons={0, 1}, plan_bad=[0], buckets=513)


@_case
def collide_alternating_empty():
    """one-point segments alternating with empty ones: point j goes to bucket 2 j, so 256 consecutive points touch buckets 0, 2, ...,
    510 — 0 and 256, 2 and 258, ... share an entry of the slot table"""
    rng = np.random.default_rng(31)
    nseg = 2048
    cnt = np.where(np.arange(nseg) % 2 == 0, 1, 0)
    p = vc.box_points(rng, int(cnt.sum()), (32, 16, 8), 0.5, (-16, -8, -4))
    return Case("", p, vc._off(cnt), 0.5, 1.0, reasons=set(), collide=True, buckets=nseg)


@_case
def straddle_inside_workgroup():
    """4200 + 4500 points, three buckets each: the workgroup of positions 4096 .. 4351 leads with segment 0 and holds 152 points of
    segment 1, which search global memory"""
    return _segments(np.random.default_rng(41), "", [4200, 4500], reasons=set(), straddle=[4200], straddle_inside=[4200], nbuckets=[3, 3])


@_case
def straddle_at_256():
    """the same with the boundary at 17 * 256: no workgroup holds both segments"""
    return _segments(np.random.default_rng(42), "", [4352, 4500], reasons=set(), straddle=[4352], straddle_inside=[], nbuckets=[3, 3])


BUCKET_COUNTS = [4096, 1, 0, 511, 4095, 512, 513, 4096, 3000, 1, 0, 3000, 3000, 3000, 3000, 3000]


@_case
def bucket_counts():
    """16 buckets of exactly 4096, 1, 0, 511, 4095, 512, 513, 4096 (ONE voxel: thread 0's run goes on through LDS to the end of the
    buffer), 3000, 1, 0, 3000 ...: wave_has, the sentinel behind the last element, the head byte behind the last thread, duplicate
    splitters"""
    rng = np.random.default_rng(51)
    fill = lambda c: [200] + vc._fill(c - 200) if c > 200 else ([c] if c else [])
    buckets = [fill(c) for c in BUCKET_COUNTS]
    buckets[7] = [4096]
    p = planted_row(rng, buckets)
    return Case("", p, [0, len(p)], 1.0, reasons=set(), cnt=BUCKET_COUNTS, counts={0, 1, 511, 512, 513, 4095, 4096}, one_voxel=4096, dup=True,
                runs={"span"})


@_case
def one_voxel_4096():
    """4096 points in one voxel: both splitters equal, bucket 0 empty, bucket 1 one run of 4096"""
    rng = np.random.default_rng(52)
    p = vc._row_of_runs(rng, [4096])
    return Case("", p, [0, 4096], 1.0, reasons=set(), cnt=[0, 4096], one_voxel=4096)


@_case
def one_voxel_4097():
    """one more: the last bucket receives 4097 points"""
    rng = np.random.default_rng(53)
    p = vc._row_of_runs(rng, [4097])
    return Case("", p, [0, 4097], 1.0, reasons={5}, cnt=[0, 0, 4097])


@_case
def run_edges():
    """one bucket; runs in sorted order: [0, 7), [7, 16) — starts on the last of thread 0's eight elements, ends at a multiple of 8 —
    [16, 24), [24, 25), [25, 55) over four threads, [55, 57), [57, 64), then threes and one run of 100"""
    rng = np.random.default_rng(54)
    counts = [7, 9, 8, 1, 30, 2, 7] + vc._fill(301) + [100] + vc._fill(500)
    p = vc._row_of_runs(rng, counts)
    return Case("", p, [0, len(p)], 1.0, reasons=set(), runs={"start7", "end8", "span"})


# passes: key_bits + pos_bits of a ONE-bucket segment is that of its box and its length; seven passes need 49 bits, i.e. more position
# bits than a one-bucket segment has (12) beside at most 31 key bits: see passes_7
PASSES = {1: (2, (1, 1, 1)), 2: (2000, (4, 4, 2)), 3: (2000, (32, 16, 16)), 4: (2000, (128, 128, 128)), 5: (2000, (1024, 1024, 512)),
          6: (2000, (2**11, 2**10, 2**10 - 1))}


@_family(PASSES)
def passes(k):
    n, dims = PASSES[k]
    rng = np.random.default_rng(60 + k)
    origin = tuple(-(d // 2) for d in dims)
    return Case("", vc.box_points(rng, n, dims, 0.5, origin), [0, n], reasons=set(), passes={k})


@_case
def passes_7():
    """131073 points (18 position bits, 65 buckets) in a box of 2^15 x 2^14 x 3 voxels (31 key bits, still filtered by PCL): layers
    0 and 2 hold the points, layer 1 only two, in its extreme corners.  The bucket whose key range runs from the end of layer 0
    into layer 2 has the whole box as its own: 49 bits, seven passes.  No other bucket can: the buckets of one segment share its
    at most INT_MAX voxels"""
    rng = np.random.default_rng(67)
    n, leaf = 131073, 0.5
    half = (n - 2) // 2
    lo = vc.box_points(rng, half, (2**15, 2**14, 1), leaf, (-2**14, -2**13, 0))
    hi = vc.box_points(rng, n - 2 - half, (2**15, 2**14, 1), leaf, (-2**14, -2**13, 2))
    mid = vc.box_points(rng, 2, (2**15, 2**14, 1), leaf, (-2**14, -2**13, 1))
    p = np.concatenate([lo, mid, hi])
    return Case("", _plant(rng, p, _keys(p, leaf)), [0, n], leaf, reasons=set(), has_passes={7}, nbuckets=[65])


NSEG = (1, 2, 3, 511, 512, 513, 4096)


@_family(NSEG)
def nseg(k):
    """k ragged segments with empty ones among them, both leaves, a pose per sweep; the source-pointer table where k is odd"""
    rng = np.random.default_rng(700 + k)
    n = 2000 if k <= 3 else 6000 if k < 4096 else 9000
    empty = vc._empties(k) if k >= 4 else ()
    cnt = vc._lengths(rng, n, k, empty)
    ang = rng.uniform(-0.05, 0.05, ((k + 1) // 2, 3))
    tr = rng.uniform(-3, 3, ((k + 1) // 2, 3))
    return _segments(rng, "", cnt, poses=_poses(*np.concatenate([ang, tr], axis=1)), flags=SRC_POINTERS if k & 1 else 0, reasons=set(), buckets=k)


@_case
def empties_lead_mid_trail():
    return _segments(np.random.default_rng(71), "", [0, 0, 1500, 0, 2500, 0, 0, 1200, 0], reasons=set(), nbuckets=[1, 1, 1, 1, 2, 1, 1, 1, 1])


@_case
def all_empty_but_one():
    cnt = np.zeros(64, np.int64)
    cnt[37] = 3000
    return _segments(np.random.default_rng(72), "", cnt, reasons=set(), buckets=65)


@_case
def ragged():
    return _segments(np.random.default_rng(73), "", [0, 5000, 1, 0, 0, 2049, 7, 0, 300, 0], flags=SRC_POINTERS, reasons=set(),
                     nbuckets=[1, 3, 1, 1, 1, 2, 1, 1, 1, 1])


@_case
def ragged_concatenated():
    c = get("ragged")
    return Case("", c.pts, c.seg_off, c.leaf_even, c.leaf_odd, reasons=set(), nbuckets=c.claims["nbuckets"])


def _faces(seed, poses=None, **claims):
    rng = np.random.default_rng(seed)
    off = np.array([0, 1300, 2700, 2700, 4000], np.uint32)
    q = np.concatenate([vc._face_points(rng, 1300, 0.2), vc._face_points(rng, 1400, 0.4), vc._face_points(rng, 1300, 0.2)])
    return Case("", q, off, 0.2, 0.4, poses=poses, reasons=set(), **claims)


@_case
def faces_identity():
    """points on voxel faces, negative coordinates, zeros of both signs; the identity pose keeps every voxel"""
    return _faces(81, moved=False)


@_case
def faces_small_rotation():
    return _faces(82, poses=_poses((0.01, -0.02, 0.03, 0.5, -0.25, 1.0), (-0.02, 0.015, 0.01, -1.0, 2.0, 0.5)), moved=True)


@_case
def faces_large_translation():
    """x + t - t with t in the thousands rounds at 1e-4: points that sat on a face cross it"""
    return _faces(83, poses=_poses((0, 0, 0, 3000.0, -2000.0, 1500.0), (0, 0, 0, -2500.0, 1000.0, 3500.0)), moved=True)


@_case
def zero_sign():
    """single-point voxels whose intensity is -0.0: pcl::VoxelGrid's accumulators start at 0, and 0 + -0.0 is +0.0"""
    rng = np.random.default_rng(84)
    p = vc.box_points(rng, 600, (16, 8, 8), 0.5, (-8, -4, -4), per_voxel=1)
    p[::3, 3] = np.float32(-0.0)
    p[1::7, 0] = np.float32(-0.0)
    return Case("", p, [0, 600], 0.5, reasons=set(), zero_sign=True)


def _edge(x_voxel):
    """a one-bucket segment (nothing is sampled: k_vb_stack judges every point) with one point in voxel x_voxel, leaf 0.5"""
    rng = np.random.default_rng(90)
    p = vc.box_points(rng, 500, (16, 8, 8), 0.5, (0, -4, -4) if x_voxel > 0 else (-16, -4, -4))
    p[250, 0] = np.float32((x_voxel + 0.5) * 0.5)
    return p


@_family(("plus", "minus"))
def edge_accepted(sign):
    """+-(2^20 - 1) voxels: the last coordinate the key holds"""
    v = (2**20 - 1) * (1 if sign == "plus" else -1)
    return Case("", _edge(v), [0, 500], 0.5, reasons=set(), passes={5})


@_family(("plus", "minus"))
def edge_refused(sign):
    v = 2**20 * (1 if sign == "plus" else -1)
    return Case("", _edge(v), [0, 500], 0.5, reasons={0}, plan_bad=[])


@_family(("nan_sampled", "nan_unsampled", "inf_sampled", "inf_unsampled"))
def bad(kind):
    """three buckets, so the plan samples positions t * 5000 / 512: position 0 is sampled (the plan gives the segment up), 1 is not
    (k_vb_stack meets it)"""
    rng = np.random.default_rng(91)
    p = vc.box_points(rng, 5000, (16, 8, 8), 0.5, (-8, -4, -4))
    at = 0 if kind.endswith("_sampled") else 1
    p[at, 1] = np.nan if kind.startswith("nan") else -np.inf
    return Case("", p, [0, 5000], 0.5, reasons={0}, plan_bad=[0] if at == 0 else [])


def _through(rng, n):
    return vc.box_points(rng, n, (2**11, 2**10, 2**10), 0.5, (-1024, -512, -512))


@_case
def pass_through_single():
    """2^31 voxels, every extent below 2^21: PCL copies the cloud through, the last bucket raises reason 2"""
    return Case("", _through(np.random.default_rng(95), 1500), [0, 1500], 0.5, reasons={2})


@_family(("last", "earlier"))
def pass_through(where):
    rng = np.random.default_rng(96)
    small = lambda n: vc.box_points(rng, n, (16, 8, 8), 0.5, (-8, -4, -4))
    parts = [small(2100), small(2400), _through(rng, 1500)] if where == "last" else [small(2100), _through(rng, 1500), small(2400)]
    return Case("", np.concatenate(parts), vc._off([len(q) for q in parts]), 0.5, reasons={2})


@_case
def pass_through_and_sort_bits():
    """a box of 2^20 voxels along every axis: 60 key bits + 11 position bits (reason 3) in a segment PCL passes through (reason 2);
    reason 3 cannot occur alone, a segment of at most INT_MAX voxels has at most 31 key bits"""
    rng = np.random.default_rng(97)
    return Case("", vc.box_points(rng, 1500, (2**20, 2**20, 2**20), 0.5, (-2**19, -2**19, -2**19)), [0, 1500], 0.5, reasons={2, 3})


REUSE = ("large_131073", "ns_513", "one_voxel_4097", "ns_513", "nseg_513", "large_131073")


def reuse_sequence():
    """on the process's one object: large, small, a give-up, the same small again, another segment count, the large again"""
    return [get(k) for k in REUSE]


def shuffled_overflows(n, seeds):
    """of the seeds, how many give a uniformly shuffled segment of n points (the box and density of large_<n>, nothing planted) in
    which some bucket receives more than VB_CAP points — a count from the model, recorded in CHANGELOG.md"""
    over = 0
    for seed in seeds:
        rng = np.random.default_rng(seed)
        dims = LARGE[n][1]
        p = vc.box_points(rng, n, dims, 0.5, tuple(-(d // 2) for d in dims))
        over += 5 in vm.run(p, [0, n], vm.IDENTITY, 0.5, 0.5).reasons
    return over


NAMES = sorted(BUILDERS)
