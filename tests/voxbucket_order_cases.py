"""Edge-shape cases for the ORDER the bucketed voxel grid works in (csrc/voxbucket.hip): k_vb_stack leaves one 16-bit bucket word per
point and a bucket range per chunk of 256 points, and every bucket of k_vb_reduce collects its own points from them in input order,
sorts on the voxel bits alone and lets the stable sort keep the input order inside a voxel.  The cases are the smallest shapes at
which that can go wrong; they are built from the blocks of tests/voxbucket_cases.py and carry `claims` as the cases there do.

Claims beyond those of voxbucket_cases.facts():
  key_bits        the set of voxel-index widths over the non-empty buckets (the sort's pass count is ceil(key_bits / 8))
  alternate       consecutive points of the segment never share a bucket
  bucket_chunks   {bucket: the chunks (global index // 256) that hold its points}; bucket_chunks_of: the same for the buckets named
  range_without   {bucket: chunks whose bucket range [min, max] contains the bucket although they hold none of its points}
  seg_mod         the inner segment boundaries modulo 256
  shared_words    every chunk that two segments share holds, from both, points with the same bucket-inside-segment word
  order_matters   the means change when every segment's points are summed in reverse input order
  special_mean_w  the intensity mean of the one voxel at x >= 20 (sum_order)
  special_spread  (chunks, 64-point groups) the points of that voxel are spread over
  voxels_of       {bucket: (voxels, points per voxel)} for a bucket of equal voxels
"""
import functools

import numpy as np

import voxbucket_cases as bc
import voxbucket_model as vm
import voxel_cases as vc
from voxbucket_cases import Case, planted_row, _segments

CHUNK, GROUP = 256, 64


def facts(case, R):
    f = bc.facts(case, R)
    off = case.seg_off.astype(np.int64)
    seg = np.repeat(np.arange(case.nseg), np.diff(off))
    bucket = R.bucket
    chunk = np.arange(case.n) // CHUNK
    f["seg_mod"] = [int(o) % CHUNK for o in off[1:-1]]
    f["alternate"] = bool(np.all(bucket[1:] != bucket[:-1]))
    f["bucket_chunks"] = {int(b): sorted(int(c) for c in np.unique(chunk[bucket == b])) for b in np.unique(bucket[bucket >= 0])}
    rng_of = {}
    for c in np.unique(chunk):
        bb = bucket[(chunk == c) & (bucket >= 0)]
        if len(bb):
            rng_of[int(c)] = (int(bb.min()), int(bb.max()), set(int(v) for v in bb))
    f["bucket_chunks_of"] = {k: f["bucket_chunks"].get(k) for k in case.claims.get("bucket_chunks_of", {})}
    f["range_without"] = {}
    for c, (lo, hi, have) in rng_of.items():
        for b in range(lo, hi + 1):
            if b not in have:
                f["range_without"].setdefault(b, []).append(c)
    rel = bucket - R.segs["bucket0"].astype(np.int64)[seg]
    shared = []
    for o in off[1:-1]:
        c = int(o) // CHUNK
        if o % CHUNK and 0 < o < case.n:
            m = chunk == c
            a, b = set(rel[m & (np.arange(case.n) < o) & (bucket >= 0)]), set(rel[m & (np.arange(case.n) >= o) & (bucket >= 0)])
            shared.append(bool(a & b))
    f["shared_words"] = bool(shared) and all(shared)
    if not R.gave_up:
        bseg = np.repeat(np.arange(case.nseg), np.maximum(1, -(-np.diff(off) // vm.VB_T)))
        f["key_bits"] = {int(bits - R.segs["pos_bits"][bseg[b]]) for b, bits in enumerate(R.bucket_bits) if bits}
        rev = np.concatenate([np.arange(off[s], off[s + 1])[::-1] for s in range(case.nseg)]) if case.n else np.zeros(0, np.int64)
        if int(np.maximum(1, -(-np.diff(off) // vm.VB_T)).max()) == 1:   # (no splitter: the plan does not depend on the order)
            other = vm.run(case.pts[rev], case.seg_off, case.poses, case.leaf_even, case.leaf_odd)
            f["order_matters"] = not np.array_equal(other.out.view(np.uint32), R.out.view(np.uint32))
        far = np.flatnonzero(R.out[:, 0] >= 20.0)
        if len(far) == 1:
            f["special_mean_w"] = float(R.out[far[0], 3])
            at = np.flatnonzero(case.pts[:, 0] >= 20.0)
            f["special_spread"] = (len(set(at // CHUNK)), len(set(at // GROUP)))
        b_of_run = np.searchsorted(R.bucket_start, R.run_start, side="right") - 1
        f["voxels_of"] = {}
        for b in np.unique(b_of_run):
            cnts = R.run_count[b_of_run == b]
            if len(set(cnts)) == 1:
                f["voxels_of"][int(b)] = (len(cnts), int(cnts[0]))
    return f


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


def _classed_row(rng, cls, width=40):
    """one segment along a row of voxels (leaf 1) whose point at position i belongs to class cls[i]: class k owns the voxels
    [100 k, 100 k + width).  Every position k_vb_plan samples holds a point of its class's FIRST voxel, so the sorted sample is one
    block of equal keys per class: where block k contains rank k * 512 / classes, the buckets are the classes.  Several points to a
    voxel, intensities of mixed magnitudes: the means depend on the order of the sums."""
    cls = np.asarray(cls, np.int64)
    ns = len(cls)
    at = (np.arange(vm.VB_SAMPLE, dtype=np.int64) * ns) // vm.VB_SAMPLE
    vox = 100 * cls + rng.integers(0, width, ns)
    vox[at] = 100 * cls[at]
    p = np.empty((ns, 4), np.float32)
    p[:, 0] = vox + rng.uniform(0.25, 0.75, ns)
    p[:, 1:3] = rng.uniform(0.25, 0.75, (ns, 2))
    p[:, 3] = vc._intensity(rng, ns)
    return p


@_case
def sum_order():
    """1000 points, one bucket, four chunks.  One voxel (x = 20.25, far from the rest) holds four points with intensities 1e8, 1, -1e8,
    0.5 at positions 10, 300, 600 and 990: four chunks, four 64-point groups, and — 1000 elements give every wave 128 ranks — the waves
    0, 2, 4 and 7.  In input order the float32 sum is ((1e8 + 1) - 1e8) + 0.5 = 0.5, the mean 0.125; any other order gives another."""
    rng = np.random.default_rng(101)
    p = vc.box_points(rng, 1000, (16, 8, 8), 0.5, (-8, -4, -4))
    at = [10, 300, 600, 990]
    p[at, 0] = np.float32(20.25)
    p[at, 1] = p[at, 2] = np.float32(0.25)
    p[at, 3] = np.array([1e8, 1.0, -1e8, 0.5], np.float32)
    return Case("", p, [0, 1000], 0.5, reasons=set(), nbuckets=[1], order_matters=True, special_mean_w=0.125, special_spread=(4, 4))


@_case
def interleaved():
    """4096 points, two buckets, alternating point by point: the odd positions hold the low voxels (bucket 0), the even ones — all the
    plan samples — the high ones (bucket 1: every sampled point sits in the first high voxel, which is therefore the splitter).  Every
    chunk matches both buckets and the compaction takes every other word."""
    rng = np.random.default_rng(102)
    cls = 1 - (np.arange(4096) & 1)
    return Case("", _classed_row(rng, cls), [0, 4096], 1.0, reasons=set(), cnt=[2048, 2048], alternate=True,
                bucket_chunks={0: list(range(16)), 1: list(range(16))})


def _sparse_classes():
    """17 chunks, three classes: chunk 0 low and mid, 1-5 low, 6 low and high (its range holds the mid bucket, it holds no mid point),
    7-15 high, 16 mid and high.  Sampled positions: mid in chunks 0 and 16, high in chunk 6."""
    ns = 17 * CHUNK
    i = np.arange(ns)
    c = i // CHUNK
    cls = np.where(c <= 5, 0, 2)
    at = np.zeros(ns, bool)
    at[(np.arange(vm.VB_SAMPLE, dtype=np.int64) * ns) // vm.VB_SAMPLE] = True
    cls = np.where((c == 0) & ((i & 1) == 1), 0, cls)
    cls = np.where((c == 0) & (((i & 1) == 0) | at), 1, cls)
    cls = np.where((c == 6) & ((i & 1) == 1) & ~at, 0, cls)
    cls = np.where((c == 16) & (((i & 1) == 0) | at), 1, cls)
    return cls


@_case
def sparse_chunks():
    """the mid bucket's points sit in the first and the last chunk only; the chunks between touch the other buckets — eight of them one
    bucket alone (the summary skip) — and chunk 6 touches buckets 0 and 2: its range contains bucket 1, it holds none of its points"""
    rng = np.random.default_rng(103)
    cls = _sparse_classes()
    cnt = [int(v) for v in np.bincount(cls, minlength=3)]
    return Case("", _classed_row(rng, cls), [0, len(cls)], 1.0, reasons=set(), cnt=cnt, nbuckets=[3],
                bucket_chunks={0: list(range(7)), 1: [0, 16], 2: list(range(6, 17))}, range_without={1: [6]})


@_case
def sparse_large():
    """40960 points, 20 buckets, each one a stretch of about eight consecutive chunks: a segment of more than 32 Ki points is scanned
    in two rounds and looks at the chunk ranges first, so every bucket leaves out nine tenths of the chunks.  The stretches begin at
    sampled positions (every 80th), where splitter k = rank k * 512 / 20 of the sample falls."""
    rng = np.random.default_rng(105)
    ns, nb = 40960, 20
    t = np.arange(ns) // (ns // vm.VB_SAMPLE)
    cls = np.searchsorted((np.arange(1, nb) * vm.VB_SAMPLE) // nb, t, side="right")
    cnt = [int(v) for v in np.bincount(cls, minlength=nb)]
    chunks = {k: sorted(set(int(c) for c in np.flatnonzero(cls == k) // CHUNK)) for k in (0, 7, 19)}
    assert all(len(v) <= 10 for v in chunks.values())
    return Case("", _classed_row(rng, cls), [0, ns], 1.0, reasons=set(), cnt=cnt, nbuckets=[nb], bucket_chunks_of=chunks)


@_case
def chunk_edges():
    """three segments of three buckets each; the middle one starts at 4607 = 255 (mod 256) and ends at 8961 = 1 (mod 256): one point in
    its first chunk, one in its last, among its neighbours' points with the same words"""
    return _segments(np.random.default_rng(104), "", [4607, 4354, 4500], reasons=set(), nbuckets=[3, 3, 3], seg_mod=[255, 1], shared_words=True)


KEY_BITS = {8: (8, 8, 4), 9: (8, 8, 5), 16: (64, 32, 32), 17: (64, 32, 33), 24: (256, 256, 256), 25: (256, 256, 257)}


@_family(KEY_BITS)
def key_bits(k):
    """one bucket of 2000 points whose box needs exactly k voxel bits: the sort takes ceil(k / 8) passes, whatever the position bits"""
    dims = KEY_BITS[k]
    rng = np.random.default_rng(110 + k)
    return Case("", vc.box_points(rng, 2000, dims, 0.5, tuple(-(d // 2) for d in dims)), [0, 2000], reasons=set(), key_bits={k}, pos_bits=[11])


_fill = lambda c, first=200: [first] + vc._fill(c - first) if c > first else ([c] if c else [])


@_case
def exactly_full():
    """a bucket of exactly 4096 points in 1024 voxels of four, between two buckets of 1024: every rank is taken, 1024 run heads"""
    rng = np.random.default_rng(121)
    p = planted_row(rng, [_fill(1024), [4] * 1024, _fill(1024, 600)])
    return Case("", p, [0, len(p)], 1.0, reasons=set(), cnt=[1024, 4096, 1024], voxels_of={1: (1024, 4)})


@_case
def share_edges():
    """buckets of 513 points (every wave's share becomes 128 ranks: four waves full, one rank in the fifth, three idle), of one point and
    of none"""
    rng = np.random.default_rng(122)
    counts = [513, 1, 0, 4000, 4000]
    p = planted_row(rng, [_fill(c, 600 if c == 4000 else 200) for c in counts])
    return Case("", p, [0, len(p)], 1.0, reasons=set(), cnt=counts, dup=True)


@_case
def refused_between():
    """a point that is not finite between two accepted points of one voxel: its bucket word is the refusal marker, the run gives up
    with reason 0, and the stack is the model's at every finite point"""
    rng = np.random.default_rng(123)
    p = vc.box_points(rng, 500, (16, 8, 8), 0.5, (-8, -4, -4))
    p[249, :3] = p[251, :3] = np.array([1.3, 0.3, 0.3], np.float32)
    p[250, :3] = np.array([1.3, np.nan, 0.3], np.float32)
    return Case("", p, [0, 500], 0.5, reasons={0}, plan_bad=[])


NAMES = sorted(BUILDERS)
