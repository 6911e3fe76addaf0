"""Executable specification of the bucketed voxel grid (loam_velodyne_amd/csrc/voxbucket.hip) in NumPy: what k_vb_plan, k_vb_stack and
k_vb_reduce are DESIGNED to compute, word for word, from the same inputs loamx_voxbucket_probe takes.

Two layers.  The single-segment functions (plan_splitters, bucketed_voxel_grid, GiveUp) state the algorithm in plain Python integers
and are what tests/test_voxbucket_model.py pins against the oracle.  run() is the whole stage in vectorised form — many segments, the
leaf by parity, bucket0 per segment with empty segments owning one bucket, the pose round trip in float32 with one rounding per
operation, the plan words (lo, VbSeg, cnt), the keys as uint64 through searchsorted, and the SET of give-up reasons the device can
raise for the input — so that a million points take about a second.

Give-up reasons, as the kernels raise them:
  1  k_vb_plan: a segment of more than VB_SAMPLE buckets.  The plan then leaves the segment without buckets, and every one of its points
     raises reason 0 in k_vb_stack ("its points raise the fail word again, harmlessly"): such an input carries {0, 1}.
  0  k_vb_plan: a SAMPLED raw point whose voxel is beyond +-2^20 or not finite (the segment is left without buckets, as above);
     k_vb_stack: any round-trip point with such a voxel.
  5  k_vb_stack: a bucket that receives more than VB_CAP points.
  2, 3  k_vb_reduce, and only when the run reaches it alive (every workgroup of it leaves at once when the fail word is already up):
     3 a bucket whose own box needs more than 63 sort bits — raised by that bucket's workgroup while others run; 2 a segment box of
     more than INT_MAX voxels — raised by the last bucket, unless it started after another bucket's reason 3.  So where both are in
     the set, the device reports a non-empty subset.
"""
import numpy as np

VB_CAP, VB_T, VB_SAMPLE, VB_OFF, VB_MAXSEG = 4096, 2048, 512, 1 << 20, 4096
INT_MAX = 2**31 - 1
SEG_DTYPE = np.dtype([("bucket0", "<u4"), ("nbuckets", "<u4"), ("pos_bits", "<u4"), ("pad", "<u4")])


class GiveUp(Exception):
    def __init__(self, reason):
        super().__init__(f"give-up reason {reason}")
        self.reason = reason


def _bits(v):
    return int(v).bit_length()


def _voxels(pts, leaf):
    """floor(v * inverse leaf) in float arithmetic, as pcl::VoxelGrid and vb_voxel() form it; reason 0 beyond +-2^20 or not finite"""
    inv = np.float32(1.0) / np.float32(leaf)
    f = np.floor(pts[:, :3] * inv)
    if not np.all(np.abs(f) < np.float32(VB_OFF)):   # (also catches NaN / inf)
        raise GiveUp(0)
    return f.astype(np.int64)


def _key(v):
    """vb_key(): (iz, iy, ix) lexicographically, 21 bits each"""
    return [((int(z) + VB_OFF) << 42) | ((int(y) + VB_OFF) << 21) | (int(x) + VB_OFF) for x, y, z in v]


def plan_splitters(pts, leaf):
    """k_vb_plan: ceil(n / VB_T) buckets; VB_SAMPLE evenly spaced points ranked by voxel key, every (m / buckets)-th one a splitter"""
    n = len(pts)
    nb = max(1, -(-n // VB_T))
    if nb > VB_SAMPLE:
        raise GiveUp(1)
    if nb == 1:
        return [0]
    m = min(n, VB_SAMPLE)
    sample = pts[[(t * n) // m for t in range(m)]]
    keys = sorted(_key(_voxels(sample, leaf)))
    return [0] + [keys[(k * m) // nb] for k in range(1, nb)]


def bucketed_voxel_grid(pts, leaf, splitters=None, rng=None):
    """one segment through k_vb_plan / k_vb_stack / k_vb_reduce; rng: shuffles the arrival order inside every bucket"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    if n == 0:
        return np.zeros((0, 4), np.float32)
    lo = plan_splitters(pts, leaf) if splitters is None else list(splitters)
    assert lo[0] == 0 and all(a <= b for a, b in zip(lo, lo[1:]))
    v = _voxels(pts, leaf)                                   # k_vb_stack: exact voxel of every point (reason 0)
    keys = _key(v)
    lo_arr = np.array(lo, dtype=object)
    # bucket = the last splitter <= key (the binary search of k_vb_stack: "if (s[mid] <= key) lo = mid; else hi = mid")
    bucket = np.array([int(np.searchsorted(lo_arr, k, side="right")) - 1 for k in keys])
    pos_bits = max(1, _bits(n - 1))
    # PCL's own pass-through test on the segment's box (the last bucket does it on the device, reason 2)
    dims = v.max(0) - v.min(0) + 1
    if int(dims[0]) * int(dims[1]) * int(dims[2]) > 2147483647:
        raise GiveUp(2)
    out = []
    for b in range(len(lo)):
        el = np.flatnonzero(bucket == b)                     # input positions, in arrival order (any)
        if len(el) > VB_CAP:
            raise GiveUp(5)
        if rng is not None:
            el = rng.permutation(el)
        if not len(el):
            continue
        vb = v[el]
        b0 = vb.min(0)
        dx, dy, dz = (int(d) for d in (vb.max(0) - b0 + 1))
        key_bits = _bits(dx * dy * dz - 1)
        if max(key_bits, 1) + pos_bits > 63:
            raise GiveUp(3)
        lin = [(int(x) - int(b0[0])) + dx * ((int(y) - int(b0[1])) + dy * (int(z) - int(b0[2]))) for x, y, z in vb]
        words = sorted((l << pos_bits) | int(p) for l, p in zip(lin, el))   # the LSD radix sort's result: ascending words, all distinct
        s = 0
        while s < len(words):                                # run heads -> one mean per voxel, summed in sorted = input order
            e, acc = s, np.zeros(4, np.float32)
            while e < len(words) and words[e] >> pos_bits == words[s] >> pos_bits:
                acc = (acc + pts[words[e] & ((1 << pos_bits) - 1)]).astype(np.float32)
                e += 1
            out.append(acc / np.float32(e - s))
            s = e
    return np.array(out, np.float32).reshape(-1, 4)


# ---- the whole stage, vectorised ------------------------------------------------------------------------------------------------

def pose_words(rx, ry, rz, tx, ty, tz):
    """the 12 words of one Pose: the angles and translation in float32, sine / cosine rounded from double as pose_set_angles() does"""
    a = np.array([rx, ry, rz], np.float32)
    sc = np.stack([np.sin(a.astype(np.float64)), np.cos(a.astype(np.float64))], axis=1).astype(np.float32)
    return np.concatenate([a, np.array([tx, ty, tz], np.float32), sc.reshape(-1)]).astype(np.float32)


IDENTITY = pose_words(0, 0, 0, 0, 0, 0)


def _rot(a, b, c, s):
    """rot_z(x, y) / rot_x(y, z): a' = c a - s b, b' = s a + c b — float32, every product and sum rounded on its own"""
    return c * a - s * b, s * a + c * b


def _rot_y(x, z, c, s):
    return c * x + s * z, c * z - s * x


def round_trip(pts, poses12_per_point):
    """to_map then to_be_mapped (dev_math.hpp) on float32 columns, from the 12 pose words of every point's sweep"""
    T = np.ascontiguousarray(poses12_per_point, np.float32)
    tx, ty, tz = T[:, 3], T[:, 4], T[:, 5]
    srx, crx, sry, cry, srz, crz = (T[:, k] for k in range(6, 12))
    x, y, z = (np.ascontiguousarray(pts[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        x, y = _rot(x, y, crz, srz)
        y, z = _rot(y, z, crx, srx)
        x, z = _rot_y(x, z, cry, sry)
        x, y, z = x + tx, y + ty, z + tz
        x, y, z = x - tx, y - ty, z - tz
        x, z = _rot_y(x, z, cry, -sry)
        y, z = _rot(y, z, crx, -srx)
        x, y = _rot(x, y, crz, -srz)
    out = np.empty((len(pts), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x, y, z, pts[:, 3]
    return out


def voxels(xyz, inv):
    """vb_voxel() on three columns: (int64 voxel, ok); ok is False beyond +-2^20 voxels and for NaN / inf"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(xyz, np.float32) * np.asarray(inv, np.float32)[:, None])
        ok = np.all(np.abs(f) < np.float32(VB_OFF), axis=1)
    return np.where(ok[:, None], f, 0).astype(np.int64), ok


def keys_u64(v):
    """vb_key() on int64 voxel rows -> uint64"""
    v = (v + VB_OFF).astype(np.uint64)
    return (v[:, 2] << np.uint64(42)) | (v[:, 1] << np.uint64(21)) | v[:, 0]


def _sequential_means(rows, starts, counts, from_first=False):
    """per run [starts[k], starts[k] + counts[k]) of rows: the float32 sum accumulated from 0 in row order, divided by the count
    (from_first: the sum starts from the run's first row instead — the variant a case about the sign of zero must tell apart)"""
    nrun = len(starts)
    order = np.argsort(-counts, kind="stable")
    st, cn = starts[order], counts[order]
    acc = np.zeros((nrun, 4), np.float32)
    j0 = 0
    if from_first and nrun:
        acc[:] = rows[st]
        j0 = 1
    for j in range(j0, int(cn[0]) if nrun else 0):
        live = int(np.searchsorted(-cn, -j, side="left"))   # runs longer than j: a prefix
        acc[:live] += rows[st[:live] + j]
    res = np.empty_like(acc)
    res[order] = acc / cn.astype(np.float32)[:, None]
    return res


class Result:
    """what one run leaves: stack, lo / segs / cnt (the plan), buckets, reasons (set), gave_up; out / out_off when it did not give up;
    bucket (per point, -1 where the point raised reason 0), bucket_bits (key_bits + pos_bits per non-empty bucket, else 0), voxel / seg
    (per point), plan_bad (per segment: the plan gave it up), run_start / run_count / bucket_start (sorted order, when it did not give up)"""


def run(pts, seg_off, poses12, leaf_even, leaf_odd, arrival=None, from_first=False):
    """arrival: a permutation of the points — the order in which they reach their buckets' slot arrays (the device's atomics decide
    it; the result must not depend on it)"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
    off = np.asarray(seg_off, np.int64)
    n, nseg = len(pts), len(off) - 1
    assert 1 <= nseg <= VB_MAXSEG and 1 <= n < (1 << 24) and off[0] == 0 and off[-1] == n and np.all(np.diff(off) >= 0)
    poses = np.asarray(poses12, np.float32).reshape(-1, 12)
    assert len(poses) == (nseg + 1) // 2
    R = Result()
    R.reasons = set()
    ns = np.diff(off)
    seg = np.repeat(np.arange(nseg), ns)
    inv2 = (np.float32(1.0) / np.array([leaf_even, leaf_odd], np.float32)).astype(np.float32)
    inv = inv2[seg & 1]
    # ---- k_vb_plan
    nbk = np.maximum(1, -(-ns // VB_T))
    bucket0 = np.concatenate([[0], np.cumsum(nbk)[:-1]])
    R.buckets = nb = int(nbk.sum())
    R.segs = np.zeros(nseg, SEG_DTYPE)
    R.segs["bucket0"] = bucket0
    R.segs["pos_bits"] = [max(1, _bits(max(int(m) - 1, 0))) for m in ns]
    R.lo = np.zeros(nb, np.uint64)
    bad = np.zeros(nseg, bool)
    for s in np.flatnonzero(nbk > 1):
        m, k = int(ns[s]), int(nbk[s])
        if k > VB_SAMPLE:
            R.reasons.add(1)   # (the plan writes lo = 0 for the first VB_SAMPLE buckets and nothing for the others)
            bad[s] = True
            continue
        t = np.arange(VB_SAMPLE, dtype=np.int64)   # (m > VB_T: the sample is VB_SAMPLE points)
        sample = pts[off[s] + (t * m) // VB_SAMPLE, :3]
        v, ok = voxels(sample, np.full(VB_SAMPLE, inv2[s & 1], np.float32))
        if not ok.all():
            R.reasons.add(0)
            bad[s] = True
            continue
        sk = np.sort(keys_u64(v))
        R.lo[bucket0[s] + 1:bucket0[s] + k] = sk[(np.arange(1, k, dtype=np.int64) * VB_SAMPLE) // k]
    R.segs["nbuckets"] = np.where(bad, 0, nbk)
    R.plan_bad = bad
    # ---- k_vb_stack
    R.stack = round_trip(pts, poses[seg >> 1])
    v, ok = voxels(R.stack[:, :3], inv)
    act = ok & ~bad[seg]
    if not act.all():
        R.reasons.add(0)
    key = keys_u64(v)
    bucket = bucket0[seg].copy()
    for s in np.flatnonzero((nbk > 1) & ~bad):
        a, b = int(off[s]), int(off[s + 1])
        # the number of splitters of buckets 1 .. that are <= key: "if (splitter[mid] <= key) lo = mid; else hi = mid"
        bucket[a:b] += np.searchsorted(R.lo[bucket0[s] + 1:bucket0[s] + int(nbk[s])], key[a:b], side="right")
    R.bucket = np.where(act, bucket, -1)
    R.cnt = np.bincount(bucket[act], minlength=nb).astype(np.uint32)   # (every arrival counts, whether or not it finds a slot)
    if (R.cnt > VB_CAP).any():
        R.reasons.add(5)
    R.bucket_bits = np.zeros(nb, np.int64)
    R.voxel, R.seg = v, seg
    if R.reasons:   # k_vb_reduce leaves at once
        R.gave_up = True
        return R
    # ---- k_vb_reduce
    arrival = np.arange(n) if arrival is None else np.asarray(arrival)
    by_bucket = arrival[np.argsort(bucket[arrival], kind="stable")]   # every bucket's slot array, in arrival order
    bstart = np.concatenate([[0], np.cumsum(R.cnt.astype(np.int64))])
    pos = np.arange(n) - off[seg]
    sorted_pts = np.empty(n, np.int64)
    head = np.zeros(n, bool)
    bseg = np.repeat(np.arange(nseg), nbk)
    for b in np.flatnonzero(R.cnt):
        el = by_bucket[bstart[b]:bstart[b + 1]]
        vb = v[el]
        b0 = vb.min(0)
        dx, dy, dz = (int(d) for d in (vb.max(0) - b0 + 1))
        pbits = int(R.segs["pos_bits"][bseg[b]])
        kb = _bits(dx * dy * dz - 1)
        R.bucket_bits[b] = max(kb, 1) + pbits
        if R.bucket_bits[b] > 63:
            R.reasons.add(3)
            continue
        r = (vb - b0).astype(np.uint64)
        lin = r[:, 0] + np.uint64(dx) * (r[:, 1] + np.uint64(dy) * r[:, 2])
        w = np.sort((lin << np.uint64(pbits)) | pos[el].astype(np.uint64))   # the radix sort's result: ascending words, all distinct
        sorted_pts[bstart[b]:bstart[b + 1]] = off[bseg[b]] + (w & np.uint64((1 << pbits) - 1)).astype(np.int64)
        vox = w >> np.uint64(pbits)
        head[bstart[b]] = True
        head[bstart[b] + 1:bstart[b + 1]] = vox[1:] != vox[:-1]
    # PCL's pass-through test on every segment's box, by the last bucket
    live = np.flatnonzero(ns > 0)
    mn, mx = np.minimum.reduceat(v, off[live]), np.maximum.reduceat(v, off[live])
    for d in (mx - mn + 1):
        if int(d[0]) * int(d[1]) > INT_MAX or int(d[0]) * int(d[1]) * int(d[2]) > INT_MAX:
            R.reasons.add(2)
    if R.reasons:
        R.gave_up = True
        return R
    R.gave_up = False
    starts = np.flatnonzero(head)
    counts = np.diff(np.concatenate([starts, [n]]))
    R.run_start, R.run_count, R.bucket_start = starts, counts, bstart
    R.out = _sequential_means(R.stack[sorted_pts], starts, counts, from_first)
    R.out_off = np.concatenate([[0], np.cumsum(np.bincount(seg[sorted_pts[starts]], minlength=nseg))]).astype(np.uint32)
    return R


def workgroup_collisions(R, wg=256):
    """workgroups of k_vb_stack (wg consecutive positions) that touch two different buckets equal mod 256: the second one finds its
    entry of the slot table taken and goes to the global counter directly"""
    i = np.flatnonzero(R.bucket >= 0)
    pairs = np.unique(np.stack([i // wg, R.bucket[i]], axis=1), axis=0)
    slot = pairs[:, 0] * 256 + (pairs[:, 1] & 255)
    u, c = np.unique(slot, return_counts=True)
    return np.unique(u[c > 1] // 256)
