"""Model of the sweep re-projection (transformToEnd, BasicLaserOdometry.cpp:57-87, and transformToStart, :40-53) and of what
k_transform_to_end_batch does beside it: the ring-first table with its order stamp, and the folded cloud bounds.

to_end_f32 / to_start_f32 restate the kernel operation for operation in float32 (one rounding per operation, no fused
multiply-add: the library is built with -ffp-contract=off).  They are valid only when the transform's rotation is zero: the three
per-point sincosf calls then see +-0 and return (+-0, 1) exactly.  to_end_f64 / to_start_f64 start from the same float32 words, form
`s` as the kernel forms it, and do everything behind that in float64 with true sines and cosines of the per-point angles.

KAPPA is MEASURED, not chosen (tests/test_reproject_cases_cpu.py measures it again): the smallest factor, rounded up to two digits,
with which  KAPPA * 2^-24 * (|x| + |y| + |z| + |T.pos|_1 + |shift|_1)  covers the deviation of the ORACLE (oracle/oracle_odometry.hpp,
plain float arithmetic with the host's sinf / cosf) from the f64 model over all general-class cases.  The kernels get DEVICE_FACTOR
times that: the device's sincosf is good to 2 ulp against the host's 1, and three dependent per-point rotations carry it."""
import numpy as np

RF_N = 320
PARAMS = np.dtype([("T", "<f4", 6), ("sT", "<f4", 3), ("cT", "<f4", 3), ("shift", "<f4", 3), ("s_start", "<f4", 3),
                   ("c_start", "<f4", 3), ("s_end", "<f4", 3), ("c_end", "<f4", 3), ("scan_period", "<f4"), ("enabled", "<i4")])
KAPPA = 3.5          # measured: the oracle's worst ratio over the general-class cases is 3.475 (general_K1_n4097)
DEVICE_FACTOR = 4.0
F32 = np.float32


def identity_params(scan_period=0.1, enabled=1):
    p = np.zeros((), PARAMS)
    for k in ("cT", "c_start", "c_end"):
        p[k] = 1.0
    p["scan_period"] = scan_period
    p["enabled"] = enabled
    return p


def make_params(T=None, shift=None, imu_start=None, imu_end=None, scan_period=0.1, enabled=1):
    """a record from angles: every sine / cosine word is the float32 nearest to the true value of the float32 angle"""
    p = identity_params(scan_period, enabled)
    if T is not None:
        p["T"] = np.asarray(T, F32)
        p["sT"] = np.sin(p["T"][:3].astype(np.float64)).astype(F32)
        p["cT"] = np.cos(p["T"][:3].astype(np.float64)).astype(F32)
    if shift is not None:
        p["shift"] = np.asarray(shift, F32)
    for key, ang in (("start", imu_start), ("end", imu_end)):
        if ang is not None:
            a = np.asarray(ang, F32).astype(np.float64)
            p["s_" + key] = np.sin(a).astype(F32)
            p["c_" + key] = np.cos(a).astype(F32)
    return p


# ---- float32, operation for operation (dev_math.hpp rot_x / rot_y / rot_z; every product and every sum is rounded once) ----
def _rot_x(y, z, c, s):
    return c * y - s * z, s * y + c * z


def _rot_y(x, z, c, s):
    return c * x + s * z, c * z - s * x


def _rot_z(x, y, c, s):
    return c * x - s * y, s * x + c * y


def _s_of(w, period):
    """s = (1.f / scan_period) * (w - (float)(int)w), float32"""
    w = np.asarray(w, F32)
    return (F32(1.0) / F32(period)) * (w - np.trunc(w))


def _deskew_f32(x, y, z, s, T):
    x = x - s * T[3]
    y = y - s * T[4]
    z = z - s * T[5]
    # sincosf(-s * T[k]) with T[k] == +-0: the angle is a zero, its sine that same zero, its cosine 1
    one = F32(1.0)
    sx, sy, sz = -s * T[0], -s * T[1], -s * T[2]
    x, y = _rot_z(x, y, one, sz)
    y, z = _rot_x(y, z, one, sx)
    x, z = _rot_y(x, z, one, sy)
    return x, y, z


def to_start_f32(points, P):
    pts = np.asarray(points, F32).reshape(-1, 4)
    T = P["T"].astype(F32)
    assert (T[:3] == 0).all(), "the float32 restatement needs a zero rotation"
    with np.errstate(all="ignore"):
        x, y, z = _deskew_f32(pts[:, 0], pts[:, 1], pts[:, 2], _s_of(pts[:, 3], P["scan_period"]), T)
    return np.stack([x, y, z, pts[:, 3]], axis=1).astype(F32)


def to_end_f32(points, P):
    pts = np.asarray(points, F32).reshape(-1, 4)
    T = P["T"].astype(F32)
    assert (T[:3] == 0).all(), "the float32 restatement needs a zero rotation"
    sT, cT, sh = P["sT"], P["cT"], P["shift"]
    ss, cs, se, ce = P["s_start"], P["c_start"], P["s_end"], P["c_end"]
    x, y, z = _deskew_f32(pts[:, 0], pts[:, 1], pts[:, 2], _s_of(pts[:, 3], P["scan_period"]), T)
    x, z = _rot_y(x, z, cT[1], sT[1]); y, z = _rot_x(y, z, cT[0], sT[0]); x, y = _rot_z(x, y, cT[2], sT[2])
    x = x + (T[3] - sh[0])
    y = y + (T[4] - sh[1])
    z = z + (T[5] - sh[2])
    x, y = _rot_z(x, y, cs[2], ss[2]); y, z = _rot_x(y, z, cs[0], ss[0]); x, z = _rot_y(x, z, cs[1], ss[1])
    x, z = _rot_y(x, z, ce[1], -se[1]); y, z = _rot_x(y, z, ce[0], -se[0]); x, y = _rot_z(x, y, ce[2], -se[2])
    return np.stack([x, y, z, np.trunc(pts[:, 3])], axis=1).astype(F32)


# ---- float64 behind the float32 inputs and the kernel's s ----
def _deskew_f64(pts, P):
    T = P["T"].astype(np.float64)
    s = _s_of(pts[:, 3], P["scan_period"]).astype(np.float64)
    x, y, z = (pts[:, k].astype(np.float64) - s * T[3 + k] for k in range(3))
    ax, ay, az = -s * T[0], -s * T[1], -s * T[2]
    x, y = _rot_z(x, y, np.cos(az), np.sin(az))
    y, z = _rot_x(y, z, np.cos(ax), np.sin(ax))
    x, z = _rot_y(x, z, np.cos(ay), np.sin(ay))
    return x, y, z


def to_start_f64(points, P):
    pts = np.asarray(points, F32).reshape(-1, 4)
    x, y, z = _deskew_f64(pts, P)
    return np.stack([x, y, z, pts[:, 3].astype(np.float64)], axis=1)


def to_end_f64(points, P):
    pts = np.asarray(points, F32).reshape(-1, 4)
    d = lambda k: P[k].astype(np.float64)
    T, sT, cT, sh, ss, cs, se, ce = d("T"), d("sT"), d("cT"), d("shift"), d("s_start"), d("c_start"), d("s_end"), d("c_end")
    x, y, z = _deskew_f64(pts, P)
    x, z = _rot_y(x, z, cT[1], sT[1]); y, z = _rot_x(y, z, cT[0], sT[0]); x, y = _rot_z(x, y, cT[2], sT[2])
    x = x + (T[3] - sh[0]); y = y + (T[4] - sh[1]); z = z + (T[5] - sh[2])
    x, y = _rot_z(x, y, cs[2], ss[2]); y, z = _rot_x(y, z, cs[0], ss[0]); x, z = _rot_y(x, z, cs[1], ss[1])
    x, z = _rot_y(x, z, ce[1], -se[1]); y, z = _rot_x(y, z, ce[0], -se[0]); x, y = _rot_z(x, y, ce[2], -se[2])
    return np.stack([x, y, z, np.trunc(pts[:, 3]).astype(np.float64)], axis=1)


def scale(points, P):
    """|x| + |y| + |z| + |T.pos|_1 + |shift|_1 per point: what the bound of a point is proportional to"""
    pts = np.asarray(points, F32).reshape(-1, 4).astype(np.float64)
    return np.abs(pts[:, :3]).sum(axis=1) + float(np.abs(P["T"][3:].astype(np.float64)).sum() + np.abs(P["shift"].astype(np.float64)).sum())


def bound(points, P, factor=1.0):
    return factor * KAPPA * 2.0 ** -24 * scale(points, P)


def batch(fn, points, off, params, passthrough=True):
    """fn per cloud with the record of the cloud's stream, c % ns; a stream with enabled == 0 keeps its clouds word for word"""
    pts = np.asarray(points, F32).reshape(-1, 4)
    params = np.asarray(params, PARAMS).reshape(-1)
    out = np.zeros((len(pts), 4), np.float64 if fn in (to_end_f64, to_start_f64) else F32)
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        P = params[c % len(params)]
        out[a:b] = fn(pts[a:b], P) if (P["enabled"] or not passthrough) else pts[a:b]
    return out


# ---- the ring-first table and the order stamp, in Python integers ----
def ring_table(w_out, off, epoch, table_in):
    """-> (table, choices).  table: (K, 320) uint32 after the call.  Entry r < 319 of a cloud is written, epoch << 24 | index inside
    the cloud, for every point that is first in its cloud or whose predecessor in the cloud has another ring; entry 319 becomes the
    epoch when any point has a ring >= 255 or a ring below its predecessor's.  Everything else keeps table_in.  choices: {(cloud,
    ring): set of admissible words} for a ring with several run heads (an unordered cloud: whichever head was written last stays) —
    table holds the first head there."""
    w = np.asarray(w_out, F32)
    table = np.array(table_in, np.uint32).reshape(len(off) - 1, RF_N).copy()
    choices = {}
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        heads, unordered, prev = {}, False, None
        for i in range(a, b):
            ring = int(w[i])
            if ring < RF_N - 1 and (prev is None or prev != ring):
                heads.setdefault(ring, []).append((int(epoch) << 24) | (i - a))
            if ring >= 255 or (prev is not None and prev > ring):
                unordered = True
            prev = ring
        for ring, words in heads.items():
            table[c, ring] = words[0]
            if len(words) > 1:
                choices[(c, ring)] = set(words)
        if unordered:
            table[c, RF_N - 1] = int(epoch)
    return table, choices


def descents(w, off):
    """global indices of the points whose ring is below their predecessor's inside the same cloud"""
    r = np.trunc(np.asarray(w, F32)).astype(np.int64)
    d = np.flatnonzero(r[1:] < r[:-1]) + 1
    starts = set(int(o) for o in off)
    return [int(i) for i in d if int(i) not in starts]


# ---- the folded bounds ----
def enc_f32(f):
    u = np.asarray(f, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def dec_f32(e):
    e = np.asarray(e, np.uint32)
    return np.where(e & np.uint32(0x80000000), e & np.uint32(0x7fffffff), ~e).astype(np.uint32).view(F32)


RESET = np.array([0xffffffff] * 3 + [0] * 3, np.uint32)


def bounds(points_out, off, bounds_in):
    """-> (K, 6) encoded words: min x y z / max x y z of every cloud folded into bounds_in; an empty cloud keeps its words"""
    pts = np.asarray(points_out, F32).reshape(-1, 4)
    bb = np.array(bounds_in, np.uint32).reshape(len(off) - 1, 6).copy()
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b > a:
            e = enc_f32(pts[a:b, :3])
            bb[c, :3] = np.minimum(bb[c, :3], e.min(axis=0))
            bb[c, 3:] = np.maximum(bb[c, 3:], e.max(axis=0))
    return bb
