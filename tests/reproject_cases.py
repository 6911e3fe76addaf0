"""Seeded, named cases for the sweep re-projection probe (loamx_reproject_probe), each with the claim it is there for.  Smallest
shapes at which the kernels can still go wrong; no case exceeds ~70,000 points.  (The ring-first table's index-wider-than-24-bits
branch needs a 16.8 M-point cloud and is deliberately left out.)

Classes:
  exact    T[0..2] == 0: the points equal reproject_model.to_end_f32 word for word
  order    the same, and the claim is about the ring-first table and the order stamp
  bounds   the same, and the claim is about the folded bounds
  general  rotations up to +-0.3 rad, translations up to +-3 m, IMU angles up to +-0.5 rad, shifts up to +-2 m, points out to 120 m"""
import zlib
from dataclasses import dataclass, field

import numpy as np

import reproject_model as rm

F32 = np.float32
FILL = 0x5a000000 | 0x00a5a5a5      # the caller's fill of the ring-first table: epoch byte 0x5a, never an epoch a case uses


@dataclass
class Case:
    name: str
    cls: str
    claim: str
    pts: np.ndarray
    off: np.ndarray
    params: np.ndarray
    epoch: int = 7
    n_corner_all: int = 0
    table_in: np.ndarray = None
    bounds_in: np.ndarray = None
    claims: dict = field(default_factory=dict)
    imu_angles: list = None      # general class: per stream, the six float32 IMU angles (pitch yaw roll at the start, then at the end) the words were made from

    @property
    def n(self):
        return len(self.pts)

    @property
    def K(self):
        return len(self.off) - 1

    @property
    def ns(self):
        return len(self.params)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _w(rings, rng, period):
    """ring + a time fraction in [0, period), as the float32 the kernel sees"""
    rings = np.asarray(rings, np.int64)
    w = (rings + rng.uniform(0, period, len(rings))).astype(F32)
    over = (w - np.trunc(w)) >= F32(period)      # (rounding at a large ring may reach the period: step back)
    w[over] = np.nextafter(w[over], F32(0))
    w[np.trunc(w) != rings] = rings[np.trunc(w) != rings].astype(F32)
    return w


def _cloud(rng, rings, ext=60.0, period=0.1):
    n = len(rings)
    p = np.zeros((n, 4), F32)
    p[:, :3] = rng.uniform(-ext, ext, (n, 3))
    p[:, 3] = _w(rings, rng, period)
    return p


def _ordered_rings(n, lo=0, hi=63):
    return lo + (np.arange(n, dtype=np.int64) * (hi - lo + 1)) // max(n, 1)


def _unit(angles):
    a = np.asarray(angles, np.float64)
    return np.sin(a).astype(F32), np.cos(a).astype(F32)


def _params(kind, period=0.1, rng=None, enabled=1):
    """exact-class records: zero transform rotation"""
    p = rm.identity_params(period, enabled)
    if kind in ("translation", "trans_shift", "all"):
        p["T"][3:] = rng.uniform(-3, 3, 3).astype(F32)
    if kind in ("shift", "trans_shift", "all"):
        p["shift"] = rng.uniform(-2, 2, 3).astype(F32)
    if kind in ("imu_rot", "all"):
        p["s_start"], p["c_start"] = _unit(rng.uniform(-3.1, 3.1, 3))     # arbitrary unit words: no small-angle shortcut survives
        p["s_end"], p["c_end"] = _unit(rng.uniform(-3.1, 3.1, 3))
    return p


def _general_params(rng, period=0.1):
    ang = rng.uniform(-0.5, 0.5, 6).astype(F32)
    return rm.make_params(T=np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-3, 3, 3)]), shift=rng.uniform(-2, 2, 3),
                          imu_start=ang[:3], imu_end=ang[3:], scan_period=period), ang


def _split(rng, n, K):
    cuts = np.sort(rng.integers(0, n + 1, K - 1)) if K > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [n]]).astype(np.uint32)


def _case(name, cls, claim, pts, off, params, **kw):
    params = np.asarray(params, rm.PARAMS).reshape(-1)
    off = np.asarray(off, np.uint32)
    K = len(off) - 1
    kw.setdefault("table_in", np.full((K, rm.RF_N), FILL, np.uint32))
    kw.setdefault("bounds_in", np.tile(rm.RESET, (K, 1)))
    kw.setdefault("n_corner_all", int(off[K // 2]))     # the fused form splits where the corner clouds end: half of the clouds
    return Case(name, cls, claim, np.ascontiguousarray(pts, F32).reshape(-1, 4), off, params, **kw)


def _tiny_clouds(rng):
    """64 clouds of 1-3 points inside two waves (126 points)"""
    return np.concatenate([[0], np.cumsum(rng.permutation([1] * 22 + [2] * 22 + [3] * 20))]).astype(np.uint32)


def _per_cloud_rings(rng, off, lo=0, hi=63):
    r = np.zeros(int(off[-1]), np.int64)
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        r[a:b] = np.sort(rng.integers(lo, hi + 1, b - a))
    return r


# ------------------------------------------------------------------------------------------------------------------------------
def exact_cases():
    out = []
    for kind in ("translation", "shift", "imu_rot", "trans_shift", "all"):
        for period in (0.1, 0.05):
            name = f"exact_{kind}_p{period}"
            rng = _rng(name)
            out.append(_case(name, "exact", f"{kind} only, scan period {period}", _cloud(rng, _ordered_rings(257, 0, 15), period=period), [0, 257],
                             [_params(kind, period, rng)], claims=dict(imu_zero=kind in ("translation", "shift", "trans_shift"))))
    # point fields: fractions 0 / one float32 step / just under the period at rings where .w keeps few fraction bits; +-300 m; both zeros
    for kind in ("trans_shift", "all"):
        name = f"exact_fields_{kind}"
        rng = _rng(name)
        rows = []
        for ring in (0, 1, 127, 254):
            under = np.nextafter(F32(ring) + F32(0.1), F32(0))
            while under - np.trunc(under) >= F32(0.1):
                under = np.nextafter(under, F32(0))
            for w in (F32(ring), np.nextafter(F32(ring), F32(1e9)), under):
                for xyz in ((300.0, -300.0, 299.99), (-300.0, 300.0, -0.0), (0.0, -0.0, 0.0), (-0.0, 0.0, -0.0), tuple(rng.uniform(-300, 300, 3))):
                    rows.append((*xyz, w))
        pts = np.array(rows, F32)
        out.append(_case(name, "exact", "edge fractions, rings 0 1 127 254, +-300 m, both signs of zero", pts, [0, len(pts)], [_params(kind, 0.1, rng)],
                         claims=dict(imu_zero=kind == "trans_shift", fields=True)))
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 4097):
        name = f"exact_n{n}"
        rng = _rng(name)
        out.append(_case(name, "exact", f"{n} points in one cloud", _cloud(rng, _ordered_rings(n), ext=100.0), [0, n], [_params("trans_shift", 0.1, rng)],
                         claims=dict(imu_zero=True)))
    for K in (1, 2, 6, 64):
        for ns in (1, 2, 3):
            if ns > K:
                continue
            name = f"exact_K{K}_ns{ns}"
            rng = _rng(name)
            if K == 64:
                off = _tiny_clouds(rng)
            else:
                off = _split(rng, 1000, K)
            # records that differ strongly: a stream that takes a neighbour's record lands metres away
            params = [_params("all", 0.1, rng) for _ in range(ns)]
            for s, p in enumerate(params):
                p["T"][3:] = F32(3.0) * np.array([1, -1, 1], F32) * F32((-1) ** s) + F32(s)
            out.append(_case(name, "exact", f"{K} clouds over {ns} streams: cloud c takes record c % ns",
                             _cloud(rng, _per_cloud_rings(rng, off)), off, params, claims=dict(distinct_params=ns > 1)))
    for name, off in (("exact_empty_front_mid_end_run", [0, 0, 100, 100, 100, 100, 300, 420, 420]),
                      ("exact_boundaries_64_256_midwave", [0, 64, 256, 300, 512, 700]),
                      ("exact_all_but_one_empty", [0, 0, 0, 70, 70])):
        rng = _rng(name)
        off = np.array(off, np.uint32)
        out.append(_case(name, "exact", "cloud layout: " + name[6:], _cloud(rng, _per_cloud_rings(rng, off)), off,
                         [_params("all", 0.1, rng), _params("trans_shift", 0.1, rng)]))
    name = "exact_passthrough_stream1"
    rng = _rng(name)
    off = _split(rng, 900, 6)
    params = [_params("all", 0.1, rng), _params("all", 0.1, rng, enabled=0), _params("trans_shift", 0.1, rng)]
    out.append(_case(name, "exact", "enabled = 0 on stream 1 only: its clouds come back word for word, the table reads (int) of the raw .w",
                     _cloud(rng, _per_cloud_rings(rng, off)), off, params, claims=dict(passthrough=[1, 4])))
    return out


def _with_descent(rings, idx, by=2):
    r = np.asarray(rings, np.int64).copy()
    r[idx:] -= (r[idx] - r[idx - 1]) + by
    assert r.min() >= 0
    return r


def order_cases():
    out = []
    P = lambda rng: [_params("trans_shift", 0.1, rng)]

    def add(name, claim, rings_per_cloud, **kw):
        rng = _rng(name)
        off = np.concatenate([[0], np.cumsum([len(r) for r in rings_per_cloud])]).astype(np.uint32)
        rings = np.concatenate([np.asarray(r, np.int64) for r in rings_per_cloud]) if len(rings_per_cloud) else np.zeros(0, np.int64)
        params = kw.pop("params", None) or P(rng)
        out.append(_case(name, "order", claim, _cloud(rng, rings), off, params, **kw))

    add("order_all_rings", "a ring-ordered cloud with all rings present: 64 entries, no stamp", [_ordered_rings(4097)], claims=dict(stamped=[]))
    add("order_rings_missing", "rings 0 3 7 100 254 only: the other entries keep the caller's fill",
        [np.repeat([0, 3, 7, 100, 254], [300, 1, 64, 500, 35])], claims=dict(stamped=[], rings=[0, 3, 7, 100, 254]))
    base = _ordered_rings(4097, 10, 49)
    for idx in (1, 63, 64, 65, 255, 256, 257, 4096):
        add(f"order_descent_at_{idx}", f"one single descent, at index {idx} of an otherwise ordered 4097-point cloud", [_with_descent(base, idx)],
            claims=dict(stamped=[0], descents=[idx]))
    add("order_descent_at_64_midwave_cloud", "one single descent 64 points into a cloud that starts in mid-wave (at 100)",
        [_ordered_rings(100), _with_descent(base, 64)], claims=dict(stamped=[1], descents=[164]))
    add("order_descent_by_one_at_2048", "a descent of exactly one ring, at the first thread of a workgroup", [_with_descent(base, 2048, by=1)],
        claims=dict(stamped=[0], descents=[2048], by_one=True))
    add("order_descent_by_one_at_1000", "a descent of exactly one ring in mid-wave", [_with_descent(base, 1000, by=1)],
        claims=dict(stamped=[0], descents=[1000], by_one=True))
    add("order_equal_rings", "equal rings throughout: one entry, no stamp", [np.full(300, 5)], claims=dict(stamped=[], rings=[5]))
    for tag, first in (("midwave", 100), ("at_64", 64), ("at_256", 256)):
        add(f"order_drop_across_boundary_{tag}", f"the ring drops from the last point of a cloud to the first of the next ({tag}): no violation",
            [_ordered_rings(first, 20, 60), _ordered_rings(200, 0, 30)], claims=dict(stamped=[]))
    add("order_drop_across_empty_cloud", "the same across an empty cloud", [_ordered_rings(128, 20, 60), [], _ordered_rings(200, 0, 30)], claims=dict(stamped=[]))
    for ring, stamped in ((254, []), (255, [0]), (318, [0]), (319, [0]), (400, [0])):
        add(f"order_ring_{ring}", f"ring {ring}: " + ("an entry" if ring < 319 else "no entry") + (", a stamp" if stamped else ", no stamp"),
            [np.array([0, 0, 1, ring, ring])], claims=dict(stamped=stamped, rings=[0, 1] + ([ring] if ring < 319 else [])))
    six = [_ordered_rings(m) for m in (200, 64, 191, 321, 100, 150)]
    six[3] = _with_descent(_ordered_rings(321, 10, 49), 129)
    rng = _rng("order_one_violating_among_six")
    add("order_one_violating_among_six", "six clouds, one violation in cloud 3: only its word 319 changes", six,
        params=[_params("trans_shift", 0.1, rng) for _ in range(3)], claims=dict(stamped=[3], descents=[200 + 64 + 191 + 129]))
    add("order_unordered_whole_rings_swapped", "whole rings swapped: several run heads per ring, any of them may stay",
        [np.concatenate([np.repeat([3, 1, 2, 1, 3], 40), [0]])], claims=dict(stamped=[0], multi_head=True))
    return out


def epoch_sequence():
    """three calls on the same table, epochs 254, 255, 1: entries of rings absent from the later clouds keep the earlier epoch; the
    stamp of a cloud that was unordered at 254 and is ordered afterwards stays 254"""
    rng = _rng("order_epoch_sequence")
    P = [_params("trans_shift", 0.1, rng)]
    seq = []
    for k, (epoch, clouds) in enumerate(((254, [_with_descent(_ordered_rings(500, 10, 40), 77), _ordered_rings(300, 0, 20)]),
                                         (255, [_ordered_rings(400, 15, 30), _ordered_rings(300, 5, 12)]),
                                         (1, [_ordered_rings(130, 20, 25), _ordered_rings(10, 5, 6)]))):
        off = np.concatenate([[0], np.cumsum([len(r) for r in clouds])]).astype(np.uint32)
        seq.append(_case(f"order_epoch_sequence_{k}_e{epoch}", "order", "epochs 254, 255, 1 on one table", _cloud(rng, np.concatenate(clouds)), off, P, epoch=epoch))
    return seq


def bounds_cases():
    out = []

    def add(name, claim, off, **kw):
        rng = _rng(name)
        off = np.array(off, np.uint32)
        pts = _cloud(rng, _per_cloud_rings(rng, off))
        edit = kw.pop("edit", None)
        if edit:
            edit(pts)
        out.append(_case(name, "bounds", claim, pts, off, [_params("trans_shift", 0.1, rng), _params("shift", 0.1, rng)][:min(2, len(off) - 1)], **kw))

    add("bounds_whole_waves", "every wave belongs to one cloud (workgroup-level reduction, one atomic per word)", [0, 64, 128, 320, 576])
    prefilled = np.tile(rm.RESET, (3, 1))
    prefilled[0, 0] = rm.enc_f32(F32(-1000.0))      # a minimum already below every point stays
    prefilled[2, 5] = rm.enc_f32(F32(-1000.0))      # a maximum below every point is replaced
    add("bounds_straddling", "waves across cloud boundaries (every lane for itself), folded into words that already hold something", [0, 100, 300, 333],
        bounds_in=prefilled, claims=dict(mixed=True))
    rng = _rng("bounds_tiny_off")
    add("bounds_tiny_clouds", "64 clouds of 1-3 points", _tiny_clouds(rng))
    add("bounds_one_point", "a cloud of one point: minimum == maximum", [0, 1])
    add("bounds_with_empty_clouds", "empty clouds keep their words", [0, 0, 130, 130, 256, 256])

    def extremes(p):
        p[:, :3] = np.clip(p[:, :3], -50, 50)
        p[0, 0], p[-1, 0] = 200.0, -200.0        # first / last point of the cloud
        p[63, 1], p[64, 1] = 210.0, -210.0       # lane 63 / lane 0 of the next wave
        p[255, 2], p[256, 2] = 220.0, -220.0     # last thread of a workgroup / first of the next
    add("bounds_extremes_at_edges", "extremes at the first and last point of a cloud, at lane 63 / lane 0 and across a workgroup", [0, 600], edit=extremes,
        claims=dict(extremes=True))
    return out


def general_cases():
    out = []
    for name, n, K, ns, period in (("general_K1_n4097", 4097, 1, 1, 0.1), ("general_K6_ns3", 3000, 6, 3, 0.1), ("general_K2_ns2_p0.05", 1000, 2, 2, 0.05),
                                   ("general_K4_ns1_n257", 257, 4, 1, 0.1)):
        rng = _rng(name)
        off = _split(rng, n, K)
        pts = _cloud(rng, _per_cloud_rings(rng, off, 0, 127), ext=120.0 / np.sqrt(3.0), period=period)
        recs = [_general_params(rng, period) for _ in range(ns)]
        out.append(_case(name, "general", "rotations to 0.3 rad, translations to 3 m, IMU angles to 0.5 rad, shifts to 2 m, points to 120 m",
                         pts, off, [r[0] for r in recs], imu_angles=[r[1] for r in recs]))
    return out


def all_cases():
    return exact_cases() + order_cases() + bounds_cases() + general_cases()
