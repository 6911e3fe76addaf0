"""CPU: alignment from many start poses (include/loamx.h, loamx_densemap_align_many and what stands beside it) — the new symbols
declared and exported, loamx_densemap_align_best (host only) against hand-written results, loamx.pose_grid (shape, order, the centre's
image, the base bit for bit, and the sign of its yaw against the place-recognition model's shift), refusals that need no device, and
the reason the feature exists, in the model: in the box scene one wide start ends "converged" in the wrong place, the best of a grid
of starts by (matched descending, rms ascending) ends inside the bars of the single alignment's tests (0.01 rad, leaf / 10).

The multi-start case runs the 12 yaws of the full grid with the centre column of offsets (x offset 0) and the offset nearest the
truth: 48 alignments of 1,000 points in numpy."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
import densemap_align_model as am
import densemap_moments_model as mm
import place_model as pm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_align_step_many", "loamx_densemap_align_many", "loamx_densemap_align_many_from_map",
               "loamx_densemap_align_many_from_pipeline", "loamx_densemap_align_best", "loamx_densemap_get_align_stats")
NONE = 0xFFFFFFFF   # UINT32_MAX


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "#define LOAMX_ALIGN_MAX_POSES 4096" in hdr and loamx.ALIGN_MAX_POSES == 4096
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("align_step_many", "align_many", "align_many_from", "align_many_from_pipeline", "align_stats"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert callable(loamx.align_best) and callable(loamx.pose_grid)


def _result(status, matched, rms):
    r = loamx.AlignResult()
    r.status, r.rms, r.counts[4] = status, rms, matched
    return r


def _best(results):
    arr = (loamx.AlignResult * max(len(results), 1))(*results)
    best = C.c_uint32(12345)
    assert loamx.lib().loamx_densemap_align_best(arr, C.c_uint32(len(results)), C.byref(best)) == loamx.OK
    assert loamx.align_best(results) == (None if best.value == NONE else best.value)
    return best.value


def test_align_best():
    assert _best([_result(2, 900, 0.01), _result(2, 10, 0.0)]) == NONE       # no candidate: still OK
    assert _best([]) == NONE
    assert _best([_result(0, 500, 0.03)]) == 0
    # most matched first; a converged status does not outrank a better-matched status 1
    assert _best([_result(0, 500, 0.01), _result(1, 501, 0.05), _result(0, 499, 0.001)]) == 1
    # a tie on matched is decided by rms, then by index
    assert _best([_result(0, 1000, 0.031), _result(0, 1000, 0.0275), _result(0, 1000, 0.0275), _result(0, 999, 0.001)]) == 1
    assert _best([_result(1, 7, 0.5), _result(0, 7, 0.5)]) == 0
    # a status-2 result with the most matches (and the smallest rms) is ignored
    assert _best([_result(2, 2000, 0.0), _result(0, 40, 0.2), _result(2, 3000, 0.0)]) == 1


def test_refusals_without_a_device():
    L = loamx.lib()
    arr, best = (loamx.AlignResult * 2)(), C.c_uint32(7)
    for args, name in (((None, C.c_uint32(2), C.byref(best)), "results"), ((arr, C.c_uint32(2), None), "best")):
        assert L.loamx_densemap_align_best(*args) == loamx.E_INVALID
        assert name in L.loamx_last_error().decode()
    assert best.value == 7    # nothing written
    # a NULL handle is refused before anything touches a device, and nothing is written
    cloud = loamx.cloud_of(np.zeros((4, 4), np.float32))
    rtc, poses = np.zeros(15, np.float32), np.zeros(12, np.float64)
    sums, counts, stats = np.full(28, 5, np.int64), np.full(5, 5, np.uint64), np.full(3, 5, np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.loamx_densemap_align_step_many(None, C.byref(cloud), ptr(rtc), C.c_uint32(1), C.c_uint32(1), C.c_float(0.5), ptr(sums),
                                            ptr(counts)) == loamx.E_INVALID
    assert "NULL argument: h" in L.loamx_last_error().decode()
    assert L.loamx_densemap_align_many(None, C.byref(cloud), ptr(poses), C.c_uint32(1), None, None, arr, C.byref(best)) == loamx.E_INVALID
    assert L.loamx_densemap_align_many_from_map(None, None, ptr(poses), C.c_uint32(1), None, arr, C.byref(best)) == loamx.E_INVALID
    assert L.loamx_densemap_align_many_from_pipeline(None, None, C.c_uint32(0), ptr(poses), C.c_uint32(1), None, arr,
                                                     C.byref(best)) == loamx.E_INVALID
    assert L.loamx_densemap_get_align_stats(None, ptr(stats)) == loamx.E_INVALID
    assert np.all(sums == 5) and np.all(counts == 5) and np.all(stats == 5) and best.value == 7
    assert bytes(arr) == bytes(C.sizeof(arr))


def test_pose_grid_shape_order_and_centre():
    base = np.concatenate([am.exp_so3([0.05, -0.12, 0.3]), np.array([[0.3], [0.5], [-0.2]])], axis=1)
    c = np.array([1.5, -0.25, 2.0])
    yaws = [0.0, 0.5, -1.25]
    offsets = [(0, 0, 0), (1.0, 0, 0), (0, 0, -2.0), (0.5, 0.25, 0.125)]
    G = loamx.pose_grid(base, c, yaws, offsets)
    assert G.shape == (12, 3, 4) and G.dtype == np.float64
    anchor = base[:, :3] @ c + base[:, 3]
    for i, a in enumerate(yaws):
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        for j, o in enumerate(offsets):
            P = G[i * len(offsets) + j]    # yaw-major
            assert np.abs(P[:, :3] - Ry @ base[:, :3]).max() < 1e-15
            assert np.abs(P[:, :3] @ c + P[:, 3] - (anchor + np.array(o))).max() < 1e-14    # the image of the centre moves by the offset
    assert G[0].tobytes() == base.tobytes()    # yaw 0, offset 0: the base bit for bit
    # the defaults: one pose, the base; without a centre the rotation is about the map's origin image of 0, i.e. t' = t + o
    assert loamx.pose_grid(base).tobytes() == base[None].tobytes()
    P = loamx.pose_grid(base, None, [0.3], [(1.0, 2.0, 3.0)])[0]
    assert np.abs(P[:, 3] - (base[:, 3] + [1.0, 2.0, 3.0])).max() < 1e-15


def test_pose_grid_yaw_sign_is_the_place_models():
    """a cloud and its copy turned by k * 2 pi / S about +y: turned by -k steps (the sensor has turned by +k steps) the query gets shift
    k, turned by +k steps shift S - k; pose_grid(yaws=[shift * 2 pi / S]) then carries the query cloud back onto the stored one"""
    rng = np.random.default_rng(11)
    S, k = 60, 7
    n = 4000
    stored = np.zeros((n, 4), np.float32)
    phi, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(3.0, 70.0, n)
    stored[:, 0], stored[:, 2] = r * np.sin(phi), r * np.cos(phi)
    stored[:, 1] = -1.5 + 2.0 * (np.floor(phi * 9 / np.pi) % 5) + rng.uniform(0.0, 1.0, n)    # heights that depend on the bearing
    a = k * 2.0 * np.pi / S
    Ry = lambda a: np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])

    def turned(angle):
        q = stored.copy()
        q[:, :3] = (stored[:, :3].astype(np.float64) @ Ry(angle).T).astype(np.float32)
        return q

    D = pm.descriptor(stored, S=S)
    d_minus, shift_minus = pm.pair_distance(pm.descriptor(turned(-a), S=S), D)
    d_plus, shift_plus = pm.pair_distance(pm.descriptor(turned(+a), S=S), D)
    assert shift_minus == k and shift_plus == S - k
    assert d_minus < 0.05 and d_plus < 0.05
    # the stored sweep at the (levelled) pose base; the query cloud is the stored cloud turned by -a: the sensor turned by +a
    base = np.concatenate([Ry(0.4), np.array([[2.0], [0.5], [-1.0]])], axis=1)
    P = loamx.pose_grid(base, yaws=[shift_minus * 2.0 * np.pi / S])[0]
    q = turned(-a)[:, :3].astype(np.float64)
    err = np.abs((q @ P[:, :3].T + P[:, 3]) - (stored[:, :3].astype(np.float64) @ base[:, :3].T + base[:, 3])).max()
    assert err < 1e-4    # (f32 rounding of the turned cloud at 70 m)


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    m = mm.MomentsModel(leaf=S["leaf"])
    for p, o in S["sweeps"]:
        assert m.add(p, o)
    S["keys"], S["recs"] = am.frozen_of(m.keys, m.surfels()[0])
    S["cloud"] = S["cloud"][::4].copy()
    return S


def test_model_multi_start_recovers_a_wide_start(box):
    truth, leaf = box["truth"], box["leaf"]
    n = len(box["cloud"])
    assert n == 1000
    wide = loamx.pose_grid(truth, yaws=[1.1], offsets=[(1.5, 0.0, -1.0)])[0]
    inside = lambda r: (lambda e: e[0] <= 0.01 and e[1] <= leaf / 10)(am.pose_error(r["pose"], truth))
    single = am.align(box["keys"], box["recs"], box["cloud"], wide, leaf)
    rot, trans = am.pose_error(single["pose"], truth)
    print(f"single: status {single['status']}, {rot:.3f} rad, {trans:.3f} m, matched {single['counts'][am.MATCHED]} of {n}")
    assert single["status"] == 0 and not inside(single) and rot > 1.0 and trans > 1.0    # "converged", and wrong
    assert single["counts"][am.MATCHED] == 487
    offsets = [(0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (-1.0, 0.0, 1.0)]
    grid = loamx.pose_grid(wide, yaws=np.arange(12) * np.pi / 6, offsets=offsets)
    res = [am.align(box["keys"], box["recs"], box["cloud"], P, leaf) for P in grid]
    cands = [k for k, r in enumerate(res) if r["status"] != 2]
    best = min(cands, key=lambda k: (-int(res[k]["counts"][am.MATCHED]), res[k]["rms"], k))
    rot, trans = am.pose_error(res[best]["pose"], truth)
    print(f"best of {len(grid)}: start {best}, {rot:.2e} rad, {trans:.2e} m, rms {res[best]['rms']:.5f}; "
          f"{sum(inside(r) for r in res)} starts inside the bars")
    assert inside(res[best]) and res[best]["counts"][am.MATCHED] == n
    # the rule agrees with the library's
    arr = []
    for r in res:
        a = loamx.AlignResult()
        a.status, a.rms = r["status"], r["rms"]
        for j in range(5):
            a.counts[j] = int(r["counts"][j])
        arr.append(a)
    assert loamx.align_best(arr) == best
    # the rms tie-break at work: starts that end with every point matched and are not the truth (the box's half-turn look-alike)
    full = [k for k in cands if res[k]["counts"][am.MATCHED] == n]
    wrong = [k for k in full if not inside(res[k])]
    assert wrong and all(res[k]["rms"] > res[best]["rms"] for k in wrong)
    assert any(res[k]["status"] == 0 for k in wrong)    # a converged status is no evidence
