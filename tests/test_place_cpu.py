"""CPU: the place-recognition C-ABI (loamx_place_*; include/loamx.h) — declared and exported, laid out as a C compiler lays it out, failing
loudly without a GPU; the host-only sector table; and the numpy model the GPU tests check the device against (tests/place_model.py),
checked here against cells computed by hand, for its invariances, and on the revisit cases the GPU test uses."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import place_model as pm
from loam_velodyne_amd import loamx

F = np.float32
NEW_SYMBOLS = ("loamx_place_default_config", "loamx_place_create", "loamx_place_destroy", "loamx_place_reset", "loamx_place_size",
               "loamx_place_sector_table", "loamx_place_add", "loamx_place_add_from_map", "loamx_place_add_from_pipeline",
               "loamx_place_query_entry", "loamx_place_query", "loamx_place_get_descriptor", "loamx_place_save", "loamx_place_load")


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays


@pytest.mark.parametrize("c_name,struct", [("loamx_place_config", "PlaceConfig"), ("loamx_place_match", "PlaceMatch")])
def test_layouts_match_c(tmp_path, c_name, struct):
    st = getattr(loamx, struct)
    fields = [f for f, _ in st._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) +
                     '  printf("%d\\n", LOAMX_PLACE_MAX_RESULTS);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(st)
    assert got[1:-1] == [getattr(st, f).offset for f in fields]
    assert got[-1] == loamx.PLACE_MAX_RESULTS


def test_default_config():
    c = loamx.PlaceConfig()
    c.n_rings, c.n_candidates, c.device = 7, 3, 5
    loamx.lib().loamx_place_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.n_rings, c.n_sectors, c.max_range, c.min_range, c.height_offset) == (20, 60, 80.0, 0.0, 2.0)
    assert (c.n_candidates, c.exclude_recent, c.max_entries, c.initial_entries, c.device) == (0, 50, 0, 1024, 0)


def test_create_fails_without_gpu():
    if loamx.device_count() > 0:
        pytest.skip("a GPU is visible")
    L = loamx.lib()
    L.loamx_place_create.restype = C.c_void_p
    assert not L.loamx_place_create(None)
    assert "no HIP device" in L.loamx_last_error().decode()
    with pytest.raises(loamx.LoamxError) as e:
        loamx.PlaceDB()
    assert "no HIP device" in str(e.value)


@pytest.mark.parametrize("bad", [dict(n_rings=0), dict(n_rings=65), dict(n_sectors=3), dict(n_sectors=129), dict(max_range=0.0),
                                 dict(max_range=float("nan")), dict(min_range=-1.0), dict(min_range=80.0), dict(n_candidates=-1),
                                 dict(n_candidates=257), dict(initial_entries=0), dict(initial_entries=1000),
                                 dict(height_offset=float("inf"))])
def test_bad_configs_are_refused(bad):
    # (the configuration is checked before the device is looked for: the text names the field with or without a GPU)
    with pytest.raises(loamx.LoamxError) as e:
        loamx.PlaceDB(**bad)
    assert list(bad)[0] in str(e.value)


@pytest.mark.parametrize("S", [4, 60, 64, 128])
def test_sector_table_equals_the_model(S):
    assert loamx.place_sector_table(S).tobytes() == pm.sector_table(S).tobytes()


def test_sector_table_rejects_bad_arguments():
    L = loamx.lib()
    buf = np.zeros(512, np.float32)
    assert L.loamx_place_sector_table(3, buf.ctypes.data_as(C.c_void_p)) == loamx.E_INVALID
    assert L.loamx_place_sector_table(129, buf.ctypes.data_as(C.c_void_p)) == loamx.E_INVALID
    assert L.loamx_place_sector_table(60, None) == loamx.E_INVALID


# a dozen points, R = 4 rings of 10 m to max_range 40, S = 8 sectors of 45 degrees (angle from +z towards +x), height_offset 2
HAND_CLOUD = np.array([
    [0.0, 0.0, 5.0, 0],           # on the boundary of sector 0 (a > 0, b = 0): cross(0) = 0 >= 0 -> sector 0, ring 0, h 2
    [5.0, 1.0, 0.0, 0],           # on the boundary of sector 2 (straight left): sector 2, ring 0, h 3
    [1.0, 0.5, 12.0, 0],          # ring 1, sector 0, h 2.5
    [1.0, 4.0, 12.5, 0],          # the same cell, higher: h 6
    [-3.0, 0.0, -25.0, 0],        # behind, slightly right: angle just above 180 degrees -> sector 4, ring 2, h 2
    [-20.0, -1.0, 20.0, 0],       # exactly on the 315-degree diagonal: sector 7 (boundary belongs to the sector it starts), r = 28.28 ring 2, h 1
    [0.0, 0.0, 40.0, 0],          # exactly at max_range: r2 < max_range^2 fails, dropped
    [0.0, 3.0, 39.5, 0],          # just inside: ring 3, sector 0, h 5
    [7.0, -2.0, 7.0, 0],          # h = 0: dropped
    [7.0, -2.5, 7.0, 0],          # h < 0: dropped
    [np.nan, 0.0, 1.0, 0],        # not finite: dropped
    [1.0, np.inf, 1.0, 0],        # not finite: dropped
    [0.0, 1.0, 0.0, 0],           # a = b = 0: no sector qualifies, dropped
], np.float32)
HAND = dict(R=4, S=8, max_range=40.0, height_offset=2.0)


def test_model_against_cells_computed_by_hand():
    used, ring, sector, h, amb = pm.cells_of(HAND_CLOUD, (0, 0, 0), **HAND)
    assert used.tolist() == [True] * 6 + [False, True] + [False] * 5
    assert ring[used].tolist() == [0, 0, 1, 1, 2, 2, 3]
    assert sector[used].tolist() == [0, 2, 0, 0, 4, 7, 0]
    assert not amb.any()
    D = pm.descriptor(HAND_CLOUD, (0, 0, 0), **HAND)
    want = np.zeros((4, 8), F)
    want[0, 0], want[0, 2], want[1, 0], want[2, 4], want[2, 7], want[3, 0] = 2, 3, 6, 2, 1, 5
    assert np.array_equal(D, want)
    assert np.array_equal(pm.ring_key(D), np.array([5, 6, 3, 5], F) / F(8))
    # a non-zero origin: the same cloud moved with it gives the same cells (small dyadic offsets: the subtraction is exact)
    o = np.array([0.5, -0.25, 2.0], F)
    moved = HAND_CLOUD.copy()
    moved[:, :3] += o
    assert np.array_equal(pm.descriptor(moved, o, **HAND), want)
    # min_range
    assert pm.descriptor(HAND_CLOUD, (0, 0, 0), min_range=5.0, **HAND)[0].tolist() == [2, 0, 3, 0, 0, 0, 0, 0]    # r2 >= 25 keeps r = 5
    assert pm.descriptor(HAND_CLOUD, (0, 0, 0), min_range=5.5, **HAND)[0].tolist() == [0] * 8


def test_model_distance_computed_by_hand():
    # two columns in use.  Q: col 0 = (3, 4), col 1 = (1, 0);  C = Q shifted by one column plus an empty rest
    Q = np.zeros((2, 4), F)
    Q[:, 0], Q[:, 1] = (3, 4), (1, 0)
    Cm = np.zeros((2, 4), F)
    Cm[:, 1], Cm[:, 2] = (3, 4), (1, 0)     # C[i][(j + 1) mod 4] = Q[i][j]
    d = pm.distances(Q, Cm[None])[0]
    # shift 1: both columns meet themselves: cos = 25 / (5 * 5) = 1 and 1 / (1 * 1) = 1 -> d = 1 - 2 / 2 = 0
    # shift 0: only Q col 1 meets a used column, C col 1 = (3, 4): cos = 3 / (1 * 5) -> d = 1 - 0.6
    # shift 2: only Q col 0 meets C col 2 = (1, 0): cos = 3 / 5;  shift 3: nothing meets: d = 1
    assert d[1] == F(0.0)
    assert d[0] == F(1.0) - F(3.0) / F(5.0) and d[2] == d[0]
    assert d[3] == F(1.0)
    assert pm.pair_distance(Q, Cm) == (F(0.0), 1)
    assert pm.ring_key_distance(np.array([1, 2], F), np.array([[1.5, 4], [1, 2]], F)).tolist() == [4.25, 0.0]


def _direction_cloud(S, rng, n_per=6):
    """points on the bisectors of the S sectors at dyadic ranges / heights, built from ONE table of directions: rotating by m sectors is
    a permutation of the directions, not trigonometry"""
    ang = 2.0 * np.pi * (np.arange(S) + 0.5) / S
    dirs = np.stack([np.sin(ang), np.cos(ang)], 1).astype(F)     # (x, z) per sector
    sec = np.repeat(np.arange(S), n_per)
    rng_m = rng.integers(1, 78 * 4, len(sec)).astype(F) / F(4) + F(0.125)   # (never on a ring boundary, a multiple of 4 m)
    y = rng.integers(-4, 40, len(sec)).astype(F) / F(4)
    return dirs, sec, rng_m, y


def _assemble(dirs, sec, rng_m, y):
    p = np.zeros((len(sec), 4), F)
    p[:, 0], p[:, 1], p[:, 2] = dirs[sec, 0] * rng_m, y, dirs[sec, 1] * rng_m
    return p


def test_model_invariances():
    rng = np.random.default_rng(3)
    S = 60
    dirs, sec, r, y = _direction_cloud(S, rng)
    p = _assemble(dirs, sec, r, y)
    D = pm.descriptor(p)
    assert (D > 0).sum() > 100
    assert pm.descriptor(p[rng.permutation(len(p))]).tobytes() == D.tobytes()      # the order of the points does not matter
    for m in (1, 7, 59):
        # every point moves m sectors on (its direction replaced by the one m further): Q[i][j + m] = D[i][j], i.e. Q[i][j] ~ D[i][j - m]
        q = _assemble(dirs, (sec + m) % S, r, y)
        Q = pm.descriptor(q)
        assert np.array_equal(Q, np.roll(D, m, axis=1))
        assert pm.pair_distance(D, Q) == (F(0.0), m)            # D[i][j] = Q[i][(j + m) mod S]
        assert pm.pair_distance(Q, D) == (F(0.0), (S - m) % S)
        assert np.allclose(pm.ring_key(Q), pm.ring_key(D), rtol=1e-5)   # (the row sums start elsewhere: equal up to rounding)


def test_model_search_order_and_candidates():
    rng = np.random.default_rng(9)
    m = pm.Model(R=6, S=8, n_candidates=4, exclude_recent=3)
    ex = pm.Model(R=6, S=8, n_candidates=0, exclude_recent=3)
    clouds = [np.concatenate([rng.uniform(-60, 60, (40, 1)), rng.uniform(-2, 6, (40, 1)), rng.uniform(-60, 60, (40, 1)), np.zeros((40, 1))], 1)
              .astype(F) for _ in range(14)]
    for c in clouds:
        assert m.add(c) == ex.add(c)
    m.add(clouds[2])      # entry 14 = entry 2 again
    ex.add(clouds[2])
    res = ex.query_entry(14, n_results=20)
    assert [r[0] for r in res][0] == 2 and res[0][2] == F(0.0) and res[0][1] == 0
    assert sorted(r[0] for r in res) == list(range(11))               # id + 3 < 14
    assert all((a[2], a[0]) < (b[2], b[0]) for a, b in zip(res, res[1:]))
    ids, rkd = m.candidates(m.keys[14], 14, 3)
    assert len(ids) == 4 and 2 in ids
    cut = m.query_entry(14, n_results=20)
    assert cut == ex.query_entry(14, n_results=20, only=ids)
    assert m.query(clouds[5], n_results=1)[0][0] == 5                 # not stored, exclude_recent 0: every entry is a candidate
    assert ex.query_entry(3) == [] and ex.query_entry(4)[0][0] == 0   # no candidate / exactly one
    cap = pm.Model(max_entries=2)
    assert cap.add(clouds[0]) == 0 and cap.add(clouds[1]) == 1 and cap.add(clouds[2]) is None and len(cap) == 2


def test_revisits_are_solved_by_the_model():
    """The cases tests/test_gpu_place.py runs on the device: 40 HDL-64E sweeps (az_steps 1024) at rest along
    synth.trajectory(40, step=2.5, yaw_step_deg=1.0) in synth.World(half_extent=125), and three queries at pose k turned by dyaw and
    displaced by (+off, 0, -off).  The best match is k, its shift is dyaw in sectors within +-1, entry k is first by ring-key distance,
    and the second-best distance is larger by at least 0.05."""
    db, queries = pm.revisit_case()
    m = pm.Model()
    dropped = ambiguous = 0
    for p in db:
        used, _, sector, h, amb = pm.cells_of(p)
        ambiguous += int(amb.sum())
        dropped += int((sector < 0).sum())
        m.add(p)
    assert (dropped, ambiguous) == (0, 0)      # the sector rule names exactly one sector for every point of these sweeps
    for k, dyaw, q in queries:
        res = m.query(q, n_results=5)
        want_shift = int(round(dyaw / 360.0 * m.S)) % m.S
        print(f"revisit k={k} dyaw={dyaw}: best {res[0]}, second {res[1]}")
        assert res[0][0] == k
        assert min((res[0][1] - want_shift) % m.S, (want_shift - res[0][1]) % m.S) <= 1
        assert res[1][2] - res[0][2] >= 0.05
        _, rk = m.describe(q)
        ids, rkd = m.candidates(rk, len(m), 0)
        assert ids[np.lexsort((ids, rkd))][0] == k
