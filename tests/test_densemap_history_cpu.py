"""CPU: the dense map's correction and the arithmetic of its sweep log and rebuild (include/loamx.h, loamx_densemap_enable_history and
what follows it; loam_velodyne_amd/csrc/densemap_history.hpp — standard library only).

loamx_densemap_correct is host only: the library's bytes are held to the model of tests/densemap_rebuild_model.py, which is the
expression of the header in numpy float32.  The log's capacity, the max_bytes refusal, the call table and the table sizes a rebuild
tries are arithmetic between HIP calls: tests/densemap_history_driver.cpp uses the header the way DenseMap does, with the HIP calls left
out, under UBSan; the rows are worked out by hand."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_rebuild_model as rm
from loam_velodyne_amd import loamx

SOURCES = ["-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "densemap_history_driver.cpp")]


def lib_correct(c12, xyz):
    """loamx_densemap_correct through ctypes: (status, output); the output starts as a pattern that no result has"""
    src = np.ascontiguousarray(xyz, np.float32)
    dst = np.full_like(src, np.float32(-12345.5))
    c = np.ascontiguousarray(c12, np.float64)
    rc = loamx.lib().loamx_densemap_correct(c.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                            C.c_uint64(len(src)))
    return rc, dst


EDGE_ROWS = np.float32([[-0.0, 0.0, -0.0], [1e-45, -1e-40, 3e-39], [1e30, -1e30, 1e30], [np.nan, 1.0, 2.0], [1.0, np.inf, 2.0],
                        [1.0, 2.0, -np.inf], [np.inf, np.inf, 1.0], [3.4e38, 3.4e38, 3.4e38], [0.0, 0.0, 0.0]])


def random_corrections(rng, n):
    return [rm.rigid(rng.normal(size=3) * 0.3, rng.uniform(-5, 5, 3), rng.uniform(-20, 20, 3)) for _ in range(n)]


def test_correct_equals_the_model_byte_for_byte():
    rng = np.random.default_rng(7)
    xyz = np.concatenate([rng.uniform(-120, 120, (6000, 3)).astype(np.float32), EDGE_ROWS])
    quarter = rm.rigid([0.0, np.pi / 2, 0.0], [0.25, -1.0, 3.0])
    for c in random_corrections(rng, 4) + [quarter, np.diag([1.0, 1.0, 1.0, 1.0])[:3] * 1e-30, rng.normal(size=(3, 4)) * 1e20]:
        rc, got = lib_correct(c, xyz)
        assert rc == loamx.OK
        assert got.tobytes() == rm.correct(c, xyz).tobytes()
        # the Python entry point is the same call; w rides along untouched
        p4 = np.concatenate([xyz, rng.normal(size=(len(xyz), 1)).astype(np.float32)], axis=1)
        assert loamx.correct(c, p4).tobytes() == rm.correct(c, p4).tobytes()
    assert not np.array_equal(rm.correct(quarter, xyz[:100]), xyz[:100])


def test_one_row_by_hand():
    # R = quarter turn about +z, t = (1, 2, 3): (x, y, z) -> (-y + 1, x + 2, z + 3); every product and sum is exact here
    c = np.float64([[0, -1, 0, 1], [1, 0, 0, 2], [0, 0, 1, 3]])
    rc, got = lib_correct(c, np.float32([[4, 5, 6]]))
    assert rc == loamx.OK and got.tolist() == [[-4.0, 6.0, 9.0]]
    # the order of the sums: (R_a0 x + R_a1 y) first.  With x = 2^24, y = 1, z = -2^24 and a row (1, 1, 1 | 0): (2^24 + 1) rounds to
    # 2^24 in f32, then - 2^24 gives 0; any other order, or a fused multiply-add, gives 1
    c = np.float64([[1, 1, 1, 0], [1, 0, 0, 0], [0, 0, 1, 0]])
    rc, got = lib_correct(c, np.float32([[2 ** 24, 1, -2 ** 24]]))
    assert rc == loamx.OK and got[0, 0] == 0.0
    # one rounding of the correction to f32: 1 + 2^-30 is 1 in f32, so this is the identity although the doubles are not
    c = np.float64(rm.IDENTITY) * (1.0 + 2.0 ** -30)
    assert rm.is_identity(c) and lib_correct(c, EDGE_ROWS)[1].tobytes() == EDGE_ROWS.tobytes()


def test_the_identity_copies_bytes():
    rng = np.random.default_rng(8)
    raw = rng.integers(0, 1 << 32, (4000, 3), dtype=np.uint64).astype(np.uint32)   # every bit pattern: NaN payloads, denormals, -0.0
    xyz = np.concatenate([raw.view(np.float32), EDGE_ROWS])
    minus = np.float64(rm.IDENTITY).copy()
    minus[minus == 0.0] = -0.0
    assert np.signbit(minus[0, 1]) and rm.is_identity(minus)
    for c in (np.float64(rm.IDENTITY), minus, np.eye(4)):
        rc, got = lib_correct(np.asarray(c)[:3], xyz)
        assert rc == loamx.OK and got.tobytes() == xyz.tobytes() == rm.correct(c, xyz).tobytes()
    # (not the identity: 0 * inf is NaN, -0.0 + 0.0 is +0.0 — the arithmetic would have changed these rows)
    # (one non-finite component per row: which of two NaNs an addition hands on is not part of the definition)
    xyz = np.concatenate([rng.uniform(-9, 9, (1000, 3)).astype(np.float32), EDGE_ROWS])
    almost = np.float64(rm.IDENTITY).copy()
    almost[0, 3] = 1e-30
    rc, got = lib_correct(almost, xyz)
    assert rc == loamx.OK and got.tobytes() != xyz.tobytes() and got.tobytes() == rm.correct(almost, xyz).tobytes()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("where", [0, 5, 11])
def test_a_non_finite_correction_is_refused(bad, where):
    c = np.float64(rm.rigid([0.1, 0.2, -0.1], [1, 2, 3])).reshape(-1)
    c[where] = bad
    rc, got = lib_correct(c, np.float32([[1, 2, 3], [4, 5, 6]]))
    assert rc == loamx.E_INVALID and np.all(got == np.float32(-12345.5))
    assert "finite" in loamx.lib().loamx_last_error().decode()
    with pytest.raises(loamx.LoamxError):
        loamx.correct(c.reshape(3, 4), np.float32([[1, 2, 3]]))


def test_default_configuration():
    c = loamx.DenseMapHistoryConfig(7, 7)
    loamx.lib().loamx_densemap_history_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.max_bytes, c.initial_points) == (0, 1 << 20)
    loamx.lib().loamx_densemap_history_default_config(None)


def test_model_rebuild_is_the_fresh_model_of_the_corrected_sweeps():
    import densemap_file_model as fm
    rng = np.random.default_rng(9)
    sweeps = [(np.concatenate([rng.uniform(-8, 8, (500, 4)).astype(np.float32), np.float32([[np.nan, 0, 0, 1], [-0.0, np.inf, 1, 2]])]),
               rng.uniform(-1, 1, 3).astype(np.float32)) for _ in range(3)] + [(np.zeros((0, 4), np.float32), (0, 0, 0))]
    cs = random_corrections(rng, 4)
    for flags in range(4):
        factory = lambda: fm.model_of(flags, 0.5, ray_stride=2)   # noqa: E731
        by_hand = factory()
        for (p, o), c in zip(sweeps[:3], cs):
            by_hand.add(rm.correct(c, p), rm.correct(c, np.float32(o))[0])
        assert fm.to_bytes(rm.rebuild(factory, sweeps, cs)) == fm.to_bytes(by_hand)
        plain = factory()
        for p, o in sweeps[:3]:
            plain.add(p, o)
        assert fm.to_bytes(rm.rebuild(factory, sweeps)) == fm.to_bytes(plain) == fm.to_bytes(rm.rebuild(factory, sweeps, [np.eye(4)] * 4))
        assert fm.to_bytes(plain) != fm.to_bytes(by_hand)


# ---- densemap_history.hpp under UBSan -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("densemap_history") / "densemap_history_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all"] + SOURCES + ["-o", path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def run(exe, args, text=""):
    r = subprocess.run([exe] + [str(a) for a in args], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    return [dict(kv.split("=") for kv in ln.split()) if "=" in ln else ln for ln in r.stdout.splitlines()]


def log_rows(exe, max_bytes, initial_points, events):
    rows = run(exe, ["log", max_bytes, initial_points], "".join(e + "\n" for e in events))
    return [tuple(int(r[k]) for k in ("admitted", "capacity", "points", "calls", "blocks")) if "admitted" in r else r for r in rows]


def test_log_capacity_doubles(exe):
    rows = log_rows(exe, 0, 1000, ["add 1000 0 0 0", "add 1 0 0 0", "add 999 0 0 0", "add 6001 0 0 0", "add 0 0 0 0", "reset", "add 8001 1 2 3"])
    assert rows == [(1, 1000, 1000, 1, 1),     # exactly full: no growth
                    (1, 2000, 1001, 2, 2),     # one point more: doubled
                    (1, 2000, 2000, 3, 2),
                    (1, 16000, 8001, 4, 3),    # 2000 -> 4000 -> 8000 -> 16000 in one step, one new block
                    (1, 16000, 8001, 4, 3),    # an empty call is admitted and not logged
                    (-1, 16000, 0, 0, 3),      # reset: the log is empty, the block stays
                    (1, 16000, 8001, 1, 3)]
    # 64-bit point indices: a log past 2^32 points
    big = log_rows(exe, 0, 1 << 20, ["add 4000000000 0 0 0", "add 4000000000 0 0 0", "add 7 0 0 0", "call 2"])
    assert big[2][:4] == (1, 1 << 33, 8000000007, 3) and big[3]["first"] == "8000000000" and big[3]["count"] == "7"


def test_log_max_bytes_refuses_exactly_at_the_cap(exe):
    cap = 16 * 8199   # one point short of two sweeps of 4100
    rows = log_rows(exe, cap, 1 << 20, ["add 4100 0 0 0", "add 4100 0 0 0", "add 4099 0 0 0", "add 1 0 0 0", "add 0 0 0 0"])
    assert rows == [(1, 8199, 4100, 1, 1),     # the first block is clamped to the cap
                    (0, 8199, 4100, 1, 1),     # one point too many: refused, nothing changes
                    (1, 8199, 8199, 2, 1),     # exactly the cap
                    (0, 8199, 8199, 2, 1),
                    (1, 8199, 8199, 2, 1)]
    # the cap between two doublings: the block grows to the cap, not past it; bytes that are no multiple of 16 round down
    rows = log_rows(exe, 16 * 3000 + 15, 1000, ["add 1500 0 0 0", "add 1500 0 0 0", "add 1 0 0 0"])
    assert rows == [(1, 2000, 1500, 1, 2), (1, 3000, 3000, 2, 3), (0, 3000, 3000, 2, 3)]
    assert run(exe, ["log", 15, 1000]) == ["refused"] and run(exe, ["log", 0, 0]) == ["refused"]
    assert log_rows(exe, 16, 1000, ["add 2 0 0 0", "add 1 0 0 0"]) == [(0, 1, 0, 0, 1), (1, 1, 1, 1, 1)]


def test_call_table(exe):
    f32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]   # noqa: E731
    rows = log_rows(exe, 0, 64, ["add 10 1.5 -2.25 0.1", "add 0 9 9 9", "add 5 -0 3 4", "call 0", "call 1"])
    assert rows[2][:4] == (1, 64, 15, 2)      # the empty call took no index
    assert rows[3] == dict(first="0", count="10", o0=f32(1.5), o1=f32(-2.25), o2=f32(0.1))
    assert rows[4] == dict(first="10", count="5", o0=f32(-0.0), o1=f32(3.0), o2=f32(4.0))


def test_replay_call_record(exe):
    f32 = lambda v: "%08x" % struct.unpack("<I", struct.pack("<f", np.float32(v)))[0]   # noqa: E731
    o = np.float32([1.5, -0.0, 3.25])
    # NULL and a matrix that rounds to the identity: flagged, the origin's bytes kept (-0.0 stays -0.0)
    for extra in ([], [repr(float(v)) for v in (np.float64(rm.IDENTITY) * (1.0 + 2.0 ** -40)).reshape(-1)]):
        r = run(exe, ["replay_call", 77, 5, "1.5", "-0.0", "3.25"] + extra)[0]
        assert r["first"] == "77" and r["identity"] == "1" and [r["o0"], r["o1"], r["o2"]] == [f32(v) for v in o]
        assert [r["m%d" % k] for k in range(12)] == [f32(v) for v in rm.IDENTITY.reshape(-1)]
    c = rm.rigid([0.1, -0.15, 0.05], [0.7, -0.2, 1.1], centre=(3, 4, 5))
    r = run(exe, ["replay_call", 1 << 40, 5, "1.5", "-0.0", "3.25"] + [repr(float(v)) for v in c.reshape(-1)])[0]
    assert r["first"] == str(1 << 40) and r["identity"] == "0"
    assert [r["m%d" % k] for k in range(12)] == [f32(v) for v in rm.rounded(c).reshape(-1)]
    assert [r["o0"], r["o1"], r["o2"]] == [f32(v) for v in rm.correct(c, o)[0]]
    bad = [repr(float(v)) for v in c.reshape(-1)]
    bad[7] = "nan"
    assert run(exe, ["replay_call", 0, 5, "0", "0", "0"] + bad) == ["refused"]


# (initial_slots, voxels before, the words read back after each attempt: occupancy, too small, overflow) -> the slots tried
ATTEMPT_ROWS = [
    # the map of the GPU test: 400 voxels before, 1,200 after.  1024: the kernels stopped somewhere past 512; 2048: past 1024; 4096 holds
    (1024, 400, [(517, 1, 0), (1100, 1, 0), (1200, 0, 0)], [1024, 2048, 4096]),
    # the occupancy exactly at half: 512 voxels in 1024 slots is not a failure
    (1024, 512, [(512, 0, 0)], [1024]),
    # one more before: the first table is already 2048; one more after: 1024 would have failed
    (1024, 513, [(513, 0, 0)], [2048]),
    (1024, 100, [(513, 0, 0), (513, 0, 0)], [1024, 2048]),
    # each sign alone fails the attempt: the exact count (no block saw it in time), the kernels' word, the probe overflow
    (1024, 0, [(600, 0, 0), (700, 1, 0), (2048, 0, 1), (3000, 0, 0)], [1024, 2048, 4096, 8192]),
    # a map that shrinks (prune, then rebuild with the pruned voxels back — or corrections that fold sweeps together): from the
    # voxels before, never below initial_slots
    (4096, 5000, [(900, 0, 0)], [16384]),
    (1 << 20, 3, [(3, 0, 0)], [1 << 20]),
]


@pytest.mark.parametrize("initial,before,words,tried", ATTEMPT_ROWS)
def test_attempt_rule(exe, initial, before, words, tried):
    rows = run(exe, ["attempts", initial, before], "".join("%d %d %d\n" % w for w in words))
    assert [int(r["slots"]) for r in rows] == tried
    assert [int(r["failed"]) for r in rows] == [1] * (len(tried) - 1) + [0]
    assert tried == rm.attempts(initial, before, words[-1][0])


def test_attempts_end_at_two_to_the_31(exe):
    rows = run(exe, ["attempts", 1 << 30, 0], "0 1 0\n0 1 0\n")
    assert rows == [dict(slots=str(1 << 30), failed="1"), dict(slots=str(1 << 31), failed="1"), "refused"]
