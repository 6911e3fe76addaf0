"""CPU: WHICH launches an odometry pass enqueues, and in what order (loam_velodyne_amd/csrc/odom_schedule.hpp — host logic without HIP).

The GPU suite pins that the launch-pair policy changes no result (test_launch_pairs_as_needed_change_nothing); this pins the policy
itself.  tests/odom_schedule_driver.cpp runs odom_schedule_pairs() against a scripted mirror — every stream converged once pair N - 1
has run, optionally silent from pair B on — and prints the calls.  The expected sequences were derived by hand from the two loops
OdometryBatch::process held before the schedule became a function of its own (C_k / L_k = correspondence / iteration launch of pair k,
late = the hook behind the first launches)."""
import os
import subprocess

import pytest

from conftest import ROOT

MODES = ("all", "lag", "exact", "lag2")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("odom_schedule") / "odom_schedule_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"),
                        os.path.join(ROOT, "tests", "odom_schedule_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*scripts):
        """(calls, return value) of every script (mode, maxp, pred, n, silent)"""
        out = subprocess.run([exe] + [str(v) for sc in scripts for v in sc], capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(scripts) and all(ln.split()[-1].startswith("ret=") for ln in out)
        return [(ln.split()[:-1], int(ln.split()[-1][4:])) for ln in out]
    return run


def script(mode, maxp=5, pred=5, n=5, silent=-1):
    return (mode, maxp, pred, n, silent)


def launches(calls):
    """the calls without the waits and the convergence tests"""
    return " ".join(c for c in calls if c[0] in "CL" or c == "late")


def pairs(lo, hi):
    return " ".join(f"C{k} L{k}" for k in range(lo, hi))


TABLE = [
    # mode, script, launches in order, pairs whose iterations were enqueued
    ("lag", dict(n=1), "C0 L0 C1 late", 1),
    ("lag", dict(n=3), "C0 L0 C1 late L1 C2 L2 C3", 3),
    ("lag", dict(n=5), "C0 L0 C1 late L1 C2 L2 C3 L3 C4 L4", 5),
    ("lag", dict(n=9), "C0 L0 C1 late L1 C2 L2 C3 L3 C4 L4", 5),          # never converges before the iteration bound
    ("lag", dict(n=5, maxp=1), "C0 L0 late", 1),
    ("lag", dict(n=5, silent=0), "C0 L0 C1 late L1 C2 L2 C3 L3 C4 L4", 5),
    ("lag2", dict(n=1), "C0 L0 C1 L1 late", 2),
    ("lag2", dict(n=3), "C0 L0 C1 L1 late C2 L2 C3 L3", 4),
    ("lag2", dict(n=5, silent=0), pairs(0, 2) + " late " + pairs(2, 5), 5),
    ("exact", dict(pred=1, n=3), "C0 L0 late C1 L1 C2 L2", 3),
    ("exact", dict(pred=4, n=2), pairs(0, 4) + " late", 4),
    ("exact", dict(pred=0, n=3), "C0 L0 late C1 L1 C2 L2", 3),
    ("exact", dict(pred=9, n=1), pairs(0, 5) + " late", 5),                # (the prediction is capped by the iteration bound)
    ("exact", dict(pred=1, n=5, silent=0), "C0 L0 late " + pairs(1, 5), 5),
    ("all", dict(n=1), pairs(0, 5) + " late", 5),
    ("all", dict(n=5), pairs(0, 5) + " late", 5),
]


@pytest.mark.parametrize("mode,script_,want,want_ret", TABLE, ids=[f"{m}-" + "-".join(f"{k}{v}" for k, v in s.items()) for m, s, _, _ in TABLE])
def test_schedule_table(driver, mode, script_, want, want_ret):
    (calls, ret), = driver(script(mode, **script_))
    assert launches(calls) == want, calls
    assert ret == want_ret
    assert not any(c.startswith("STUCK") for c in calls), calls
    if script_.get("silent", -1) >= 0:   # one copy of the blind fall-back: a single unanswered wait, then no look at the mirror at all
        assert [c for c in calls if c[0] == "W"] == ["W0!"] and not any(c.startswith("conv") for c in calls), calls


@pytest.mark.parametrize("mode", MODES)
def test_no_needed_launch_is_missing(driver, mode):
    """every mode, N and iteration bound, with and without a mirror that falls silent: L_k is enqueued for every k < min(N, maxp), each
    launch at most once, C_k before L_k, k ascending, the hook exactly once, and no wait for a pair that was never enqueued"""
    scripts = [script(mode, maxp, pred, n, silent) for maxp in range(1, 6) for n in range(1, 6) for pred in (0, 1, 3, 5) for silent in (-1, 0, 1, 3)]
    for (_, maxp, pred, n, silent), (calls, ret) in zip(scripts, driver(*scripts)):
        what = (mode, maxp, n, pred, silent, calls)
        ls = [int(c[1:]) for c in calls if c[0] == "L"]
        cs = [int(c[1:]) for c in calls if c[0] == "C"]
        assert ls == list(range(len(ls))) and cs == list(range(len(cs))), what
        assert min(n, maxp) <= len(ls) <= maxp and len(ls) <= len(cs) <= min(len(ls) + 1, maxp), what
        assert all(calls.index(f"C{k}") < calls.index(f"L{k}") for k in ls), what
        assert calls.count("late") == 1 and ret == len(ls), what
        assert not any(c.startswith("STUCK") for c in calls), what
        unanswered = [i for i, c in enumerate(calls) if c.endswith("!")]
        if unanswered:   # blind from the first unanswered wait on: everything that is left, without another look
            assert len(unanswered) == 1 and len(ls) == maxp, what
            assert not any(c[0] == "W" or c.startswith("conv") for c in calls[unanswered[0] + 1:]), what


def test_launches_ahead_of_need(driver):
    """what the modes are for: launches behind the last needed one (L_N-1) — `exact` none when its prediction is not too high, `lag` at
    most one (a correspondence launch), `lag2` at most one pair"""
    for n in range(1, 6):
        extra = {m: len(launches(calls).replace(" late", "").split()) - 2 * n for m, (calls, _) in zip(MODES, driver(*[script(m, pred=1, n=n) for m in MODES]))}
        assert extra["exact"] == 0 and extra["lag"] == min(1, 2 * (5 - n)) and extra["lag2"] == min(2, 2 * (5 - n)) and extra["all"] == 2 * (5 - n), (n, extra)
