"""CPU: the look-ahead gate of the batched pipeline (loam_velodyne_amd/csrc/odom_lookahead.hpp — standard library only).

The gate decides which odometry chain may run which step, and how the thread that calls Pipeline::step waits for, parks and restarts the
chains' workers and takes a worker's error.  On a GPU it is only reached with whatever timing a run happens to have, and no GPU test makes
a worker fail; tests/odom_lookahead_driver.cpp runs the contract written at the top of the header with plain callables that record
(chain, step) and are gated by atomics, so every interleaving below is forced, and prints one line per scenario.

The second half checks lookahead_window(), the arithmetic of Pipeline::step's three points of release, against old_window() below: the
statements of the step() that had the arithmetic inline, replayed one by one (990 rows), and against rows worked out by hand.

Time limit: the driver's scenarios take ~0.1 s together here (the 1,000 allow / wait rounds: 4-5 ms), ~1.2 s under ThreadSanitizer and
1.7 s with every thread pinned to one core (the rounds: 1.3 s — every hand-over then costs a time slice).  60 s as in
test_helper_thread.py: a lost wake-up hangs for ever, so the margin costs nothing."""
import os
import subprocess

import pytest

from conftest import ROOT

LIMIT_S = 60
SOURCES = ["-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "odom_lookahead_driver.cpp")]
N_LINES = 17


def run_driver(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=LIMIT_S)
    assert out.returncode == 0, out.stderr[-4000:]
    return {ln.split()[0]: dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in out.stdout.splitlines()}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("odom_lookahead") / "odom_lookahead_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + SOURCES + ["-o", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


@pytest.fixture(scope="module")
def lines(exe):
    got = run_driver(exe)
    assert len(got) == N_LINES
    return got


STEPS = ",".join(str(k) for k in range(7))


@pytest.mark.parametrize("depth", [0, 1, 2, 6])
@pytest.mark.parametrize("n_chains", [2, 3])
def test_order_and_bound(lines, n_chains, depth):
    """12 steps, unequal job lengths, the caller allows min(t + depth, last) and waits for t: every chain runs every step once and in order,
    no job starts above the limit, and behind wait(t) the job of step t has ended on every chain and is published"""
    assert lines[f"order_c{n_chains}_d{depth}"] == {"in_order_once": "1", "above_limit": "0", "wait_ok": "1", "drained": "11", "done_max": "11",
                                                    "thread_starts": str(n_chains)}


def test_park_waits_for_the_step_a_worker_is_inside(lines):
    """ADVICE round 3.  Chain 0 is held inside step 2 (published: 1) while the caller parks with restart < 0: park returns only after
    the job has ended, both chains then stand behind step 2, steps 3 and 4 run inline, and after allow(6) no step has run twice"""
    assert lines["park_mid_flight"] == {"done0_inside": "1", "returned_early": "0", "job_ended_at_return": "1", "done0": "2", "done1": "2", "limit": "-1",
                                        "jumped3": "0", "c0": STEPS, "c1": STEPS}


def test_a_jump_moves_only_the_chain_that_is_behind(lines):
    """to step 3 with chain 0 behind step 3 already, chain 1 standing at it and chain 2 at step 1"""
    assert lines["jump"] == {"jumped0_fresh": "0", "jumped3": "1", "jumped1": "0", "jumped4": "1", "done0": "3", "done1": "2", "done2": "2",
                             "jumped3_after": "0", "c0": "4", "c1": "3,4", "c2": "3,4"}


def test_a_failing_step_stops_every_chain_and_is_rethrown_once(lines):
    """chain 1 throws in step 3 while chain 0 is inside step 4 of the 6 allowed: wait(2) returns while the failing job still runs; chain 0
    ends step 4 and starts nothing new; wait(3) rethrows, a second wait does not (step 2 is published, step 3 is "stopped before the
    requested step"); allowed again, chain 1 runs step 3 again — not 4 — and chain 0 repeats nothing"""
    assert lines["failing_step"] == {"wait_published": "ok", "wait_k": "E1", "c0_when_stopped": "0,1,2,3,4", "done0": "4", "done1": "2",
                                     "wait_published_again": "ok", "wait_k_again": "stopped", "wait_end": "ok", "c0": STEPS, "c1": "0,1,2,3,3,4,5,6"}


def test_the_first_of_two_errors_is_reported(lines):
    """chain 1 throws E1 in step 2 once chain 0 is inside its step 2, where chain 0 then throws E0: wait(2) reports E1, E0 is dropped"""
    assert lines["two_failing"] == {"wait_k": "E1", "e0_thrown": "1", "wait_k_again": "stopped", "wait_published": "ok", "done_min": "1", "done_max": "1"}


def test_a_kept_error_comes_out_of_the_first_wait(lines):
    """... also of one for a step that every chain has published, as Pipeline::wait_odometry reported it: an error is never left lying"""
    assert lines["error_first_wait"] == {"wait_published": "E", "wait_again": "ok"}


def test_park_drops_a_kept_error(lines):
    assert lines["park_drops_error"] == {"wait": "ok", "c0": "0,1,2", "c1": "0,1,1,2"}


def test_reset_waits_for_a_running_worker(lines):
    assert lines["reset_running"] == {"returned_early": "0", "job_ended_at_return": "1", "done_min": "-1", "done_max": "-1", "limit": "-1", "jumped0": "0",
                                      "c0_before": "0,1", "c0": "0,1,0,1"}


def test_destructor_joins(lines):
    """workers never started, asleep on the condition variable, in their spin phase, inside a job, and with an error nobody took"""
    assert lines["destructor"] == {"never": "ok", "blocked": "ok", "spinning": "ok", "job_finished": "1", "untaken": "ok"}


def test_no_lost_wake_up_in_1000_rounds(lines):
    """1,000 allow / wait rounds with empty jobs on two chains, inside LIMIT_S (see the module's docstring)"""
    assert lines["rounds"]["n"] == "1000" and lines["rounds"]["ran"] == "2000"
    assert float(lines["rounds"]["ms"]) < 1000.0 * LIMIT_S


def test_clean_under_thread_sanitizer(tmp_path):
    """the same driver, host code on the CPU, built with -fsanitize=thread: no report (a report makes the program exit with 66)"""
    path = str(tmp_path / "odom_lookahead_driver_tsan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=thread"] + SOURCES + ["-o", path],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this g++ cannot build with -fsanitize=thread: " + r.stderr.strip().splitlines()[-1][:200])
    out = subprocess.run([path], capture_output=True, text=True, timeout=4 * LIMIT_S)
    if "FATAL: ThreadSanitizer" in out.stderr:   # (its start-up, e.g. an address-space layout it does not know; a finding is a WARNING)
        pytest.skip("the ThreadSanitizer runtime does not start on this machine: " + out.stderr.strip().splitlines()[0][:200])
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr, out.stderr[-4000:]
    assert len(out.stdout.splitlines()) == N_LINES


# ---- the look-ahead window ----------------------------------------------------------------------------------------------------------

DEPTHS = range(15)
LASTS = (0, 1, 2, 5, 20)


def old_window(t, depth, last_staged, prefetch):
    """Pipeline::step as it was, statement by statement, with launch_upto(k) and allow_odometry(k) recording k instead of acting
    (-1: not called).  `depth` is what depth() returned with the look-ahead on; with it off depth() was 0."""
    rec = {"feat_join": -1, "odom_join": -1, "feat_reg": -1, "odom_reg": -1, "feat_late": -1, "odom_late": -1}

    def launch_upto(name, k):                 # if (k > last_staged) k = last_staged; while (f_hi < k) ...
        rec[name] = min(k, last_staged)

    def allow_odometry(name, k):
        rec[name] = k

    ti = t
    # if (ti > done_min()) {
    launch_upto("feat_join", ti + 1 if prefetch else ti)
    if prefetch:
        allow_odometry("odom_join", min(ti + 1, last_staged))
    # }
    D = depth if prefetch else 0
    FD = max(D, 2)
    if prefetch:
        launch_upto("feat_reg", ti + FD - 1)
        allow_odometry("odom_reg", min(ti + min(D, FD - 1), last_staged))
    f2_pending = prefetch and ti + 2 <= last_staged
    if f2_pending:                            # launch_f2
        launch_upto("feat_late", ti + FD)
        if D >= 2:
            allow_odometry("odom_late", min(ti + D, last_staged))
    return [rec["feat_join"], rec["odom_join"], rec["feat_reg"], rec["odom_reg"], rec["feat_late"], rec["odom_late"], int(f2_pending)]


@pytest.fixture(scope="module")
def window(exe):
    return {k: [int(x) for x in v["v"].split(",")] for k, v in run_driver(exe, "window").items()}


def test_window_equals_the_old_step_for_every_input(window):
    n = 0
    for p in (0, 1):
        for last in LASTS:
            for d in DEPTHS:
                for t in range(last + 1):
                    assert window[f"window_p{p}_l{last}_d{d}_t{t}"] == old_window(t, d, last, bool(p)), (p, last, d, t)
                    n += 1
    assert n == len(window) == 2 * 15 * sum(last + 1 for last in LASTS)


# worked out by hand from the old step(): [features, odometry] before the join, before the registration, in the late release, late?
HAND_ROWS = {
    # depth 6, the default, in the middle of a long run: features one step further than the odometry only in the late release
    (1, 20, 6, 3): [4, 4, 8, 8, 9, 9, 1],
    # ... and within two steps of the end: capped, and no late release behind step last - 1
    (1, 20, 6, 18): [19, 19, 20, 20, 20, 20, 1],
    (1, 20, 6, 19): [20, 20, 20, 20, -1, -1, 0],
    (1, 20, 6, 20): [20, 20, 20, 20, -1, -1, 0],
    # depth 1: features of two steps ahead, odometry of one; the late release launches features only
    (1, 5, 1, 0): [1, 1, 1, 1, 2, -1, 1],
    # depth 0 (not reachable through depth(), which is >= 1 with the look-ahead on): the odometry of t itself before the registration
    (1, 5, 0, 2): [3, 3, 3, 2, 4, -1, 1],
    # depth 2: FD = 2, the late release brings the second step of odometry
    (1, 5, 2, 1): [2, 2, 2, 2, 3, 3, 1],
    # the streaming cap RING - 2 = 6 is depth 6; depth 14 = OR - 2, the largest
    (1, 20, 14, 0): [1, 1, 13, 13, 14, 14, 1],
    (1, 2, 14, 0): [1, 1, 2, 2, 2, 2, 1],
    (1, 1, 3, 0): [1, 1, 1, 1, -1, -1, 0],
    (1, 0, 6, 0): [0, 0, 0, 0, -1, -1, 0],
    # look-ahead off: the step's own features, nothing else, whatever the depth
    (0, 20, 6, 3): [3, -1, -1, -1, -1, -1, 0],
    (0, 0, 0, 0): [0, -1, -1, -1, -1, -1, 0],
}


@pytest.mark.parametrize("key", sorted(HAND_ROWS))
def test_window_rows_by_hand(window, key):
    p, last, d, t = key
    assert window[f"window_p{p}_l{last}_d{d}_t{t}"] == HAND_ROWS[key]
