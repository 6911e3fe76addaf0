"""CPU: the mapper's helper thread (loam_velodyne_amd/csrc/helper_thread.hpp — standard library only) keeps what its jobs throw.

The mapper posts a job per sweep and, since the next sweep waits for the job's FRONT part only, can reach the next post() without a
wait(): an error of the job's tail (the surround cloud) must then come out of that post(), not be overwritten by the next job's normal
end.  No GPU test injects a device fault; tests/helper_thread_driver.cpp runs the contract written at the top of the header with plain
std::function jobs gated by atomics and promises, and prints one line per scenario.

Time limit: the driver's six scenarios take 5-60 ms as a rule (the 2 x 1,000 post rounds: 3-30 ms); one run in ~40 on a small virtual
machine took 1.3 s (both threads on one core: every hand-over then costs a time slice).  60 s is ~50 times that — a lost wake-up hangs
for ever, so the margin costs nothing."""
import os
import subprocess

import pytest

from conftest import ROOT

LIMIT_S = 60
SOURCES = ["-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "helper_thread_driver.cpp")]


def run_driver(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=LIMIT_S)
    assert out.returncode == 0, out.stderr[-4000:]
    return {ln.split()[0]: dict(kv.split("=", 1) for kv in ln.split()[1:]) for ln in out.stdout.splitlines()}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("helper_thread") / "helper_thread_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread"] + SOURCES + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return run_driver(exe)


def test_a_thrown_error_comes_out_of_wait_once(lines):
    assert lines["throw_once"] == {"wait1": "A", "wait2": "ok"}


def test_tail_error_comes_out_of_the_next_post(lines):
    """job A releases its front and throws in its tail; the caller, which saw front_done, posts B without a wait(): post throws A's
    error, B does not run, nothing is left for wait(), and the post after that is accepted"""
    assert lines["tail_error"] == {"front_failed": "0", "post_b": "A", "b_ran": "0", "wait_b": "ok", "post_c": "ok", "c_ran": "1", "wait_c": "ok"}


def test_an_error_is_taken_exactly_once(lines):
    assert lines["taken_once"] == {"post1": "A", "post2": "ok", "wait1": "B", "wait2": "ok"}


def test_a_front_that_throws_releases_the_front(lines):
    assert lines["front_throws"] == {"front_failed": "1", "front_done": "1", "wait": "F"}


def test_destructor_joins(lines):
    """with a job still running, with no job ever posted, and with an error nobody took"""
    assert lines["destructor"] == {"job_finished": "1", "idle": "ok", "untaken": "ok"}


def test_no_lost_wake_up_in_1000_rounds(lines):
    """1,000 post / wait rounds and 1,000 posts back to back with an empty job, inside LIMIT_S (see the module's docstring)"""
    assert lines["rounds"]["n"] == "1000" and lines["rounds"]["ran"] == "2000"
    assert float(lines["rounds"]["ms"]) < 1000.0 * LIMIT_S


def test_clean_under_thread_sanitizer(tmp_path):
    """the same driver, host code on the CPU, built with -fsanitize=thread: no report (a report makes the program exit with 66)"""
    exe = str(tmp_path / "helper_thread_driver_tsan")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=thread"] + SOURCES + ["-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("this g++ cannot build with -fsanitize=thread: " + r.stderr.strip().splitlines()[-1][:200])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=4 * LIMIT_S)
    if "FATAL: ThreadSanitizer" in out.stderr:   # (its start-up, e.g. an address-space layout it does not know; a finding is a WARNING)
        pytest.skip("the ThreadSanitizer runtime does not start on this machine: " + out.stderr.strip().splitlines()[0][:200])
    assert out.returncode == 0 and "ThreadSanitizer" not in out.stderr, out.stderr[-4000:]
    assert len(out.stdout.splitlines()) == 6
