"""CPU: WHICH launches a registration run enqueues, and in what order (loam_velodyne_amd/csrc/reg_schedule.hpp — host logic without HIP).

tests/reg_schedule_driver.cpp runs reg_schedule() against a scripted mirror — sweep s is done once need[s] launches have run, the
bucketed voxel stage optionally found to have given up at the first look — and prints the calls: G<it> = Gauss-Newton launch, F<mode> =
full-resolution launch (k_transform_full: 0 every sweep, 1 the sweeps done when it runs, 2 the sweeps no F1 has marked), mark / late /
wait = event record, the caller's hand-off, the wait for the mirrors.  The hand rows were derived from the statements Registrar::
run_iterations held before the schedule became a function of its own; `old_run_iterations` below replays those statements one by one
and knows nothing of the new function.  The one intended difference: a run whose first look finds a sweep not done and whose later look
finds every sweep done used to end without F2 — the clouds of the sweeps that converged in between stayed in the sensor frame."""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("reg_schedule") / "reg_schedule_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"),
                        os.path.join(ROOT, "tests", "reg_schedule_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(scripts):
        """(calls, outcome) of every script"""
        text = "".join(f"{int(s['early'])} {s['maxit']} {s['pred']} {s['ahead']} {int(s['want'])} {int(s['gave_up'])} {','.join(map(str, s['need']))}\n"
                       for s in scripts)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(scripts)
        res = []
        for ln in out:
            tok = ln.split()
            k = next(i for i, t in enumerate(tok) if "=" in t)
            res.append((tok[:k], {t.split("=")[0]: int(t.split("=")[1]) for t in tok[k:]}))
        return res
    return run


def script(pred=4, need=(3,), maxit=10, ahead=1, want=True, early=True, gave_up=False):
    return dict(early=early, maxit=maxit, pred=pred, ahead=ahead, want=want, gave_up=gave_up, need=tuple(need))


def old_run_iterations(early, maxit, pred, ahead, want, gave_up, need):
    """the statements of the parent's Registrar::run_iterations in their order (and of the scripted mirror), HIP calls as tokens"""
    calls = []
    it, looks = 0, 0
    waited = spec_full = all_done = full_enqueued = False
    chunk = min(max(pred + ahead, 2), maxit) if early else maxit
    while it < maxit:
        end = min(maxit, it + chunk)
        while it < end:
            calls.append(f"G{it}")
            it += 1
        if not early:
            break
        if not spec_full and want:
            calls.append("F1")
            spec_full = True
        if it >= maxit:
            break
        calls.append("mark")
        if not waited:
            waited = True
            calls.append("late")
        calls.append("wait")
        looks += 1
        if looks == 1 and gave_up:
            return calls, dict(launched=it, pred=pred, looks=looks, gave_up=1, all_done=0, full=0)
        need_max, all_done = 0, True
        for n in need:
            all_done = all_done and n <= it
            need_max = max(need_max, min(n, it))
        if all_done:
            pred = need_max
            break
        pred = it + 1
        chunk = 1
    if early and want:
        if not spec_full:
            calls.append("F0")
        elif not all_done:
            calls.append("F2")
        full_enqueued = True
    return calls, dict(launched=it, pred=pred, looks=looks, gave_up=0, all_done=int(all_done), full=int(full_enqueued))


def is_item1(s):
    """a later look, not the first, finds every sweep done (looks follow the launches chunk .. maxit - 1)"""
    chunk = min(max(s["pred"] + s["ahead"], 2), s["maxit"])
    return s["early"] and s["want"] and not s["gave_up"] and chunk < max(s["need"]) <= s["maxit"] - 1


def coverage(calls, need):
    """how often each sweep's full-resolution cloud is transformed, by the kernel's rules: F0 every sweep; F1 the sweeps done when it runs,
    which it marks; F2 the sweeps without a mark"""
    ran, cov, marked = 0, [0] * len(need), [False] * len(need)
    for c in calls:
        if c[0] == "G":
            ran += 1
        elif c[0] == "F":
            for k, n in enumerate(need):
                if c == "F0" or (c == "F1" and n <= ran) or (c == "F2" and not marked[k]):
                    cov[k] += 1
                if c == "F1" and n <= ran:
                    marked[k] = True
    return cov


def check_invariants(s, calls, out):
    gs = [int(c[1:]) for c in calls if c[0] == "G"]
    assert gs == list(range(len(gs))) and out["launched"] == len(gs)
    if not out["gave_up"]:
        assert len(gs) >= min(max(s["need"]), s["maxit"])
    assert calls.count("F1") <= 1 and ("F1" not in calls or "wait" not in calls or calls.index("F1") < calls.index("wait"))
    assert calls.count("late") <= 1
    if "late" in calls:
        i = calls.index("late")
        assert calls[i - 1] == "mark" and calls[i + 1] == "wait" and i - 1 == calls.index("mark") and i + 1 == calls.index("wait")
    assert out["looks"] == calls.count("wait") == calls.count("mark")
    if s["early"] and s["want"] and not out["gave_up"]:
        assert coverage(calls, s["need"]) == [1] * len(s["need"]) and out["full"] == 1
    else:   # (a run that gave up is repeated: no closing launch; its F1 found the voxel stage's fail word and did nothing)
        assert not any(c[0] == "F" for c in calls if not (out["gave_up"] and c == "F1")) and out["full"] == 0


G = lambda lo, hi: " ".join(f"G{k}" for k in range(lo, hi))
LOOK1, LOOK = "mark late wait", "mark wait"
TABLE = [
    # script, calls, next pred, all done
    ("done-at-first-look", script(4, (3,)), f"{G(0, 5)} F1 {LOOK1}", 3, 1),
    ("one-more-needed", script(4, (5,)), f"{G(0, 5)} F1 {LOOK1}", 5, 1),
    ("chunk-at-least-2", script(1, (1,)), f"G0 G1 F1 {LOOK1}", 1, 1),
    ("second-sweep-later", script(4, (3, 7)), f"{G(0, 5)} F1 {LOOK1} G5 {LOOK} G6 {LOOK} F2", 7, 1),   # item 1: the old statements give no F2
    ("never-done", script(4, (99,)), f"{G(0, 5)} F1 {LOOK1} G5 {LOOK} G6 {LOOK} G7 {LOOK} G8 {LOOK} G9 F2", 10, 0),
    ("pred-at-bound", script(9, (3,)), f"{G(0, 10)} F1 F2", 9, 0),                                   # early exit lost for good
    ("gave-up", script(4, (3,), gave_up=True), f"{G(0, 5)} F1 {LOOK1}", 4, 0),
    ("early-exit-off", script(4, (3,), early=False), G(0, 10), 4, 0),                                # (the F0 is run_async's)
    ("zero-iterations", script(4, (3,), maxit=0), "F0", 4, 0),
]


@pytest.mark.parametrize("script_,want,pred,all_done", [t[1:] for t in TABLE], ids=[t[0] for t in TABLE])
def test_schedule_table(driver, script_, want, pred, all_done):
    (calls, out), = driver([script_])
    assert " ".join(calls) == want
    assert (out["pred"], out["all_done"], out["gave_up"]) == (pred, all_done, int(script_["gave_up"]))
    assert out["full"] == int(script_["early"] and not script_["gave_up"])
    check_invariants(script_, calls, out)


def test_no_full_resolution_launch_when_not_wanted(driver):
    rows = [t for t in TABLE if t[0] != "zero-iterations"]
    for (_, s, want, pred, all_done), (calls, out) in zip(rows, driver([dict(t[1], want=False) for t in rows])):
        assert " ".join(calls) == " ".join(c for c in want.split() if c[0] != "F") and (out["pred"], out["all_done"], out["full"]) == (pred, all_done, 0)


@pytest.fixture(scope="module")
def exhaustive(driver):
    needs = [(a,) for a in range(1, 13)] + list(itertools.product(range(1, 13), repeat=2))
    scripts = [script(pred, need, maxit, ahead, want, early, gave_up)
               for maxit in range(1, 11) for pred in range(12) for ahead in range(3) for need in needs for want in (True, False)
               for early, gave_up in ((True, False),)]
    scripts += [script(pred, need, maxit, 1, want, early, gave_up) for maxit in (1, 5, 10) for pred in (0, 4, 11) for need in needs for want in (True, False)
                for early, gave_up in ((False, False), (True, True))]
    return scripts, driver(scripts)


def test_every_row_against_the_old_statements(exhaustive):
    differing = 0
    for s, (calls, out) in zip(*exhaustive):
        old_calls, old_out = old_run_iterations(**s)
        if is_item1(s):
            differing += 1
            assert calls == old_calls + ["F2"] and out == old_out, (s, calls, old_calls)
        else:
            assert calls == old_calls and out == old_out, (s, calls, old_calls)
    assert differing > 0


def test_invariants(exhaustive):
    for s, (calls, out) in zip(*exhaustive):
        try:
            check_invariants(s, calls, out)
        except AssertionError as e:
            raise AssertionError(f"{s}: {calls} {out}") from e


def test_the_old_statements_leave_a_cloud_unregistered(exhaustive):
    """the invariants fail against the old replay on exactly the rows of the intended difference — a sweep's cloud covered by no launch —
    and on no other row"""
    for s in exhaustive[0]:
        old_calls, old_out = old_run_iterations(**s)
        if is_item1(s):
            cov = coverage(old_calls, s["need"])
            assert 0 in cov and all(c == 1 for c, n in zip(cov, s["need"]) if n <= min(max(s["pred"] + s["ahead"], 2), s["maxit"])), (s, old_calls, cov)
            with pytest.raises(AssertionError):
                check_invariants(s, old_calls, old_out)
        else:
            check_invariants(s, old_calls, old_out)
