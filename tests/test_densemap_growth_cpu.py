"""CPU: the dense map's growth and capacity rule (loam_velodyne_amd/csrc/densemap_growth.hpp — standard library only), under UBSan.

The rule keeps the table's load at one half or less, which bounds every probe loop on the device and keeps the overflow flag from ever
being set.  It is arithmetic between HIP calls, and no GPU test can force its interleavings (a snapshot that lands between two adds, one
that a wait abandons, a bound exactly at half the table).  tests/densemap_growth_driver.cpp uses the header the way DenseMap does, with
the HIP calls left out, and prints one line per event (replay) or per scenario (the simulated device).

Old below is DenseMap as it was when the arithmetic stood inline in admit, poll_snapshot, grow_for, enqueue_add, wait_adds, read_counters,
merge and reset: its statements one by one.  The replay holds the header to it after every event of seeded scripts; the rows worked out
by hand hold both to the rule itself."""
import os
import random
import subprocess

import pytest

from conftest import ROOT

SOURCES = ["-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "densemap_growth_driver.cpp")]
FIELDS = ("occ", "pend", "pend_snap", "snap_pending", "slots", "want", "start", "by_bound", "admitted", "refused")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("densemap_growth") / "densemap_growth_driver")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all"] + SOURCES + ["-o", path],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return path


def replay(exe, slots, max_voxels, events):
    """the driver's state after every event, as tuples in the order of FIELDS"""
    text = "".join(" ".join(str(x) for x in e) + "\n" for e in events)
    r = subprocess.run([exe, "replay", str(slots), str(max_voxels)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    rows = [dict(kv.split("=") for kv in ln.split()) for ln in r.stdout.splitlines()]
    assert len(rows) == len(events)
    return [tuple(int(row[f]) for f in FIELDS) for row in rows]


class Old:
    """DenseMap's occupancy fields and the statements that touched them, as they were; a HIP call is left out or replaced by the value
    the script gives for what it would have returned.  want, start, by_bound, admitted, refused record what an event decided (-1: not asked)"""

    def __init__(self, slots, max_voxels):
        self.occ_ = self.pend_ = self.pend_snap_ = 0
        self.snap_pending_ = False
        self.slots_ = slots
        self.max_voxels = max_voxels

    def begin_event(self):
        self.want, self.start, self.by_bound, self.admitted, self.refused = -1, -1, -1, -1, 0

    def wait_adds(self):
        self.snap_pending_ = False

    def read_counters(self, v):
        self.wait_adds()
        self.occ_ = v                      # occ_ = c[0]
        self.pend_ = self.pend_snap_ = 0

    def poll_snapshot(self, v):            # (the event has completed)
        if not self.snap_pending_:
            return
        self.occ_ = v
        self.pend_ = self.pend_snap_
        self.snap_pending_ = False

    def admit(self, n, v):
        if not self.max_voxels:
            self.by_bound = 1
            return True
        if self.occ_ + self.pend_ + n <= self.max_voxels:
            self.by_bound = 1
            return True
        self.by_bound = 0
        self.read_counters(v)
        return self.occ_ + n <= self.max_voxels

    def grow_for(self, n):
        want = self.slots_
        while self.occ_ + self.pend_ + n > want // 2:
            want *= 2
        self.want = want
        if not want <= (1 << 31):          # LX_REQUIRE(want <= (1ull << 31), ...)
            self.refused = 1
            return False
        if want != self.slots_:
            self.slots_ = want
        return True

    def add(self, n, v):                   # DenseMap::add, then enqueue_add
        self.admitted = int(self.admit(n, v))
        if not self.admitted:
            return
        if not self.grow_for(n):
            return
        self.pend_ += n
        if self.snap_pending_:
            self.pend_snap_ += n
            self.start = 0
        else:
            self.start = 1                 # store_to_pinned_u32, hipEventRecord(ev_snap_)
            self.snap_pending_ = True
            self.pend_snap_ = 0

    def merge(self, s_occ, v, v2):         # merge, then merge_records
        self.read_counters(v)
        self.admitted = int(not (self.max_voxels and self.occ_ + s_occ > self.max_voxels))
        if not self.admitted:
            return
        if not self.grow_for(s_occ):
            return
        self.read_counters(v2)

    def reset(self):
        self.wait_adds()
        self.occ_ = self.pend_ = self.pend_snap_ = 0

    def size(self, slots, n):              # merge_file's target (slots = initial_slots) and DmFrozen::build's (slots = 1024)
        target = slots
        while target < 2 * n:
            target *= 2
        self.want = target

    def run(self, events):
        out = []
        for e in events:
            self.begin_event()
            {"add": self.add, "land": self.poll_snapshot, "wait": self.wait_adds, "read": self.read_counters, "merge": self.merge,
             "size": self.size, "reset": self.reset}[e[0]](*e[1:])
            out.append((self.occ_, self.pend_, self.pend_snap_, int(self.snap_pending_), self.slots_, self.want, self.start, self.by_bound,
                        self.admitted, self.refused))
        return out


def script(seed, n_events, max_voxels):
    """a seeded script; the values a read returns stay at or below the bound, as a device's would, but are otherwise free"""
    rng = random.Random(seed)
    model = Old(1024, max_voxels)
    events = []
    for _ in range(n_events):
        bound = model.occ_ + model.pend_
        r = rng.random()
        if r < 0.55:
            n = rng.choice([0, 1, rng.randrange(4000), rng.randrange(200000), max(0, model.slots_ // 2 - bound), max(0, model.slots_ // 2 - bound) + 1])
            e = ("add", n, rng.randint(0, bound))
        elif r < 0.75:
            e = ("land", rng.randint(0, bound))
        elif r < 0.80:
            e = ("wait",)
        elif r < 0.88:
            e = ("read", rng.randint(0, bound))
        elif r < 0.94:
            s_occ, v = rng.randrange(300000), rng.randint(0, bound)
            e = ("merge", s_occ, v, rng.randint(v, v + s_occ))
        elif r < 0.98:
            e = ("size", 1 << rng.randrange(10, 21), rng.randrange(3000000))
        else:
            e = ("reset",)
        events.append(e)
        model.run([e])
    return events


@pytest.mark.parametrize("seed,max_voxels", [(1, 0), (2, 0), (3, 50000), (4, 400000)])
def test_replay_equals_the_former_statements_after_every_event(exe, seed, max_voxels):
    events = script(seed, 3000, max_voxels)
    got, want = replay(exe, 1024, max_voxels, events), Old(1024, max_voxels).run(events)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, events[k], dict(zip(FIELDS, g)), dict(zip(FIELDS, w)))
    kinds = {e[0] for e in events}
    assert kinds == {"add", "land", "wait", "read", "merge", "size", "reset"}
    assert any(w[6] == 0 for w in want) and any(w[6] == 1 for w in want) and want[-1][4] > 1024      # adds behind a snapshot, adds that start one, growth
    if max_voxels:
        assert any(w[7] == 0 and w[8] == 1 for w in want) and any(w[8] == 0 for w in want)          # exact reads that admit, refusals


def test_the_load_stays_at_half_or_below_and_the_bound_never_below_the_truth(exe):
    """the simulated device: every point a new voxel, every point the same voxel, a seeded mix; snapshots land late or are abandoned"""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    rows = {ln.split()[0]: {k: int(v) for k, v in (kv.split("=") for kv in ln.split()[1:])} for ln in r.stdout.splitlines()}
    assert sorted(rows) == ["every_point_new", "every_point_same", "mixed"]
    for name, row in rows.items():
        assert row["over_half"] == 0 and row["bound_below_truth"] == 0, (name, row)
        assert row["max_load_x1000"] <= 500 and row["adds"] > 3000 and row["landed"] > 100 and row["abandoned"] > 100 and row["exact_reads"] > 100, (name, row)
    assert rows["every_point_new"]["max_load_x1000"] > 250 and rows["every_point_new"]["grows"] >= 10   # (the bound is tight there: growth when needed)
    assert rows["every_point_same"]["truth"] == 1 and rows["mixed"]["grows"] >= 8


# ---- rows worked out by hand: (slots, max_voxels, events, the fields to look at, their values after the last event) -----------------

HAND = {
    "an add of 0 points starts a snapshot and needs no growth":
        (1024, 0, [("add", 0, 0)], ("pend", "snap_pending", "slots", "want", "start", "admitted"), (0, 1, 1024, 1024, 1, 1)),
    "a second add behind that snapshot starts none and is counted behind it":
        (1024, 0, [("add", 0, 0), ("add", 7, 0)], ("pend", "pend_snap", "snap_pending", "start"), (7, 7, 1, 0)),
    "the snapshot lands: what was enqueued behind it stays pending":
        (1024, 0, [("add", 5, 0), ("add", 7, 0), ("land", 4)], ("occ", "pend", "pend_snap", "snap_pending"), (4, 7, 7, 0)),
    "an abandoned snapshot leaves the bound where it was, and its late value is not taken":
        (1024, 0, [("add", 5, 0), ("add", 7, 0), ("wait",), ("land", 4)], ("occ", "pend", "snap_pending"), (0, 12, 0)),
    "a bound exactly at half the table gives no growth":
        (1024, 0, [("read", 500), ("add", 12, 0)], ("occ", "pend", "slots", "want"), (500, 12, 1024, 1024)),
    "and one more record doubles it":
        (1024, 0, [("read", 500), ("add", 12, 0), ("add", 1, 0)], ("occ", "pend", "slots", "want"), (500, 13, 2048, 2048)),
    "one call that needs three doublings (4096 / 2 < 3000 <= 8192 / 2)":
        (1024, 0, [("add", 3000, 0)], ("slots", "want", "refused"), (8192, 8192, 0)),
    "a merge grows by the source's voxels on top of the exact count":
        (1024, 0, [("merge", 600, 10, 610)], ("occ", "pend", "slots", "want", "admitted"), (610, 0, 2048, 2048, 1)),
    "2^30 voxels and one more would need 2^32 slots: reported, not clamped, nothing changed":
        (1024, 0, [("read", 1 << 30), ("add", 1, 0)], ("occ", "pend", "snap_pending", "slots", "want", "refused"), (1 << 30, 0, 0, 1024, 1 << 32, 1)),
    "2^30 voxels fit the largest table, 2^31 slots":
        (1024, 0, [("read", (1 << 30) - 1), ("add", 1, 0)], ("slots", "want", "refused"), (1 << 31, 1 << 31, 0)),
    "max_voxels: exactly at the cap the add is admitted without an exact read":
        (1024, 1000, [("read", 800), ("add", 100, 0), ("add", 100, 850)], ("occ", "pend", "by_bound", "admitted"), (800, 200, 1, 1)),
    "max_voxels: one above the cap the exact count is read, and admits":
        (1024, 1000, [("read", 800), ("add", 100, 0), ("add", 101, 899)], ("occ", "pend", "by_bound", "admitted"), (899, 101, 0, 1)),
    "max_voxels: one above the cap the exact count is read, and refuses":
        (1024, 1000, [("read", 800), ("add", 100, 0), ("add", 101, 900)], ("occ", "pend", "snap_pending", "by_bound", "admitted", "start"),
         (900, 0, 0, 0, 0, -1)),
    "max_voxels: a merge is decided on the exact count":
        (1024, 1000, [("merge", 500, 501, 0)], ("occ", "slots", "admitted"), (501, 1024, 0)),
    "load sizing from initial_slots, n = 0": (1024, 0, [("size", 1024, 0)], ("want",), (1024,)),
    "load sizing from initial_slots, n = initial_slots / 2": (1024, 0, [("size", 1024, 512)], ("want",), (1024,)),
    "load sizing from initial_slots, n = initial_slots / 2 + 1": (1024, 0, [("size", 1024, 513)], ("want",), (2048,)),
    "load sizing of a million voxels from 2^20 slots": (1024, 0, [("size", 1 << 20, 1000000)], ("want",), (1 << 21,)),
    "reset clears the bound": (1024, 0, [("add", 3000, 0), ("reset",)], ("occ", "pend", "pend_snap", "snap_pending", "slots"), (0, 0, 0, 0, 8192)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_rows_by_hand(exe, name):
    slots, max_voxels, events, fields, values = HAND[name]
    for last in (replay(exe, slots, max_voxels, events)[-1], Old(slots, max_voxels).run(events)[-1]):
        assert tuple(dict(zip(FIELDS, last))[f] for f in fields) == values


def test_the_header_needs_no_hip():
    src = open(os.path.join(ROOT, "loam_velodyne_amd", "csrc", "densemap_growth.hpp")).read()
    assert "hip/" not in src and '#include "' not in src
