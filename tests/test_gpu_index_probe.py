"""GPU: the counting-sorted grid index on its own (csrc/submap_index.hip: SubMapIndex and SubMapIndexBatch through loamx_index_probe)
against the numpy model of tests/submap_index_model.py — every comparison on words, no tolerance.  tests/index_cases.py builds the
cases and tests/test_index_cases_cpu.py proves that each one reaches the path it claims: sizes around the wave and the workgroup, cell
runs cut at lane 0 / 63, points on cell faces, signed zeros, grids that grow (single: a 3 000 m cube, a 5 000 m slab; batch: K = 64,
65, 4096; one 1e6 m cube, the largest extent any test shows the device), K = 1 .. 4096 through the fused and the unfused set-up, empty
clouds and all-empty builds, ring bytes 0 / 254 / 255 / 300 / -1 / 3.7, bounds folded by a producer kernel, and sequences of builds on
the process's one single index and one batch index.  A cloud of more than 2^24 points (pack_ring's other fallback) is left out: too
large for a test of a few seconds.

Checked for every build: the descriptors word for word; independently of the model inv_h <= 1 / cell_edge, ncell == nx * ny * nz <=
budget, one growth step fewer would not have fitted, origin == the cloud's minimum; the table does not decrease, cloud c's cells cover
exactly [off[c], off[c + 1]), the last entry is n; every slot of cell j holds a point of the right cloud whose model cell is j, with
the xyz words of the input point its .w names, the .w indices of a cloud a permutation, the ring byte as specified.  The order of the
slots inside a cell comes from atomics: cells are compared as sets."""
import numpy as np
import pytest

import index_cases as ic
import submap_index_model as sm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

_MODEL = {}


def _model(case):
    key = case.name[:-5] if case.flags & ic.FOLD else case.name
    if key not in _MODEL:
        _MODEL[key] = sm.build(case.pts, case.off, case.cell, case.flags)
    return _MODEL[key]


def _fits(mn, mx, h, budget):
    """does the table fit at edge h — exact integers from the float quotients"""
    q = np.floor((mx - mn) * (np.float32(1.0) / np.float32(h)))
    return int(q[0] + 1) * int(q[1] + 1) * int(q[2] + 1) <= budget


def compare(case, where=None):
    where = where or case.name
    got = loamx.index_probe(case.pts, case.off, case.cell, case.flags)
    m = _model(case)
    K, n, off = case.K, case.n, case.off.astype(np.int64)
    d, table, out = got["desc"], got["table"].astype(np.int64), got["sorted"]
    single = bool(case.flags & ic.SINGLE)
    budget = sm.budget_of(K, single)
    # ---- descriptors: word for word, then on their own terms
    a, b = d.view(np.uint32).reshape(K, 10), m["desc"].view(np.uint32).reshape(K, 10)
    if not np.array_equal(a, b):
        c = int(np.flatnonzero((a != b).any(axis=1))[0])
        raise AssertionError(f"{where}: descriptor of cloud {c} differs: {d[c]} != {m['desc'][c]}")
    lens = np.diff(off)
    for c in (range(K) if K <= 64 else np.linspace(0, K - 1, 64).astype(int)):
        g = d[c]
        assert int(g["ncell"]) == int(g["nx"]) * int(g["ny"]) * int(g["nz"]) <= budget and min(g["nx"], g["ny"], g["nz"]) >= 1, f"{where}: cloud {c}: {g}"
        assert g["pt_base"] == off[c], f"{where}: cloud {c}: pt_base"
        if lens[c]:
            P = case.pts[off[c]:off[c + 1], :3]
            mn, mx = P.min(axis=0), P.max(axis=0)
            assert g["inv_h"] <= np.float32(1.0) / np.float32(case.cell), f"{where}: cloud {c}: cell edge below the initial one"
            assert (np.array([g["ox"], g["oy"], g["oz"]], np.float32) == mn).all(), f"{where}: cloud {c}: origin is not the minimum"
            h, prev = np.float32(case.cell), None
            while np.float32(1.0) / h != g["inv_h"]:
                prev, h = h, np.float32(h * np.float32(1.25))
                assert h < 1e9, f"{where}: cloud {c}: inv_h {g['inv_h']} is no 1 / (cell * 1.25^k)"
            assert _fits(mn, mx, h, budget) and (prev is None or not _fits(mn, mx, prev, budget)), f"{where}: cloud {c}: not the first edge that fits"
    # ---- the table
    total = int(d["cell_base"][-1]) + int(d["ncell"][-1])
    assert len(table) == total + 1, f"{where}: table length {len(table)} != {total + 1}"
    assert np.array_equal(d["cell_base"].astype(np.int64), np.concatenate([[0], np.cumsum(d["ncell"].astype(np.int64))[:-1]])), f"{where}: cell_base is not the scan of ncell"
    if (np.diff(table) < 0).any():
        j = int(np.flatnonzero(np.diff(table) < 0)[0])
        raise AssertionError(f"{where}: the table decreases at entry {j}: {table[j]} > {table[j + 1]}")
    assert table[-1] == n, f"{where}: last table entry {table[-1]} != n = {n}"
    base = d["cell_base"].astype(np.int64)
    if not np.array_equal(table[base], off[:-1]):
        c = int(np.flatnonzero(table[base] != off[:-1])[0])
        raise AssertionError(f"{where}: cloud {c}: its first cell starts at slot {table[base[c]]}, not at off = {off[c]}")
    if not np.array_equal(table, m["table"].astype(np.int64)):
        j = int(np.flatnonzero(table != m["table"])[0])
        c = int(np.searchsorted(base, j, side="right") - 1)
        raise AssertionError(f"{where}: table differs first at entry {j} (cloud {c}, its cell {j - base[c]}): {table[j]} != {m['table'][j]}")
    if n == 0:
        return got
    # ---- every slot
    slot = np.arange(n)
    cell_of_slot = np.searchsorted(table, slot, side="right") - 1
    cloud_of_slot = sm.cloud_of(off, n)          # (slots of cloud c are [off[c], off[c + 1]): checked above)
    w = out[:, 3].view(np.uint32)
    li = (w & 0xffffff).astype(np.int64) if case.flags & ic.PACK_RING else w.astype(np.int64)

    def fail(mask, what):
        s = int(np.flatnonzero(mask)[0])
        c, j = int(cloud_of_slot[s]), int(cell_of_slot[s])
        raise AssertionError(f"{where}: {int(mask.sum())} slots: {what}; first slot {s} (cloud {c}, its cell {j - base[c]}): {out[s, :3]} .w = {w[s]:#x}")
    if (li >= lens[cloud_of_slot]).any():
        fail(li >= lens[cloud_of_slot], ".w names an index beyond its cloud")
    src = off[cloud_of_slot] + li
    if (out[:, :3].view(np.uint32) != case.pts[src, :3].view(np.uint32)).any():
        fail((out[:, :3].view(np.uint32) != case.pts[src, :3].view(np.uint32)).any(axis=1), "xyz is not the input point .w names")
    if len(np.unique(src)) != n:
        dup = np.zeros(n, bool)
        dup[np.argsort(src, kind="stable")[1:][np.diff(np.sort(src)) == 0]] = True
        fail(dup, "an input point appears twice (the .w of a cloud are no permutation)")
    if (m["cell"][src] != cell_of_slot).any():
        fail(m["cell"][src] != cell_of_slot, "the point's cell is another one")
    if (w != m["w"][src]).any():
        fail(w != m["w"][src], ".w is not the packed word specified")
    return got


_by_name = lambda cases: pytest.mark.parametrize("case", cases, ids=lambda c: c.name)


@_by_name(ic.group(["single_n", "batch_n", "batch_cloud8193"]))
def test_sizes(case):
    compare(case)


@_by_name([c for c in ic.pattern_cases()])
def test_cell_patterns(case):
    compare(case)


@_by_name(ic.geometry_cases())
def test_geometry(case):
    compare(case)


@_by_name(ic.growth_cases())
def test_growth(case):
    got = compare(case)
    assert got["desc"]["inv_h"].min() < np.float32(1.0) / np.float32(case.cell)


@pytest.mark.parametrize("K", ic.KS)
def test_cloud_counts(K):
    for case in ic.group([f"K{K}_"]):
        compare(case)


@_by_name(ic.group(["empty_", "one_point_", "short_clouds", "boundaries_"]))
def test_empty_clouds_and_boundaries(case):
    got = compare(case)
    if case.n == 0:
        assert not got["table"].any() and len(got["table"]) == case.K + 1


@_by_name(ic.ring_cases())
def test_ring_bytes(case):
    got = compare(case)
    if case.flags & ic.PACK_RING:
        w = got["sorted"][:, 3].view(np.uint32)
        src = case.off[sm.cloud_of(case.off, case.n)].astype(np.int64) + (w & 0xffffff)
        assert np.array_equal(w >> 24, np.array(ic.RING_BYTES, np.uint32)[src % 6])


@pytest.mark.parametrize("name", list(ic.sequences()))
def test_sequences_on_the_one_object(name):
    """the process's index objects, build after build: the cell counters the scan clears behind itself, the bounds accumulators the
    scatter or k_bb_setup resets, the accumulators regrown when K grows — every build of the sequence must equal the model"""
    for step, case in enumerate(ic.sequences()[name]):
        compare(case, f"{name} step {step} ({case.name})")


def test_invalid_arguments_are_refused():
    p = np.zeros((4, 4), np.float32)
    bad = [dict(off=[0, 3, 2, 4]),                                  # offsets that decrease
           dict(off=[0, 2, 3]),                                     # offsets that do not end at n
           dict(off=np.concatenate([np.zeros(4097), [4]])),         # K = 4097
           dict(off=[0, 4], cell_edge=0.2), dict(off=[0, 4], cell_edge=16.5), dict(off=[0, 4], cell_edge=float("nan")),
           dict(off=[0, 4], flags=8),
           dict(off=[0, 2, 4], flags=loamx.INDEX_SINGLE), dict(off=[0, 4], cell_edge=2.1, flags=loamx.INDEX_SINGLE),
           dict(off=[0, 4], flags=loamx.INDEX_SINGLE | loamx.INDEX_PACK_RING)]
    for kw in bad:
        with pytest.raises(loamx.LoamxError) as e:
            loamx.index_probe(p, **kw)
        assert e.value.code == loamx.E_INVALID, kw
    for v in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[2, 1] = v
        with pytest.raises(loamx.LoamxError) as e:
            loamx.index_probe(q, [0, 4])
        assert e.value.code == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.index_probe(np.zeros((0, 4), np.float32), [0, 0], flags=loamx.INDEX_SINGLE)   # the single index skips an empty build
    assert e.value.code == loamx.E_INVALID
