"""Python model of the dense map's connected components (include/loamx.h, loamx_densemap_segment and what goes with it), in Python
integers over tests/densemap_model.py (Model) or tests/densemap_carve_model.py (CarveModel, needed for which != ALL): the selection,
the components by a plain breadth-first search over index tuples, their ranks by min_key, the labels in model.keys order and the
records as a numpy array of the SEGMENT dtype.  The checker of tests/test_densemap_segment_cpu.py and tests/test_gpu_densemap_segment.py."""
from collections import deque

import numpy as np

import densemap_carve_model as cm
import densemap_model as dm

NONE = 0xffffffff
ALL, STATIC, DYNAMIC = range(3)
IMAX = 1 << dm.QBITS
LIM = IMAX - 1
SEGMENT = np.dtype([("min_key", "<u8"), ("voxels", "<u8"), ("points", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum_idx", "<i8", 3)])
DEFAULTS = dict(which=ALL, connectivity=26, min_points=1, min_voxels=1, lo=(-LIM,) * 3, hi=(LIM,) * 3)
STAT_KEYS = ("selected", "components", "kept", "kept_voxels", "largest")   # the five exact words of stats


def check(cfg):
    """None when the configuration passes loamx_densemap_segment_check, otherwise the name of the first field that does not"""
    if not 0 <= cfg["which"] <= 2:
        return "which"
    if cfg["connectivity"] not in (6, 18, 26):
        return "connectivity"
    if cfg["min_points"] < 1:
        return "min_points"
    if cfg["min_voxels"] < 1:
        return "min_voxels"
    for a in range(3):
        if not -LIM <= cfg["lo"][a] <= LIM:
            return "lo"
        if not -LIM <= cfg["hi"][a] <= LIM:
            return "hi"
        if cfg["lo"][a] > cfg["hi"][a]:
            return "lo"
    return None


def cell_of(key):
    m = (1 << dm.KBITS) - 1
    return (key & m) - IMAX, ((key >> dm.KBITS) & m) - IMAX, ((key >> (2 * dm.KBITS)) & m) - IMAX


def offsets(connectivity):
    """the non-zero d with every |d_a| <= 1 and |dx| + |dy| + |dz| <= 1, 2 or 3"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if 0 < abs(dx) + abs(dy) + abs(dz) <= most]


def selected_cells(model, which=ALL, min_points=1, lo=DEFAULTS["lo"], hi=DEFAULTS["hi"], rule=None):
    """{cell: n} of the selected voxels"""
    rule = cm.DEFAULT_RULE if rule is None else rule
    out = {}
    for k, n in zip(model.keys.tolist(), model.vals[:, 0].tolist()):
        c = cell_of(k)
        if n < min_points or any(c[a] < lo[a] or c[a] > hi[a] for a in range(3)):
            continue
        if which != ALL and cm.is_dynamic(rule, n, model.miss.get(k, 0)) != (which == DYNAMIC):
            continue
        out[c] = n
    return out


def components(cells, connectivity):
    """the components of a set (or dict) of cells as lists of cells, in no particular order"""
    offs = offsets(connectivity)
    seen, out = set(), []
    for start in cells:
        if start in seen:
            continue
        seen.add(start)
        comp, queue = [], deque([start])
        while queue:
            c = queue.popleft()
            comp.append(c)
            for d in offs:
                nb = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
                if any(abs(v) >= IMAX for v in nb):   # no such voxel
                    continue
                if nb in cells and nb not in seen:
                    seen.add(nb)
                    queue.append(nb)
        out.append(comp)
    return out


def segment(model, rule=None, **cfg):
    """(labels, records, stats): labels uint32 per voxel in model.keys order, records the kept components as SEGMENT records in
    ascending min_key, stats the five exact words of loamx_densemap_segment's stats as a dict"""
    c = dict(DEFAULTS, **cfg)
    assert check(c) is None, check(c)
    sel = selected_cells(model, c["which"], c["min_points"], c["lo"], c["hi"], rule)
    comps = components(sel, c["connectivity"])
    comps.sort(key=lambda comp: min(cm.key_of(v) for v in comp))
    kept = [comp for comp in comps if len(comp) >= c["min_voxels"]]
    rec = np.zeros(len(kept), SEGMENT)
    label_of = {}
    for r, comp in enumerate(kept):
        rec[r]["min_key"] = min(cm.key_of(v) for v in comp)
        rec[r]["voxels"] = len(comp)
        rec[r]["points"] = sum(sel[v] for v in comp)
        for a in range(3):
            rec[r]["lo"][a] = min(v[a] for v in comp)
            rec[r]["hi"][a] = max(v[a] for v in comp)
            rec[r]["sum_idx"][a] = sum(v[a] for v in comp)
        for v in comp:
            label_of[cm.key_of(v)] = r
    labels = np.array([label_of.get(k, NONE) for k in model.keys.tolist()], np.uint32)
    stats = dict(selected=len(sel), components=len(comps), kept=len(kept), kept_voxels=sum(len(comp) for comp in kept),
                 largest=max((len(comp) for comp in comps), default=0))
    return labels, rec, stats


def sizes(model, rule=None, **cfg):
    """the sizes of the components before min_voxels, largest first"""
    c = dict(DEFAULTS, **cfg)
    sel = selected_cells(model, c["which"], c["min_points"], c["lo"], c["hi"], rule)
    return sorted((len(comp) for comp in components(sel, c["connectivity"])), reverse=True)


def segment_box(rec, leaf):
    """loamx_segment_box: (lo_m, hi_m, centre) as float32 triples"""
    leaf = np.float64(np.float32(leaf))
    lo = np.array([np.float32(np.float64(int(rec["lo"][a])) * leaf) for a in range(3)], np.float32)
    hi = np.array([np.float32(np.float64(int(rec["hi"][a]) + 1) * leaf) for a in range(3)], np.float32)
    ce = np.array([np.float32((np.float64(int(rec["sum_idx"][a])) / np.float64(int(rec["voxels"])) + 0.5) * leaf) for a in range(3)], np.float32)
    return lo, hi, ce


def model_of_cells(cells, leaf=0.5, counts=None):
    """a densemap_model.Model holding one voxel per cell, fed with counts[i] (default 1) points at the voxel's centre"""
    m = dm.Model(leaf=leaf)
    m.add(points_of_cells(cells, leaf, counts), (0.0, 0.0, 0.0))
    return m


def points_of_cells(cells, leaf=0.5, counts=None):
    """(n, 4) float32: counts[i] (default 1) points at the centre of cell i.  With leaf 0.5 the centres 0.5 i + 0.25 are exact in f32
    for every |i| < 2^20, and so is their product with 1 / leaf = 2"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    counts = np.ones(len(cells), np.int64) if counts is None else np.asarray(counts, np.int64)
    p = np.zeros((int(counts.sum()), 4), np.float32)
    p[:, :3] = np.repeat((cells.astype(np.float64) + 0.5) * leaf, counts, axis=0)
    assert np.array_equal(np.floor(p[:, :3].astype(np.float64) / leaf), np.repeat(cells, counts, axis=0))
    return p
