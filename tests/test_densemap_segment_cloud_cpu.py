"""CPU: the objects of a sweep that is not in the map (include/loamx.h, loamx_densemap_segment_cloud ... loamx_segments_match) — every
new symbol declared and exported, the header as C99 and C++11, the configuration's layout and defaults, every bound of the check,
loamx_segments_match against its model on hand-made records; and the model the GPU tests check the device against
(tests/densemap_segment_cloud_model.py), checked here against an independent brute force (a union-find over a dense array that uses
none of the model's functions) and for its own invariants."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_model as dm
import densemap_segment_cloud_model as scm
import densemap_segment_model as sm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_segment_cloud_default_config", "loamx_densemap_segment_cloud_check", "loamx_densemap_segment_cloud",
               "loamx_densemap_segment_cloud_from_map", "loamx_densemap_segment_cloud_from_pipeline", "loamx_segments_match")
LEAF = 0.5
LIM = 2 ** 20 - 1


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_segment_cloud_config;" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for k, name in enumerate(("ALL", "NEW", "KNOWN")):
        assert f"#define LOAMX_CLOUD_{name} {k}u" in hdr and getattr(loamx, "CLOUD_" + name) == getattr(scm, name) == k
    for name in ("segment_cloud", "segment_cloud_from", "segment_cloud_from_pipeline"):
        assert callable(getattr(loamx.DenseMap, name))
    assert callable(loamx.segments_match) and callable(loamx.SegmentCloudConfig)
    assert loamx.SEGMENT_CLOUD_STATS[:12] == scm.STAT_KEYS and len(loamx.SEGMENT_CLOUD_STATS) == 13


def test_header_compiles_as_c99_and_cxx11(tmp_path):
    body = ('#include "loamx.h"\nint main(void) { loamx_densemap_segment_cloud_config c; loamx_densemap_segment_cloud_default_config(&c);\n'
            '  return loamx_segments_match(0, 0, 0, 0, 0u, 0) + (int)c.which - LOAMX_CLOUD_NEW; }\n')
    for cc, std, ext in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "cpp")):
        probe = tmp_path / ("probe." + ext)
        probe.write_text(body)
        subprocess.run([cc, std, "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(probe)], check=True)


def test_struct_layout_matches_c(tmp_path):
    struct = loamx.SegmentCloudConfig
    fields = [f for f, _ in struct._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     '  printf("%zu\\n", sizeof(loamx_densemap_segment_cloud_config));\n' +
                     "".join(f'  printf("%zu\\n", offsetof(loamx_densemap_segment_cloud_config, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(struct) == 48 and fields == list(scm.DEFAULTS)
    assert got[1:] == [getattr(struct, f).offset for f in fields]


def as_dict(c):
    return {f: (tuple(getattr(c, f)) if f in ("lo", "hi") else getattr(c, f)) for f, _ in c._fields_}


def test_defaults():
    c = loamx.SegmentCloudConfig()
    assert as_dict(c) == scm.DEFAULTS
    assert scm.DEFAULTS == dict(which=1, margin=1, map_min_points=1, connectivity=26, min_points=1, min_voxels=1, lo=(-LIM,) * 3, hi=(LIM,) * 3)
    loamx.lib().loamx_densemap_segment_cloud_default_config(None)   # NULL: nothing to fill
    assert c.check() is c and scm.check(scm.DEFAULTS) is None
    d = loamx.SegmentCloudConfig(margin=2, lo=(1, 2, 3)).copy(min_voxels=5)
    assert (d.margin, tuple(d.lo), d.min_voxels, tuple(d.hi), d.which) == (2, (1, 2, 3), 5, (LIM,) * 3, 1)


def axis(a, v, other=0):
    return tuple(v if k == a else other for k in range(3))


# (id, the field the message names, configurations accepted at the edge of the bound, configurations refused just beyond it)
BOUNDS = [("which", "which", [dict(which=0), dict(which=2)], [dict(which=3), dict(which=2 ** 32 - 1)]),
          ("margin", "margin", [dict(margin=0), dict(margin=2)], [dict(margin=3), dict(margin=2 ** 32 - 1)]),
          ("map_min_points", "map_min_points", [dict(map_min_points=1), dict(map_min_points=2 ** 32 - 1)], [dict(map_min_points=0)]),
          ("connectivity", "connectivity", [dict(connectivity=6), dict(connectivity=18), dict(connectivity=26)],
           [dict(connectivity=v) for v in (0, 7, 8, 19, 27)]),
          ("min_points", "min_points", [dict(min_points=1), dict(min_points=2 ** 32 - 1)], [dict(min_points=0)]),
          ("min_voxels", "min_voxels", [dict(min_voxels=1), dict(min_voxels=2 ** 32 - 1)], [dict(min_voxels=0)])]
for _a in range(3):
    BOUNDS.append((f"lo{_a}", "lo", [dict(lo=axis(_a, -LIM, -5)), dict(lo=axis(_a, LIM, -5), hi=axis(_a, LIM, 7))],
                   [dict(lo=axis(_a, -LIM - 1, -5)), dict(lo=axis(_a, LIM + 1, -5))]))
    BOUNDS.append((f"hi{_a}", "hi", [dict(hi=axis(_a, LIM, 5))], [dict(hi=axis(_a, LIM + 1, 5)), dict(hi=axis(_a, -LIM - 1, 5), lo=axis(_a, -LIM, -7))]))
    BOUNDS.append((f"lo{_a}_le_hi{_a}", "lo", [dict(lo=axis(_a, 3), hi=axis(_a, 3))], [dict(lo=axis(_a, 4), hi=axis(_a, 3))]))
# the first bad field is the one named: each pair breaks two
FIRST = [("which", dict(which=3, margin=3)), ("margin", dict(margin=3, map_min_points=0)), ("map_min_points", dict(map_min_points=0, connectivity=7)),
         ("connectivity", dict(connectivity=7, min_points=0)), ("min_points", dict(min_points=0, min_voxels=0)),
         ("min_voxels", dict(min_voxels=0, lo=(1, 0, 0), hi=(0, 0, 0)))]


@pytest.mark.parametrize("name,field,good,bad", BOUNDS, ids=[b[0] for b in BOUNDS])
def test_check_bounds(name, field, good, bad):
    L = loamx.lib()
    for kw in good:
        c = loamx.SegmentCloudConfig(**kw)
        assert L.loamx_densemap_segment_cloud_check(C.byref(c)) == loamx.OK, kw
        assert scm.check(dict(scm.DEFAULTS, **kw)) is None
    for kw in bad:
        c = loamx.SegmentCloudConfig(**kw)
        assert L.loamx_densemap_segment_cloud_check(C.byref(c)) == loamx.E_INVALID, kw
        assert field.encode() in L.loamx_last_error(), (kw, L.loamx_last_error())
        assert scm.check(dict(scm.DEFAULTS, **kw)) == field
        with pytest.raises(loamx.LoamxError):
            c.check()


@pytest.mark.parametrize("field,kw", FIRST, ids=[f[0] for f in FIRST])
def test_check_names_the_first_bad_field(field, kw):
    L = loamx.lib()
    c = loamx.SegmentCloudConfig(**kw)
    assert L.loamx_densemap_segment_cloud_check(C.byref(c)) == loamx.E_INVALID
    assert L.loamx_last_error().split()[0].startswith(field.encode()), L.loamx_last_error()
    assert scm.check(dict(scm.DEFAULTS, **kw)) == field


def test_check_null_arguments():
    L = loamx.lib()
    assert L.loamx_densemap_segment_cloud_check(None) == loamx.E_INVALID and b"cfg" in L.loamx_last_error()
    n, st = C.c_uint64(7), (C.c_uint64 * 13)()
    rc = L.loamx_densemap_segment_cloud(None, None, None, None, None, None, C.c_uint64(0), C.byref(n), None, C.c_uint64(0), C.byref(n), st)
    assert rc == loamx.E_INVALID and b"h is NULL" in L.loamx_last_error() and n.value == 7


# ---- loamx_segments_match against its model on hand-made records
def rec(lo, hi, min_key=None):
    r = np.zeros(1, sm.SEGMENT)
    r["lo"], r["hi"], r["voxels"], r["points"] = lo, hi, 1, 1
    r["min_key"] = (int(lo[0]) + 2 ** 20) | ((int(lo[1]) + 2 ** 20) << 21) | ((int(lo[2]) + 2 ** 20) << 42) if min_key is None else min_key
    return r[0]


def records(*rs):
    return np.array(list(rs), sm.SEGMENT) if rs else np.zeros(0, sm.SEGMENT)


def match_both(prev, cur, gap=0):
    got, want = loamx.segments_match(prev, cur, gap), scm.segments_match(prev, cur, gap)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes(), (got, want)
    return got.tolist()


def test_segments_match_cases():
    a, b = rec((0, 0, 0), (3, 3, 3)), rec((10, 0, 0), (12, 3, 3))
    # no overlap at all, and overlap only through the gap (6 cells apart on x)
    far = rec((20, 20, 20), (21, 21, 21))
    assert match_both(records(a, b), records(far)) == [sm.NONE]
    c = rec((5, 0, 0), (8, 3, 3))   # one cell beyond a's box grown by 1, inside it grown by 2; b's box needs 2 as well
    assert match_both(records(a, b), records(c), 0) == [sm.NONE]
    assert match_both(records(a), records(c), 1) == [sm.NONE]
    assert match_both(records(a), records(c), 2) == [0]
    assert match_both(records(a, b), records(c), 1) == [sm.NONE] and match_both(records(a, b), records(c), 2) == [0]   # equal: the smaller key
    # the larger overlap wins whatever the order, equal overlaps go to the smaller min_key whatever the order
    cur = rec((2, 0, 0), (11, 3, 3))   # 2 x 4 x 4 cells with a, 2 x 4 x 4 with b
    assert match_both(records(a, b), records(cur)) == [0] and match_both(records(b, a), records(cur)) == [1]
    cur2 = rec((3, 0, 0), (11, 3, 3))  # 1 x 16 with a, 2 x 16 with b
    assert match_both(records(a, b), records(cur2)) == [1] and match_both(records(b, a), records(cur2)) == [0]
    same_box_other_key = rec((0, 0, 0), (3, 3, 3), min_key=5)
    assert match_both(records(a, same_box_other_key), records(a)) == [1] and match_both(records(same_box_other_key, a), records(a)) == [0]
    # several current records in one call; n_prev = 0; n_cur = 0
    assert match_both(records(a, b), records(far, cur2, a, b)) == [sm.NONE, 1, 0, 1]
    assert match_both(records(), records(a, b)) == [sm.NONE, sm.NONE]
    assert match_both(records(a), records()) == []


def test_segments_match_whole_key_range():
    whole = rec((-LIM, -LIM, -LIM), (LIM, LIM, LIM), min_key=9)   # (2^21 - 1)^3 cells shared with itself: just below 2^63
    less = rec((-LIM, -LIM, -LIM), (LIM, LIM, LIM - 1), min_key=1)  # one slab fewer: a product that differs from it beyond 64 - 21 bits
    assert (2 ** 21 - 1) ** 3 > 2 ** 62 and (2 ** 21 - 1) ** 3 - (2 ** 21 - 1) ** 2 * (2 ** 21 - 2) == (2 ** 21 - 1) ** 2
    assert match_both(records(less, whole), records(whole)) == [1] and match_both(records(whole, less), records(whole)) == [0]
    assert match_both(records(less, whole), records(whole), 1024) == [0]    # grown, `less` covers it too: equal products near 2^63, the smaller key
    corner = rec((LIM, LIM, LIM), (LIM, LIM, LIM))
    other = rec((-LIM, -LIM, -LIM), (-LIM, -LIM, -LIM))
    assert match_both(records(other, corner), records(corner, other, whole)) == [1, 0, 0]   # one cell each with `whole`: the smaller key
    assert match_both(records(corner), records(other), 1024) == [sm.NONE]


def test_segments_match_refusals():
    L = loamx.lib()
    a = records(rec((0, 0, 0), (1, 1, 1)))
    out = np.full(1, 7, np.uint32)
    args = lambda gap, o=out: (a.ctypes.data_as(C.c_void_p), C.c_uint64(1), a.ctypes.data_as(C.c_void_p), C.c_uint64(1), C.c_uint32(gap),
                               None if o is None else o.ctypes.data_as(C.c_void_p))
    assert L.loamx_segments_match(*args(1025)) == loamx.E_INVALID and b"gap" in L.loamx_last_error() and out[0] == 7
    assert L.loamx_segments_match(*args(0, None)) == loamx.E_INVALID and b"prev_of_cur" in L.loamx_last_error()
    assert L.loamx_segments_match(None, C.c_uint64(1), *args(0)[2:]) == loamx.E_INVALID and b"prev" in L.loamx_last_error() and out[0] == 7
    assert L.loamx_segments_match(*args(1024)) == loamx.OK and out[0] == 0


# ---- the model against an independent brute force: dense arrays and a union-find, none of the model's functions
G = 8            # the scenes live in cells -4 .. 3 per axis
PAD = 2          # the margin's reach beyond them


def brute(map_pts, cloud, origin, min_range, max_range, which, margin, map_min_points, connectivity, min_points, min_voxels, lo, hi):
    """the definition of include/loamx.h restated over dense arrays; coordinates are multiples of 1/8 of small magnitude, so float64
    arithmetic is exact and agrees with the library's f32 expressions"""
    def cell(p):
        return tuple(int(np.floor(float(v) / LEAF)) for v in p[:3])

    def admitted(p):
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = float(sum((np.float64(p[a]) - origin[a]) ** 2 for a in range(3)))   # (an infinite coordinate: inf, or nan beside another)
        if not d2 >= min_range ** 2 or (max_range > 0 and not d2 <= max_range ** 2):
            return "range"
        if not all(np.isfinite(float(v)) and abs(np.floor(float(v) / LEAF)) < 2 ** 20 for v in p[:3]):
            return "key"
        return None

    side = G + 2 * PAD
    off = G // 2 + PAD
    mapn = np.zeros((side,) * 3, np.int64)
    for p in map_pts:
        if admitted(p) is None:
            c = cell(p)
            mapn[c[0] + off, c[1] + off, c[2] + off] += 1
    mapped = mapn >= map_min_points
    st = dict.fromkeys(scm.STAT_KEYS, 0)
    st["offered"] = len(cloud)
    cnt = np.zeros((side,) * 3, np.int64)
    cell_of_point = [None] * len(cloud)
    for i, p in enumerate(cloud):
        why = admitted(p)
        if why is not None:
            st["dropped_" + why] += 1
            continue
        c = cell(p)
        x, y, z = (c[a] + off for a in range(3))
        near = bool(mapped[x - margin:x + margin + 1, y - margin:y + margin + 1, z - margin:z + margin + 1].any())
        if which != 0 and near != (which == 2):
            st["rejected"] += 1
            continue
        st["entered"] += 1
        cnt[x, y, z] += 1
        cell_of_point[i] = (x, y, z)
    st["voxels"] = int((cnt > 0).sum())
    sel = cnt >= min_points
    idx = np.indices(sel.shape) - off
    for a in range(3):
        sel &= (idx[a] >= lo[a]) & (idx[a] <= hi[a])
    st["selected"] = int(sel.sum())
    parent = {c: c for c in map(tuple, np.argwhere(sel).tolist())}

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    most = {6: 1, 18: 2, 26: 3}[connectivity]
    for c in list(parent):
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    if 0 < abs(dx) + abs(dy) + abs(dz) <= most:
                        nb = (c[0] + dx, c[1] + dy, c[2] + dz)
                        if nb in parent:
                            ra, rb = find(c), find(nb)
                            if ra != rb:
                                parent[ra] = rb
    groups = {}
    for c in parent:
        groups.setdefault(find(c), []).append(c)
    key = lambda c: (c[0] - off + 2 ** 20) | ((c[1] - off + 2 ** 20) << 21) | ((c[2] - off + 2 ** 20) << 42)
    comps = sorted(groups.values(), key=lambda g: min(key(c) for c in g))
    st["components"] = len(comps)
    st["largest"] = max((len(g) for g in comps), default=0)
    kept = [g for g in comps if len(g) >= min_voxels]
    st["kept"], st["kept_voxels"] = len(kept), sum(len(g) for g in kept)
    out = np.zeros(len(kept), sm.SEGMENT)
    label_of = {}
    for r, g in enumerate(kept):
        out[r]["min_key"], out[r]["voxels"], out[r]["points"] = min(key(c) for c in g), len(g), sum(int(cnt[c]) for c in g)
        for a in range(3):
            out[r]["lo"][a], out[r]["hi"][a] = min(c[a] for c in g) - off, max(c[a] for c in g) - off
            out[r]["sum_idx"][a] = sum(c[a] - off for c in g)
        for c in g:
            label_of[c] = r
    labels = np.array([label_of.get(c, sm.NONE) if c is not None else sm.NONE for c in cell_of_point], np.uint32).reshape(-1)
    st["labelled"] = int((labels != sm.NONE).sum())
    return labels, out, st


def random_scene(rng):
    def pts(n):
        p = np.zeros((n, 4), np.float32)
        p[:, :3] = rng.integers(-16, 16, (n, 3)) / 8.0   # inside cells -4 .. 3 at leaf 0.5
        return p
    map_pts, cloud = pts(int(rng.integers(0, 60))), pts(int(rng.integers(0, 120)))
    if len(cloud) and rng.random() < 0.5:   # some points that the filters drop
        for i in rng.integers(0, len(cloud), 3):
            cloud[i, int(rng.integers(0, 3))] = [np.nan, np.inf, -np.inf, 2.0 ** 19, -(2.0 ** 19) - 0.25][int(rng.integers(0, 5))]
    origin = tuple((rng.integers(-8, 8, 3) / 8.0).tolist())
    min_range = float(rng.choice([0.0, 0.5, 1.0]))
    max_range = float(rng.choice([0.0, 2.0, 3.0]))
    lo = tuple(int(v) for v in rng.integers(-5, 0, 3)) if rng.random() < 0.3 else (-LIM,) * 3
    hi = tuple(int(v) for v in rng.integers(0, 5, 3)) if rng.random() < 0.3 else (LIM,) * 3
    cfg = dict(which=int(rng.integers(0, 3)), margin=int(rng.integers(0, 3)), map_min_points=int(rng.integers(1, 3)),
               connectivity=int(rng.choice([6, 18, 26])), min_points=int(rng.integers(1, 3)), min_voxels=int(rng.integers(1, 4)), lo=lo, hi=hi)
    return map_pts, cloud, origin, min_range, max_range, cfg


def model_of(map_pts, origin, min_range, max_range):
    live = dm.Model(leaf=LEAF, min_range=min_range, max_range=max_range)
    if len(map_pts):
        live.add(map_pts, origin)
    return live


def test_model_against_brute_force():
    rng = np.random.default_rng(77)
    seen = dict(entered=0, rejected=0, dropped=0, multi=0, dropped_comp=0)
    for _ in range(300):
        map_pts, cloud, origin, min_range, max_range, cfg = random_scene(rng)
        live = model_of(map_pts, origin, min_range, max_range)
        labels, recs, st, _ = scm.segment_cloud(live, cloud, origin, **cfg)
        bl, br, bst = brute(map_pts, cloud, origin, min_range, max_range, **cfg)
        assert st == bst, (cfg, st, bst)
        assert labels.tobytes() == bl.tobytes() and recs.tobytes() == br.tobytes(), cfg
        seen["entered"] += st["entered"] > 0
        seen["rejected"] += st["rejected"] > 0
        seen["dropped"] += st["dropped_range"] > 0 and st["dropped_key"] > 0
        seen["multi"] += st["components"] > 1
        seen["dropped_comp"] += st["kept"] < st["components"]
    assert all(v >= 20 for v in seen.values()), seen   # the scenes reach every branch often


def test_model_invariants():
    rng = np.random.default_rng(5)
    for _ in range(40):
        map_pts, cloud, origin, min_range, max_range, cfg = random_scene(rng)
        live = model_of(map_pts, origin, min_range, max_range)
        labels, recs, st, fresh = scm.segment_cloud(live, cloud, origin, **cfg)
        assert st["offered"] == len(cloud) == st["dropped_range"] + st["dropped_key"] + st["rejected"] + st["entered"]
        assert st["voxels"] == len(fresh) >= st["selected"] >= st["kept_voxels"] and st["components"] >= st["kept"] == len(recs)
        assert st["labelled"] == int(recs["points"].sum()) and int(fresh.vals[:, 0].sum()) == st["entered"]
        perm = rng.permutation(len(cloud))
        pl, pr, pst, _ = scm.segment_cloud(live, cloud[perm], origin, **cfg)
        assert pl.tobytes() == labels[perm].tobytes() and pr.tobytes() == recs.tobytes() and pst == st
        # NEW and KNOWN split the admitted points; ALL enters both halves
        by = {w: scm.segment_cloud(live, cloud, origin, **dict(cfg, which=w))[2] for w in (scm.ALL, scm.NEW, scm.KNOWN)}
        assert by[scm.ALL]["entered"] == by[scm.NEW]["entered"] + by[scm.KNOWN]["entered"] and by[scm.ALL]["rejected"] == 0
        assert by[scm.NEW]["rejected"] == by[scm.KNOWN]["entered"]


def test_model_by_hand():
    live = sm.model_of_cells([(0, 0, 0)], LEAF, counts=[2])
    cloud = sm.points_of_cells([(0, 0, 0), (0, 1, 1), (2, 0, 0), (3, 0, 0), (6, 0, 0)], LEAF, counts=[1, 1, 2, 1, 1])
    labels, recs, st, _ = scm.segment_cloud(live, cloud)    # NEW, margin 1: the first two cells are near
    assert labels.tolist() == [sm.NONE, sm.NONE, 0, 0, 0, 1] and recs["voxels"].tolist() == [2, 1] and recs["points"].tolist() == [3, 1]
    assert st == dict(offered=6, dropped_range=0, dropped_key=0, rejected=2, entered=4, voxels=3, selected=3, components=2, kept=2, kept_voxels=3,
                      largest=2, labelled=4)
    assert scm.segment_cloud(live, cloud, margin=0)[0].tolist() == [sm.NONE, 2, 0, 0, 0, 1]   # (0, 1, 1) enters; its key is the largest
    assert scm.segment_cloud(live, cloud, margin=2)[0].tolist() == [sm.NONE, sm.NONE, sm.NONE, sm.NONE, 0, 1]
    assert scm.segment_cloud(live, cloud, which=scm.KNOWN)[0].tolist() == [0, 0, sm.NONE, sm.NONE, sm.NONE, sm.NONE]
    assert scm.segment_cloud(live, cloud, map_min_points=3)[0].tolist() == [0, 0, 1, 1, 1, 2]   # the map voxel holds two points only
    assert scm.segment_cloud(live, cloud, which=scm.ALL, min_voxels=2)[0].tolist() == [0, 0, 1, 1, 1, sm.NONE]
    assert scm.segment_cloud(live, cloud, which=scm.ALL, min_points=2)[0].tolist() == [sm.NONE, sm.NONE, 0, 0, sm.NONE, sm.NONE]
