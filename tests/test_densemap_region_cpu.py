"""CPU: the dense map's regions, tiles and file merge (include/loamx.h, loamx_densemap_region_* ... loamx_densemap_page) — every new
symbol declared and exported, both structs laid out as a C compiler lays them out, the host-only helpers against the model
(tests/densemap_region_model.py) at the edges of the index range, loamx_densemap_file_merge against the model's merge on files the
model wrote, and the same files through tests/densemap_tiles_driver.cpp, a program of its own around
loam_velodyne_amd/csrc/densemap_tiles.hpp built with -fsanitize=address,undefined.  Everything compared is an integer or a byte
string: no tolerance."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_file_model as fm
import densemap_region_model as rm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_region_default", "loamx_densemap_region_check", "loamx_densemap_region_about", "loamx_densemap_tile_of",
               "loamx_densemap_tile_region", "loamx_densemap_tile_name", "loamx_densemap_file_merge", "loamx_densemap_count_region",
               "loamx_densemap_download_region", "loamx_densemap_save_region", "loamx_densemap_evict", "loamx_densemap_page")
LEAF = 0.5
CARVE = dict(carve_max_range=30.0, ray_stride=2, end_margin=1, max_steps=512)
IMAX = rm.IMAX


def line_model(flags, n, first=None, leaf=LEAF, far=40.0):
    """a model with exactly n voxels of one point each on a line along x from cell `first` (default: centred), fed in two calls from
    two origins (so that rays carve)"""
    m = fm.model_of(flags, leaf, **CARVE)
    first = -(n // 2) if first is None else first
    p = rm.line(n, leaf, first)
    m.add(p[: n // 2], ((first + n + far) * leaf, 0.1, 0.2))
    m.add(p[n // 2:], ((first - far) * leaf, 0.1, 0.2))    # (from beyond the first half: these rays cross its voxels)
    assert len(m) == n
    return m


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert "} loamx_densemap_region;" in hdr and "} loamx_densemap_page_config;" in hdr
    assert "#define LOAMX_REGION_INSIDE 0u" in hdr and "#define LOAMX_REGION_OUTSIDE 1u" in hdr
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("count_region", "region_points", "save_region", "evict", "page"):
        assert callable(getattr(loamx.DenseMap, name)), name
    for name in ("densemap_region_about", "densemap_tile_of", "densemap_tile_region", "densemap_tile_name", "densemap_file_merge"):
        assert callable(getattr(loamx, name)), name
    assert issubclass(loamx.DenseMapRegion, C.Structure) and issubclass(loamx.DenseMapPageConfig, C.Structure)
    assert (loamx.REGION_INSIDE, loamx.REGION_OUTSIDE) == (0, 1)


@pytest.mark.parametrize("c_name,t,fields", [("loamx_densemap_region", "DenseMapRegion", ["lo", "hi", "side", "reserved"]),
                                            ("loamx_densemap_page_config", "DenseMapPageConfig", ["dir", "tile_voxels", "radius"])])
def test_struct_layout_matches_c(tmp_path, c_name, t, fields):
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    t = getattr(loamx, t)
    assert got[0] == C.sizeof(t)
    assert got[1:] == [getattr(t, f).offset for f in fields]
    assert [f for f, _ in t._fields_] == fields


def _invalid(call):
    with pytest.raises(loamx.LoamxError) as e:
        call()
    assert e.value.code == loamx.E_INVALID, str(e.value)
    return str(e.value)


def test_region_default_and_check():
    r = loamx.DenseMapRegion()
    assert r.as_dict() == rm.region() and r.reserved == 0
    r.check()
    loamx.DenseMapRegion([-IMAX] * 3, [-IMAX] * 3, 1).check()    # a single voxel at the edge, outside
    for a in range(3):
        lo, hi = [0, 0, 0], [5, 5, 5]
        lo[a] = 6
        assert f"lo[{a}] > hi[{a}]" in _invalid(loamx.DenseMapRegion(lo, hi).check)
        lo[a] = -IMAX - 1
        assert f"lo[{a}]" in _invalid(loamx.DenseMapRegion(lo, hi).check)
        lo[a], hi[a] = 0, IMAX + 1
        assert f"hi[{a}]" in _invalid(loamx.DenseMapRegion(lo, hi).check)
    assert "side" in _invalid(loamx.DenseMapRegion(side=2).check)
    bad = loamx.DenseMapRegion()
    bad.reserved = 1
    assert "reserved" in _invalid(bad.check)
    assert loamx.lib().loamx_densemap_region_check(None) == loamx.E_INVALID


ABOUT = [(0.5, (0.0, 0.0, 0.0), (1.0, 2.0, 0.0)), (0.5, (-0.25, 10.3, -7.77), (0.25, 0.0, 3.1)), (0.1, (1.05, -1.05, 0.3), (0.05, 0.05, 0.3)),
         (0.5, (5e5, -5e5, 0.0), (1e5, 1e5, 6e5)), (0.3, (-1e9, 1e9, 12.0), (1.0, 1.0, 1.0)), (2.0, (-0.001, 0.001, -2.0), (0.0, 0.0, 0.0))]


def test_region_about_equals_the_model():
    for leaf, c, h in ABOUT:
        assert loamx.densemap_region_about(leaf, c, h).as_dict() == rm.region_about(leaf, c, h), (leaf, c, h)
    assert loamx.densemap_region_about(0.5, (5e5, -5e5, 0.0), (1e5, 1e5, 6e5)).as_dict() == rm.region([800000, -IMAX, -IMAX], [IMAX, -800000, IMAX])
    assert "half" in _invalid(lambda: loamx.densemap_region_about(0.5, (0, 0, 0), (1, -1, 1)))
    assert "half" in _invalid(lambda: loamx.densemap_region_about(0.5, (0, 0, 0), (1, float("nan"), 1)))
    assert "centre" in _invalid(lambda: loamx.densemap_region_about(0.5, (0, float("inf"), 0), (1, 1, 1)))
    assert "leaf" in _invalid(lambda: loamx.densemap_region_about(0.0, (0, 0, 0), (1, 1, 1)))
    assert "leaf" in _invalid(lambda: loamx.densemap_region_about(float("nan"), (0, 0, 0), (1, 1, 1)))


TILE_CASES = [(T, i) for T in (1, 8, 1000, 1 << 20) for i in (0, 1, -1, T - 1, T, -T, -T - 1, -T + 1, IMAX, -IMAX, 12345, -12345)
              if abs(i) <= IMAX]


def test_tiles_equal_the_model():
    assert loamx.densemap_tile_of((-1, -8, -9), 8) == (-1, -1, -2)    # index -1 -> tile -1, -T -> -1, -T - 1 -> -2
    for T, i in TILE_CASES:
        idx = (i, -i, i // 2)
        t = loamx.densemap_tile_of(idx, T)
        assert t == rm.tile_of(idx, T), (T, i)
        assert loamx.densemap_tile_region(t, T).as_dict() == rm.tile_region(t, T), (T, i)
        assert loamx.densemap_tile_name(t) == rm.tile_name(t)
        w = rm.tile_region(t, T)
        assert all(w["lo"][a] <= idx[a] <= w["hi"][a] for a in range(3))
    assert loamx.densemap_tile_of((IMAX, -IMAX, 0), 1) == (IMAX, -IMAX, 0)
    assert loamx.densemap_tile_of((IMAX, -IMAX, -1), 1 << 20) == (0, -1, -1)
    assert loamx.densemap_tile_region((0, -1, -1), 1 << 20).as_dict() == rm.region([0, -IMAX, -IMAX], [IMAX, -1, -1])
    assert loamx.densemap_tile_name((-3, 0, 1048575)) == "tile_-3_0_1048575.lxdm"
    for T in (0, (1 << 20) + 1):
        assert "tile_voxels" in _invalid(lambda: loamx.densemap_tile_of((0, 0, 0), T))
        assert "tile_voxels" in _invalid(lambda: loamx.densemap_tile_region((0, 0, 0), T))
    assert "tile" in _invalid(lambda: loamx.densemap_tile_region((1, 0, 0), 1 << 20))     # holds no index of the key range
    assert "tile" in _invalid(lambda: loamx.densemap_tile_region((0, 0, -2), 1 << 20))
    buf = C.create_string_buffer(8)
    t3 = (C.c_int32 * 3)(1, 2, 3)
    assert loamx.lib().loamx_densemap_tile_name(t3, buf, C.c_uint64(8)) == loamx.E_INVALID
    assert loamx.lib().loamx_densemap_tile_name(t3, None, C.c_uint64(64)) == loamx.E_INVALID


# ---- file merge ---------------------------------------------------------------------------------------------------------------------
# (n_a, first_a, n_b, first_b): disjoint, overlapping, identical key sets, and the empty and the one-voxel file on either side
MERGE_CASES = [(65, 0, 65, 100), (65, 0, 65, 30), (65, 0, 65, 0), (0, 0, 65, 0), (65, 0, 0, 0), (0, 0, 0, 0), (1, 3, 1, 3), (1, 3, 1, 4),
               (1, 10, 65, 0)]


def _merge_files(tmp_path, flags, case):
    na, fa, nb, fb = case
    a, b = line_model(flags, na, fa), line_model(flags, nb, fb, far=25.0)
    pa, pb = str(tmp_path / "a.lxdm"), str(tmp_path / "b.lxdm")
    fm.write(pa, a)
    fm.write(pb, b)
    return a, b, pa, pb


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_file_merge_equals_the_model(tmp_path, flags):
    for k, case in enumerate(MERGE_CASES):
        a, b, pa, pb = _merge_files(tmp_path, flags, case)
        want = fm.to_bytes(fm.merge(a, b))
        out = str(tmp_path / f"out{k}.lxdm")
        loamx.densemap_file_merge(pa, pb, out)
        assert open(out, "rb").read() == want, case
        assert loamx.densemap_file_info(out, deep=True)["voxels"] == len(fm.merge(a, b)["keys"])
        raw_b = open(pb, "rb").read()
        loamx.densemap_file_merge(pa, pb, pa)    # path_out == path_a
        assert open(pa, "rb").read() == want and open(pb, "rb").read() == raw_b
    if flags & 1:
        r = fm.merge(*_merge_files(tmp_path, flags, MERGE_CASES[1])[:2])
        assert r["miss"].sum() > 0 and r["carve_stats"][5] > 0
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".part")]


def test_file_merge_refusals(tmp_path):
    a, b, pa, pb = _merge_files(tmp_path, 3, MERGE_CASES[1])
    out = str(tmp_path / "out.lxdm")
    other_leaf = float(np.nextafter(np.float32(LEAF), np.float32(1.0)))
    p_leaf, p_flags, p_bad = str(tmp_path / "leaf.lxdm"), str(tmp_path / "flags.lxdm"), str(tmp_path / "bad.lxdm")
    fm.write(p_leaf, line_model(3, 65, 30, leaf=other_leaf))
    fm.write(p_flags, line_model(2, 65, 30))
    raw = bytearray(open(pb, "rb").read())
    raw[128:136], raw[136:144] = raw[136:144], raw[128:136]    # two keys swapped: only the deep check sees it
    open(p_bad, "wb").write(bytes(raw))
    before = {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path)}
    assert "leaf" in _invalid(lambda: loamx.densemap_file_merge(pa, p_leaf, out))
    assert "flags" in _invalid(lambda: loamx.densemap_file_merge(pa, p_flags, out))
    assert "keys[1]" in _invalid(lambda: loamx.densemap_file_merge(pa, p_bad, out))
    assert "keys[1]" in _invalid(lambda: loamx.densemap_file_merge(p_bad, pa, pa))
    assert "cannot open" in _invalid(lambda: loamx.densemap_file_merge(pa, str(tmp_path / "missing.lxdm"), out))
    assert "cannot open" in _invalid(lambda: loamx.densemap_file_merge(pa, pb, str(tmp_path / "no_such_dir" / "out.lxdm")))
    assert loamx.lib().loamx_densemap_file_merge(None, os.fsencode(pb), os.fsencode(out)) == loamx.E_INVALID
    assert {f: open(tmp_path / f, "rb").read() for f in os.listdir(tmp_path)} == before    # nothing left behind, nothing touched


# ---- the driver under the sanitizers ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("densemap_tiles") / "densemap_tiles_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "densemap_tiles_driver.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, *args):
    r = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout.splitlines()


def test_the_driver_gives_the_same_verdicts_under_the_sanitizers(driver, tmp_path):
    for flags in (0, 1, 2, 3):
        for k, case in enumerate(MERGE_CASES):
            a, b, pa, pb = _merge_files(tmp_path, flags, case)
            want = fm.merge(a, b)
            out = str(tmp_path / f"out{flags}{k}.lxdm")
            assert _run(driver, "merge", pa, pb, out) == [f"OK {len(want['keys'])}"]
            assert open(out, "rb").read() == fm.to_bytes(want)
            assert _run(driver, "merge", pa, pb, pa) == [f"OK {len(want['keys'])}"] and open(pa, "rb").read() == fm.to_bytes(want)
    # the refusals, with the field named
    a, b, pa, pb = _merge_files(tmp_path, 3, MERGE_CASES[1])
    p_leaf, p_flags, p_bad = str(tmp_path / "leaf.lxdm"), str(tmp_path / "flags.lxdm"), str(tmp_path / "bad.lxdm")
    fm.write(p_leaf, line_model(3, 65, 30, leaf=float(np.nextafter(np.float32(LEAF), np.float32(1.0)))))
    fm.write(p_flags, line_model(2, 65, 30))
    raw = bytearray(open(pb, "rb").read())
    raw[128:136], raw[136:144] = raw[136:144], raw[128:136]
    open(p_bad, "wb").write(bytes(raw))
    gone = str(tmp_path / "refused.lxdm")
    for other, word in ((p_leaf, "leaf"), (p_flags, "flags"), (p_bad, "keys[1]")):
        line, = _run(driver, "merge", pa, other, gone)
        assert line.startswith("INVALID") and word in line, line
    assert not os.path.exists(gone) and not [f for f in os.listdir(tmp_path) if f.endswith(".part")]
    # buckets of a map that spans tiles on both signs, with carving and moments
    m = line_model(3, 65, -40)
    src = str(tmp_path / "src.lxdm")
    fm.write(src, m)
    for T in (1, 8, 1 << 20):
        d = tmp_path / f"tiles{T}"
        d.mkdir()
        want = rm.bucket(m, T)
        assert _run(driver, "bucket", src, T, d) == [f"{rm.tile_name(t)} {len(f['keys'])}" for t, f in
                                                     sorted(want.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0]))]
        assert sorted(os.listdir(d)) == sorted(rm.tile_name(t) for t in want)
        for t, f in want.items():
            assert open(d / rm.tile_name(t), "rb").read() == fm.to_bytes(f), (T, t)
    assert len(rm.bucket(m, 8)) == 9 and len(rm.bucket(m, 1)) == 65 and len(rm.bucket(m, 1 << 20)) == 2
    # the tile arithmetic at the edges of the index range
    for T in (1, 8, 1 << 20):
        idx = [i for t, i in TILE_CASES if t == T]
        got = _run(driver, "tiles", T, *idx)
        for i, line in zip(idx, got):
            t = rm.tile_of((i, i, i), T)
            w = rm.tile_region(t, T)
            assert line == f"{t[0]} {w['lo'][0]} {w['hi'][0]} {rm.tile_name(t)}", (T, i, line)


def test_the_header_needs_no_hip():
    src = open(os.path.join(ROOT, "loam_velodyne_amd", "csrc", "densemap_tiles.hpp")).read()
    assert "hip/" not in src and "__global__" not in src and "__device__" not in src
    assert [ln for ln in src.splitlines() if ln.startswith('#include "')] == ['#include "densemap_file.hpp"']


# ---- the model of paging, alone -----------------------------------------------------------------------------------------------------
def test_the_paging_scene_exercises_the_host_merge_on_the_model():
    """the scene of the GPU test on the model alone: far returns land in tiles that were paged out earlier, so page-outs meet files
    that exist (stats[4]), and a final page with a radius that covers the run brings every voxel back"""
    T, radius = 8, (1, 1, 1)
    sweeps, centres = rm.march(LEAF, T)
    whole = fm.model_of(2, LEAF)
    resident, tiles, total = fm.records_of(fm.model_of(2, LEAF)), {}, [0] * 6
    for (p, o), c in zip(sweeps, centres):
        whole.add(p, o)
        m = rm.model_from(resident)
        m.add(p, o)
        resident, tiles, st = rm.page(m, tiles, T, radius, c)
        total = [x + y for x, y in zip(total, st)]
        sum_all = resident
        for f in tiles.values():
            sum_all = fm.merge(sum_all, f)
        assert fm.to_bytes(sum_all) == fm.to_bytes(whole)    # the invariant: resident + every tile file = the map of the whole run
    assert total[4] > 0 and total[0] == 0 and total[2] > total[4] and len(tiles) >= 3
    resident, tiles, st = rm.page(resident, tiles, T, (16, 16, 16), centres[-1])
    assert tiles == {} and st[0] >= 3 and st[3] == 0 and fm.to_bytes(resident) == fm.to_bytes(whole)
