"""GPU: the dense map's regions, eviction and paging (include/loamx.h, loamx_densemap_count_region ... loamx_densemap_page) against
their model (tests/densemap_region_model.py over tests/densemap_file_model.py and the models of the map, of carving and of the
moments).  Leaf 0.5, initial_slots 1024, the box scene of tests/densemap_align_model.py.  Every compared quantity is an integer word
or a byte string: a region's export is the model's export of the subset, a region file and a tile file are the model's files byte for
byte, and whatever an evict took out into a file and merge_file brought back restores the saved map header included.  No tolerance
anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import densemap_align_model as am
import densemap_file_model as fm
import densemap_model as dm
import densemap_region_model as rm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
ALL_FLAGS = [0, 1, 2, 3]
IMAX = rm.IMAX
EVERYTHING = rm.region()
NOTHING = rm.region([1000, 1000, 1000], [1010, 1010, 1010])
HALF = rm.region([-IMAX, -IMAX, -IMAX], [0, IMAX, IMAX])    # x index <= 0: a cut through the box


def new_map(flags, leaf=LEAF, initial_slots=1024, **kw):
    d = loamx.DenseMap(leaf=leaf, initial_slots=initial_slots, **kw)
    if flags & 1:
        d.enable_carving(ray_stride=2)
    if flags & 2:
        d.enable_moments()
    return d


def new_model(flags):
    return fm.model_of(flags, LEAF, ray_stride=2)


def feed(target, sweeps):
    for p, o in sweeps:
        r = target.add(p, o)
        assert r == loamx.OK or r is True
    return target


def exports(d, flags):
    """every export of a handle as bytes (stats without slots)"""
    st = d.stats()
    st.pop("slots")
    out = dict(stats=st, loam=d.points().tobytes(), sensor=d.points(axes="sensor").tobytes())
    if flags & 1:
        out.update(misses=d.misses().tobytes(), carve_stats=d.carve_stats(), static=d.points(static=loamx.StaticRule(1, 1, 4)).tobytes())
    if flags & 2:
        out.update(moments=d.moments().tobytes(), surfels=d.surfels().tobytes())
    return out


def saved(d, tmp_path, name="map.lxdm"):
    path = str(tmp_path / name)
    d.save(path)
    return path, open(path, "rb").read()


def side_of(reg, side):
    return rm.region(reg["lo"], reg["hi"], side)


def handle_region(reg):
    return loamx.DenseMapRegion(reg["lo"], reg["hi"], reg["side"])


def no_parts(tmp_path):
    return not [f for f in os.listdir(tmp_path) if f.endswith(".part")]


def clutter(rng, n):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(am.BOX_LO + 0.6, am.BOX_HI - 0.6, (n, 3))
    return p


@pytest.fixture(scope="module")
def scene():
    S = am.box_scene()
    # (as in tests/test_gpu_densemap_file.py: 100 points in mid-air behind each sweep give the later calls something to carve)
    rng = np.random.default_rng(99)
    S["sweeps"] = [(np.concatenate([p, clutter(rng, 100)]), o) for p, o in S["sweeps"]]
    cache = {}

    def records(flags, k=3):
        """the records of the model fed the first k sweeps, computed once and left unchanged"""
        if (flags, k) not in cache:
            cache[(flags, k)] = fm.records_of(feed(new_model(flags), S["sweeps"][:k]))
        return cache[(flags, k)]

    S["records"] = records
    return S


def check_region(d, want_all, reg, tmp_path, axes=("loam", "sensor")):
    """count_region, region_points and save_region of the handle against the model's selection"""
    want = rm.select(want_all, reg)
    hr = handle_region(reg)
    assert d.count_region(hr) == (len(want["keys"]), want["stats"][0]), reg
    for ax in axes:
        assert d.region_points(hr, axes=ax).tobytes() == dm.export(want["keys"], want["vals"], LEAF, ax).tobytes(), (reg, ax)
    path = str(tmp_path / "region.lxdm")
    d.save_region(hr, path)
    assert open(path, "rb").read() == fm.to_bytes(want), reg
    return want


# ---- reading a region ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_reading_a_region(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    r = scene["records"](flags)
    before = exports(d, flags)
    one = [int(v) for v in rm.indices(r["keys"][len(r["keys"]) // 2:][:1])[0]]
    sizes = []
    for reg in (EVERYTHING, NOTHING, rm.region(one, one), HALF):
        for side in (rm.INSIDE, rm.OUTSIDE):
            sizes.append(len(check_region(d, r, side_of(reg, side), tmp_path)["keys"]))
    n = len(r["keys"])
    assert sizes[:6] == [n, 0, 0, n, 1, n - 1] and 0 < sizes[6] < n and sizes[6] + sizes[7] == n
    i = loamx.densemap_file_info(str(tmp_path / "region.lxdm"), deep=True)
    assert i["flags"] == flags and i["dropped_range"] == i["dropped_key"] == 0 and i["carve_stats"] == [0] * 6
    if flags & 1:
        assert i["carve"]["ray_stride"] == 2
    # a region file is a file like any other: a fresh handle loads it and exports the subset
    e = new_map(0)
    e.load(str(tmp_path / "region.lxdm"))
    assert e.points().tobytes() == d.region_points(handle_region(side_of(HALF, rm.OUTSIDE))).tobytes()
    assert exports(d, flags) == before and no_parts(tmp_path)    # the handle was only read


def test_download_region_capacity(scene):
    d = feed(new_map(0), scene["sweeps"][:1])
    hr = handle_region(HALF)
    n = d.count_region(hr)[0]
    out = np.full((n, 4), 7.0, np.float32)
    c = loamx.cloud_of(out)
    c.count = n - 1
    assert loamx.lib().loamx_densemap_download_region(d.h, C.byref(hr), C.byref(c), 0) == loamx.E_CAPACITY
    assert c.count == n and np.all(out == 7.0)    # the needed count, and nothing else written
    assert loamx.lib().loamx_densemap_download_region(d.h, C.byref(hr), C.byref(c), 0) == loamx.OK
    assert c.count == n and out.tobytes() == d.region_points(hr).tobytes()


def test_wave_and_block_edges(tmp_path):
    flags = 3
    sweeps = [(rm.line(600, LEAF), (0.0, 3.0, 0.2))]
    d, r = feed(new_map(flags), sweeps), fm.records_of(feed(new_model(flags), sweeps))
    assert len(d) == 600 and d.stats()["slots"] == 2048    # eight blocks of 256 slots
    for k in (0, 1, 63, 64, 65, 255, 256, 257, 600):
        reg = rm.region([0, 0, 0], [k - 1, 0, 0]) if k else rm.region([-10, 0, 0], [-1, 0, 0])
        for side in (rm.INSIDE, rm.OUTSIDE):
            want = check_region(d, r, side_of(reg, side), tmp_path, axes=("loam",))
            assert len(want["keys"]) == (k if side == rm.INSIDE else 600 - k)


def edge_patch(ks):
    """voxels in the last cells of the key range on both signs, |i| = 2^20 - 1 and inwards, as test_merge_at_the_edge_of_the_key_range
    of tests/test_gpu_densemap_file.py builds them"""
    x_edge = float(1 << 19)
    hi, lo = rm.line(len(ks), LEAF), rm.line(len(ks), LEAF)
    hi[:, 0] = [x_edge - 0.25 - 0.5 * k for k in ks]
    lo[:, 0] = [-x_edge + 0.75 + 0.5 * k for k in ks]
    return [(hi, (x_edge - 4.0, 0.1, 0.2)), (lo, (-x_edge + 4.0, 0.1, 0.2))]


def test_the_edge_of_the_key_range(tmp_path):
    flags = 3
    sweeps = edge_patch(range(0, 4))
    d, r = feed(new_map(flags), sweeps), fm.records_of(feed(new_model(flags), sweeps))
    ix = rm.indices(r["keys"])[:, 0]
    assert len(d) == 8 and ix.min() == -IMAX and ix.max() == IMAX
    sizes = []
    for lo, hi in ((IMAX, IMAX), (IMAX - 1, IMAX - 1), (-IMAX, -IMAX), (-IMAX + 1, -IMAX + 1), (-IMAX + 1, IMAX - 1), (-IMAX, IMAX),
                   (-IMAX, IMAX - 1), (-IMAX + 1, IMAX)):
        for side in (rm.INSIDE, rm.OUTSIDE):
            sizes.append(len(check_region(d, r, rm.region([lo, 0, 0], [hi, 0, 0], side), tmp_path)["keys"]))
    assert sizes == [1, 7, 1, 7, 1, 7, 1, 7, 6, 2, 8, 0, 7, 1, 7, 1]
    # the two outermost voxels leave and come back
    path, before = saved(d, tmp_path)
    out = str(tmp_path / "edge.lxdm")
    reg = rm.region([-IMAX + 1, 0, 0], [IMAX - 1, 0, 0], rm.OUTSIDE)
    removed, kept = rm.split(r, reg)
    assert d.evict(handle_region(reg), out) == (2, 2)
    assert open(out, "rb").read() == fm.to_bytes(removed) and saved(d, tmp_path, "kept.lxdm")[1] == fm.to_bytes(kept)
    d.merge_file(out)
    assert saved(d, tmp_path, "again.lxdm")[1] == before


# ---- evict --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [rm.INSIDE, rm.OUTSIDE])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_evict_round_trip(scene, tmp_path, flags, side):
    d = feed(new_map(flags), scene["sweeps"])
    r = scene["records"](flags)
    _, before = saved(d, tmp_path)
    assert before == fm.to_bytes(r)
    before_x = exports(d, flags)
    reg = side_of(HALF, side)
    removed, kept = rm.split(r, reg)
    assert 0 < len(removed["keys"]) < len(r["keys"])
    out = str(tmp_path / "out.lxdm")
    assert d.evict(handle_region(reg), out) == (len(removed["keys"]), removed["stats"][0])
    assert open(out, "rb").read() == fm.to_bytes(removed)
    assert saved(d, tmp_path, "kept.lxdm")[1] == fm.to_bytes(kept)
    assert len(d) == len(kept["keys"]) and d.stats()["offered"] == r["stats"][0] - removed["stats"][0]
    assert d.count_region(handle_region(reg)) == (0, 0) and no_parts(tmp_path)
    d.merge_file(out)
    assert saved(d, tmp_path, "again.lxdm")[1] == before    # header included: the statistics are back
    assert exports(d, flags) == before_x


def test_table_size_and_the_trivial_evicts(tmp_path):
    d = new_map(3)
    d.add(rm.line(4000, LEAF), (0.0, 3.0, 0.2))    # 4000 points in one call: 8192 slots
    assert d.stats()["slots"] == 8192 and len(d) == 4000
    before = exports(d, 3)
    assert d.evict(handle_region(NOTHING)) == (0, 0)    # an evict of nothing
    assert exports(d, 3) == before
    keep = rm.region([0, 0, 0], [99, 0, 0], rm.OUTSIDE)
    assert d.evict(handle_region(keep)) == (3900, 3900)    # path None: discarded
    assert len(d) == 100 and d.stats()["slots"] == 1024 and d.stats()["offered"] == 100
    assert d.points().tobytes() == dm.export(*[fm.records_of(feed(new_model(0), [(rm.line(100, LEAF), (0.0, 3.0, 0.2))]))[k]
                                               for k in ("keys", "vals")], LEAF).tobytes()
    assert d.evict(handle_region(EVERYTHING)) == (100, 100)
    assert len(d) == 0 and d.stats()["offered"] == 0 and d.stats()["slots"] == 1024 and len(d.points()) == 0
    assert os.listdir(tmp_path) == []
    d.add(rm.line(10, LEAF), (0.0, 3.0, 0.2))    # and the empty map takes points again
    assert len(d) == 10


@pytest.mark.parametrize("flags", [0, 2, 3])
def test_life_goes_on_after_an_evict(scene, tmp_path, flags):
    sw = scene["sweeps"]
    d = feed(new_map(flags), sw[:2])
    reg = side_of(HALF, rm.INSIDE)
    out = str(tmp_path / "out.lxdm")
    d.evict(handle_region(reg), out)
    kept_path, kept_raw = saved(d, tmp_path, "kept.lxdm")
    assert kept_raw == fm.to_bytes(rm.split(scene["records"](flags, 2), reg)[1])
    feed(d, sw[2:])
    if flags & 1:
        # a second handle that loaded the kept file and was fed the same add
        e = new_map(0)
        e.load(kept_path)
        feed(e, sw[2:])
        assert exports(d, flags) == exports(e, flags) and d.carve_stats()["misses"] > fm.read(kept_path)["carve_stats"][5]
        assert saved(d, tmp_path, "d.lxdm")[1] == saved(e, tmp_path, "e.lxdm")[1]
    else:
        # the model that loaded the kept records and was fed the same add
        m = feed(rm.model_from(fm.read(kept_path)), sw[2:])
        assert saved(d, tmp_path, "d.lxdm")[1] == fm.to_bytes(m)


def test_capacity_is_freed_by_an_evict():
    d = new_map(0, max_voxels=150)
    d.add(rm.line(100, LEAF), (0.0, 3.0, 0.2))
    more = rm.line(100, LEAF, 100)
    with pytest.raises(loamx.LoamxError) as e:
        d.add(more, (0.0, 3.0, 0.2))
    assert e.value.code == loamx.E_CAPACITY and len(d) == 100
    assert d.evict(handle_region(rm.region([0, 0, 0], [59, 0, 0]))) == (60, 60)
    assert d.add(more, (0.0, 3.0, 0.2)) == loamx.OK
    assert len(d) == 140 and d.stats()["offered"] == 140


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(scene, tmp_path):
    flags = 3
    d = feed(new_map(flags), scene["sweeps"][:1])
    before = exports(d, flags)
    L = loamx.lib()
    bad = loamx.DenseMapRegion([1, 0, 0], [0, 5, 5])
    good = handle_region(HALF)
    ok_path, missing = str(tmp_path / "ok.lxdm"), str(tmp_path / "no_such_dir" / "out.lxdm")

    def refused(call, word=None):
        with pytest.raises(loamx.LoamxError) as e:
            call()
        assert e.value.code == loamx.E_INVALID and (word is None or word in str(e.value)), str(e.value)

    refused(lambda: d.count_region(bad), "lo[0] > hi[0]")
    refused(lambda: d.region_points(bad), "lo[0]")
    refused(lambda: d.save_region(bad, ok_path), "lo[0]")
    refused(lambda: d.evict(bad, ok_path), "lo[0]")
    refused(lambda: d.evict(loamx.DenseMapRegion(side=2)), "side")
    refused(lambda: d.save_region(good, missing), "cannot open")
    refused(lambda: d.evict(good, missing), "cannot open")
    refused(lambda: d.page(loamx.DenseMapPageConfig(str(tmp_path / "no_such_dir"), 8), (0, 0, 0)), "dir")
    refused(lambda: d.page(loamx.DenseMapPageConfig(str(tmp_path), 0), (0, 0, 0)), "tile_voxels")
    refused(lambda: d.page(loamx.DenseMapPageConfig(str(tmp_path), 8), (0, float("nan"), 0)), "centre")
    refused(lambda: d.page(loamx.DenseMapPageConfig(None, 8), (0, 0, 0)), "dir")
    two, six, c3 = (C.c_uint64 * 2)(), (C.c_uint64 * 6)(), (C.c_float * 3)()
    cloud = loamx.cloud_of(np.zeros((4, 4), np.float32))
    cfg = loamx.DenseMapPageConfig(str(tmp_path), 8)
    for rc in (L.loamx_densemap_count_region(None, C.byref(good), two), L.loamx_densemap_count_region(d.h, None, two),
               L.loamx_densemap_count_region(d.h, C.byref(good), None),
               L.loamx_densemap_download_region(d.h, None, C.byref(cloud), 0), L.loamx_densemap_download_region(d.h, C.byref(good), None, 0),
               L.loamx_densemap_download_region(d.h, C.byref(good), C.byref(cloud), 2),
               L.loamx_densemap_save_region(d.h, C.byref(good), None), L.loamx_densemap_save_region(d.h, None, os.fsencode(ok_path)),
               L.loamx_densemap_evict(None, C.byref(good), None, two), L.loamx_densemap_evict(d.h, None, None, two),
               L.loamx_densemap_evict(d.h, C.byref(good), None, None),
               L.loamx_densemap_page(d.h, None, c3, six), L.loamx_densemap_page(d.h, C.byref(cfg), None, six),
               L.loamx_densemap_page(d.h, C.byref(cfg), c3, None)):
        assert rc == loamx.E_INVALID
    assert exports(d, flags) == before
    assert os.listdir(tmp_path) == []    # no file, no .part, no directory


# ---- snapshot isolation and history -------------------------------------------------------------------------------------------------
def test_snapshot_isolation(scene, tmp_path):
    d = feed(new_map(2), scene["sweeps"])
    n = d.freeze()
    P = scene["start"]
    rtc = am.rtc_of(P[:, :3], P[:, 3])
    s, c = d.align_step(scene["cloud"], rtc, 1)
    d.evict(handle_region(HALF), str(tmp_path / "out.lxdm"))
    s2, c2 = d.align_step(scene["cloud"], rtc, 1)
    assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes() and c[am.MATCHED] > 500 and d.frozen_size == n
    assert 0 < d.freeze() < n    # a new freeze sees the smaller map
    assert d.align_step(scene["cloud"], rtc, 1)[0].tobytes() != s.tobytes()


def test_rebuild_brings_the_evicted_voxels_back(scene, tmp_path):
    flags = 3
    d, plain = new_map(flags), feed(new_map(flags), scene["sweeps"])
    d.enable_history()
    feed(d, scene["sweeps"])
    removed = d.evict(handle_region(HALF))
    assert removed[0] > 0 and len(d) == len(plain) - removed[0]
    d.rebuild()
    assert saved(d, tmp_path, "d.lxdm")[1] == saved(plain, tmp_path, "plain.lxdm")[1] == fm.to_bytes(scene["records"](flags))
    assert exports(d, flags) == exports(plain, flags)


# ---- paging -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 2, 3])
def test_paging(tmp_path, flags):
    T, radius = 8, (1, 1, 1)
    sweeps, centres = rm.march(LEAF, T)
    tiles_dir = tmp_path / "tiles"
    tiles_dir.mkdir()
    cfg = loamx.DenseMapPageConfig(str(tiles_dir), T, radius)
    d, never = new_map(flags), new_map(flags)
    resident, tiles, total = fm.records_of(new_model(flags)), {}, [0] * 6
    for (p, o), c in zip(sweeps, centres):
        feed(d, [(p, o)])
        feed(never, [(p, o)])
        resident, tiles, want = rm.page(feed(rm.model_from(resident), [(p, o)]), tiles, T, radius, c)
        got = d.page(cfg, c)
        assert list(got.values()) == want
        assert sorted(os.listdir(tiles_dir)) == sorted(rm.tile_name(t) for t in tiles)
        for t, f in tiles.items():
            assert open(tiles_dir / rm.tile_name(t), "rb").read() == fm.to_bytes(f), t
        assert saved(d, tmp_path, "resident.lxdm")[1] == fm.to_bytes(resident)
        total = [x + y for x, y in zip(total, want)]
    assert total[4] > 0 and total[2] > total[4] and len(tiles) >= 3    # page-outs met files that existed: the host merge ran
    # a radius that covers the run: everything comes back and no file is left
    got = d.page(loamx.DenseMapPageConfig(str(tiles_dir), T, (16, 16, 16)), centres[-1])
    assert os.listdir(tiles_dir) == [] and got["tiles_in"] == len(tiles) and got["voxels_out"] == 0 and got["resident"] == len(never)
    a, b = fm.read(saved(d, tmp_path, "paged.lxdm")[0]), fm.read(saved(never, tmp_path, "never.lxdm")[0])
    if flags & 1:
        # (the rays of a paged map did not see the voxels that were on disk: the miss words differ by design)
        assert a["keys"].tobytes() == b["keys"].tobytes() and a["vals"].tobytes() == b["vals"].tobytes()
        assert a["mom"].tobytes() == b["mom"].tobytes() and a["stats"] == b["stats"]
    else:
        assert open(tmp_path / "paged.lxdm", "rb").read() == open(tmp_path / "never.lxdm", "rb").read()


def test_paging_stops_at_the_cap(tmp_path):
    """LOAMX_E_CAPACITY from a page-in ends the call: the tile that did not fit stays on disk and the map is as it was"""
    T = 8
    tiles_dir = tmp_path / "tiles"
    tiles_dir.mkdir()
    cfg = loamx.DenseMapPageConfig(str(tiles_dir), T, (0, 0, 0))
    d = new_map(0, max_voxels=100)
    d.add(rm.line(80, LEAF, 0, y=0.1), (0.0, 3.0, 0.2))    # the tiles 0 .. 9 along x
    st = d.page(cfg, (0.5, 0.1, 0.2))
    assert st["files_written"] == 9 and st["resident"] == 8 and len(os.listdir(tiles_dir)) == 9
    d.add(rm.line(88, LEAF, 0, y=0.7), (0.0, 3.0, 0.2))    # 88 voxels of their own, one row above: 96 resident
    assert len(d) == 96
    before, names = exports(d, 0), sorted(os.listdir(tiles_dir))
    with pytest.raises(loamx.LoamxError) as e:
        d.page(cfg, (6.0, 0.1, 0.2))    # tile 1: its 8 voxels do not fit under the cap
    assert e.value.code == loamx.E_CAPACITY
    assert exports(d, 0) == before and sorted(os.listdir(tiles_dir)) == names
