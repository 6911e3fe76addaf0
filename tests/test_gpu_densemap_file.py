"""GPU: the dense map's native save / load and the merge of two maps on the device (include/loamx.h, loamx_densemap_save and what follows
it) against their model (tests/densemap_file_model.py over the models of the map, of carving and of the moments).  Leaf 0.5,
initial_slots 1024, the box scene and the lattice plane of tests/densemap_align_model.py.  Every compared quantity is an integer word
or a byte string: a saved file is the model's file byte for byte, a loaded handle answers every export, freeze and align with the
bytes of the saving handle, and a merge holds the words of the model's merge.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import densemap_align_model as am
import densemap_file_model as fm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

LEAF = 0.5
ALL_FLAGS = [0, 1, 2, 3]


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


@pytest.fixture(scope="module")
def scene():
    S = am.box_scene()
    # (the box is convex: its walls alone are never crossed by a ray.  100 points in mid-air behind each sweep give the later calls
    # something to carve; one point per voxel, they never have a surfel and stay out of the alignment)
    rng = np.random.default_rng(99)
    S["sweeps"] = [(np.concatenate([p, clutter(rng, 100)]), o) for p, o in S["sweeps"]]
    S["offered"] = sum(len(p) for p, _ in S["sweeps"])
    S["fourth"] = (np.concatenate([am.box_points(rng, 4000), clutter(rng, 100)]), (0.2, 0.1, -0.3))
    S["models"] = {f: feed(new_model(f), S["sweeps"]) for f in ALL_FLAGS}            # the three sweeps
    S["model_a"] = {f: feed(new_model(f), S["sweeps"][:2]) for f in ALL_FLAGS}       # A = sweeps 0 and 1
    S["model_b"] = {f: feed(new_model(f), S["sweeps"][1:]) for f in ALL_FLAGS}       # B = sweeps 1 and 2
    return S


def clutter(rng, n):
    p = np.zeros((n, 4), np.float32)
    p[:, :3] = rng.uniform(am.BOX_LO + 0.6, am.BOX_HI - 0.6, (n, 3))
    return p


def line(n, first=0, y=0.1):
    """n points, one per voxel, on a line along x from cell `first`"""
    p = np.zeros((n, 4), np.float32)
    p[:, 0] = (first + np.arange(n) + 0.25) * LEAF
    p[:, 1], p[:, 2] = y, 0.2
    return p


# ---- save ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_save_equals_the_model(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    path, got = saved(d, tmp_path)
    want = fm.to_bytes(scene["models"][flags])
    assert got == want
    assert len(got) == fm.file_size(flags, len(d)) and not [f for f in os.listdir(tmp_path) if f.endswith(".part")]
    i = loamx.densemap_file_info(path, deep=True)
    assert i["voxels"] == len(d) and i["flags"] == flags and i["offered"] == scene["offered"] == 12300
    if flags & 1:
        assert i["carve"]["ray_stride"] == 2 and i["carve_stats"][5] > 0 and i["carve_stats"] == list(d.carve_stats().values())
    if flags == 2:
        # the same sweeps in another order, their points shuffled (a large first call: the table is rehashed), and in a table that
        # never grows: the same bytes
        rng = np.random.default_rng(4)
        other = [(scene["sweeps"][k][0][rng.permutation(4100)], scene["sweeps"][k][1]) for k in (2, 0, 1)]
        d2 = feed(new_map(flags), other)
        d3 = feed(new_map(flags, initial_slots=1 << 16), scene["sweeps"])
        assert d2.rehashes >= 1 and d3.rehashes == 0 and d3.stats()["slots"] == 1 << 16
        assert saved(d2, tmp_path, "other.lxdm")[1] == want and saved(d3, tmp_path, "wide.lxdm")[1] == want


# ---- round trip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_round_trip(scene, tmp_path, flags):
    d = feed(new_map(flags), scene["sweeps"])
    path, raw = saved(d, tmp_path)
    e = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    if flags == 3:
        e.enable_moments()    # (a feature the handle already has; the load enables the other one)
    e.load(path)
    assert exports(e, flags) == exports(d, flags)
    assert saved(e, tmp_path, "again.lxdm")[1] == raw
    assert 512 < len(e) <= 1024 and e.stats()["slots"] == 2048    # the smallest power of two >= initial_slots and >= 2 x count
    if flags & 1:
        assert e.carve_stats() == d.carve_stats()
    if flags & 2:
        # relocalisation in the prior map, end to end: the snapshot and the alignment of the loaded handle are the saving handle's
        static = loamx.StaticRule() if flags & 1 else None
        assert e.freeze(static=static) == d.freeze(static=static) > 300
        P = scene["start"]
        rtc = am.rtc_of(P[:, :3], P[:, 3])
        for nb in (0, 1):
            s1, c1 = d.align_step(scene["cloud"], rtc, nb)
            s2, c2 = e.align_step(scene["cloud"], rtc, nb)
            assert s1.tobytes() == s2.tobytes() and c1.tobytes() == c2.tobytes() and c1[am.MATCHED] > 1000
        r1, r2 = d.align(scene["cloud"], P), e.align(scene["cloud"], P)
        assert r1["pose"].tobytes() == r2["pose"].tobytes() and r1["iterations"] == r2["iterations"] and r1["status"] == 0
        rot, trans = am.pose_error(r2["pose"], scene["truth"])
        assert rot <= 0.01 and trans <= LEAF / 10


def test_round_trip_of_the_exact_plane(tmp_path):
    d = new_map(2)
    d.add(am.lattice_plane(), am.PLANE_ORIGIN)
    e = new_map(0)
    e.load(saved(d, tmp_path)[0])
    assert e.freeze() == d.freeze() == 256 and np.all(e.surfels()[:, 4:7] == np.float32([0, 0, 1]))
    cloud = am.lattice_plane()[::3].copy()
    P = np.concatenate([am.exp_so3([0.01, -0.02, 0.0]), np.array([[0.05], [-0.03], [0.04]])], axis=1)
    r1, r2 = d.align(cloud, P), e.align(cloud, P)
    assert r1["pose"].tobytes() == r2["pose"].tobytes() and r2["status"] == 0 and r2["degenerate_dims"] == 3


def test_load_sizes_the_table_and_replaces_a_reset_map(scene, tmp_path):
    # 2000 voxels: the smallest power of two >= 2 x count is 4096, whatever the handle held before its reset
    src = new_map(2)
    src.add(np.concatenate([line(1000), line(1000, y=0.7)]), (0.0, 3.0, 0.2))
    path, raw = saved(src, tmp_path)
    e = new_map(2)
    e.add(am.box_points(np.random.default_rng(5), 20000), (0.0, 0.0, 0.0))
    assert e.stats()["slots"] > 4096
    e.reset()
    e.load(path)
    assert len(e) == 2000 and e.stats()["slots"] == 4096
    assert exports(e, 2) == exports(src, 2) and saved(e, tmp_path, "again.lxdm")[1] == raw


def test_life_goes_on(scene, tmp_path):
    flags = 3
    d = feed(new_map(flags), scene["sweeps"])
    path, _ = saved(d, tmp_path)
    e = loamx.DenseMap(leaf=LEAF, initial_slots=1024)
    e.load(path)
    m = feed(new_model(flags), scene["sweeps"])
    for t in (d, e, m):
        feed(t, [scene["fourth"]])
    assert exports(e, flags) == exports(d, flags)
    want = fm.to_bytes(m)
    assert saved(d, tmp_path, "d.lxdm")[1] == want and saved(e, tmp_path, "e.lxdm")[1] == want    # carved as the model continues
    assert m.carve_stats()["misses"] > fm.records_of(scene["models"][flags])["carve_stats"][5]


# ---- merge --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_merge_equals_the_model(scene, tmp_path, flags):
    sw = scene["sweeps"]
    a, b = feed(new_map(flags), sw[:2]), feed(new_map(flags), sw[1:])
    want_rec = fm.merge(scene["model_a"][flags], scene["model_b"][flags])
    want = fm.to_bytes(want_rec)
    # n, S and the moments are those of one map fed all four adds; the misses are the sums over the union of the keys
    whole = fm.records_of(feed(new_model(flags & 2), [sw[0], sw[1], sw[1], sw[2]]))
    assert want_rec["keys"].tobytes() == whole["keys"].tobytes() and want_rec["vals"].tobytes() == whole["vals"].tobytes()
    common = len(np.intersect1d(scene["model_a"][flags].keys, scene["model_b"][flags].keys))
    assert 2 * common > len(whole["keys"]) > common    # most keys overlap, and some are new
    if flags & 2:
        assert want_rec["mom"].tobytes() == whole["mom"].tobytes()
    path_a, raw_a = saved(a, tmp_path, "a.lxdm")
    path_b, raw_b = saved(b, tmp_path, "b.lxdm")
    assert raw_a == fm.to_bytes(scene["model_a"][flags]) and raw_b == fm.to_bytes(scene["model_b"][flags])
    before_b = exports(b, flags)
    a.merge(b)
    assert saved(a, tmp_path, "ab.lxdm")[1] == want
    st = a.stats()
    assert st["offered"] == 16400 and st["voxels"] == len(whole["keys"])
    if flags & 1:
        assert list(a.carve_stats().values()) == list(want_rec["carve_stats"])
        assert a.misses().tobytes() == want_rec["miss"].tobytes() and want_rec["miss"].sum() > 0
    assert exports(b, flags) == before_b and saved(b, tmp_path, "b_after.lxdm")[1] == raw_b    # src is only read
    # merge_file from B's file, and the merge the other way round: the same bytes
    a2 = new_map(flags)
    a2.load(path_a)
    a2.merge_file(path_b)
    assert saved(a2, tmp_path, "a2.lxdm")[1] == want
    a3 = new_map(flags)
    a3.load(path_a)
    b.merge(a3)
    assert saved(b, tmp_path, "ba.lxdm")[1] == want == fm.to_bytes(fm.merge(scene["model_b"][flags], scene["model_a"][flags]))


def _merge_case(tmp_path, flags, dst_sweeps, src_sweeps, via_file=False, src_slots=1024):
    """dst.merge(src) (or merge_file of src's file) against the model's merge; returns (dst, src)"""
    dst, src = feed(new_map(flags), dst_sweeps), feed(new_map(flags, initial_slots=src_slots), src_sweeps)
    want = fm.to_bytes(fm.merge(feed(new_model(flags), dst_sweeps), feed(new_model(flags), src_sweeps)))
    if via_file:
        dst.merge_file(saved(src, tmp_path, "src.lxdm")[0])
    else:
        dst.merge(src)
    assert saved(dst, tmp_path, "dst.lxdm")[1] == want
    return dst, src


@pytest.mark.parametrize("via_file", [False, True])
@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_merge_source_sizes(tmp_path, n, flags, via_file):
    # dst: the cells 0 .. 99 of the line; src: n cells from cell 50 on (some common, some new for n > 50)
    # (each map in two calls, the second from beyond the first: its rays cross the first call's voxels, so both maps hold misses)
    far, near = (200.0, 0.1, 0.2), (-3.0, 0.1, 0.2)
    dst, src = _merge_case(tmp_path, flags, [(line(50), far), (line(50, 50), near)],
                           [(line(n // 2, 50), far), (line(n - n // 2, 50 + n // 2), near)], via_file)
    assert len(src) == n and len(dst) == max(100, 50 + n)
    if flags & 1 and n >= 63:
        assert src.misses().sum() > 0 and dst.misses().sum() > src.misses().sum()


@pytest.mark.parametrize("via_file", [False, True])
def test_merge_all_keys_common_and_none(tmp_path, via_file):
    dst, _ = _merge_case(tmp_path, 3, [(line(100), (60.0, 0.1, 0.2))], [(line(100), (-3.0, 0.3, 0.2))], via_file)
    assert len(dst) == 100 and dst.points()[:, 3].tolist() == [2.0] * 100
    dst, _ = _merge_case(tmp_path, 3, [(line(100), (60.0, 0.1, 0.2))], [(line(100, 100), (-3.0, 0.3, 0.2))], via_file)
    assert len(dst) == 200 and dst.points()[:, 3].tolist() == [1.0] * 200


@pytest.mark.parametrize("via_file", [False, True])
def test_merge_doubles_the_table(tmp_path, via_file):
    d0 = new_map(3)
    d0.add(line(400), (0.0, 3.0, 0.2))
    assert d0.stats()["slots"] == 1024 and d0.rehashes == 0
    dst, src = _merge_case(tmp_path, 3, [(line(400), (0.0, 3.0, 0.2))], [(line(400, 400), (0.0, 3.0, 0.2))], via_file)
    assert dst.rehashes == 1 and dst.stats()["slots"] == 2048 and len(dst) == 800 and src.stats()["slots"] == 1024


def test_merge_at_the_edge_of_the_key_range(tmp_path):
    # voxels in the last cells of the key range on both signs, |i| = 2^20 - 1, as test_step_at_the_edge_of_the_key_range builds them
    x_edge = float(1 << 19)

    def patch(ks):
        hi, lo = line(len(ks)), line(len(ks))
        hi[:, 0] = [x_edge - 0.25 - 0.5 * k for k in ks]
        lo[:, 0] = [-x_edge + 0.75 + 0.5 * k for k in ks]
        return [(hi, (x_edge - 4.0, 0.1, 0.2)), (lo, (-x_edge + 4.0, 0.1, 0.2))]

    dst, src = _merge_case(tmp_path, 3, patch(range(0, 4)), patch(range(2, 6)))
    keys = fm.read(str(tmp_path / "dst.lxdm"))["keys"]
    ix = (keys & np.uint64((1 << 21) - 1)).astype(np.int64) - (1 << 20)
    assert len(dst) == 12 and ix.min() == -(1 << 20) + 1 and ix.max() == (1 << 20) - 1
    assert dst.stats()["dropped_key"] == 0


def test_merge_from_a_grown_table(scene, tmp_path):
    src_sweeps = [(scene["sweeps"][0][0][50:4050], scene["sweeps"][0][1])]    # 4000 points in one call: 8192 slots
    dst, src = _merge_case(tmp_path, 3, [(line(10, -2), (1.0, 0.4, 0.2))], src_sweeps)
    assert src.stats()["slots"] == 8192 and src.rehashes >= 1 and dst.stats()["slots"] in (1024, 2048)
    d1 = new_map(3)
    d1.add(line(10, -2), (1.0, 0.4, 0.2))
    assert d1.stats()["slots"] == 1024


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _refused(code, call, *watched):
    """call() raises LoamxError(code) and every watched (handle, flags) exports what it did before"""
    before = [exports(d, f) for d, f in watched]
    with pytest.raises(loamx.LoamxError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert [exports(d, f) for d, f in watched] == before
    return str(e.value)


def test_refusals(scene, tmp_path):
    sw = scene["sweeps"]
    dst = feed(new_map(2), sw[:1])
    other_leaf = float(np.nextafter(np.float32(LEAF), np.float32(1.0)))
    near = feed(new_map(2, leaf=other_leaf), sw[1:2])
    path2 = saved(feed(new_map(2), sw[1:2]), tmp_path, "moments.lxdm")[0]
    path0 = saved(feed(new_map(0), sw[1:2]), tmp_path, "plain.lxdm")[0]
    assert "leaf" in _refused(loamx.E_INVALID, lambda: dst.merge(near), (dst, 2), (near, 2))    # one bit of the leaf
    assert "leaf" in _refused(loamx.E_INVALID, lambda: near.merge_file(path2), (near, 2))
    assert "leaf" in _refused(loamx.E_INVALID, lambda: new_map(0, leaf=other_leaf).load(path2))
    plain, both = feed(new_map(0), sw[1:2]), feed(new_map(3), sw[1:2])
    for a, fa, b, fb in ((dst, 2, plain, 0), (plain, 0, dst, 2), (dst, 2, both, 3), (both, 3, dst, 2)):
        assert "features" in _refused(loamx.E_INVALID, lambda: a.merge(b), (a, fa), (b, fb))
    assert "features" in _refused(loamx.E_INVALID, lambda: dst.merge_file(path0), (dst, 2))
    assert "features" in _refused(loamx.E_INVALID, lambda: plain.merge_file(path2), (plain, 0))
    assert "itself" in _refused(loamx.E_INVALID, lambda: dst.merge(dst), (dst, 2))
    assert "empty" in _refused(loamx.E_INVALID, lambda: dst.load(path2), (dst, 2))
    # a moments file into a handle that has carving: refused, and the handle has not gained the moments
    carved = new_map(1)
    assert "lacks" in _refused(loamx.E_INVALID, lambda: carved.load(path2), (carved, 1))
    with pytest.raises(loamx.LoamxError):
        carved.moments()
    assert carved.stats()["offered"] == 0
    # a corrupt file (two keys swapped: only the deep validation sees it)
    raw = bytearray(open(path2, "rb").read())
    raw[128:136], raw[136:144] = raw[136:144], raw[128:136]
    bad = str(tmp_path / "bad.lxdm")
    open(bad, "wb").write(bytes(raw))
    assert "keys[1]" in _refused(loamx.E_INVALID, lambda: dst.merge_file(bad), (dst, 2))
    fresh = new_map(2)
    assert "keys[1]" in _refused(loamx.E_INVALID, lambda: fresh.load(bad), (fresh, 2))
    assert "cannot open" in _refused(loamx.E_INVALID, lambda: fresh.load(str(tmp_path / "missing.lxdm")), (fresh, 2))
    # a save into a missing directory leaves no file behind
    _refused(loamx.E_INVALID, lambda: dst.save(str(tmp_path / "no_such_dir" / "map.lxdm")), (dst, 2))
    assert not os.path.exists(tmp_path / "no_such_dir") and not [f for f in os.listdir(tmp_path) if f.endswith(".part")]


def test_capacity(tmp_path):
    src = new_map(0)
    src.add(line(50, 80), (0.0, 3.0, 0.2))    # 20 cells in common with dst: the bound counts them twice
    path = saved(src, tmp_path, "src.lxdm")[0]
    for cap, fits in ((150, True), (149, False)):
        for via_file in (False, True):
            dst = new_map(0, max_voxels=cap)
            dst.add(line(100), (0.0, 3.0, 0.2))
            call = (lambda: dst.merge_file(path)) if via_file else (lambda: dst.merge(src))
            if fits:
                call()
                assert len(dst) == 130
            else:
                _refused(loamx.E_CAPACITY, call, (dst, 0), (src, 0))
    for cap, fits in ((50, True), (49, False)):
        e = new_map(0, max_voxels=cap)
        if fits:
            e.load(path)
            assert exports(e, 0) == exports(src, 0)
        else:
            _refused(loamx.E_CAPACITY, lambda: e.load(path), (e, 0))
            assert len(e) == 0


# ---- snapshot isolation -------------------------------------------------------------------------------------------------------------
def test_snapshot_isolation(scene):
    sw = scene["sweeps"]
    dst, src = feed(new_map(2), sw[:2]), feed(new_map(2), sw[2:])
    n_dst, n_src = dst.freeze(), src.freeze()
    P = scene["start"]
    rtc = am.rtc_of(P[:, :3], P[:, 3])
    before = [h.align_step(scene["cloud"], rtc, 1) for h in (dst, src)]
    dst.merge(src)
    for h, (s, c), n in zip((dst, src), before, (n_dst, n_src)):
        s2, c2 = h.align_step(scene["cloud"], rtc, 1)
        assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes() and c[am.MATCHED] > 500 and h.frozen_size == n
    assert before[0][0].tobytes() != before[1][0].tobytes()
    assert dst.freeze() >= n_dst    # a new freeze sees the merged map
    assert dst.align_step(scene["cloud"], rtc, 1)[0].tobytes() != before[0][0].tobytes()
