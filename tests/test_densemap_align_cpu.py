"""CPU: the alignment against the dense map's frozen snapshot (include/loamx.h, loamx_densemap_freeze ...) — every new symbol declared and
exported, the two new structs laid out as a C compiler lays them out, the default configuration, loamx_densemap_align_solve (host
only) against the model's solve (tests/densemap_align_model.py: numpy's eigh) on sums the model's step produced, bad arguments refused
without a device, and the model's own properties: sums that do not depend on the order of the points, the tie rule, recovery of a
known pose in the box scene.

Tolerance of the solve, 1e-9 of the largest component of x: two double-precision eigen-solvers on a 6x6 system whose condition number
in the compared cases is below 1e4 (about 1e-12).  Bars of the recovery: leaf / 10 and 0.01 rad, the bars of the GPU test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import densemap_align_model as am
import densemap_moments_model as mm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_densemap_freeze", "loamx_densemap_frozen_size", "loamx_densemap_align_step", "loamx_densemap_align_default_config",
               "loamx_densemap_align_solve", "loamx_densemap_align", "loamx_densemap_align_from_map", "loamx_densemap_align_from_pipeline")
CONFIG_FIELDS = ["max_iterations", "neighbourhood", "max_residual", "min_matched", "eps_rot", "eps_trans", "degenerate_ratio"]
RESULT_FIELDS = ["pose", "iterations", "degenerate_dims", "status", "rms", "counts"]


def frozen_of_scene(sweeps, leaf):
    """the model's snapshot of a map fed with (points, origin) sweeps: (keys, records)"""
    m = mm.MomentsModel(leaf=leaf)
    for p, o in sweeps:
        assert m.add(p, o)
    return am.frozen_of(m.keys, m.surfels()[0])


@pytest.fixture(scope="module")
def box():
    S = am.box_scene()
    S["keys"], S["recs"] = frozen_of_scene(S["sweeps"], S["leaf"])
    return S


@pytest.fixture(scope="module")
def plane():
    keys, recs = frozen_of_scene([(am.lattice_plane(), am.PLANE_ORIGIN)], 0.5)
    return dict(keys=keys, recs=recs, cloud=am.lattice_plane()[::3].copy())


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    for name in ("freeze", "align_step", "align", "align_from", "align_from_pipeline"):
        assert callable(getattr(loamx.DenseMap, name)), name
    assert isinstance(loamx.DenseMap.frozen_size, property) and callable(loamx.align_solve)
    assert loamx.ALIGN_COUNTS == ("far", "outside", "unmatched", "rejected", "matched")


@pytest.mark.parametrize("c_name,py,fields", [("loamx_densemap_align_config", "AlignConfig", CONFIG_FIELDS),
                                              ("loamx_densemap_align_result", "AlignResult", RESULT_FIELDS)])
def test_struct_layout_matches_c(tmp_path, c_name, py, fields):
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    t = getattr(loamx, py)
    assert got[0] == C.sizeof(t)
    assert got[1:] == [getattr(t, f).offset for f in fields]
    assert [f for f, _ in t._fields_] == fields


def test_default_configuration():
    c = loamx.AlignConfig()
    got = {f: getattr(c, f) for f in CONFIG_FIELDS}
    assert got == {k: (np.float32(v) if isinstance(v, float) else v) for k, v in am.DEFAULTS.items()}
    c.max_iterations, c.min_matched = 3, 7
    loamx.lib().loamx_densemap_align_default_config(C.byref(c))   # (host only: no device needed)
    assert (c.max_iterations, c.min_matched) == (20, 50)
    loamx.lib().loamx_densemap_align_default_config(None)
    assert loamx.AlignConfig(neighbourhood=0, max_residual=0.25).neighbourhood == 0


def test_solve_equals_the_models_solve(box):
    cases = 0
    for case in range(3):
        S = am.box_scene(case=case)
        P = S["start"]
        for nb in (0, 1):
            sums, counts = am.step(box["keys"], box["recs"], S["cloud"], am.rtc_of(P[:, :3], P[:, 3]), S["leaf"], nb)
            assert counts[am.MATCHED] > 1000
            H = am.system_of(sums)[0]
            assert np.linalg.cond(H) < 1e4
            for ratio in (1e-4, 0.0, 0.5):
                want, want_dropped = am.solve(sums, ratio)
                got, dropped = loamx.align_solve(sums, ratio)
                assert dropped == want_dropped and (dropped == 0) == (ratio < 0.5)
                assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (got, want)
                cases += 1
            assert np.linalg.norm(am.solve(sums)[0]) > 0.01   # (a real update, not a comparison of zeros)
    assert cases == 18


def test_exact_plane_drops_three_directions(plane):
    P = np.concatenate([am.exp_so3([0.01, -0.02, 0.0]), np.array([[0.05], [-0.03], [0.04]])], axis=1)
    sums, counts = am.step(plane["keys"], plane["recs"], plane["cloud"], am.rtc_of(P[:, :3], P[:, 3]), 0.5)
    assert counts[am.MATCHED] == len(plane["cloud"])
    H = am.system_of(sums)[0]
    assert not H[2:5].any() and not H[:, 2:5].any()   # normals exactly (0, 0, 1): nothing sees rotation about z, nor x and y
    x, dropped = loamx.align_solve(sums)
    assert dropped == 3
    assert x[2] == 0.0 and x[3] == 0.0 and x[4] == 0.0
    want, want_dropped = am.solve(sums)
    assert want_dropped == 3 and np.abs(x - want).max() <= 1e-9 * np.abs(want).max()
    assert abs(x[5] + 0.04) < 1e-3 and abs(x[0] + 0.01) < 1e-3 and abs(x[1] - 0.02) < 1e-3
    # nothing matched: every direction is dropped and the update is zero
    x, dropped = loamx.align_solve(np.zeros(28, np.int64))
    assert dropped == 6 and not x.any()


def test_invalid_arguments():
    L = loamx.lib()
    sums = (C.c_int64 * 28)()
    x = (C.c_double * 6)()
    dropped = C.c_uint32(0)
    assert L.loamx_densemap_align_solve(sums, C.c_float(1e-4), x, C.byref(dropped)) == loamx.OK
    for args in ((None, C.c_float(1e-4), x, C.byref(dropped)), (sums, C.c_float(1e-4), None, C.byref(dropped)),
                 (sums, C.c_float(1e-4), x, None), (sums, C.c_float(-0.1), x, C.byref(dropped)),
                 (sums, C.c_float(1.0), x, C.byref(dropped)), (sums, C.c_float(float("nan")), x, C.byref(dropped))):
        assert L.loamx_densemap_align_solve(*args) == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.align_solve(np.zeros(28, np.int64), 2.0)
    assert e.value.code == loamx.E_INVALID and "degenerate_ratio" in str(e.value)


def test_model_sums_do_not_depend_on_the_order(box, plane):
    rng = np.random.default_rng(5)
    P = box["start"]
    for S, rtc, leaf in ((box, am.rtc_of(P[:, :3], P[:, 3]), box["leaf"]), (plane, am.rtc_of(t=(0.01, 0.02, 0.03)), 0.5)):
        for nb in (0, 1):
            sums, counts = am.step(S["keys"], S["recs"], S["cloud"], rtc, leaf, nb)
            perm = rng.permutation(len(S["cloud"]))
            sums2, counts2 = am.step(S["keys"], S["recs"], S["cloud"][perm], rtc, leaf, nb)
            assert sums.tobytes() == sums2.tobytes() and counts.tobytes() == counts2.tobytes()
            assert sums.any() and counts[am.MATCHED] > 1000


def test_model_tie_goes_to_the_earlier_candidate():
    # two voxels side by side along x whose means and normals differ; the point is exactly as far from one mean as from the other
    keys = am._keys_of_cells(np.array([[-1, 0, 0], [0, 0, 0]], np.int64))
    recs = np.array([[-0.3125, 0.1875, 0.0, 0.0, 0.0, 1.0], [0.1875, 0.1875, 0.25, 0.0, 0.0, 1.0]], np.float32)
    p = np.array([[-0.0625, 0.1875, 0.125, 0.0]], np.float32)
    cls, a, e, which = am.match(keys, recs, p, am.rtc_of(), 0.5, 1)
    assert which.tolist() == [0] and e.tolist() == [[0.25, 0.0, 0.125]]
    e1 = p[0, :3] - recs[1, :3]
    assert float(e1 @ e1) == float(e[0] @ e[0])    # a tie indeed
    sums, counts = am.step(keys, recs, p, am.rtc_of(), 0.5, 1)
    assert counts.tolist() == [0, 0, 0, 0, 1] and sums[26] == int(0.125 * 2 ** 24) and sums[27] == int(0.125 ** 2 * 2 ** 24)
    # with its own cell alone the point never sees the second voxel; one cell further it is unmatched
    assert am.step(keys, recs, p, am.rtc_of(), 0.5, 0)[0][26] == int(0.125 * 2 ** 24)
    assert am.step(keys, recs, p - np.float32([1.0, 0, 0, 0]), am.rtc_of(), 0.5, 0)[1].tolist() == [0, 0, 1, 0, 0]


def test_model_filters():
    keys = am._keys_of_cells(np.array([[0, 0, 0]], np.int64))
    recs = np.array([[0.25, 0.25, 0.25, 0.0, 0.0, 1.0]], np.float32)
    p = np.array([[0.25, 0.25, 0.3, 0], [np.nan, 0, 0, 0], [1024.0, 0, 0, 0], [1023.0, 0, 0, 0], [0.25, 0.25, 0.45, 0]], np.float32)
    sums, counts = am.step(keys, recs, p, am.rtc_of(), 0.5, 1, max_residual=0.1)
    assert counts.tolist() == [2, 0, 1, 1, 1]
    # a translation that puts the cells at the edge of the key range: the last cell inside, and one beyond it
    edge = np.float32((1 << 20) * 0.5)
    sums, counts = am.step(keys, recs, p[:1], am.rtc_of(t=(edge - 0.5, 0, 0)), 0.5, 1)
    assert counts.tolist() == [0, 0, 1, 0, 0]
    sums, counts = am.step(keys, recs, p[:1], am.rtc_of(t=(edge, 0, 0)), 0.5, 1)
    assert counts.tolist() == [0, 1, 0, 0, 0]
    assert am.table_slots(0) == 1024 == am.table_slots(512) and am.table_slots(513) == 2048


@pytest.mark.parametrize("case", [0, 1, 2])
def test_model_recovers_the_pose_in_the_box(box, case):
    S = am.box_scene(case=case)
    r = am.align(box["keys"], box["recs"], S["cloud"], S["start"], S["leaf"])
    rot, trans = am.pose_error(r["pose"], S["truth"])
    rot0, trans0 = am.pose_error(S["start"], S["truth"])
    print(f"case {case}: {r['iterations']} iterations, {rot:.2e} rad, {trans:.2e} m from {rot0:.2e} rad, {trans0:.2e} m; rms {r['rms']:.4f}")
    assert 0.02 <= rot0 + 1e-12 and rot0 <= 0.1 and 0.1 <= trans0 + 1e-12 and trans0 <= 0.4
    assert r["status"] == 0 and r["degenerate_dims"] == 0 and r["iterations"] <= 10
    assert rot <= 0.01 and trans <= S["leaf"] / 10
    assert r["counts"][am.MATCHED] > 0.95 * len(S["cloud"])


def test_model_plane_loop_and_too_few_matches(plane):
    P = np.concatenate([am.exp_so3([0.01, -0.02, 0.0]), np.array([[0.05], [-0.03], [0.04]])], axis=1)
    r = am.align(plane["keys"], plane["recs"], plane["cloud"], P, 0.5)
    assert r["status"] == 0 and r["degenerate_dims"] == 3 and r["iterations"] <= 4
    assert abs(r["pose"][0, 3] - 0.05) < 1e-9 and abs(r["pose"][1, 3] + 0.03) < 1e-9 and abs(r["pose"][2, 3]) < 1e-6
    far = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [50.0]])], axis=1)
    r = am.align(plane["keys"], plane["recs"], plane["cloud"], far, 0.5)
    assert r["status"] == 2 and r["iterations"] == 1 and r["pose"].tobytes() == far.tobytes()
    assert r["counts"].tolist() == [0, 0, len(plane["cloud"]), 0, 0]
