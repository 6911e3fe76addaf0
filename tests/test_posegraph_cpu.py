"""CPU: the pose-graph C-ABI (loamx_posegraph_*; include/loamx.h) — declared and exported, laid out as a C compiler lays it out, its
configuration check, its host-only functions against the numpy model (tests/posegraph_model.py), the model itself against central
differences and on a zero-residual ring, and the launch / Levenberg-Marquardt schedules (loam_velodyne_amd/csrc/posegraph_schedule.hpp)
driven on a CPU with scripted costs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import posegraph_model as pm
from loam_velodyne_amd import loamx

NEW_SYMBOLS = ("loamx_posegraph_default_config", "loamx_posegraph_check", "loamx_posegraph_between", "loamx_posegraph_residual",
               "loamx_posegraph_info_diagonal", "loamx_posegraph_check_gauge", "loamx_posegraph_corrections", "loamx_posegraph_create",
               "loamx_posegraph_destroy", "loamx_posegraph_reset", "loamx_posegraph_add_nodes", "loamx_posegraph_set_fixed",
               "loamx_posegraph_set_poses", "loamx_posegraph_get_poses", "loamx_posegraph_add_edges", "loamx_posegraph_size",
               "loamx_posegraph_linearise", "loamx_posegraph_optimize", "loamx_posegraph_get_stats")
TWO_M40 = 2.0 ** -40


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "loamx.h")).read()
    L = loamx.lib()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
    assert L.loamx_abi_version() == 6   # additive: the ABI number stays
    assert "#define LOAMX_ABI_VERSION 6" in hdr


@pytest.mark.parametrize("c_name,struct", [("loamx_posegraph_config", "PoseGraphConfig"), ("loamx_posegraph_edge", "PoseGraphEdge"),
                                           ("loamx_posegraph_result", "PoseGraphResult")])
def test_layouts_match_c(tmp_path, c_name, struct):
    st = getattr(loamx, struct)
    fields = [f for f, _ in st._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "loamx.h"\nint main(void) {\n'
                     f'  printf("%zu\\n", sizeof({c_name}));\n' +
                     "".join(f'  printf("%zu\\n", offsetof({c_name}, {f}));\n' for f in fields) +
                     '  printf("%u\\n", LOAMX_PG_EDGE_ROBUST);\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(st)
    assert got[1:-1] == [getattr(st, f).offset for f in fields]
    assert got[-1] == loamx.PG_EDGE_ROBUST == pm.ROBUST
    if struct == "PoseGraphEdge":
        assert got[0] == 280 == loamx.POSEGRAPH_EDGE.itemsize == pm.EDGE.itemsize and loamx.POSEGRAPH_EDGE == pm.EDGE
        assert got[1:-1] == [loamx.POSEGRAPH_EDGE.fields[f][1] for f in fields]


def test_default_config():
    c = loamx.PoseGraphConfig()
    assert {f: getattr(c, f) for f, _ in c._fields_} == pm.DEFAULTS
    assert c.check() is c
    assert loamx.lib().loamx_posegraph_check(None) == loamx.E_INVALID


BAD_FIELDS = [dict(max_iterations=10001), dict(max_cg_iterations=0), dict(max_cg_iterations=100001), dict(cg_batch=0), dict(cg_batch=65),
              dict(initial_nodes=0), dict(initial_edges=0), dict(cg_tolerance=0.0), dict(cg_tolerance=1.0), dict(cg_tolerance=float("nan")),
              dict(eps_step=0.0), dict(eps_step=float("inf")), dict(eps_cost=-1e-3), dict(eps_cost=float("nan")), dict(lambda_init=-1.0),
              dict(lambda_init=float("inf")), dict(huber_delta=-0.5), dict(huber_delta=float("nan")), dict(device=-1)]


@pytest.mark.parametrize("bad", BAD_FIELDS, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_check_names_the_bad_field(bad):
    with pytest.raises(loamx.LoamxError) as e:
        loamx.PoseGraphConfig(**bad).check()
    assert e.value.code == loamx.E_INVALID and list(bad)[0] in str(e.value)
    with pytest.raises(loamx.LoamxError) as e:   # (create checks the configuration before it looks for a device)
        loamx.PoseGraph(**bad)
    assert list(bad)[0] in str(e.value)


def test_check_accepts_the_bounds_and_names_the_first_bad_field():
    for ok in (dict(max_iterations=0), dict(max_iterations=10000), dict(max_cg_iterations=1), dict(max_cg_iterations=100000), dict(cg_batch=1),
               dict(cg_batch=64), dict(initial_nodes=1, initial_edges=1), dict(eps_cost=0.0), dict(lambda_init=0.0), dict(huber_delta=0.0),
               dict(cg_tolerance=0.999)):
        loamx.PoseGraphConfig(**ok).check()
    with pytest.raises(loamx.LoamxError) as e:
        loamx.PoseGraphConfig(huber_delta=-1.0, cg_batch=99, eps_step=-1.0).check()
    assert "cg_batch" in str(e.value) and "huber_delta" not in str(e.value) and "eps_step" not in str(e.value)


def test_create_fails_without_gpu():
    if loamx.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(loamx.LoamxError) as e:
        loamx.PoseGraph()
    assert "no HIP device" in str(e.value)


def _pair_with_residual_angle(rng, angle):
    """(Ti, Tj, Z) whose residual rotation has exactly this angle up to rounding: Z = between * (small translation, Exp(-w))"""
    Ti, Tj = pm.random_pose(rng), pm.random_pose(rng)
    w = rng.normal(size=3)
    w *= angle / np.linalg.norm(w)
    Z = pm.pose(pm.rot(pm.between(Ti, Tj)) @ pm.exp(-w), pm.trans(pm.between(Ti, Tj)) + rng.normal(0, 0.2, 3))
    return Ti, Tj, Z


def test_residual_equals_the_model():
    rng = np.random.default_rng(11)
    angles = [0.0, 1e-10, 1e-4, 1.5, 3.0] + list(rng.uniform(0, 3.0, 195))
    worst = 0.0
    for k, a in enumerate(angles):
        Ti, Tj, Z = _pair_with_residual_angle(rng, a)
        if a == 0.0:
            Z = pm.pose(pm.rot(pm.between(Ti, Tj)), pm.trans(Z))
        r, want = loamx.posegraph_residual(Ti, Tj, Z), pm.residual(Ti, Tj, Z)
        if k < 5:
            assert abs(np.linalg.norm(want[3:]) - a) <= 1e-9 * max(a, 1e-7), (a, want)
        worst = max(worst, float(np.abs(r - want).max()))
    print(f"largest |residual - model| over {len(angles)} pairs: {worst:.3e}")
    assert worst <= TWO_M40


def test_between_gives_a_zero_residual():
    rng = np.random.default_rng(12)
    for _ in range(50):
        Ti, Tj = pm.random_pose(rng, 1e4), pm.random_pose(rng, 1e4)
        z = loamx.posegraph_between(Ti, Tj)
        assert z.tobytes() == pm.between(Ti, Tj).tobytes()
        r = loamx.posegraph_residual(Ti, Tj, z)
        assert np.array_equal(r[:3], np.zeros(3))
        assert np.abs(r[3:]).max() < 1e-15


def test_host_functions_refuse_bad_arguments():
    L = loamx.lib()
    T = pm.pose(np.eye(3), [1, 2, 3])
    out = np.zeros(12)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.loamx_posegraph_between(None, p(T), p(out)) == loamx.E_INVALID
    bad = T.copy()
    bad[0] = np.nan
    assert L.loamx_posegraph_between(p(bad), p(T), p(out)) == loamx.E_INVALID and "Ti" in L.loamx_last_error().decode()
    skew = pm.pose(np.eye(3) + 1e-5, [0, 0, 0])
    assert L.loamx_posegraph_residual(p(T), p(skew), p(T), p(out)) == loamx.E_INVALID and "Tj" in L.loamx_last_error().decode()
    mirror = pm.pose(np.diag([1.0, 1.0, -1.0]), [0, 0, 0])
    assert L.loamx_posegraph_residual(p(T), p(T), p(mirror), p(out)) == loamx.E_INVALID and "z" in L.loamx_last_error().decode()
    assert not out.any()
    with pytest.raises(loamx.LoamxError):
        loamx.posegraph_info_diagonal(0.0, 1.0)
    assert loamx.posegraph_info_diagonal(0.05, 0.01).tobytes() == pm.info_diagonal(0.05, 0.01).tobytes()
    assert np.array_equal(pm.info_matrix(loamx.posegraph_info_diagonal(0.5, 0.25)), np.diag([4.0] * 3 + [16.0] * 3))


def test_corrections_move_points_as_rebuild_does():
    """C_k = after_k * before_k^-1 handed to loamx_densemap_correct takes a point given in the map by before_k to where after_k puts it"""
    rng = np.random.default_rng(13)
    before = np.array([pm.random_pose(rng, 50.0) for _ in range(6)])
    after = pm.perturb(before, rng, 0.5, 0.05, keep=())
    Cs = loamx.posegraph_corrections(before, after)
    assert np.abs(Cs - pm.corrections(before, after)).max() <= TWO_M40 * 100.0
    for k in range(6):
        x = rng.uniform(-20, 20, (40, 3))                                       # points in the frame of node k
        in_map = (x @ pm.rot(before[k]).T + pm.trans(before[k])).astype(np.float32)
        want = x @ pm.rot(after[k]).T + pm.trans(after[k])
        got = loamx.correct(Cs[k].reshape(3, 4), in_map)
        assert np.abs(got - want).max() < 3e-5   # (f32 points at 64..128 m: an ulp is 7.6e-6; rounded going in, in the products, coming out)


def test_check_gauge():
    T = pm.pose(np.eye(3), [0, 0, 0])
    I = pm.info_diagonal(1, 1)
    none = pm.edges_of([], [], np.zeros((0, 12)), I)
    cases = [
        ([0], none, 0),                                                                  # a single free node
        ([1], none, None),                                                               # a fixed isolated node
        ([0, 0, 1, 0, 0], pm.edges_of([0, 3], [1, 4], [T, T], I), 0),                    # two components, the fixed node in neither
        ([0, 0, 1, 0, 0], pm.edges_of([0, 3, 1], [1, 4, 2], [T, T, T], I), 3),           # ... now in the first
        ([0, 0, 1, 0, 1], pm.edges_of([0, 3, 1], [1, 4, 2], [T, T, T], I), None),
        ([0, 0, 1, 0, 1], pm.edges_of([1, 4, 2], [0, 3, 1], [T, T, T], I), None),        # the edges given as (j, i)
        ([0, 0, 0, 1], pm.edges_of([3, 2], [2, 1], [T, T], I), 0),                       # node 0 isolated and free
    ]
    for fixed, edges, want in cases:
        assert pm.check_gauge(fixed, edges) == want
        assert loamx.posegraph_check_gauge(fixed, edges) == want
    L = loamx.lib()
    e = pm.edges_of([0], [5], [T], I)
    f = np.zeros(2, np.uint8)
    assert L.loamx_posegraph_check_gauge(2, f.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_uint64(1), None) == loamx.E_INVALID
    assert "edges[0]" in L.loamx_last_error().decode()


@pytest.mark.parametrize("angle", [1e-10, 0.3, 1.5, 3.0])
def test_model_jacobians_against_central_differences(angle):
    rng = np.random.default_rng(14)
    Ti, Tj, Z = _pair_with_residual_angle(rng, angle)
    Ji, Jj = pm.jacobians(Ti, Tj, Z)
    h, worst = 1e-6, 0.0
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        fi = (pm.residual(pm.retract(Ti, d), Tj, Z) - pm.residual(pm.retract(Ti, -d), Tj, Z)) / (2 * h)
        fj = (pm.residual(Ti, pm.retract(Tj, d), Z) - pm.residual(Ti, pm.retract(Tj, -d), Z)) / (2 * h)
        worst = max(worst, float(np.abs(fi - Ji[:, c]).max()), float(np.abs(fj - Jj[:, c]).max()))
    print(f"residual angle {angle}: largest |analytic - central difference| {worst:.2e}")
    assert worst < 1e-7   # (step 1e-6: truncation ~1e-12, rounding ~1e-16 / 1e-6 times the size of the entries)


def test_model_exp_log_branches():
    for w in ([0, 0, 0], [3e-9, -4e-9, 0], [1e-8, 0, 0], [0.3, -0.2, 0.1], [0, 3.0, 0], [1.8, -1.8, 1.8]):
        w = np.array(w, np.float64)
        R = pm.exp(w)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and np.abs(pm.log(R) - w).max() < 1e-15 * max(1.0, 1.0 / np.sinc(np.linalg.norm(w) / np.pi))
    assert np.abs(pm.jr_inv([1e-9, 0, 0]) - pm.jr_inv([1.0001e-8, 0, 0])).max() < 1e-8   # the series branch meets the closed form


def test_model_cost_with_huber():
    assert pm.huber(0.81, True, 1.0) == (1.0, 0.81) and pm.huber(1.0, True, 1.0) == (1.0, 1.0)
    assert pm.huber(4.0, True, 1.0) == (0.5, 3.0) and pm.huber(4.0, False, 1.0) == (1.0, 4.0) and pm.huber(4.0, True, 0.0) == (1.0, 4.0)
    truth, e = pm.ring_graph(6, loops=())
    P = truth.copy()
    P[3] = pm.retract(P[3], np.array([0.4, 0, 0, 0, 0, 0]))      # two edges see it: chi2 = (0.4 / 0.05)^2 = 64 each
    assert abs(pm.cost(P, e) - 128.0) < 1e-9
    e["flags"][2] = pm.ROBUST
    assert abs(pm.cost(P, e, 2.0) - (64.0 + 2 * 2.0 * 8.0 - 4.0)) < 1e-9
    lin = pm.linearise(P, [1, 0, 0, 0, 0, 0], e, 2.0)
    assert abs(lin["cost"] - 92.0) < 1e-9 and not lin["grad"][0].any() and not lin["diag"][0].any() and lin["grad"][3].any()


def test_model_dense_lm_recovers_a_zero_residual_ring():
    rng = np.random.default_rng(15)
    truth, e = pm.ring_graph()
    fixed = np.zeros(40, bool)
    fixed[0] = True
    start = pm.perturb(truth, rng)
    P, res = pm.optimize(start, fixed, e)
    print(f"dense LM: {res}, largest pose error {np.abs(P - truth).max():.2e}")
    assert res["status"] == 0 and res["iterations"] <= 8 and res["cost_final"] < 1e-20 and np.abs(P - truth).max() < 1e-12
    assert P[0].tobytes() == start[0].tobytes()
    Q, res2 = pm.optimize(start, fixed, e, solver="pcg")
    assert res2["status"] == 0 and np.abs(Q - truth).max() < 1e-8


# ---- the schedules --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("posegraph_schedule") / "posegraph_schedule_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "loam_velodyne_amd", "csrc"), os.path.join(ROOT, "tests", "posegraph_schedule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, args, script=()):
    r = subprocess.run([driver] + [str(a) for a in args], input="".join(f"{a!r} {b!r}\n" for a, b in script), capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    last = lines[-1].split()
    return lines[:-1], dict(zip(last[1::2], map(float, last[2::2])))


def _names(ops):
    return [o.split()[0] for o in ops]


def _lambdas(ops):
    return [float(o.split()[1]) for o in ops if o.startswith("solve")]


@pytest.mark.parametrize("batch,cap,stop,looks,enqueued", [
    (8, 100, 1, 1, 8),        # the stop falls on the first iteration of a batch
    (8, 100, 12, 2, 16),      # ... in the middle of the second
    (8, 100, 16, 2, 16),      # ... on the last of the second
    (8, 100, 17, 3, 24),      # ... on the first of the third
    (8, 100, 0, 1, 8),        # the start already meets it: the first look finds out
    (1, 5, 3, 3, 3),          # batches of one: a look per iteration
    (64, 100, 100, 2, 100),   # exactly at the cap, the second batch cut to 36
    (7, 20, 21, 3, 20),       # never: the cap ends it, 7 + 7 + 6
    (0, 3, 99, 3, 3), (1000, 70, 99, 2, 70),   # batch clamped to 1..64
])
def test_cg_schedule(driver, batch, cap, stop, looks, enqueued):
    ops, out = _run(driver, ["cg", batch, cap, stop])
    assert ops[0] == "begin" and ops.count("begin") == 1
    assert ops.count("iterate") == enqueued == out["enqueued"] and out["looks"] == looks == sum(o.startswith("look") for o in ops)
    assert out["iterations"] == min(stop, cap) and out["stopped"] == (stop <= cap)
    b = min(max(batch, 1), 64)
    runs, n = [], 0                                                              # iterations per batch
    for o in ops[1:]:
        if o == "iterate":
            n += 1
        else:
            runs.append(n)
            n = 0
    assert n == 0 and all(r == b for r in runs[:-1]) and 1 <= runs[-1] <= b and sum(runs) == enqueued


def test_lm_schedule_accepts_and_converges_by_step(driver):
    ops, out = _run(driver, ["lm", 50, 1e-9, 1e-12, 1e-6, 100.0], [(10.0, 0.5), (1.0, 0.1), (0.9, 1e-10)])
    assert _names(ops) == ["linearise", "cost", "solve", "apply", "linearise", "solve", "apply", "linearise", "solve", "apply"]
    assert np.allclose(_lambdas(ops), [1e-6, 1e-7, 1e-8], rtol=1e-12, atol=0)
    assert (out["iterations"], out["accepted"], out["status"], out["cost_initial"], out["cost_final"]) == (3, 3, 0, 100.0, 0.9)
    assert out["last_step"] == 1e-10 and abs(out["lambda_final"] - 1e-9) < 1e-20


def test_lm_schedule_converges_by_cost(driver):
    ops, out = _run(driver, ["lm", 50, 1e-9, 1e-3, 0.0, 100.0], [(50.0, 0.5), (49.99, 0.2)])
    assert (out["iterations"], out["accepted"], out["status"], out["cost_final"], out["lambda_final"]) == (2, 2, 0, 49.99, 0.0)
    _, out = _run(driver, ["lm", 50, 1e-9, 0.0, 0.0, 100.0], [(50.0, 0.5), (49.99, 0.2), (49.0, 0.1), (48.0, 1e-9)])   # eps_cost 0 never fires
    assert (out["iterations"], out["status"]) == (4, 0)


def test_lm_schedule_rejects_restores_and_raises_lambda(driver):
    ops, out = _run(driver, ["lm", 50, 1e-9, 1e-12, 0.0, 100.0],
                    [(100.0, 0.5), (float("nan"), 0.5), (120.0, 0.4), (60.0, 0.3), (60.0, 1e-9)])
    # an equal cost and a NaN cost are rejections; the linearisation is kept through them; lambda 0 -> 1e-6 -> 1e-5 -> 1e-4, then / 10
    assert _names(ops) == ["linearise", "cost", "solve", "apply", "restore", "solve", "apply", "restore", "solve", "apply", "restore",
                           "solve", "apply", "linearise", "solve", "apply", "restore"]
    assert np.allclose(_lambdas(ops), [0.0, 1e-6, 1e-5, 1e-4, 1e-5], rtol=1e-12, atol=0)
    # the last step did not lower F but is no longer than eps_step: converged, poses restored
    assert (out["iterations"], out["accepted"], out["status"], out["cost_final"]) == (5, 1, 0, 60.0)


def test_lm_schedule_lambda_cap_and_max_iterations(driver):
    ops, out = _run(driver, ["lm", 50, 1e-9, 1e-12, 1.0, 100.0], [(200.0, 0.5)] * 13)
    assert (out["iterations"], out["accepted"], out["status"], out["cost_final"]) == (13, 0, 2, 100.0) and out["lambda_final"] > 1e12
    assert ops.count("restore") == 13 and ops.count("linearise") == 1
    ops, out = _run(driver, ["lm", 3, 1e-9, 1e-12, 1.0, 100.0], [(90.0, 0.5), (95.0, 0.5), (80.0, 0.5)])
    assert (out["iterations"], out["accepted"], out["status"], out["cost_final"]) == (3, 2, 1, 80.0)
    ops, out = _run(driver, ["lm", 0, 1e-9, 1e-12, 1.0, 100.0])
    assert ops == ["linearise", "cost"] and (out["iterations"], out["status"], out["cost_initial"], out["cost_final"]) == (0, 1, 100.0, 100.0)
