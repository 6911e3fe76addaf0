"""GPU: the pose graph on the device (include/loamx.h, loamx_posegraph_*) against the numpy model (tests/posegraph_model.py): the
linearisation entry by entry, zero-residual graphs back to the truth, a noisy graph with a robust outlier against the model's dense
Levenberg-Marquardt, the exact properties (reproducible bytes, independence of cg_batch, fixed nodes untouched), growth, every refusal,
and the hand-over of the corrections to loamx_densemap_rebuild."""
import ctypes as C

import numpy as np
import pytest

import posegraph_model as pm
from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

TWO_M40 = 2.0 ** -40
SHIFT = np.array([1e4, -2e4, 5e3])


def graph_on_device(poses, fixed, edges, **cfg):
    g = loamx.PoseGraph(**cfg)
    assert g.add_nodes(poses) == 0
    for n in np.flatnonzero(fixed):
        g.set_fixed(int(n))
    g.add_edges(edges)
    return g


def fixed_first(n, *more):
    f = np.zeros(n, bool)
    f[[0, *more]] = True
    return f


def set_residual_rotation(edges, k, poses, angle, rng):
    """edge k gets the z whose residual at these poses has zero translation and a rotation of exactly this angle (0: z = between)"""
    i, j = int(edges["i"][k]), int(edges["j"][k])
    z = pm.between(poses[i], poses[j])
    if angle:
        w = rng.normal(size=3)
        w *= angle / np.linalg.norm(w)
        z = pm.pose(pm.rot(z) @ pm.exp(-w), pm.trans(z))
    edges["z"][k] = z


def chain_case(n, loops, seed, shift=None):
    """a chain of n nodes with `loops` loop edges (some given with i > j), poses 0.3 m / 0.1 rad off the measurements; edges with a
    residual rotation of exactly 0, 1e-10 and 3.0 rad; dense random information matrices; ROBUST edges on both sides of delta = 1"""
    rng = np.random.default_rng(seed)
    truth = pm.ring_truth(n, 3.0 * n / 6.3)
    if shift is not None:
        truth[:, [3, 7, 11]] += shift
    pairs = [(k, k + 1) for k in range(n - 1)]
    for a in rng.choice(n - 12, loops, replace=False):
        b = int(a) + int(rng.integers(8, 12))
        pairs.append((int(a), b) if rng.random() < 0.5 else (b, int(a)))
    e = pm.edges_of([p[0] for p in pairs], [p[1] for p in pairs], [pm.between(truth[a], truth[b]) for a, b in pairs], pm.info_diagonal(0.05, 0.01))
    poses = pm.perturb(truth, rng)
    for k, angle in ((3, 0.0), (4, 1e-10), (5, 3.0), (len(e) - 1, 3.0)):
        set_residual_rotation(e, k, poses, angle, rng)
    for k in range(0, len(e), 5):                                    # a dense Omega = B B^T
        B = rng.normal(size=(6, 6)) * np.array([20, 20, 20, 100, 100, 100])[:, None]
        e["info"][k] = (B @ B.T)[np.triu_indices(6)]
    for k in (7, 8, 9, 10):                                          # ROBUST, inside delta: z a hair off the current relative pose
        set_residual_rotation(e, k, poses, 0.0, rng)
        e["z"][k] = pm.retract(e["z"][k], rng.normal(0, 1.0, 6) * np.array([0.01, 0.01, 0.01, 0.002, 0.002, 0.002]))
    e["flags"][[7, 8, 9, 10, 11, 12, 13, len(e) - 2]] = pm.ROBUST   # ... and outside it
    return poses, fixed_first(n), e, 1.0


def hub_case():
    rng = np.random.default_rng(5)
    truth, e = pm.hub_graph(rng)
    fixed = np.zeros(len(truth), bool)
    fixed[17] = True                                                 # (the hub itself is free: its row is walked)
    return pm.perturb(truth, rng, keep=()), fixed, e, 0.0


def two_node_case():
    rng = np.random.default_rng(6)
    Ti, Tj = pm.random_pose(rng), pm.random_pose(rng)
    z = pm.retract(pm.between(Ti, Tj), np.array([0.2, -0.1, 0.3, 0.05, 0.3, -0.2]))
    return np.array([Ti, Tj]), np.array([False, True]), pm.edges_of([1], [0], [z], pm.info_diagonal(0.05, 0.01)), 0.0


LINEARISE_CASES = {"two_nodes": two_node_case, "chain65": lambda: chain_case(65, 7, 7), "hub300": hub_case,
                   "chain257_shifted": lambda: chain_case(257, 9, 8, SHIFT)}


@pytest.mark.parametrize("name", list(LINEARISE_CASES))
def test_linearise_equals_the_model(name):
    """chi2, grad, diag and cost within 2^-40 * max |array| of the model (about 4,000 ulp of the largest entry: the two differ in the
    order of their sums and in sin / cos / atan2).  Measured on the MI355X: 2^-52 to 2^-54.3 on every array of every graph"""
    poses, fixed, e, delta = LINEARISE_CASES[name]()
    want = pm.linearise(poses, fixed, e, delta)
    g = graph_on_device(poses, fixed, e, huber_delta=delta, initial_nodes=4, initial_edges=4)
    got = g.linearise()
    for key in ("chi2", "grad", "diag"):
        scale = float(np.abs(want[key]).max())
        err = float(np.abs(got[key] - want[key]).max())
        print(f"{name} {key}: largest difference {err:.3e} = 2^{np.log2(max(err, 1e-300) / scale):.1f} * max |{key}| ({scale:.3e})")
        assert err <= TWO_M40 * scale, key
    print(f"{name} cost: {got['cost']!r} against {want['cost']!r}")
    assert abs(got["cost"] - want["cost"]) <= TWO_M40 * want["cost"]
    assert not got["grad"][fixed].any() and not got["diag"][fixed].any()
    if name.startswith("chain"):
        robust = want["chi2"][(e["flags"] & pm.ROBUST) != 0]
        assert (robust < 1.0).sum() >= 3 and (robust > 1.0).sum() >= 3            # Huber on both sides of delta
        assert got["chi2"][3] < 1e-24 and got["chi2"][4] < 1e-12                   # the residuals of exactly 0 and of 1e-10 rad
        assert abs(np.linalg.norm(pm.residual(poses[e["i"][-1]], poses[e["j"][-1]], e["z"][-1])[3:]) - 3.0) < 1e-9
    if name == "hub300":
        assert len(e) == 300 and ((e["i"] == 0) | (e["j"] == 0)).all() and (e["i"] > e["j"]).sum() > 100
    assert g.stats()["linearisations"] == 1 and g.stats()["looks"] == 1


def two_component_case():
    t1, e1 = pm.ring_graph(17, loops=((2, 9),))
    t2, e2 = pm.ring_graph(23, loops=((0, 11), (4, 19)))
    t2 = t2.copy()
    t2[:, [3, 7, 11]] += [100.0, 0.0, -50.0]
    e2 = e2.copy()
    e2["i"] += 17
    e2["j"] += 17
    return np.concatenate([t1, t2]), fixed_first(40, 17 + 5), np.concatenate([e1, e2])


def ring_case():
    truth, e = pm.ring_graph()
    return truth, fixed_first(40), e


def hub_truth_case():
    truth, e = pm.hub_graph(np.random.default_rng(5))
    fixed = np.zeros(len(truth), bool)
    fixed[3] = True                                                  # (a spoke holds the gauge: the hub is free, its row enters every product)
    return truth, fixed, e


@pytest.mark.parametrize("case", [ring_case, hub_truth_case, two_component_case], ids=["ring40", "hub300", "two_components"])
def test_zero_residual_graphs_return_to_the_truth(case):
    """edges from between() of the true poses, the start 0.3 m / 0.1 rad off, the gauge held by fixed nodes at the truth: converged,
    and every pose entry within 10 * eps_step of the truth (inexact steps contract by at most cg_tolerance per step, so the error
    after the stop is below 2 * eps_step).  Measured: 1.8e-15 (ring), 1.8e-14 (hub), 1.4e-14 (two components)"""
    truth, fixed, e = case()
    start = pm.perturb(truth, np.random.default_rng(31), keep=tuple(np.flatnonzero(fixed)))
    g = graph_on_device(start, fixed, e)
    res = g.optimize()
    err = float(np.abs(g.poses() - truth).max())
    print(f"{case.__name__}: {res}, largest pose error {err:.3e}")
    assert res["status"] == 0 and res["bad_pivots"] == 0
    assert err <= 10 * 1e-9
    assert res["cost_final"] <= res["cost_initial"] and res["cost_final"] < 1e-9 * res["cost_initial"]


@pytest.fixture(scope="module")
def noisy():
    start, e = pm.noisy_graph(np.random.default_rng(21))
    fixed = fixed_first(len(start))
    dense, rd = pm.optimize(start, fixed, e, huber_delta=1.0)
    pcg, rp = pm.optimize(start, fixed, e, solver="pcg", huber_delta=1.0)
    return dict(start=start, fixed=fixed, edges=e, dense=dense, result=rd, spread=float(np.abs(dense - pcg).max()))


def test_noisy_graph_equals_the_model(noisy):
    """120 nodes, edge noise 0.05 m / 0.01 rad, 10 loops, one gross outlier loop flagged ROBUST, huber_delta 1, default tolerances.
    The model's own spread, its dense LM against its PCG variant (whose solves end at max_cg_iterations = 500 on this chain), measured
    2.1e-9 on the largest pose entry; the device, which adds rounding and another order of the sums, is allowed 4x that: 8.6e-9.
    cost_final within a relative 1e-9 of the dense model's.  Measured: poses 2.142e-9 off the dense model (the device's solves end at
    the same cap as the model's PCG), cost 1.6e-15."""
    g = graph_on_device(noisy["start"], noisy["fixed"], noisy["edges"], huber_delta=1.0)
    res = g.optimize()
    err = float(np.abs(g.poses() - noisy["dense"]).max())
    rel = abs(res["cost_final"] - noisy["result"]["cost_final"]) / noisy["result"]["cost_final"]
    print(f"device {res}\nmodel {noisy['result']}\nmodel spread {noisy['spread']:.3e}, device against the dense model {err:.3e}, cost {rel:.3e}")
    assert 1e-10 < noisy["spread"] < 1e-8           # (the bound below is the model's, and it is the one written above)
    assert res["status"] == 0
    assert rel <= 1e-9
    assert err <= 4.0 * noisy["spread"]
    chi2 = g.linearise()["chi2"]
    assert chi2[-1] > 100.0 * chi2[:-1].max() / 19.0      # the outlier stayed an outlier: it did not bend the graph


def test_runs_are_reproducible_and_do_not_depend_on_cg_batch(noisy):
    runs = []
    for batch in (16, 16, 1, 7, 64):
        g = graph_on_device(noisy["start"], noisy["fixed"], noisy["edges"], huber_delta=1.0, cg_batch=batch, max_iterations=3, max_cg_iterations=100)
        res = g.optimize()
        runs.append((g.poses().tobytes(), res["cg_iterations"], res["cost_final"], res["iterations"], res["looks"]))
    assert runs[0] == runs[1]                                        # two runs of one input: identical bytes
    assert all(r[:4] == runs[0][:4] for r in runs[2:])               # cg_batch 1, 7, 64: identical poses and CG count
    assert runs[0][1] == 300 and runs[2][4] > runs[0][4] > runs[4][4]   # (cut at the cap here; fewer looks with larger batches)
    truth, fixed, e = ring_case()                                    # ... and where the stop rule ends the solves, in mid-batch
    start = pm.perturb(truth, np.random.default_rng(32))
    ring = []
    for batch in (1, 7, 64):
        g = graph_on_device(start, fixed, e, cg_batch=batch)
        res = g.optimize()
        ring.append((g.poses().tobytes(), res["cg_iterations"], res["cost_final"], res["iterations"]))
    assert ring[0] == ring[1] == ring[2] and ring[0][1] < 500 * ring[0][3]


def test_fixed_nodes_and_rotations(noisy):
    start, e = noisy["start"].copy(), noisy["edges"]
    start[:, :3] *= 1.0 + 3e-7                                       # rotations a little off orthonormal, within what is accepted
    fixed = fixed_first(len(start), 40, 119)
    g = graph_on_device(start, fixed, e, max_iterations=0)
    res = g.optimize()
    assert g.poses().tobytes() == start.tobytes()                    # max_iterations = 0 returns the input bytes
    assert (res["iterations"], res["status"]) == (0, 1) and res["cost_final"] == res["cost_initial"] > 0
    g = graph_on_device(start, fixed, e, huber_delta=1.0)
    g.optimize()
    P = g.poses()
    assert P[fixed].tobytes() == start[fixed].tobytes()              # fixed nodes are unchanged bytewise
    assert not np.array_equal(P[~fixed], start[~fixed])
    R = P.reshape(-1, 3, 4)[~fixed, :, :3]
    worst = float(np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max())
    print(f"largest |R^T R - I| over the free nodes: {worst:.2e}")
    assert worst <= 1e-14


def test_growth_and_increments():
    """rooms of 4 growing by doubling, nodes and edges added between two optimisations: byte for byte what a fresh handle gives that is
    handed the same poses and all the edges in the same order"""
    rng = np.random.default_rng(41)
    truth = pm.ring_truth(350, 60.0)
    pairs = [(k, k + 1) for k in range(299)] + [(int(a), int(a) + 150) for a in rng.choice(149, 50, replace=False)] + \
            [(int(a), int(a) + 3) for a in rng.choice(290, 51, replace=False)]
    more = [(k, k + 1) for k in range(299, 349)]
    assert len(pairs) == 400 and len(more) == 50

    def edges(ps):
        z = [pm.retract(pm.between(truth[a], truth[b]), rng.normal(0, 1, 6) * np.array([0.02] * 3 + [0.005] * 3)) for a, b in ps]
        return pm.edges_of([p[0] for p in ps], [p[1] for p in ps], z, pm.info_diagonal(0.05, 0.01))
    e1, e2 = edges(pairs), edges(more)
    start = pm.perturb(truth, rng, 0.1, 0.02)
    cfg = dict(initial_nodes=4, initial_edges=4, max_iterations=4, max_cg_iterations=60)
    g = loamx.PoseGraph(**cfg)
    assert g.add_nodes(start[:100]) == 0 and g.add_nodes(start[100:300]) == 100
    g.set_fixed(0)
    g.add_edges(e1[:7])
    g.add_edges(e1[7:])
    assert g.size == (300, 400)
    g.optimize()
    mid = g.poses()
    assert g.add_nodes(start[300:]) == 300
    g.add_edges(e2)
    assert g.size == (350, 450)
    r1 = g.optimize()
    fresh = loamx.PoseGraph(**cfg)
    fresh.add_nodes(np.concatenate([mid, start[300:]]))
    fresh.set_fixed(0)
    fresh.add_edges(np.concatenate([e1, e2]))
    r2 = fresh.optimize()
    assert g.poses().tobytes() == fresh.poses().tobytes()
    assert {k: v for k, v in r1.items() if k != "looks"} == {k: v for k, v in r2.items() if k != "looks"} and r1["cost_final"] < r1["cost_initial"]
    s = g.stats()
    assert s["linearisations"] >= 4 and s["cg_iterations"] > r1["cg_iterations"] and s["launches"] > 5 * s["cg_iterations"]
    g.reset()
    assert g.size == (0, 0) and g.stats()["launches"] == s["launches"]           # the statistics are never cleared


def test_refusals_leave_the_graph_unchanged():
    truth, fixed, e = ring_case()
    g = graph_on_device(truth, fixed, e)
    before = g.poses().tobytes()
    L = loamx.lib()
    ok_pose, ok_edge = truth[:1].copy(), e[:1].copy()

    def refused(call, says):
        with pytest.raises(loamx.LoamxError) as err:
            call()
        assert err.value.code == loamx.E_INVALID and says in str(err.value), str(err.value)
        assert g.size == (40, 42) and g.poses().tobytes() == before

    def pose_with(**kw):
        p = ok_pose.copy()
        if "nan" in kw:
            p[0, kw["nan"]] = np.nan
        if "skew" in kw:
            p[0, 1] += 1e-5
        if "mirror" in kw:
            p[0, [2, 6, 10]] *= -1.0
        return p

    def edge_with(**kw):
        x = ok_edge.copy()
        for k, v in kw.items():
            if k in ("i", "j"):
                x[k] = v
            elif k == "z":
                x["z"][0] = v[0]
            elif k == "info":
                x["info"][0][v[0]] = v[1]
        return x
    for bad in (pose_with(nan=3), pose_with(nan=5), pose_with(skew=1), pose_with(mirror=1)):
        refused(lambda: g.add_nodes(np.concatenate([ok_pose, bad])), "poses[1]")
        refused(lambda: g.set_poses(3, bad), "poses[0]")
        refused(lambda: g.add_edges(edge_with(z=bad)), "edges[0].z")
    refused(lambda: g.set_poses(39, truth[:2]), "first + n")
    refused(lambda: g.poses(40, 1), "first + n")
    refused(lambda: g.set_fixed(40), "id")
    refused(lambda: g.add_edges(edge_with(i=40)), "edges[0].i")
    refused(lambda: g.add_edges(edge_with(j=4000000000)), "edges[0].j")
    refused(lambda: g.add_edges(edge_with(i=5, j=5)), "i == j")
    refused(lambda: g.add_edges(np.concatenate([ok_edge, edge_with(info=(0, np.inf))])), "edges[1].info")
    refused(lambda: g.add_edges(edge_with(info=(11, -1e-3))), "negative diagonal")     # entry 11 = (2, 2)
    g.add_edges(edge_with(info=(1, -5.0)))                                              # (an off-diagonal entry may be negative)
    g.reset()
    g = graph_on_device(truth, fixed, e)
    for fn, args in (("loamx_posegraph_add_nodes", (g.h, None, C.c_uint32(1), None)), ("loamx_posegraph_set_poses", (g.h, 0, C.c_uint32(1), None)),
                     ("loamx_posegraph_get_poses", (g.h, 0, C.c_uint32(1), None)), ("loamx_posegraph_add_edges", (g.h, None, C.c_uint64(1))),
                     ("loamx_posegraph_get_stats", (g.h, None)), ("loamx_posegraph_optimize", (None, None)),
                     ("loamx_posegraph_linearise", (None, None, None, None, None)), ("loamx_posegraph_size", (None, None, None))):
        assert getattr(L, fn)(*args) == loamx.E_INVALID and "NULL" in L.loamx_last_error().decode(), fn
    assert g.size == (40, 42) and g.poses().tobytes() == before
    # the gauge: a free node without edges, then a component without a fixed node
    g.add_nodes(truth[:1])
    before, size = g.poses().tobytes(), g.size
    for call in (g.optimize, g.linearise):
        with pytest.raises(loamx.LoamxError) as err:
            call()
        assert err.value.code == loamx.E_INVALID and "gauge" in str(err.value) and "node 40" in str(err.value)
        assert g.size == size and g.poses().tobytes() == before
    g.set_fixed(40)
    g.set_fixed(0, False)
    with pytest.raises(loamx.LoamxError) as err:
        g.optimize()
    assert "gauge" in str(err.value) and "node 0" in str(err.value) and g.poses().tobytes() == before
    g.set_fixed(0)
    assert g.optimize()["status"] == 0                     # (already at the truth)
    assert g.poses()[[0, 40]].tobytes() == np.concatenate([truth[:1], truth[:1]]).tobytes()


def test_all_fixed_and_empty_graphs():
    g = loamx.PoseGraph()
    assert g.optimize()["status"] == 0 and g.linearise()["cost"] == 0.0
    truth, _, e = ring_case()
    g = graph_on_device(truth[:3], [True] * 3, e[:2])
    res = g.optimize()
    assert res["status"] == 0 and res["cost_final"] == res["cost_initial"] and g.poses().tobytes() == truth[:3].tobytes()


def test_corrections_reach_rebuild(tmp_path):
    """place -> align -> edge -> optimize -> corrections -> rebuild at toy size: three sweeps of 500 points registered with drifting
    poses, a pose graph of three nodes and one loop edge, and the rebuilt map equal, word for word, to the map of a fresh handle fed
    with the corrected clouds (rebuild's contract; what is checked here is the layout of the hand-over)"""
    rng = np.random.default_rng(51)
    truth = pm.ring_truth(3, 4.0)
    drift = pm.perturb(truth, rng, 0.4, 0.05)
    cloud = rng.uniform(-6, 6, (500, 3))                                   # the same scene seen from each sensor frame
    sweeps = []
    for k in range(3):
        p = np.zeros((500, 4), np.float32)
        p[:, :3] = cloud @ pm.rot(drift[k]).T + pm.trans(drift[k])
        sweeps.append((p, pm.trans(drift[k]).astype(np.float32)))
    d = loamx.DenseMap(leaf=0.5, initial_slots=1024)
    d.enable_history()
    for p, o in sweeps:
        assert d.add(p, o) == loamx.OK
    g = loamx.PoseGraph()
    g.add_nodes(drift)
    g.set_fixed(0)
    odo = loamx.posegraph_info_diagonal(0.2, 0.05)
    g.add_edges(loamx.posegraph_edges([0, 1], [1, 2], [loamx.posegraph_between(drift[0], drift[1]), loamx.posegraph_between(drift[1], drift[2])], odo))
    g.add_edges(loamx.posegraph_edges([2], [0], [loamx.posegraph_between(truth[2], truth[0])], loamx.posegraph_info_diagonal(0.01, 0.002)))
    assert g.optimize()["status"] == 0
    after = g.poses()
    assert np.abs(pm.between(after[2], after[0]) - pm.between(truth[2], truth[0])).max() < 0.02      # the loop edge closed
    Cs = loamx.posegraph_corrections(drift, after)
    assert Cs.shape == (3, 12) and np.abs(Cs[0] - pm.pose(np.eye(3), [0, 0, 0])).max() < 1e-14 and np.abs(Cs[2] - Cs[0]).max() > 0.05
    d.rebuild(Cs.reshape(3, 3, 4))
    fresh = loamx.DenseMap(leaf=0.5, initial_slots=1024)
    for (p, o), Ck in zip(sweeps, Cs):
        assert fresh.add(loamx.correct(Ck.reshape(3, 4), p), loamx.correct(Ck.reshape(3, 4), o[None])[0]) == loamx.OK

    def saved(m, name):
        path = str(tmp_path / name)
        m.save(path)
        return open(path, "rb").read()

    def counts(m):
        st = m.stats()
        st.pop("slots")
        return st
    assert counts(d) == counts(fresh) and saved(d, "rebuilt.lxdm") == saved(fresh, "fresh.lxdm")
