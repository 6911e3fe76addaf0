"""Pose graph (loamx_posegraph_*): a synthetic run of --nodes poses, laps of --lap nodes around a circle with a slow climb, odometry
edges k -> k + 1 and --loops loop edges between the same place on different laps, every measurement with noise --sigma-t / --sigma-r;
the start is the integrated noisy odometry, node 0 fixed.
Prints the wall time of loamx_posegraph_optimize (median [min, max] of --reps, each on a fresh handle), with LM steps, CG iterations,
looks and launches;  --cg-batches 1,2,4,...,64 repeats it for each number of CG iterations per look (how the default cg_batch is
chosen);  --cpu runs the same Gauss-Newton on the host with scipy.sparse.linalg.spsolve on the full system.
There is no reference implementation to race: no time is gated."""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=10000)
ap.add_argument("--lap", type=int, default=500)
ap.add_argument("--loops", type=int, default=200)
ap.add_argument("--sigma-t", type=float, default=0.02)
ap.add_argument("--sigma-r", type=float, default=0.002)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--max-iterations", type=int, default=50)
ap.add_argument("--max-cg-iterations", type=int, default=500)
ap.add_argument("--cg-batches", default="", help="comma-separated CG iterations per look to sweep")
ap.add_argument("--cpu", action="store_true", help="also time Gauss-Newton with scipy's sparse direct solver on the host")
args = ap.parse_args()

from loam_velodyne_amd import loamx


def hat(w):
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -w[..., 2], w[..., 1], w[..., 2], -w[..., 0], -w[..., 1], w[..., 0]
    return K


def exp(w):
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a, b = np.where(small, 1.0, np.sin(ths) / ths), np.where(small, 0.5, (1.0 - np.cos(ths)) / ths ** 2)
    K = hat(w)
    return np.eye(3) + a * K + b * (K @ K)


def log(R):
    v = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.linalg.norm(v, axis=-1)
    th = np.arctan2(s, 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0))
    return v * np.where(th < 1e-8, 1.0, th / np.where(s > 0, s, 1.0))[..., None]


def jr_inv(phi):
    th = np.linalg.norm(phi, axis=-1)[..., None, None]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    q = np.where(small, 1.0 / 12.0, 1.0 / ths ** 2 - (1.0 + np.cos(ths)) / (2.0 * ths * np.sin(ths)))
    K = hat(phi)
    return np.eye(3) + 0.5 * K + q * (K @ K)


def pack(R, t):
    return np.concatenate([R, t[..., None]], -1).reshape(len(R), 12)


rng = np.random.default_rng(1)
N = args.nodes
k = np.arange(N)
ang = 2.0 * np.pi * k / args.lap
Rt = exp(np.stack([0.02 * np.sin(3 * ang), ang, 0.02 * np.cos(2 * ang)], -1))
tt = np.stack([50.0 * np.sin(ang), 0.002 * k, 50.0 * np.cos(ang)], -1)
ei = np.concatenate([k[:-1], np.zeros(0, int)])
ej = ei + 1
laps = max(N // args.lap - 1, 0)
if laps and args.loops:
    a = rng.integers(0, N - args.lap, args.loops)
    b = a + args.lap * rng.integers(1, laps + 1, args.loops)
    ok = b < N
    ei, ej = np.concatenate([ei, a[ok]]), np.concatenate([ej, b[ok]])
E = len(ei)
noise = rng.normal(0, 1, (E, 6)) * np.array([args.sigma_t] * 3 + [args.sigma_r] * 3)
RA = np.swapaxes(Rt[ei], -1, -2) @ Rt[ej]
tA = np.einsum("eki,ek->ei", Rt[ei], tt[ej] - tt[ei])
Rz, tz = RA @ exp(noise[:, 3:]), tA + np.einsum("eij,ej->ei", RA, noise[:, :3])
Rs, ts = [Rt[0]], [tt[0]]
for e in range(N - 1):                                      # the start: the noisy odometry integrated
    ts.append(ts[-1] + Rs[-1] @ tz[e])
    Rs.append(Rs[-1] @ Rz[e])
start = pack(np.array(Rs), np.array(ts))
edges = loamx.posegraph_edges(ei, ej, pack(Rz, tz), loamx.posegraph_info_diagonal(args.sigma_t, args.sigma_r))
print("graph: %d nodes, %d edges (%d loops); start off the truth by up to %.2f m" % (N, E, E - (N - 1), np.abs(start - pack(Rt, tt))[:, [3, 7, 11]].max()),
      flush=True)


def device_run(cg_batch=None):
    cfg = dict(max_iterations=args.max_iterations, max_cg_iterations=args.max_cg_iterations, initial_nodes=N, initial_edges=E)
    if cg_batch:
        cfg["cg_batch"] = cg_batch
    times = []
    for _ in range(args.reps):
        g = loamx.PoseGraph(**cfg)
        g.add_nodes(start)
        g.set_fixed(0)
        g.add_edges(edges)
        g.linearise()                                       # (the edges and the table go up, the kernels are loaded)
        s0 = g.stats()
        t0 = time.perf_counter()
        res = g.optimize()
        times.append(time.perf_counter() - t0)
        s1 = g.stats()
        err = np.abs(g.poses() - pack(Rt, tt))[:, [3, 7, 11]].max()
        g.close()
    return times, res, s1["launches"] - s0["launches"], err


def line(what, times, res, launches, err):
    print("%-14s %8.1f ms [%.1f, %.1f]  status %s, %d LM steps (%d accepted), %d CG iterations, %d looks, %d launches, cost %.6g -> %.6g, "
          "off the truth by up to %.3f m" % (what, 1e3 * np.median(times), 1e3 * min(times), 1e3 * max(times), loamx.POSEGRAPH_STATUS[res["status"]],
                                           res["iterations"], res["accepted"], res["cg_iterations"], res["looks"], launches, res["cost_initial"],
                                           res["cost_final"], err), flush=True)


line("optimize", *device_run())
for b in [int(x) for x in args.cg_batches.split(",") if x]:
    line("cg_batch %d" % b, *device_run(b))

if args.cpu:
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    info = np.diag([1.0 / args.sigma_t ** 2] * 3 + [1.0 / args.sigma_r ** 2] * 3)
    R, t = np.array(Rs), np.array(ts)

    def lin(R, t):
        RA = np.swapaxes(R[ei], -1, -2) @ R[ej]
        tA = np.einsum("eki,ek->ei", R[ei], t[ej] - t[ei])
        RE = np.swapaxes(Rz, -1, -2) @ RA
        r = np.concatenate([np.einsum("eki,ek->ei", Rz, tA - tz), log(RE)], -1)
        Q = jr_inv(r[:, 3:])
        Ji, Jj = np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
        Ji[:, :3, :3], Ji[:, :3, 3:], Ji[:, 3:, 3:] = -np.swapaxes(Rz, -1, -2), np.swapaxes(Rz, -1, -2) @ hat(tA), -Q @ np.swapaxes(RA, -1, -2)
        Jj[:, :3, :3], Jj[:, 3:, 3:] = RE, Q
        return r, Ji, Jj

    def cost(R, t):
        r = lin(R, t)[0]
        return float(np.einsum("ei,ij,ej->", r, info, r))
    t0 = time.perf_counter()
    F, steps = cost(R, t), 0
    rows = (6 * np.stack([ei, ei, ej, ej], 1)[:, :, None, None] + np.arange(6)[None, None, :, None] + np.zeros((1, 1, 1, 6), int)).ravel()
    cols = (6 * np.stack([ei, ej, ei, ej], 1)[:, :, None, None] + np.arange(6)[None, None, None, :] + np.zeros((1, 1, 6, 1), int)).ravel()
    while steps < args.max_iterations:
        r, Ji, Jj = lin(R, t)
        WJi, WJj = info @ Ji, info @ Jj
        blocks = np.stack([np.swapaxes(Ji, -1, -2) @ WJi, np.swapaxes(Ji, -1, -2) @ WJj, np.swapaxes(Jj, -1, -2) @ WJi, np.swapaxes(Jj, -1, -2) @ WJj], 1)
        H = sp.coo_matrix((blocks.ravel(), (rows, cols)), shape=(6 * N, 6 * N)).tocsc()
        g = np.zeros((N, 6))
        np.add.at(g, ei, np.einsum("eki,ek->ei", WJi, r))
        np.add.at(g, ej, np.einsum("eki,ek->ei", WJj, r))
        delta = np.zeros(6 * N)
        delta[6:] = spsolve(H[6:, 6:], -g.reshape(-1)[6:])           # (node 0 fixed: its rows and columns removed)
        delta = delta.reshape(N, 6)
        Rn, tn = R @ exp(delta[:, 3:]), t + np.einsum("nij,nj->ni", R, delta[:, :3])
        Fn = cost(Rn, tn)
        steps += 1
        if not Fn < F:
            break
        gain, F, R, t = F - Fn, Fn, Rn, tn
        if np.abs(delta).max() <= 1e-9 or gain <= 1e-12 * (F + gain):
            break
    print("host spsolve   %8.1f ms  %d Gauss-Newton steps, cost -> %.6g, off the truth by up to %.3f m (%d host threads visible)"
          % (1e3 * (time.perf_counter() - t0), steps, F, np.abs(t - tt).max(), os.cpu_count()), flush=True)
