"""Designed rings for the order-dependent picks of k_feat_ring (csrc/features.hip), a model of the reference's sequential walk and an
analysis that says which path of the kernel each case reaches.  The less-flat half of the kernel pair has tests/lfvoxel_cases.py;
this is the other half: the curvature stencil, the unreliable-point masks, the sort on (curvature bits << 32 | position), the greedy
walks in rounds of 64 candidates and the settlement of the marks that cross a region boundary.

A case is plain data: rings (float32 (len, 4), intensity = ring + k * 2^-13, so every output row names its source point), the
parameters cr, nreg, max_sharp, max_less_sharp, max_flat, thr, and `claims`, what the case was written FOR.  `leaf` defaults to
2^-9 (the device accepts no leaf below 0.001): the designed points are at least 2^-6 apart, every less-flat candidate is alone in its voxel, (0 + x) / 1 == x, and the
less-flat cloud therefore lists exactly the region points that were NOT labelled corner (sorted by voxel, as pcl::VoxelGrid does).

Geometry.  Rings are straight lines, not circles: x = X, y = (k - len / 2) * 2^-5, z = 0, with displacements in x that are multiples
of 2^-5 (spikes; a step of more than 2^-3 + 2^-4 in x would be a gap for markAsPicked) or 2^-12 (zig-zags x = X + (-1)^k b_k).  All
stencil sums are then exact in float32 and equal curvatures are equal whatever the summation order or contraction.  A spike of d at
point i gives c[i] = 4 cr^2 d^2 and a plateau c[i +- 1..cr] = d^2; a zig-zag of b linear in k gives c_k = 16 b_k^2 (cr = 1).  The
parallel-beam test flags a point when both steps exceed 0.0002 * |p|^2: at X = 64 that is 0.82 m^2 and the test is off for every
step used here; at X = 4 (0.0032 m^2 and up) a zig-zag of b = 2^-4 is flagged and one of b = 2^-6 is not.  analyse() reports what the
test did; nothing is assumed.

model(case) restates the reference's walk (BasicScanRegistration.cpp:155-386 as oracle/oracle_features.hpp reads it) in numpy:
float32 arithmetic, the comparisons the source makes in double made in double, one flag array per ring, the regions strictly one
after the other.  It shares no code with the oracle.  model(case, mutant=...) deviates in one line (MUTANTS).

analyse(case) derives from the model's data what the KERNEL does with the case: the launch sizing, the tie groups, the rounds of 64
candidates of each walk, and the settlement rule of k_feat_ring restated over the model's flags (settle(): every region first picked
as if no mark came in, then made again exactly when a final mark of the region before lands on one of its picks).  settle() must
give the sequential walk's picks; tests/test_featring_cases_cpu.py asserts it for every case.

What cannot exist, by search or by reading the source:
  * `(double)wd < 0.1` against `wd < 0.1f`: float(0.1) > 0.1, so wd == float(0.1) is `false` either way and every float below it is
    below both; the two forms agree on all floats.  `float_compares` covers the other three comparisons.
  * a ONE-axis step d with float(d * d) == float(0.05): near 0.22 the squares of neighbouring floats lie two ulps of the square
    apart and the constant falls between them (_steps_with_square finds none in +-64 ulps; the float below float(0.1) is missed the
    same way, float(0.1) itself and the float below float(0.05) are hit).  _step_for() then adds a dyadic step of 2^-6 in x and
    searches d in y: float(dx * dx + d * d) hits the value.
  * "a point the beam test would flag but the `continue` leaves unflagged": the branch that continues has just flagged points
    i - cr .. i, the point i itself included, so skipping its beam test can never be seen in the flags.  The case `mask, far to
    near` holds such a point (analyse: `beam_skipped`) and shows it flagged.
  * 0.0002 * dis: for dis a power of two the float product is exact and float(0.0002) < 0.0002 leaves no float between the two
    limits; _find_beam_disagreement() walks x up from 3 for a dis whose float product rounds ABOVE the double product and a one-axis
    step d with float(d * d) equal to it.
  * regions that depend on the ring's start: (s0 + cr)(nreg - j) + (e0 - cr) j = nreg * s0 + cr (nreg - j) + (len - 1 - cr) j, so s0
    passes through the floor unchanged and the partition of a ring is the same wherever it starts.  `s0_zero` is an equivalent
    mutant (EQUIVALENT_MUTANTS); the start-index family pins the device's handling of the offset instead: same picks at every start."""
import numpy as np

import lfvoxel_cases as lc
from test_gpu_ring_shapes import feat_sizing

F = np.float32
H = 2.0 ** -5          # spacing of a line ring
D = 2.0 ** -3          # unit of a spike
NAMES = ("sharp", "less_sharp", "flat", "less_flat")
FEAT_WAVES = 6
MAX_CR = 16            # loamx_scanreg_config: curvature_region in [1, 16]
MUTANTS = ("ties_reversed", "ties_corner_first", "float_compares", "thr_inclusive", "no_skip_round", "regions_independent",
           "no_cascade", "marks_ignore_gaps", "s0_zero", "mask_off_by_one")


class Case:
    def __init__(self, name, rings, cr=5, nreg=6, max_sharp=2, max_less_sharp=None, max_flat=4, thr=0.1, leaf=2.0 ** -9, **claims):
        self.name, self.cr, self.nreg, self.max_sharp, self.max_flat = name, int(cr), int(nreg), int(max_sharp), int(max_flat)
        self.max_less_sharp = 10 * self.max_sharp if max_less_sharp is None else int(max_less_sharp)
        self.thr, self.leaf, self.claims = F(thr), float(leaf), claims
        self.rings = [np.ascontiguousarray(r, np.float32).reshape(-1, 4) for r in rings]

    def __repr__(self):
        return self.name

    def cloud(self):
        return np.concatenate(self.rings) if self.rings else np.zeros((0, 4), np.float32)

    def sizes(self):
        return [len(r) for r in self.rings]

    def device_config(self):
        return dict(n_feature_regions=self.nreg, curvature_region=self.cr, max_corner_sharp=self.max_sharp,
                    max_corner_less_sharp=self.max_less_sharp, max_surface_flat=self.max_flat, less_flat_filter_size=self.leaf,
                    surface_curvature_threshold=float(self.thr))

    def oracle_config(self):
        return dict(nFeatureRegions=self.nreg, curvatureRegion=self.cr, maxCornerSharp=self.max_sharp,
                    maxCornerLessSharp=self.max_less_sharp, maxSurfaceFlat=self.max_flat, lessFlatFilterSize=self.leaf,
                    surfaceCurvatureThreshold=float(self.thr))


def source_of(row):
    """(ring, index in the ring) of an output row, from its intensity"""
    ring = int(np.floor(row[3]))
    return ring, int(round((float(row[3]) - ring) * 8192))


# ---- the model -----------------------------------------------------------------------------------------------------------------

def _sq(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _sqw(a, b, w):
    d = a - b * w[:, None]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _gt(a, const, mutant):
    """a > const the way the source compares: a (float32) widened to double; float_compares: const narrowed to float32"""
    return a > F(const) if mutant == "float_compares" else a.astype(np.float64) > const


def _lt(a, const, mutant):
    return a < F(const) if mutant == "float_compares" else a.astype(np.float64) < const


def point_pass(P, cr, mutant=None):
    """per point of one ring: the steps' squared lengths, the gaps of markAsPicked, the curvatures (nan where the stencil does not
    fit) and the masks of setScanBuffersFor with the branch each index took"""
    n = len(P)
    xyz = P[:, :3]
    step = _sq(xyz[1:], xyz[:-1])                      # step[k] = |p[k+1] - p[k]|^2
    gaps = np.ones(n, bool)
    gaps[:n - 1] = _gt(step, 0.05, mutant)
    curv = np.full(n, np.nan, np.float32)
    k = np.arange(cr, n - cr)
    d = F(-2 * cr) * xyz[k]
    for j in range(1, cr + 1):
        d = d + (xyz[k + j] + xyz[k - j])
    curv[k] = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    flags = np.zeros(n + 1, np.uint8)                  # (one spare entry: mask_off_by_one writes it)
    i = np.arange(cr, n - 1 - cr + (1 if mutant == "mask_off_by_one" else 0))
    branch = {}
    if len(i):
        pt, nx = xyz[i], xyz[i + 1]
        dn, dp = step[i], step[i - 1]
        d1 = np.sqrt((pt[:, 0] * pt[:, 0] + pt[:, 1] * pt[:, 1]) + pt[:, 2] * pt[:, 2])
        d2 = np.sqrt((nx[:, 0] * nx[:, 0] + nx[:, 1] * nx[:, 1]) + nx[:, 2] * nx[:, 2])
        big = _gt(dn, 0.1, mutant)
        nearer = d1 > d2
        with np.errstate(all="ignore"):
            wd = np.where(nearer, np.sqrt(_sqw(nx, pt, d2 / d1)) / d2, np.sqrt(_sqw(pt, nx, d1 / d2)) / d1).astype(np.float32)
        close = big & _lt(wd, 0.1, mutant)
        dis = (pt[:, 0] * pt[:, 0] + pt[:, 1] * pt[:, 1]) + pt[:, 2] * pt[:, 2]
        if mutant == "float_compares":
            lim = F(0.0002) * dis
            beam = (dn > lim) & (dp > lim)
        else:
            lim = 0.0002 * dis.astype(np.float64)
            beam = (dn.astype(np.float64) > lim) & (dp.astype(np.float64) > lim)
        for q, ii in enumerate(i):
            b = []
            if big[q]:
                b.append("equal_depth" if d1[q] == d2[q] else ("far_to_near" if nearer[q] else "near_to_far"))
                if close[q] and nearer[q]:
                    flags[ii - cr:ii + 1] = 1
                    b.append("occl_back")
                    if beam[q]:
                        b.append("beam_skipped")
                    branch[int(ii)] = b
                    continue
                if close[q]:
                    flags[ii + 1:ii + cr + 2] = 1
                    b.append("occl_fwd")
                else:
                    b.append("wide")
            if beam[q]:
                flags[ii] = 1
                b.append("beam")
            if b:
                branch[int(ii)] = b
    return dict(step=step, gaps=gaps, curv=curv, flags0=flags[:n].copy(), branch=branch)


def region_bounds(s0, length, cr, nreg):
    """[(j, ring-relative first index, size)] of the regions the reference processes (:180-187), s0 = the ring's start in the sweep"""
    e0 = s0 + length - 1
    out = []
    for j in range(nreg):
        sp = ((s0 + cr) * (nreg - j) + (e0 - cr) * j) // nreg
        ep = ((s0 + cr) * (nreg - 1 - j) + (e0 - cr) * (j + 1)) // nreg - 1
        if ep > sp:
            out.append((j, sp - s0, ep - sp + 1))
    return out


def sort_region(c, reverse_ties=False):
    """stable ascending order of the region's curvatures (:311-317); reverse_ties: equal curvatures in reverse position order"""
    return np.lexsort((-np.arange(len(c)), c)) if reverse_ties else np.argsort(c, kind="stable")


def _mark(flags, gaps, i, cr, lo, hi, out, mutant):
    """markAsPicked (:367-386) of ring index i.  lo / hi None: every mark goes to flags (the sequential walk).  Otherwise marks in
    [lo, hi) go to flags, marks at hi and beyond into the set `out`, marks below lo are dropped (mark_as_picked_split).  Returns
    (forward marks made, backward marks made)."""
    flags[i] = 1
    nf = nb = 0
    for t in range(1, cr + 1):
        if gaps[i + t - 1] and mutant != "marks_ignore_gaps":
            break
        nf += 1
        if hi is None or i + t < hi:
            flags[i + t] = 1
        elif out is not None:
            out.add(i + t)
    for t in range(1, cr + 1):
        if gaps[i - t] and mutant != "marks_ignore_gaps":
            break
        nb += 1
        if lo is None or i - t >= lo:
            flags[i - t] = 1
    return nf, nb


def walk_region(case, c, flags, gaps, rscan, mutant=None, split=False, confine=False):
    """the two greedy walks of one region (:197-235) over the ring's flag array, which they mark.  c: the region's curvatures.
    split: marks as mark_as_picked_split leaves them (the outgoing ones returned in `out`); confine: marks outside the region are
    dropped altogether (regions_independent).  The statistics restate region_picks' rounds of 64 candidates."""
    n, cr, thr = len(c), case.cr, case.thr
    lo, hi = (rscan, rscan + n) if (split or confine) else (None, None)
    out = set() if split else None
    asc = sort_region(c, mutant == "ties_reversed")
    desc = sort_region(c, True)[::-1] if mutant == "ties_corner_first" else asc[::-1]
    label = np.zeros(n, np.int8)
    res = dict(order=asc, out=out, label=label, cuts=[])
    above = (lambda v: v >= thr) if mutant == "thr_inclusive" else (lambda v: v > thr)
    below = (lambda v: v <= thr) if mutant == "thr_inclusive" else (lambda v: v < thr)
    for which, seq, ok, limit in (("corner", desc, above, case.max_less_sharp), ("flat", asc, below, case.max_flat)):
        picks, lanes, empty, end = [], [], 0, "exhaustion"
        start, stopped, lead = 0, False, None
        for k, e in enumerate(seq):
            if len(picks) >= limit:
                end = "limit"
                break
            if not ok(c[e]):
                if not stopped:
                    stopped, end = True, "break"
                    res[which + "_stop_lane"] = k - start
                    res[which + "_free_behind_stop"] = int(sum(1 for e2 in seq[k:start + 64] if flags[rscan + e2] == 0))
                continue                               # (the reference walks on; in sorted order nothing behind the first failure passes `ok`)
            if stopped:
                continue
            if k - start == 64:
                empty += 1
                start = k
                if mutant == "no_skip_round":
                    end = "gave up"
                    break
            if flags[rscan + e] == 0:
                if lead is None:
                    lead = k
                picks.append(int(e))
                lanes.append(k - start)
                label[e] = (2 if len(picks) <= case.max_sharp else 1) if which == "corner" else -1
                nf, nb = _mark(flags, gaps, rscan + int(e), cr, lo, hi, out, mutant)
                if nf < cr or nb < cr:
                    res["cuts"].append((int(e), nf, nb))
                start = k + 1
        else:
            if len(picks) >= limit:
                end = "limit"
        res[which] = picks
        res[which + "_lanes"] = lanes
        res[which + "_empty_rounds"] = empty
        res[which + "_end"] = end
        res[which + "_lead"] = lead
        if which == "corner":
            res["flags_after_corner"] = flags[rscan:rscan + n].copy()
    return res


def ring_starts(case):
    return np.concatenate([[0], np.cumsum(case.sizes())]).astype(np.int64)


def is_simple(bounds, nreg, cr):
    """k_feat_ring's s_simple: every region exists and holds at least cr points"""
    return len(bounds) == nreg and all(n >= cr for _, _, n in bounds)


def settle(case, pp, bounds, mutant=None):
    """k_feat_ring's side-by-side picks restated over the model's data: groups of FEAT_WAVES regions, every region first walked from
    flags0 alone (the group's first region with the final marks of the region before it), then, in order, made again exactly when a
    final mark of the region before lands on one of its picks.  no_cascade: the marks a remade region sends on are not looked at
    (the next region sees the first run's)."""
    cr = case.cr
    res, info = [], []
    prev_out, prev_first_out = set(), set()
    for g0 in range(0, len(bounds), FEAT_WAVES):
        for w, (j, rscan, n) in enumerate(bounds[g0:g0 + FEAT_WAVES]):
            c = pp["curv"][rscan:rscan + n]
            head = range(rscan, rscan + min(cr, n))
            alone = pp["flags0"].copy()
            first = walk_region(case, c, alone, pp["gaps"], rscan, split=True)
            inc = prev_first_out if mutant == "no_cascade" else prev_out
            on_picked = sorted(t for t in inc if t in head and first["label"][t - rscan] != 0)
            on_unpicked = sorted(t for t in inc if t in head and first["label"][t - rscan] == 0)
            final, remade, crossed = first, False, False
            if on_picked:
                fl = pp["flags0"].copy()
                for t in inc:
                    if t in head:
                        fl[t] = 1
                final = walk_region(case, c, fl, pp["gaps"], rscan, split=True)
                remade, crossed = w > 0, w == 0    # (wave 0 of a later group starts with the marks in place: it is never made twice)
            info.append(dict(j=j, first=first, final=final, remade=remade, crossed=crossed, on_picked=on_picked, on_unpicked=on_unpicked,
                             out_changed=first["out"] != final["out"], first_out=sorted(first["out"]), final_out=sorted(final["out"])))
            res.append(final)
            prev_out, prev_first_out = final["out"], first["out"]
    return res, info


def model(case, mutant=None):
    """{clouds: the four feature clouds, rings: per ring the point pass, the regions and their walks}"""
    assert mutant is None or mutant in MUTANTS, mutant
    starts = ring_starts(case)
    clouds = {n: [] for n in NAMES}
    rings = []
    for r, P in enumerate(case.rings):
        n, cr = len(P), case.cr
        info = dict(ring=r, s0=int(starts[r]), len=n, processed=n - 1 > 2 * cr, regions=[])
        rings.append(info)
        if not info["processed"]:
            continue
        pp = point_pass(P, cr, mutant)
        bounds = region_bounds(0 if mutant == "s0_zero" else info["s0"], n, cr, case.nreg)
        info.update(pp=pp, bounds=bounds, simple=is_simple(bounds, case.nreg, cr))
        if mutant == "no_cascade" and info["simple"]:
            walks, _ = settle(case, pp, bounds, mutant)
        else:
            flags = pp["flags0"].copy()
            walks = [walk_region(case, pp["curv"][rs:rs + m], flags, pp["gaps"], rs, mutant, confine=mutant == "regions_independent")
                     for _, rs, m in bounds]
        lf = []
        for (j, rs, m), w in zip(bounds, walks):
            info["regions"].append(dict(j=j, start=rs, n=m, **w))
            clouds["sharp"].append(P[rs + np.array(w["corner"][:case.max_sharp], np.int64)])
            clouds["less_sharp"].append(P[rs + np.array(w["corner"], np.int64)])
            clouds["flat"].append(P[rs + np.array(w["flat"], np.int64)])
            lf.append(P[rs + np.flatnonzero(w["label"] <= 0)])
        lf = np.concatenate(lf) if lf else np.zeros((0, 4), np.float32)
        if len(lf):
            clouds["less_flat"].append(voxel_grid(lf, case.leaf))
    return dict(clouds={k: (np.concatenate(v) if v else np.zeros((0, 4), np.float32)).astype(np.float32).reshape(-1, 4) for k, v in clouds.items()},
                rings=rings)


def voxel_grid(c, leaf):
    """pcl::VoxelGrid as tests/lfvoxel_cases.py models it: stable sort by the linear voxel index, float32 sums from 0 in input order"""
    _, ijk, dims, prod = lc._keys(c, leaf)
    if prod > lc.INT_MAX:
        return c.copy()
    rel = ijk - ijk.min(axis=0)
    lin = rel[:, 0] + rel[:, 1] * int(dims[0]) + rel[:, 2] * int(dims[0]) * int(dims[1])
    order = np.argsort(lin, kind="stable")
    st, en = lc._run_bounds(lin[order])
    g = np.zeros((len(st), 4), np.float32)
    for k, (a, b) in enumerate(zip(st, en)):
        g[k] = lc._fsum_rows(c[order[a:b]]) / F(b - a)
    return g


_MODEL, _ORACLE = {}, {}


def cached_model(case):
    """model(case), computed once per case name (the generators are deterministic)"""
    if case.name not in _MODEL:
        _MODEL[case.name] = model(case)
    return _MODEL[case.name]


def cached_oracle(orc, case):
    """the oracle's four feature clouds of the case, computed once per case name and handed out read-only"""
    import oracle_py as op
    if case.name not in _ORACLE:
        f = op.ScanRegistration(orc, **case.oracle_config()).process(case.cloud(), case.sizes())
        for n in NAMES:
            f[n].flags.writeable = False
        _ORACLE[case.name] = {n: f[n] for n in NAMES}
    return _ORACLE[case.name]


def first_difference(got, want):
    """(cloud name, row) of the first difference between two sets of feature clouds compared as uint32 words, or None"""
    for n in NAMES:
        a, b = got[n].view(np.uint32).reshape(-1, 4), want[n].view(np.uint32).reshape(-1, 4)
        k = min(len(a), len(b))
        bad = np.flatnonzero((a[:k] != b[:k]).any(axis=1))
        if len(bad):
            return n, int(bad[0])
        if len(a) != len(b):
            return n, k
    return None


# ---- the analysis --------------------------------------------------------------------------------------------------------------

def _tie_groups(case, reg):
    c = reg["c"]
    groups = []
    vals, inv, cnt = np.unique(c, return_inverse=True, return_counts=True)
    corner, flat = reg["corner"], reg["flat"]
    for g in np.flatnonzero(cnt > 1):
        members = np.flatnonzero(inv == g)
        mset = set(int(m) for m in members)
        d = dict(value=float(vals[g]), members=members, at_threshold=bool(vals[g] == case.thr), straddles=[])
        cin = [k for k, e in enumerate(corner) if e in mset]
        if cin and len(corner) > case.max_sharp and c[corner[case.max_sharp - 1]] == vals[g] == c[corner[case.max_sharp]]:
            d["straddles"].append("max_sharp")
        free_after_corner = [m for m in mset if m not in corner and reg["flags_after_corner"][m] == 0]
        if cin and reg["corner_end"] == "limit" and c[corner[-1]] == vals[g] and free_after_corner:
            d["straddles"].append("max_less_sharp")
        free_at_end = [m for m in mset if m not in flat and reg["flags_end"][m] == 0]
        if reg["flat_end"] == "limit" and flat and c[flat[-1]] == vals[g] and free_at_end:
            d["straddles"].append("max_flat")
        groups.append(d)
    return groups


def analyse(case):
    """per ring: the sizing of the launch it is part of, the masks' branches, the regions with their rounds, ties and cuts, and the
    settlement; see the module docstring"""
    m = cached_model(case)
    L = max(case.sizes()) if case.rings else 0
    size = feat_sizing(max(L, 1), case.nreg, case.cr, case.max_sharp, case.max_less_sharp, case.max_flat)
    stg_cap = min(case.nreg, FEAT_WAVES) * size["nmax"] * 9 // 16
    chunk = stg_cap - 2 * max(case.cr, 1) if size["staged"] else None
    out = []
    for info in m["rings"]:
        a = dict(ring=info["ring"], s0=info["s0"], len=info["len"], processed=info["processed"], sortP=size["sortP"], staged=size["staged"],
                 chunks=-(-info["len"] // chunk) if chunk else 0, chunk=chunk, accepted=size["accepted"], regions=[], simple=None)
        out.append(a)
        if not info["processed"]:
            continue
        pp = info["pp"]
        a.update(simple=info["simple"], branch=pp["branch"], bounds=[(j, s, n) for j, s, n in info["bounds"]],
                 beam_flagged=sorted(k for k, b in pp["branch"].items() if "beam" in b), flags0=pp["flags0"], gaps=pp["gaps"], curv=pp["curv"])
        flags_end = pp["flags0"].copy()
        for reg in info["regions"]:
            # (the ring's flags after everything: replay the marks of all picks)
            for e in reg["corner"] + reg["flat"]:
                _mark(flags_end, pp["gaps"], reg["start"] + e, case.cr, None, None, None, None)
        for reg in info["regions"]:
            rs, n = reg["start"], reg["n"]
            d = dict(reg, c=pp["curv"][rs:rs + n], flags_end=flags_end[rs:rs + n], size=n)
            d["ties"] = _tie_groups(case, d)
            a["regions"].append(d)
        if info["simple"]:
            walks, st = settle(case, pp, info["bounds"])
            a["settlement"] = st
            a["settle_equals_walk"] = all(w["corner"] == reg["corner"] and w["flat"] == reg["flat"] and np.array_equal(w["label"], reg["label"])
                                          for w, reg in zip(walks, info["regions"]))
            a["remade"] = [s["j"] for s in st if s["remade"]]
            a["crossed"] = [s["j"] for s in st if s["crossed"]]
    return out


def region_of(case, ring, index, analysis=None):
    """the analysis of the region that holds point `index` of ring `ring` (None: outside every region)"""
    a = (analysis or analyse(case))[ring]
    for reg in a["regions"]:
        if reg["start"] <= index < reg["start"] + reg["n"]:
            return reg
    return None


def describe_region(reg):
    if reg is None:
        return "outside every region"
    return (f"region {reg['j']} [{reg['start']}, {reg['start'] + reg['n']}) corner picks {reg['corner']} (lanes {reg['corner_lanes']}, "
            f"{reg['corner_empty_rounds']} empty rounds, ended by {reg['corner_end']}), flat picks {reg['flat']} (lanes {reg['flat_lanes']}, "
            f"{reg['flat_empty_rounds']} empty rounds, ended by {reg['flat_end']}), {len(reg['ties'])} tie groups, cuts {reg['cuts']}")


# ---- building blocks -----------------------------------------------------------------------------------------------------------

def line(n, X=64.0, ring=0, centre=None):
    """n points on x = X, y = (k - centre) * 2^-5, z = 0"""
    p = np.zeros((n, 4), np.float32)
    k = np.arange(n)
    p[:, 0] = X
    p[:, 1] = (k - (n // 2 if centre is None else centre)) * H
    p[:, 3] = (ring + k * 2.0 ** -13).astype(np.float32)
    return p


def restamp(p, ring):
    p = np.array(p, np.float32)
    p[:, 3] = (ring + np.arange(len(p)) * 2.0 ** -13).astype(np.float32)
    return p


def spikes(p, at, units=1, unit=D):
    """x += units * unit at the given indices (units: one value or one per index).  A step of more than 2^-3 + 2^-4 in x is a gap
    for markAsPicked, one of 3 * 2^-3 and more enters the occlusion test."""
    p = p.copy()
    p[np.asarray(at, np.int64), 0] += (np.broadcast_to(units, (len(at),)) * unit).astype(np.float32)
    return p


def zigzag(p, b, lo=0, hi=None):
    """x += (-1)^k * b_k for k in [lo, hi)"""
    p = p.copy()
    hi = len(p) if hi is None else hi
    k = np.arange(lo, hi)
    p[k, 0] += (np.where(k % 2 == 0, 1.0, -1.0) * np.broadcast_to(b, (hi - lo,))).astype(np.float32)
    return p


def shift_y(p, start, dy):
    """every point from `start` on moves by dy in y (a step of H + dy between start - 1 and start)"""
    p = p.copy()
    p[start:, 1] += F(dy)
    return p


def ring_len(nreg, per, cr):
    """the length of a first ring (s0 = 0) whose nreg regions hold exactly `per` points each"""
    return nreg * per + 2 * cr + 1


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def tie_cases():
    out = []
    for n in (40, 64, 65):
        out.append(Case(f"ties, all zero, region of {n}", [line(n + 11)], nreg=1, region_size=n, all_equal=0.0, flat=[0, 6, 12, 18], corner=[],
                        straddles="max_flat", corner_stop_lane=0))
    base = line(400)
    two, five = [100, 130], [60, 100, 140, 180, 220]
    for at, tag in ((two, "two"), (five, "five")):
        for ms in (1, 2):
            want = sorted(at, reverse=True)
            out.append(Case(f"ties, {tag} spikes, max_sharp {ms}", [spikes(base, at)], nreg=1, max_sharp=ms, max_less_sharp=10,
                            corner=[w - 5 for w in want], straddles="max_sharp" if ms < len(at) else None, tie_of=len(at)))
    out.append(Case("ties, five spikes across max_less_sharp", [spikes(base, five)], nreg=1, max_sharp=1, max_less_sharp=3,
                    corner=[215, 175, 135], straddles="max_less_sharp"))
    # a zig-zag of constant b: every curvature equal and positive, below the threshold: flat picks among equals
    for cr in (1, 5, MAX_CR):
        zz = zigzag(line(120 + 2 * cr + 1), 2.0 ** -6)
        out.append(Case(f"ties, equal positive curvature, cr {cr}", [zz], cr=cr, nreg=1, thr=0.5, all_equal=True, positive=True,
                        flat=[k * (cr + 1) for k in range(4)], straddles="max_flat"))
        out.append(Case(f"ties, five spikes, cr {cr}", [spikes(line(600), [100, 200, 300, 400, 500])], cr=cr, nreg=1, max_sharp=2,
                        max_less_sharp=4, thr=0.05, corner=[500 - cr, 400 - cr, 300 - cr, 200 - cr], straddles="max_sharp"))
    return out


def threshold_cases():
    """cr = 1: a zig-zag of b = 2^-4 over points [0, 40) (c = 2^-4: corners), of b = 2^-5 over [40, 80) (c = 2^-6 = 0.015625 exactly:
    the threshold) and a straight stretch behind (c = 0: flat).  At the threshold the middle stretch is neither and stops both walks."""
    out = []
    n = 120
    b = np.where(np.arange(n) < 40, 2.0 ** -4, np.where(np.arange(n) < 80, 2.0 ** -5, 0.0))
    base = zigzag(line(n), b)
    t = F(2.0 ** -6)
    for name, thr, stretch in (("at", t, "neither"), ("one ulp below", np.nextafter(t, F(0)), "corner"), ("one ulp above", np.nextafter(t, F(1)), "flat")):
        out.append(Case(f"threshold {name} the tied curvature", [base], cr=1, nreg=1, max_sharp=2, max_less_sharp=100, max_flat=100, thr=thr,
                        stretch=stretch, value=float(t), caught_by=("thr_inclusive",) if stretch == "neither" else ()))
    return out


def _lead_ring(m, kind, X=4.0, n=300):
    """kind corner: the first m points of the region zig-zag with b = 2^-4 (+ a little more each, so they lead the sorted order), which
    the beam test flags at X = 4; the rest with b = 2^-6 (admissible, above thr = 2^-9).  kind flat: m + 2 points 5 * 2^-4 apart in
    the middle of the ring, collinear (curvature 0, both steps long: flagged), the rest 2^-5 apart with a zig-zag of b = 2^-6."""
    if kind == "corner":
        p = line(n, X)
        b = np.full(n, 2.0 ** -6)
        b[1:1 + m] = 2.0 ** -4 + np.arange(m, 0, -1) * 2.0 ** -12
        return zigzag(p, b)
    p = line(n, X)
    p = zigzag(p, 2.0 ** -6)
    a = (n - m) // 2
    p[a:a + m + 2, 0] = X
    y0 = -(m + 1) / 2 * 0.3125
    p[a:a + m + 2, 1] = (y0 + np.arange(m + 2) * 0.3125).astype(np.float32)
    p[:a, 1] = (p[a, 1] - (a - np.arange(a)) * H).astype(np.float32)
    p[a + m + 2:, 1] = (p[a + m + 1, 1] + (1 + np.arange(n - a - m - 2)) * H).astype(np.float32)
    return p


def _tuned(target, kind, X):
    """the ring whose walk meets exactly `target` inadmissible candidates before its first pick"""
    key = "corner_lead" if kind == "corner" else "flat_lead"
    for m in range(max(0, target - 6), target + 7):
        c = Case("probe", [_lead_ring(m, kind, X)], cr=1, nreg=1, max_sharp=1, max_less_sharp=3, max_flat=3, thr=2.0 ** -9 if kind == "corner" else 2.0 ** -7)
        reg = model(c)["rings"][0]["regions"][0]
        if reg[key] == target:
            return c.rings[0]
    raise AssertionError((target, kind))


def round_cases():
    out = []
    for lead in (0, 63, 64, 65, 127, 128):
        out.append(Case(f"rounds, corner walk, {lead} inadmissible first", [_tuned(lead, "corner", 4.0)], cr=1, nreg=1, max_sharp=1, max_less_sharp=3,
                        max_flat=3, thr=2.0 ** -9, corner_lead=lead, corner_empty_rounds=lead // 64, corner_first_lane=lead % 64))
    for lead in (63, 64, 65, 127, 128):
        out.append(Case(f"rounds, flat walk, {lead} inadmissible first", [_tuned(lead, "flat", 1.0)], cr=1, nreg=1, max_sharp=1, max_less_sharp=3,
                        max_flat=3, thr=2.0 ** -7, flat_lead=lead, flat_empty_rounds=lead // 64, flat_first_lane=lead % 64))
    # every candidate of the region flagged by the beam test: nothing is picked, both walks run out
    out.append(Case("rounds, nothing admissible", [zigzag(line(260, 4.0), 2.0 ** -4)], cr=1, nreg=1, thr=2.0 ** -9, picks_nothing=True))
    # corners, then the stop in the same round with free points behind it
    out.append(Case("rounds, stop behind a pick", [spikes(line(120), [40, 70])], nreg=1, max_sharp=1, max_less_sharp=5, thr=0.01, stop_in_round=True))
    return out


# ---- settlement ----------------------------------------------------------------------------------------------------------------
# Regions of 10 points (2 cr), spikes in units of 2^-5.  B: a spike at the region's last point; picked, its marks cover the first five
# points of the next region.  AB: a larger spike A at point 4 whose marks cover the whole region, B included; only when A carries an
# incoming mark is B picked.  A row of AB regions behind one B is a chain in which every remake CAUSES the next.  ACB: A at 3 leaves
# point 9 free, so the first run picks B and marks the next region; the remake picks C at 5 instead, whose marks cover B and reach
# the region's last point: the mark that was sent on is withdrawn.
_B, _AB, _ACB = [(9, 3)], [(4, 6), (9, 3)], [(3, 6), (5, 4), (9, 3)]


def layout_ring(nreg, per, layout, cr=5, ring=0):
    p = line(ring_len(nreg, per, cr), ring=ring)
    for j, sp in layout.items():
        for rel, u in sp:
            p = spikes(p, [cr + j * per + rel], u, 2.0 ** -5)
    return p


def random_spike_ring(seed, nreg, per, cr=5, ring=0):
    rng = np.random.default_rng(seed)
    n = ring_len(nreg, per, cr)
    at = np.unique(rng.integers(cr, n - cr - 1, max(nreg, n // 6)))
    return spikes(line(n, ring=ring), at, rng.integers(1, 7, len(at)), 2.0 ** -5)


def settlement_summary(a):
    """what one side-by-side ring's settlement did, in the words of the claims (region numbers).  added: remade although the first
    run of the region before had sent no mark onto its picks; withdrawn: kept although the first run of the region before had"""
    st = a["settlement"]
    added, withdrawn = [], []
    for prev, s in zip(st[:-1], st[1:]):
        if not prev["remade"]:
            continue
        lo, lab = _start(a, s["j"]), s["first"]["label"]
        first_hit = any(t - lo < len(lab) and lab[t - lo] != 0 for t in prev["first_out"])
        if (s["remade"] or s["crossed"]) and not first_hit:
            added.append(s["j"])
        if not (s["remade"] or s["crossed"]) and first_hit:
            withdrawn.append(s["j"])
    return dict(remade=a["remade"], crossed=a["crossed"], added=added, withdrawn=withdrawn,
                unpicked_only=[s["j"] for s in st if s["on_unpicked"] and not s["on_picked"]],
                out_changed=[s["j"] for s in st if s["out_changed"]])


def _start(a, j):
    return [s for jj, s, n in a["bounds"] if jj == j][0]


def short_ring(ring=0):
    """30 points, two spikes: with six regions of three points each it takes the sequential walk"""
    return spikes(line(30, ring=ring), [9, 17], [2, 1])


def settlement_cases():
    chain = lambda nreg: {0: _B, **{j: _AB for j in range(1, nreg)}}
    out = [Case("settlement, one region remade", [layout_ring(6, 10, {4: _B, 5: _AB})], max_flat=1, remade=[5], crossed=[], caught_by=("regions_independent",)),
           Case("settlement, cascade", [layout_ring(6, 10, chain(6))], max_flat=1, remade=[1, 2, 3, 4, 5], crossed=[], added=[2, 3, 4, 5],
                caught_by=("regions_independent", "no_cascade"))]
    for nreg, crossed in ((7, [6]), (12, [6]), (13, [6, 12])):
        out.append(Case(f"settlement, cascade across the group boundary, {nreg} regions", [layout_ring(nreg, 10, chain(nreg))], nreg=nreg, max_flat=1,
                        remade=[j for j in range(1, nreg) if j % 6], crossed=crossed, caught_by=("regions_independent", "no_cascade")))
    out.append(Case("settlement, marks on unpicked points only", [layout_ring(6, 10, {4: _B})], max_flat=1, remade=[], crossed=[], unpicked_only=[5], caught_by=()))
    out.append(Case("settlement, mark withdrawn", [layout_ring(6, 10, {0: _B, 1: _ACB, 2: _AB})], max_flat=1, remade=[1, 4], crossed=[], withdrawn=[2],
                    caught_by=("regions_independent", "no_cascade")))
    out.append(Case("settlement, mark added", [layout_ring(6, 10, {3: _B, 4: _AB, 5: _AB})], max_flat=1, remade=[4, 5], crossed=[], added=[5],
                    caught_by=("regions_independent", "no_cascade")))
    out.append(Case("settlement, sequential ring beside a cascade", [layout_ring(6, 10, chain(6)), short_ring(1), layout_ring(6, 10, chain(6), ring=2)],
                    max_flat=1, remade=[1, 2, 3, 4, 5], crossed=[], simple=[True, False, True], caught_by=("regions_independent", "no_cascade")))
    # regions of cr, of 3 cr and of more points with spikes at random: whatever the settlement does there, settle() must follow it
    for seed, nreg, per in RANDOM_SETTLEMENT:
        out.append(Case(f"settlement, random spikes, {nreg} regions of {per} (seed {seed})", [random_spike_ring(seed, nreg, per)], nreg=nreg,
                        some_remade=True))
    return out


RANDOM_SETTLEMENT = ((0, 6, 5), (29, 7, 15), (0, 12, 7), (34, 13, 23), (96, 6, 31))


# ---- the double comparisons ----------------------------------------------------------------------------------------------------

def _steps_with_square(target, dx=0.0):
    """the float32 steps d in y with float32(dx * dx + d * d) == target, ascending (dx: a dyadic step in x made at the same time)"""
    dx2 = F(F(dx) * F(dx))
    d = F(np.sqrt(float(target) - float(dx2)))
    for _ in range(64):
        d = np.nextafter(d, F(0))
    out = []
    for _ in range(128):
        if F(dx2 + d * d) == F(target):
            out.append(d)
        d = np.nextafter(d, F(1))
    return out


def _step_for(target):
    """(dx, d): the squares of one-axis steps leave out about every other float32 near 0.05 and 0.1 (d^2 moves by 2 d ulp(d)), so a
    small dyadic dx is added until a d exists"""
    for dx in (0.0, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4, 3 * 2.0 ** -5):
        ds = _steps_with_square(target, dx)
        if ds:
            return dx, ds[0]
    raise AssertionError(target)


def _find_beam_disagreement():
    """x in [3, 5) and a one-axis step d: float32(d * d) == float32(float32(0.0002) * x * x) > 0.0002 * (double)(x * x), so the step
    is `> 0.0002 * dis` in double and not in float32"""
    x = F(3.0)
    for _ in range(200000):
        dis = F(x * x)
        tf = F(F(0.0002) * dis)
        if float(tf) > 0.0002 * float(dis):
            ds = _steps_with_square(tf)
            if ds:
                return x, ds[0], tf
        x = np.nextafter(x, F(8))
    raise AssertionError("no disagreeing input for the beam test")


def double_cases():
    out = []
    # the gap of markAsPicked: point 22 is the only corner (thr between the curvatures of 21 and 22); its backward mark stops at the
    # step 21 -> 22 exactly when that step is a gap, which leaves 21 free for the flat walk
    for name, target, free in (("step^2 == float(0.05)", F(0.05), True), ("step^2 one ulp below float(0.05)", np.nextafter(F(0.05), F(0)), False)):
        dx, d = _step_for(target)
        p = line(40, centre=21)
        p[22:, 0] += F(dx)
        p[22, 1] = d
        p[23:, 1] = (0.25 + np.arange(17) * H).astype(np.float32)
        c = point_pass(p, 1)["curv"]
        out.append(Case(f"double compare, gap, {name}", [p], cr=1, nreg=1, max_sharp=1, max_less_sharp=1, max_flat=40, thr=(float(c[21]) + float(c[22])) / 2,
                        step=(21, 0.05), is_gap=free, corner=[21], flat_has=20 if free else None, flat_lacks=None if free else 20,
                        caught_by=("float_compares", "marks_ignore_gaps") if free else ()))
    # the occlusion test's diffNext > 0.1: at the step the far point's successors 21, 22 are flagged only if the block is entered
    for name, target, enters in (("step^2 == float(0.1)", F(0.1), True), ("step^2 one ulp below float(0.1)", np.nextafter(F(0.1), F(0)), False)):
        dx, d = _step_for(target)
        p = line(40, centre=20)
        p[21:, 0] += F(dx)
        p[21, 1] = d
        p[22:, 1] = (0.375 + np.arange(18) * H).astype(np.float32)
        out.append(Case(f"double compare, occlusion, {name}", [p], cr=1, nreg=1, max_sharp=1, max_less_sharp=1, max_flat=40, thr=0.1,
                        step=(20, 0.1), enters=enters, caught_by=("float_compares",) if enters else ()))
    # the beam test's 0.0002 * dis: point 20 is the only point above thr and is flagged in double, free in float32
    x, d, tf = _find_beam_disagreement()
    p = line(40, float(x), centre=20)
    p[:20, 1] = (-2 * d * np.arange(20, 0, -1)).astype(np.float32)
    p[21, 1], p[22, 1] = d, 2 * d
    p[23:, 1] = (2 * d + (1 + np.arange(17)) * F(H)).astype(np.float32)
    out.append(Case("double compare, beam test, step^2 == float(float(0.0002) * dis)", [p], cr=1, nreg=1, max_sharp=1, max_less_sharp=1, max_flat=4,
                    thr=float(tf) * 0.75, beam_at=20, corner=[], caught_by=("float_compares",)))
    return out


# ---- the masks -----------------------------------------------------------------------------------------------------------------

def jump(p, at, X):
    """points from `at` on move out (or in) along their own bearing to x = X"""
    p = p.copy()
    p[at:, 1] *= F(X) / p[at:, 0]
    p[at:, 0] = X
    return p


def mask_cases():
    out = []
    n, cr = 120, 5
    near = lambda: line(n, 5.0)
    first, last = cr, n - cr - 2
    out.append(Case("mask, near to far at the first index", [jump(near(), first + 1, 8.0)], nreg=1, branch={first: "occl_fwd"}, flagged=list(range(first + 1, first + cr + 2))))
    out.append(Case("mask, far to near at the first index", [jump(jump(near(), 0, 8.0), first + 1, 5.0)], nreg=1, branch={first: "occl_back"},
                    flagged=list(range(0, first + 1))))
    out.append(Case("mask, far to near at the last index", [jump(jump(near(), 0, 8.0), last + 1, 5.0)], nreg=1, branch={last: "occl_back"},
                    flagged=list(range(last - cr, last + 1))))
    out.append(Case("mask, near to far at the last index", [jump(near(), last + 1, 8.0)], nreg=1, branch={last: "occl_fwd"}, flagged=list(range(last + 1, n))))
    # one index beyond the loop: nothing may be flagged (mask_off_by_one flags last - cr + 1 .. last + 1)
    out.append(Case("mask, far to near one beyond the last index", [jump(jump(near(), 0, 8.0), last + 2, 5.0)], nreg=1, branch={}, unflagged=list(range(last - cr + 1, last + 1)),
                    caught_by=("mask_off_by_one",)))
    # a lone far point: near to far in front of it, far to near at it, where the beam test would have flagged it too
    lone = near()
    lone[60, 0] = 8.0
    out.append(Case("mask, far to near", [lone], nreg=1, branch={59: "occl_fwd", 60: "beam_skipped"}, flagged=list(range(55, 66))))
    # equal depths: (5, -6 H) -> (5, +6 H) takes the else branch
    eq = line(n + 11, 5.0)
    eq = np.concatenate([eq[:60], eq[71:]])
    assert eq[59, 1] == -eq[60, 1]
    out.append(Case("mask, equal depths", [restamp(eq, 0)], nreg=1, branch={59: "equal_depth"}, flagged=list(range(60, 66))))
    # a wide step across the beam: diffNext > 0.1 and wd >= 0.1 falls through to the beam test, which does not flag (one long step) ...
    out.append(Case("mask, wide step, beam test passes", [shift_y(near(), 60, 1.0)], nreg=1, branch={59: "wide"}, unflagged=[59, 60]))
    # ... or does (two long steps around point 60)
    out.append(Case("mask, wide step, beam test flags", [shift_y(shift_y(near(), 60, 1.0), 61, 1.0)], nreg=1, branch={59: "wide", 60: "beam"}, flagged=[60]))
    # 64 regions, about 1,000 points: staging chunks of a few dozen points; jumps whose windows lie across a chunk boundary
    L = 1000
    size = feat_sizing(L, 64, cr)
    chunk = 6 * size["nmax"] * 9 // 16 - 2 * cr
    p = line(L, 5.0)
    p = jump(jump(p, 0, 8.0), 3 * chunk + 1, 5.0)        # far to near at 3 chunk: flags 3 chunk - cr .. 3 chunk
    p = jump(p, 7 * chunk, 8.0)                          # near to far at 7 chunk - 1: flags 7 chunk .. 7 chunk + cr
    out.append(Case("mask, windows across staging chunks", [p], nreg=64, branch={3 * chunk: "occl_back", 7 * chunk - 1: "occl_fwd"},
                    flagged=list(range(3 * chunk - cr, 3 * chunk + 1)) + list(range(7 * chunk, 7 * chunk + cr + 1)), chunk=chunk, min_chunks=10))
    return out


# ---- gap breaks ----------------------------------------------------------------------------------------------------------------

def gap_cases():
    """a shift of 0.25 in y from point g on: the step g - 1 -> g is a gap (0.079 m^2, below the occlusion test's 0.1), and g - 1 and g
    carry the ring's largest curvature, (5 * 0.25)^2 each: a tie.  The corner walk picks g first (its backward mark is cut at once),
    then g - 1 (its forward mark is cut at once); without the breaks g - 1 would be suppressed."""
    out = [Case("gap break beside the pick", [shift_y(line(120), 60, 0.25)], nreg=1, cuts=[(60 - 5, 5, 0), (59 - 5, 0, 5)], corner_starts=[55, 54],
                caught_by=("marks_ignore_gaps",))]
    # the same gap exactly on the boundary of regions 2 | 3 (ring of 6 x 20 + 11 points: region j = [5 + 20 j, 25 + 20 j))
    out.append(Case("gap break on a region boundary", [shift_y(line(131), 65, 0.25)], nreg=6, boundary_gap=65, caught_by=("marks_ignore_gaps",)))
    # picks at the first point of the first region and at the last point of the last region
    n = 131
    out.append(Case("picks at the ring's first and last region point", [spikes(line(n), [5, n - 7])], nreg=6, first_last=True))
    return out


# ---- the ring's start index ----------------------------------------------------------------------------------------------------
# (s0 + cr) (nreg - j) + (e0 - cr) j with e0 = s0 + len - 1 is nreg * s0 + cr (nreg - j) + (len - 1 - cr) j: s0 enters as a multiple
# of nreg, the floor of the quotient is s0 + floor(...), and the regions of a ring are the SAME wherever the ring starts in the sweep.
# `s0_zero` is therefore an equivalent mutant (EQUIVALENT_MUTANTS); the family stays, since it still moves the ring's offset, the
# sweep base and the less-flat marks to every residue of nreg, and the device must find the same picks at each.
START_OFFSETS = (0, 1, 2, 3, 4, 5, 12, 13)


def start_ring(ring):
    return spikes(line(300, ring=ring), [5, 52, 53, 101, 149, 150, 197, 245, 246, 293], [1, 2, 1, 2, 1, 2, 1, 2, 1, 2])


def start_index_cases():
    out = [Case("start index, after an empty ring", [np.zeros((0, 4), np.float32), start_ring(1)], start=0, designed=1)]
    for f in START_OFFSETS[1:]:
        out.append(Case(f"start index, after a ring of {f}", [line(f, ring=0), start_ring(1)], start=f, designed=1))
    return out


# ---- sort sizes ----------------------------------------------------------------------------------------------------------------
SORT_LENGTHS = ((56, 64), (57, 128), (120, 128), (121, 256), (248, 256), (249, 512), (504, 512), (505, 1024))


def sort_cases():
    """one region (cr = 1) of L - 3 points; zig-zag x = X + (-1)^k b_k gives c_k = 16 b_k^2 where b is linear in k"""
    out = []
    for L, sortP in SORT_LENGTHS:
        u = 2.0 ** -10 if L < 130 else 2.0 ** -12
        k = np.arange(L)
        mid = 16 * (L / 2 * u) ** 2
        contents = (("all zero", np.zeros(L), 0.1), ("all equal", np.full(L, 2.0 ** -5), 2.0 ** -8),
                    ("descending", (L - k) * u, mid), ("organ pipe", (1 + np.minimum(k, L - 1 - k)) * u, mid / 4))
        for name, b, thr in contents:
            out.append(Case(f"sort {L}, {name}", [zigzag(line(L), b)], cr=1, nreg=1, thr=max(thr, 0.001), sortP=sortP, content=name))
    return out


# ---- mixed batch ---------------------------------------------------------------------------------------------------------------

def mixed_batch_case():
    """a sequential-path ring, a ring too short for a stencil, an empty ring and a ring whose regions go through the LDS sort side
    by side, then a cascade and a gap ring: one launch sized by the longest"""
    k = np.arange(3100)
    rings = [short_ring(0), line(8, ring=1), np.zeros((0, 4), np.float32),
             zigzag(line(3100, ring=3), (1 + np.minimum(k, 3099 - k) % 517) * 2.0 ** -12),
             layout_ring(6, 10, {0: _B, **{j: _AB for j in range(1, 6)}}, ring=4), shift_y(line(131, ring=5), 65, 0.25), line(11, ring=6), line(12, ring=7)]
    return Case("mixed batch", rings, ring_lens=[30, 8, 0, 3100, 71, 131, 11, 12], sortP=1024, simple=[False, None, None, True, True, True, None, False])


def all_cases():
    return (tie_cases() + threshold_cases() + round_cases() + settlement_cases() + double_cases() + mask_cases() + gap_cases()
            + start_index_cases() + sort_cases() + [mixed_batch_case()])


_ALL = []


def cases():
    """all_cases(), generated once"""
    if not _ALL:
        _ALL.extend(all_cases())
    return _ALL


def by_name(name, cases_=None):
    return [c for c in (cases() if cases_ is None else cases_) if c.name == name][0]


EQUIVALENT_MUTANTS = ("s0_zero",)
REUSE_ORDER = ("settlement, cascade across the group boundary, 13 regions", "ties, five spikes, cr 16", "sort 505, organ pipe",
               "mask, windows across staging chunks", "rounds, corner walk, 128 inadmissible first", "double compare, gap, step^2 == float(0.05)",
               "settlement, cascade across the group boundary, 13 regions")


