"""Generated cases for the rolling map's update (tests/rolling_map_model.py states what it computes).  Every case is seeded, named and
carries the claim it is built for; tests/test_rolling_map_cases_cpu.py proves each claim from the model's facts and the model itself
against the oracle, tests/test_gpu_rolling_map.py runs every case on the device and compares words in storage order.

A case: a seed map for load_cubes (corner, surf), a list of steps (pose, corner features, surf features) and a check of the model's
facts.  Three sites carry the class patterns: under the pose POSE_SHIFT the window moves by one cube, so a stored point is valid (the
pose's own cube, V), rest (the map origin's cube, R) or dropped (the window's first x layer, which the shift pushes out, D).  Features
are classed by their x: next to the sensor (valid), 250 m off (an in-window cube outside the neighbourhood: rest), 600 m off (outside
the window: dropped).  Feature lattices sit at 0.5 m (corner) and 1.0 m (surf) with a quarter-metre offset: one feature per voxel, none
at zero; poses are dyadic, so the stack's round trip is exact for them."""
import numpy as np

import rolling_map_model as rm

D, R, V = rm.DROPPED, rm.REST, rm.VALID
POSE = np.array([0, 0, 0, 3.5, 1.25, -2.75], np.float32)            # no shift: cen stays (10, 5, 10)
POSE_SHIFT = np.array([0, 0, 0, 400.5, 1.25, -2.75], np.float32)    # window cube 18 on x: one shift, cen -> (9, 5, 10)
POSE_UP = np.array([0, 0, 0, 3.5, 150.25, -2.75], np.float32)           # window cube 8 on y: one shift, cen -> (10, 4, 10)
SITE = {V: (400.0, 0.0, 0.0), R: (0.0, 0.0, 0.0), D: (-500.0, 0.0, 0.0)}
FEATURE_X = {V: 0.25, R: 250.25, D: 600.25}
SPLIT_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4097, 65 * 2048 + 1)
INSERT_SIZES = (0, 1, 255, 256, 257, 64 * 256 + 1)
NONE = np.zeros((0, 4), np.float32)


def pattern(kind, n, unit=1):
    """class of every position: `point` cycles V, R, D per `unit` positions; `run8` per 8 units; `tile` / `block` per 2048 / 256 in the
    order R, V, D — a tile without a valid point in front of a full one"""
    j = np.arange(n) // unit
    if kind == "point":
        return np.array([V, R, D])[j % 3]
    if kind == "run8":
        return np.array([V, R, D])[(j // 8) % 3]
    if kind == "tile":
        return np.array([R, V, D])[(np.arange(n) // rm.MS_TILE) % 3]
    if kind == "block":
        return np.array([R, V, D])[(np.arange(n) // rm.INS_BLOCK) % 3]
    return np.full(n, {"all_valid": V, "all_rest": R, "all_dropped": D}[kind])


def stored(rng, cls, sites=SITE, half=2.0):
    """general float32 points, several to a voxel, around the site of their class; the intensity is the position"""
    n = len(cls)
    p = np.zeros((n, 4), np.float32)
    if n:
        p[:, :3] = np.array([sites[int(c)] for c in (D, R, V)], np.float64)[np.searchsorted([D, R, V], cls)] + rng.uniform(-half, half, (n, 3))
        p[:, 3] = np.arange(n)
    return p


def features(cls, t, dup=False):
    """one feature per voxel in feature order: position j sits at (y, z) = (j % 64, j / 64) lattice steps (surfs: pairs along x first), so
    the voxel grid's (z, y, x) order is the order of j; x carries the class"""
    n = len(cls)
    step = 0.5 if t == 0 else 1.0
    j = np.arange(n)
    p = np.zeros((n, 4), np.float32)
    if t == 0:
        col, row, sub = j % 64, j // 64, np.zeros(n)
    else:
        sub, col, row = j % 2, (j // 2) % 64, j // 128
    p[:, 0] = np.array([FEATURE_X[c] for c in (D, R, V)])[np.searchsorted([D, R, V], cls)] + sub * step if n else 0
    p[:, 1] = 0.25 + step * col
    p[:, 2] = 0.25 + step * row - 64.0
    p[:, 3] = 1000 + j
    if dup:   # a second point in every voxel: the input is larger than what the down-sizing leaves
        q = p.copy()
        q[:, 0] += 0.0625
        q[:, 3] += 0.5
        p = np.stack([p, q], axis=1).reshape(-1, 4)
    return p


class Case:
    def __init__(self, name, claim, seed, steps, check, lattice=False):
        self.name, self.claim, self.seed, self.steps, self.check, self.lattice = name, claim, seed, steps, check, lattice
        self.from_empty = not (len(seed[0]) or len(seed[1]))


BUILDERS = {}


def case(fn):
    BUILDERS[fn.__name__] = fn
    return fn


def _few_features():
    return features(np.full(3, V), 0), features(np.full(5, V), 1)


def _seed_small(rng):
    cls = np.array([V] * 40 + [R] * 20)
    sites = {V: (0.0, 0.0, 0.0), R: (250.0, 0.0, 0.0), D: (0.0, 0.0, 0.0)}
    return stored(rng, cls, sites), stored(rng, cls, sites)


# ---- k_map_split: tiles of 2048 points, two look-back chains, the bounds fold ---------------------------------------------------
def _split_case(name, claim, kinds, n, seed, check):
    def build():
        rng = np.random.default_rng(seed)
        m = [stored(rng, pattern(kinds[t], n[t], 1), SITE) for t in range(2)]
        return Case(name, claim, (m[0], m[1]), [(POSE_SHIFT,) + _few_features()], check)
    build.__name__ = name
    return case(build)


def _three_classes(F, t, n):
    f = F[0][t]
    k = n // 3
    return f["n_old"] == n and F[0]["shifts"] == (-1, 0, 0) and sum(f["split"]) == n and all(abs(c - k) <= 8 for c in f["split"])


for _n in SPLIT_SIZES:
    _split_case(f"split_{_n}", f"{_n} stored points per type: classes alternate per point (corner) and per run of 8, one thread's share (surf)",
                ("point", "run8"), (_n, _n), 100 + _n % 97,
                lambda F, n=_n: _three_classes(F, "corner", n) and _three_classes(F, "surf", n) and len(F[0]["corner"]["split_tiles"]) == -(-n // 2048))

_split_case("split_all_valid", "every stored point joins the sub-map", ("all_valid", "all_valid"), (4097, 4097), 11,
            lambda F: F[0]["corner"]["split"] == (0, 0, 4097) and F[0]["surf"]["split"] == (0, 0, 4097))
_split_case("split_all_rest", "no tile has a valid point: the bounds fold meets FLT_MAX only, the valid chain carries zeros", ("all_rest", "all_rest"), (4097, 4097), 12,
            lambda F: F[0]["corner"]["split"] == (0, 4097, 0) and not F[0]["surf"]["split_tiles"][:, V].any())
_split_case("split_all_dropped", "every stored point leaves with the shift", ("all_dropped", "all_dropped"), (4097, 4097), 13,
            lambda F: F[0]["corner"]["split"] == (4097, 0, 0) and F[0]["surf"]["split"] == (4097, 0, 0) and F[0]["cubes_pushed_out"] == 2)
_split_case("split_per_tile", "whole tiles of one class: a tile with no valid point in front of a full one, zero totals in both chains", ("tile", "tile"), (3 * 2048 + 5, 2 * 2048), 14,
            lambda F: F[0]["corner"]["split_tiles"].tolist() == [[0, 2048, 0], [0, 0, 2048], [2048, 0, 0], [0, 5, 0]] and
            F[0]["surf"]["split_tiles"].tolist() == [[0, 2048, 0], [0, 0, 2048]])
_split_case("split_corner_empty", "no corner is stored: the split of that type is not launched", ("point", "point"), (0, 2049), 15,
            lambda F: F[0]["corner"]["n_old"] == 0 and F[0]["surf"]["n_old"] == 2049)
_split_case("split_surf_empty", "no surf is stored", ("point", "point"), (2049, 0), 16, lambda F: F[0]["surf"]["n_old"] == 0 and F[0]["corner"]["n_old"] == 2049)
_split_case("split_both_empty", "an empty map", ("point", "point"), (0, 0), 17, lambda F: F[0]["surf"]["n_old"] == 0 and F[0]["corner"]["n_old"] == 0 and F[0]["corner"]["n_new"] == 3)


# ---- k_map_insert: blocks of 256 features, one look-back chain ----------------------------------------------------------------------
def _insert_case(name, claim, kinds, n, check, dup=False):
    def build():
        rng = np.random.default_rng(200 + sum(n))
        f = [features(pattern(kinds[t], n[t], 1 if t == 0 else 2), t, dup) for t in range(2)]
        return Case(name, claim, _seed_small(rng), [(POSE, f[0], f[1])], check)
    build.__name__ = name
    return case(build)


def _one_for_one(F, n):
    return all(F[0][t]["n_ds"] == n and F[0][t]["n_in"] == n and sum(F[0][t]["insert"]) == n and len(F[0][t]["insert_blocks"]) == -(-n // 256) for t in ("corner", "surf"))


for _n in INSERT_SIZES:
    _insert_case(f"insert_{_n}", f"{_n} features per type survive the down-sizing one for one; classes alternate per feature (corner) and per block of 256 (surf)",
                 ("point", "block"), (_n, _n), lambda F, n=_n: _one_for_one(F, n) and (n < 3 or min(F[0]["corner"]["insert"]) >= n // 3))

_insert_case("insert_all_valid", "every feature lands in a valid cube: the rest chain carries zeros", ("all_valid", "all_valid"), (513, 513),
             lambda F: _one_for_one(F, 513) and F[0]["corner"]["insert"] == (0, 0, 513) and F[0]["surf"]["insert"] == (0, 0, 513))
_insert_case("insert_all_rest", "every feature goes behind the rest points", ("all_rest", "all_rest"), (513, 513),
             lambda F: _one_for_one(F, 513) and F[0]["corner"]["insert"] == (0, 513, 0) and F[0]["surf"]["insert"] == (0, 513, 0))
_insert_case("insert_all_dropped", "every feature falls outside the window", ("all_dropped", "all_dropped"), (513, 513),
             lambda F: _one_for_one(F, 513) and F[0]["corner"]["insert"] == (513, 0, 0) and F[0]["surf"]["insert"] == (513, 0, 0) and F[0]["corner"]["n_new"] <= 60)
_insert_case("insert_runs", "classes alternate per run of 8", ("run8", "run8"), (769, 769),
             lambda F: _one_for_one(F, 769) and min(F[0]["corner"]["insert_blocks"][:3].min(), F[0]["surf"]["insert_blocks"][:3].min()) > 0)
_insert_case("insert_corner_none", "one type without features: its counters are cleared, not written by a launch", ("point", "point"), (0, 257),
             lambda F: F[0]["corner"]["n_in"] == 0 and F[0]["surf"]["n_ds"] == 257)
_insert_case("insert_input_larger", "two points per voxel: 514 input slots, 257 down-sized features — slots beyond b - a", ("point", "point"), (257, 257),
             lambda F: all(F[0][t]["n_in"] == 514 and F[0][t]["n_ds"] == 257 for t in ("corner", "surf")), dup=True)


# ---- k_map_append_filtered: the binary search over the per-slot offsets ---------------------------------------------------------
def valid_cubes(pose):
    """absolute cube triples of the valid slots under `pose` from the initial window (no shift)"""
    cen = [10, 5, 10]
    cc = [int(rm.cube_abs(pose[3 + a])) + cen[a] for a in range(3)]
    nb, fov, _, _ = rm.neighbourhood(pose[3:], cen, cc)
    w = nb[fov]
    return np.stack([w % rm.MW - cen[0], (w // rm.MW) % rm.MH - cen[1], w // (rm.MW * rm.MH) - cen[2]], axis=1)


def _in_cubes(rng, cubes, per, base=0):
    p = np.zeros((len(cubes) * per, 4), np.float32)
    p[:, :3] = np.repeat(np.asarray(cubes, np.float64).reshape(-1, 3) * 50.0, per, axis=0) + rng.uniform(-3, 3, (len(p), 3)) + 5.0
    p[:, 3] = base + np.arange(len(p))
    return p


def _append_case(name, claim, old_slots, new_slots, check, rest_only=False):
    def build():
        rng = np.random.default_rng(300 + len(name))
        vc = valid_cubes(POSE)
        nv = len(vc)
        pick = lambda s: [vc[k % nv] for k in s]
        rest_cubes = [(0, 2, 0), (5, 0, 0)]   # inside the neighbourhood but not in the field of view; outside the neighbourhood
        seed = [np.concatenate([_in_cubes(rng, pick(old_slots), 30), _in_cubes(rng, rest_cubes, 10, 5000)]) for _ in range(2)]
        f = []
        for t in range(2):
            m = _in_cubes(rng, pick(new_slots) + (rest_cubes if rest_only else []), 9, 9000)
            m[:, :3] = np.round(m[:, :3] * 4) / 4 + 0.125 - POSE[3:]
            f.append(m)
        return Case(name, claim, tuple(seed), [(POSE, f[0], f[1])], check)
    build.__name__ = name
    return case(build)


def _filled(F, t):
    return np.flatnonzero(F[0][t]["filtered_per_slot"]).tolist()


_append_case("append_lead_mid_trail", "valid slots without output in front of, between and behind the filled ones", [3, 4, 50], [4, 51],
             lambda F: _filled(F, "corner") == [3, 4, 50, 51] and _filled(F, "surf") == [3, 4, 50, 51] and F[0]["nvalid"] > 60)
_append_case("append_all_empty", "no valid slot has output: the filtered part is empty", [], [],
             lambda F: _filled(F, "corner") == [] and _filled(F, "surf") == [] and F[0]["corner"]["insert"][R] > 0 and F[0]["corner"]["n_new"] > 20, rest_only=True)
_append_case("append_one_slot", "one slot holds everything", [7], [7], lambda F: _filled(F, "corner") == [7] and _filled(F, "surf") == [7])
_append_case("append_first_last", "the first and the last slot are filled: no empty slot in front or behind", [0, -1], [0, -1],
             lambda F: _filled(F, "corner") == [0, F[0]["nvalid"] - 1] and _filled(F, "surf") == [0, F[0]["nvalid"] - 1])


# ---- k_map_hist: 4851 LDS bins, a grid capped at 256 blocks ----------------------------------------------------------------------
@case
def hist_grid_stride():
    rng = np.random.default_rng(41)
    cubes = [(i, j, k) for i in range(-2, 4) for j in range(-1, 3) for k in (-1, 0)]
    n = 256 * 2048 + 5712

    def spread(m, base):
        p = np.zeros((m, 4), np.float32)
        p[:, :3] = np.asarray(cubes, np.float64)[rng.integers(0, len(cubes), m)] * 50.0 + rng.uniform(-24.5, 24.5, (m, 3))
        p[:, 3] = base + np.arange(m) % 4096
        return p
    c, s = _few_features()
    return Case("hist_grid_stride", "more than 256 * 2048 surfs in 48 cubes: the histogram's grid-stride loop runs; the next update shifts the window and reads the directory",
                (spread(5000, 0), spread(n, 0)), [(POSE, c, s), (POSE_UP, c, s)],
                lambda F: F[0]["surf"]["n_old"] > 256 * 2048 and F[0]["surf"]["populated_cubes"] >= 40 and F[0]["surf"]["n_new"] > 256 * 2048 and
                F[1]["shifts"] == (0, -1, 0) and F[1]["surf"]["n_sub"] > 0 and F[1]["surf"]["split"][R] > 0)


# ---- cube faces and the window's edges ------------------------------------------------------------------------------------------
FACE_POSE = np.array([0, 0, 0, 0.5, 0.25, -0.5], np.float32)


def face_values(axis):
    f = np.float32
    lo, hi = (-275.0, 275.0) if axis == 1 else (-525.0, 525.0)
    out = []
    for b in (-75.0, -25.0, 25.0, 75.0, lo, hi):
        out += [np.nextafter(f(b), f(-np.inf)), f(b), np.nextafter(f(b), f(np.inf))]
    return np.array(out, np.float32)


def face_points(axis, base):
    """every face value on `axis`, the other two coordinates apart by a metre per point (one point per voxel)"""
    rows = []
    for k, v in enumerate(face_values(axis)):
        p = [7.25 + k, 3.25 + k, -4.75 - k]
        p[axis] = float(v)
        rows.append(p + [base + k])
    return np.array(rows, np.float32)


def _faces_case(axis):
    name = "faces_" + "xyz"[axis]

    def build():
        m = face_points(axis, 0)
        f = face_points(axis, 1000)
        target = f[:, :3].copy()
        f[:, :3] = target - FACE_POSE[3:]
        assert np.array_equal(f[:, :3] + FACE_POSE[3:], target), "the features reach the face values exactly"

        def check(F):
            c = F[0]["corner"]
            # 18 values; outside the window: below lo, above hi, hi itself and (the negative fix-up) lo itself
            return c["n_old"] == 14 and c["n_ds"] == 18 and c["insert"][D] == 4 and F[0]["surf"]["insert"][D] == 4 and c["insert"][R] > 0 and c["insert"][V] > 0
        return Case(name, "coordinates at -75, -25, 25, 75 and the window's first and last face on one axis (y: 11 cubes), exactly and one float32 step to either side - "
                    "stored and inserted", (m, m.copy()), [(FACE_POSE, f, f.copy())], check)
    build.__name__ = name
    return case(build)


for _a in range(3):
    _faces_case(_a)


# ---- the window ---------------------------------------------------------------------------------------------------------------------
def _window_seed(rng):
    """points in the outermost layer of every window face, at the origin and 400 m out on x"""
    cubes = [(-10, 0, 0), (10, 0, 0), (0, -5, 0), (0, 5, 0), (0, 0, -10), (0, 0, 10), (0, 0, 0), (8, 0, 0), (-8, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 8), (0, 0, -8)]
    return _in_cubes(rng, cubes, 12), _in_cubes(rng, cubes, 12, 500)


def _window_case(name, claim, poses, check, empty=False):
    def build():
        rng = np.random.default_rng(500 + len(name))
        steps = []
        for k, p in enumerate(poses):
            p = np.asarray([0, 0, 0] + list(p), np.float32)
            n = 40
            c, s = features(np.full(n, V), 0), features(np.full(3 * n, V), 1)
            c[:, 2] += 64.0 + 2.0 * k   # (every step's features at a place of their own)
            s[:, 2] += 64.0 + 2.0 * k
            steps.append((p, c, s))
        seed = (NONE, NONE) if empty else _window_seed(rng)
        return Case(name, claim, seed, steps, check, lattice=empty)
    build.__name__ = name
    return case(build)


for _nm, _p, _s in (("xp", (400.5, 1.25, -2.75), (-1, 0, 0)), ("xm", (-400.5, 1.25, -2.75), (1, 0, 0)), ("yp", (0.5, 150.25, -2.75), (0, -1, 0)),
                    ("ym", (0.5, -150.25, -2.75), (0, 1, 0)), ("zp", (0.5, 1.25, 400.75), (0, 0, -1)), ("zm", (0.5, 1.25, -400.75), (0, 0, 1))):
    _window_case(f"shift_{_nm}", f"the window moves by one cube ({_s}) and pushes a populated layer out", [_p],
                 lambda F, s=_s: F[0]["shifts"] == s and F[0]["cubes_pushed_out"] == 2 and F[0]["corner"]["split"][D] == 12 and F[0]["surf"]["split"][D] == 12)
_window_case("shift_several", "three cubes on x and two on z at once", [(520.5, 1.25, -470.25)],
             lambda F: F[0]["shifts"] == (-3, 0, 2) and F[0]["cubes_pushed_out"] >= 4 and F[0]["corner"]["split"][D] >= 24)
_window_case("shift_threshold_on", "a pose exactly on the shift threshold (x = 375: window cube 18) shifts", [(375.0, 1.5, 2.5)], lambda F: F[0]["shifts"] == (-1, 0, 0))
_window_case("shift_threshold_below", "one float32 step below the threshold does not", [(float(np.nextafter(np.float32(375), np.float32(0))), 1.5, 2.5)],
             lambda F: F[0]["shifts"] == (0, 0, 0) and F[0]["cc"][0] == 17)
_window_case("shift_out_and_back", "a populated layer is pushed out and the window comes back: nothing returns", [(400.5, 1.25, -2.75), (-420.5, 1.25, -2.75), (0.5, 1.25, -2.75)],
             lambda F: F[0]["cubes_pushed_out"] == 2 and F[1]["shifts"] == (2, 0, 0) and F[1]["cubes_pushed_out"] > 0 and F[1]["corner"]["split"][D] > 0 and
             F[2]["shifts"] == (0, 0, 0) and F[2]["corner"]["n_old"] == F[1]["corner"]["n_new"] and F[2]["corner"]["split"][D] == 0)
_window_case("shift_from_empty", "four updates of an empty handle, one of them with a shift, on the exact lattice", [(0.5, 1.25, -2.75), (0.75, 1.25, -2.75), (400.5, 1.25, -2.75), (400.75, 1.5, -2.75)],
             lambda F: F[2]["shifts"] == (-1, 0, 0) and F[3]["corner"]["n_sub"] > 0 and F[0]["corner"]["n_old"] == 0, empty=True)


# ---- sequences ------------------------------------------------------------------------------------------------------------------
def _plane(nx, nz, step, y, base):
    """an nx x nz lattice of features in the MAP frame on the plane `y`, a quarter off the lattice: one per voxel, never at zero"""
    i, k = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    p = np.zeros((nx * nz, 4), np.float32)
    p[:, 0] = (i.reshape(-1) - nx // 2) * step + 0.25
    p[:, 1] = y
    p[:, 2] = (k.reshape(-1) - nz // 2) * step + 0.25
    p[:, 3] = base + np.arange(len(p)) % 1024
    return p


@case
def sequence_growing():
    rng = np.random.default_rng(61)
    seed_c, seed_s = np.zeros((5000, 4), np.float32), np.zeros((60000, 4), np.float32)
    for p in (seed_c, seed_s):
        p[:, :3] = rng.uniform(-20, 20, (len(p), 3))
        p[:, 1] -= 60.0
        p[:, 3] = np.arange(len(p)) % 4096
    steps = []
    for k in range(8):
        pose = np.array([0, 0, 0, 0.5 + 0.25 * k, 1.25, -2.75], np.float32)
        c, s = _plane(30, 30, 0.5, 10.25 + 0.5 * k, 100 * k), _plane(105, 105, 1.0, -19.75 + 1.0 * k, 100 * k)
        c[:, :3] -= pose[3:]
        s[:, :3] -= pose[3:]
        steps.append((pose, c, s))
    return Case("sequence_growing", "eight updates on one handle: the map grows by some 11,000 surfs a step past 131,072 points (the buffers swap every step, the room doubles once)",
                (seed_c, seed_s), steps,
                lambda F: all(F[k]["surf"]["n_new"] - F[k]["surf"]["n_old"] >= 9000 and F[k]["surf"]["n_ds"] == 11025 and F[k]["corner"]["n_ds"] == 900 for k in range(8)) and
                F[0]["surf"]["n_new"] + 11025 + 65 < (1 << 17) < F[7]["surf"]["n_new"])


@case
def sequence_lattice():
    steps = []
    for k in range(7):
        pose = np.array([0, 0, 0, 0.5 + 0.25 * k, 1.25 - 0.25 * k, -2.75], np.float32)
        # corners and surfs of a step share voxels of the surround grid (0.2 m): at most two points a voxel, all on a 1/8 lattice
        c = np.concatenate([_plane(20, 20, 0.5, 2.25 + 0.5 * k, 0), _plane(6, 6, 0.5, 102.25 + 0.5 * k, 7)])      # (y > 75: cube (0, 2, 0), not in the field of view)
        s = np.concatenate([_plane(60, 60, 1.0, 2.25 + 0.5 * k + 0.125, 0), _plane(6, 6, 1.0, 102.25 + 0.5 * k + 0.125, 7), _plane(4, 4, 1.0, -30.75 - k, 9)])
        c[:, :3] -= pose[3:]
        s[:, :3] -= pose[3:]
        steps.append((pose, c, s))
    return Case("sequence_lattice", "seven updates from an empty handle on a 1/8 m lattice: every sum is exact, so the surround cloud (corners then surfs in the product, cube "
                "by cube in the reference) compares to the word; cubes outside the field of view feed it too", (NONE, NONE), steps,
                lambda F: all(F[k]["corner"]["insert"][R] == 36 and F[k]["corner"]["n_new"] == 436 * (k + 1) for k in range(7)) and F[6]["surf"]["n_sub"] > 100, lattice=True)


NAMES = list(BUILDERS)
_CASES, _MODEL = {}, {}


def get(name):
    if name not in _CASES:
        _CASES[name] = BUILDERS[name]()
    return _CASES[name]


def model(orc, name):
    """the model's map after every step (corner, surf in storage order; grouped by window cube; the four sizes; the facts; the surround
    cloud) — computed once per case, shared, never written to"""
    if name not in _MODEL:
        c = get(name)
        m = rm.RollingMap(orc)
        m.load_cubes(*c.seed)
        loaded = (m.pts[0].copy(), m.pts[1].copy())
        out = []
        for pose, cl, sl in c.steps:
            facts = m.update(pose, cl, sl)
            out.append(dict(corner=m.pts[0].copy(), surf=m.pts[1].copy(), grouped=(m.grouped(0), m.grouped(1)), stats=dict(m.stats), facts=facts,
                            surround=m.surround() if c.lattice else None,
                            cen=tuple(m.cen)))
        _MODEL[name] = (loaded, out)
    return _MODEL[name]


# ---- the process path: one trajectory with speculation hits, a miss and a window shift ------------------------------------------
def trajectory():
    """(seed, steps); a step is (kind, pose, corner, surf).  Every step's features lie on a plane of their own, 2 m from the planes of
    all other steps and 2 m or more from the seed: no feature has five sub-map points within a metre, so no row is selected and the
    pose stays the guess, which is the odometry pose itself (dyadic values: bef / aft cancel exactly)."""
    seed_c, seed_s = _plane(12, 12, 0.5, -9.75, 0), _plane(24, 24, 1.0, -9.75, 0)
    xs = [("process", 0.5), ("process", 0.75), ("process", 1.0), ("insert", 1.0), ("process", 1.25), ("process", 340.5), ("process", 400.5),
          ("insert", 400.5), ("process", 400.75), ("process", 401.0), ("process", 401.25), ("process", 401.5), ("process", 401.75)]
    steps = []
    for k, (kind, x) in enumerate(xs):
        pose = np.array([0, 0, 0, x, 1.25, -2.75], np.float32)
        c, s = _plane(8, 8, 0.5, -5.75 + 2.0 * k, 10 * k), _plane(14, 14, 1.0, -5.75 + 2.0 * k, 10 * k)
        c[:, 0] += np.floor(x)
        s[:, 0] += np.floor(x)
        c[:, :3] -= pose[3:]
        s[:, :3] -= pose[3:]
        steps.append((kind, pose, c, s))
    return (seed_c, seed_s), steps
