"""numpy / Python model of the dense map's ray casts (include/loamx.h, loamx_densemap_raycast and what precedes it), exact to the bit:
the end-cell check in front of the walk of tests/densemap_carve_model.py (trace), the lookup loop over a dict of the model's keys, the
position of a hit through densemap_model.export and its range in np.float32 scalars with the library's roundings (no fused
multiply-add, correctly rounded division and square root).  Built on tests/densemap_model.py and tests/densemap_carve_model.py, which
stay the models of the map and of carving.  The checker of tests/test_densemap_raycast_cpu.py and tests/test_gpu_densemap_raycast.py."""
import numpy as np

import densemap_carve_model as cm
import densemap_model as dm

F = np.float32
NOT_TRACED, MISS, HIT, HIT_END = range(4)
COUNT_KEYS = ("not_traced", "miss", "hit", "hit_end", "cells")
DEFAULTS = dict(max_steps=4096, skip_steps=0, min_points=1)
# loamx_ray_hit, 40 bytes
RAY_DTYPE = np.dtype([("key", np.uint64), ("x", np.float32), ("y", np.float32), ("z", np.float32), ("range", np.float32),
                      ("n", np.uint32), ("miss", np.uint32), ("steps", np.uint32), ("status", np.uint32)])


def end_ok(point, leaf):
    """every component of the end is finite and its cell passes the key rule"""
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            p = F(point[a])
            if not np.isfinite(p) or not abs(np.floor(p * inv)) < F(cm.IMAX):
                return False
    return True


def walk(origin, point, leaf):
    """(cells, n_steps) of the ray's walk, cells[k] the cell after k steps, k = 0 .. n_steps; cells is None when the ray is NOT_TRACED
    whatever max_steps is: the end or the origin fails its check, or n_steps is above 65536, the largest max_steps (such a walk is
    not spelled out)"""
    if not end_ok(point, leaf):
        return None, None
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        fo = [np.floor(F(origin[a]) * inv) for a in range(3)]
        if all(abs(f) < F(cm.IMAX) for f in fo):
            n_steps = sum(abs(int(np.floor(F(point[a]) * inv)) - int(fo[a])) for a in range(3))
            if n_steps > 65536:
                return None, n_steps
        return cm.trace(origin, point, leaf)


def walks_of(ends, origin, leaf):
    """walk() per ray: the part of cast() that depends on neither the map nor the settings (pass it to cast() to share it)"""
    ends = np.asarray(ends, np.float32)
    return [walk(origin, ends[i, :3], leaf) for i in range(len(ends))]


def ray_range(origin, point, pos):
    """metres along the ray origin -> point to the foot of pos, in f32 as the header orders it"""
    o, p, x = [F(v) for v in origin], [F(v) for v in point[:3]], [F(v) for v in pos[:3]]
    d = [p[a] - o[a] for a in range(3)]
    e = [x[a] - o[a] for a in range(3)]
    l2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    if l2 == 0:
        return F(0)
    return F(((d[0] * e[0] + d[1] * e[1]) + d[2] * e[2]) / np.sqrt(l2))


def cast(model, ends, origin, max_steps=4096, skip_steps=0, min_points=1, rule=None, walks=None):
    """loamx_densemap_raycast on a densemap_model.Model (a rule needs a densemap_carve_model.CarveModel): (records as a structured array
    of RAY_DTYPE, counts as a dict in the order of COUNT_KEYS).  walks: walks_of(ends, origin, model.leaf), when the caller has them"""
    assert 1 <= max_steps <= 65536 and min_points >= 1 and (rule is None or rule[2] != 0)
    ends = np.asarray(ends, np.float32)
    ends = ends if ends.size else ends.reshape(0, 4)
    walks = walks_of(ends, origin, model.leaf) if walks is None else walks
    assert len(walks) == len(ends)
    index = {int(k): j for j, k in enumerate(model.keys.tolist())}
    miss_of = getattr(model, "miss", {})
    out = np.zeros(len(ends), RAY_DTYPE)
    counts = dict.fromkeys(COUNT_KEYS, 0)
    for i in range(len(ends)):
        p = ends[i, :3]
        cells, n_steps = walks[i]
        if cells is None or n_steps > max_steps:
            counts["not_traced"] += 1
            continue   # (the record stays zero: status NOT_TRACED)
        r = out[i]
        r["status"] = MISS
        looked = 0
        for k in range(skip_steps, n_steps + 1):
            looked += 1
            key = cm.key_of(cells[k])
            j = index.get(key)
            if j is None:
                continue
            n = int(model.vals[j, 0])
            miss = int(miss_of.get(key, 0))
            if n < min_points or (rule is not None and cm.is_dynamic(rule, n, miss)):
                continue
            pos = dm.export(model.keys[j:j + 1], model.vals[j:j + 1], model.leaf)[0]
            r["key"], r["x"], r["y"], r["z"] = key, pos[0], pos[1], pos[2]
            r["range"] = ray_range(origin, p, pos)
            r["n"], r["miss"], r["steps"] = min(n, (1 << 32) - 1), miss, k
            r["status"] = HIT if k < n_steps else HIT_END
            break
        if r["status"] == MISS:
            r["steps"] = looked
        counts["cells"] += looked
        counts[COUNT_KEYS[int(r["status"])]] += 1
    assert sum(counts[k] for k in COUNT_KEYS[:4]) == len(ends)
    return out, counts


def same_records(a, b):
    """field for field, the floats by their bits"""
    return a.dtype == b.dtype == RAY_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the scene and the rays of tests/test_gpu_densemap_raycast.py (here, so that the CPU test can check their coverage too) ----------
def hand_ends(origin, leaf):
    """the ends of the hand cases that make sense from any origin, (13, 4) float32: the zero-length ray; the six axis-aligned rays of
    2 m (from an origin near 0 they cross index 0 into the negative cells); the two diagonals of 1 m per axis; a NaN end; the ends in
    the cells i = 2^20 and i = -2^20 (outside the key range on either side); the end in the last cell inside it, i = 2^20 - 1 (its
    n_steps is far above any max_steps)"""
    o = np.asarray(origin, np.float32)
    e = [o.copy()]
    for a in range(3):
        for s in (2.0, -2.0):
            p = o.copy()
            p[a] += F(s)
            e.append(p)
    e += [o + F(1.0), o - F(1.0)]
    e.append(np.array([o[0], np.nan, o[2]], np.float32))
    edge = float(cm.IMAX) * float(F(leaf))
    e.append(np.array([edge, o[1], o[2]], np.float32))
    e.append(np.array([o[0], o[1], -edge - 0.25 * float(F(leaf))], np.float32))
    e.append(np.array([o[0], edge - 0.5 * float(F(leaf)), o[2]], np.float32))
    out = np.zeros((len(e), 4), np.float32)
    out[:, :3] = np.stack(e)
    return out


def box_cast_scene():
    """dict: sweeps = the three sweeps of densemap_align_model.box_scene(), each with 12 mid-air points behind it (they give the later
    sweeps something to carve and the rays something to hit in front of the walls); origin = the first sweep's; leaf"""
    import densemap_align_model as am
    S = am.box_scene()
    rng = np.random.default_rng(3)
    sweeps = []
    for p, o in S["sweeps"]:
        air = np.zeros((12, 4), np.float32)
        air[:, :3] = rng.uniform([-2, -1.5, -1], [2, 1.5, 1], (12, 3))
        sweeps.append((np.concatenate([p, air]), o))
    return dict(sweeps=sweeps, origin=sweeps[0][1], leaf=S["leaf"])


def box_rays(n, origin, leaf, seed=11):
    """n ends, (n, 4) float32: uniform in [-4.5, 4.5]^3 (the box and a margin around it: rays that end inside, in a wall and behind
    one), the first quarter shortened to 0.3 of its length, the second quarter on the walls themselves, the hand cases in front as
    far as n has room for them"""
    import densemap_align_model as am
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, np.float64)
    p = rng.uniform(-4.5, 4.5, (n, 3))
    q = n // 4
    p[:q] = o + 0.3 * (p[:q] - o)
    p[q:2 * q] = am.box_points(rng, q)[:, :3]
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = p
    hand = hand_ends(origin, leaf)[:n]
    out[:len(hand)] = hand
    return out
