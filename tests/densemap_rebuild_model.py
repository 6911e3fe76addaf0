"""numpy model of the dense map's correction and rebuild (include/loamx.h, loamx_densemap_correct / loamx_densemap_rebuild), exact to the
bit.  A rebuild is, by definition, what a fresh handle fed with the corrected sweeps holds: the models of tests/densemap_model.py,
densemap_carve_model.py, densemap_moments_model.py and densemap_file_model.py stay the models of the map itself, and this file only
moves the sweeps.  The checker of tests/test_densemap_history_cpu.py and tests/test_gpu_densemap_rebuild.py."""
import numpy as np

IDENTITY = np.float32([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])


def rounded(correction):
    """the correction (3x4 or 4x4, any float type) as the replay reads it: rounded to float32 once, entry by entry"""
    c = np.asarray(correction, np.float64)[:3, :4]
    assert c.shape == (3, 4) and np.all(np.isfinite(c)), "a correction is 12 finite numbers"
    return c.astype(np.float32)


def is_identity(correction):
    """the 12 rounded entries compare equal (==) to the identity's (-0.0 == 0.0)"""
    return bool(np.all(rounded(correction) == IDENTITY))


def correct(correction, xyz):
    """(N, 3) or (N, 4) float32 under x -> R x + t: p'_a = ((R_a0*x + R_a1*y) + R_a2*z) + t_a in float32, each product and each sum
    rounded on its own (no fused multiply-add); further columns (w) are untouched.  The identity returns the input's bytes"""
    p = np.array(xyz, np.float32, ndmin=2)
    if is_identity(correction):
        return p
    m = rounded(correction)
    x, y, z = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            p[:, a] = ((m[a, 0] * x + m[a, 1] * y) + m[a, 2] * z) + m[a, 3]
    return p


def corrected_sweeps(sweeps, corrections=None):
    """[(points, origin)] with sweep k moved by corrections[k] (None: as they are)"""
    if corrections is None:
        return [(np.asarray(p, np.float32), np.asarray(o, np.float32)) for p, o in sweeps]
    assert len(corrections) == len(sweeps)
    return [(correct(c, p), correct(c, np.asarray(o, np.float32))[0]) for (p, o), c in zip(sweeps, corrections)]


def rebuild(model_factory, sweeps, corrections=None):
    """a fresh model (model_factory()) fed with the corrected sweeps in order; empty sweeps are no calls"""
    m = model_factory()
    for p, o in corrected_sweeps(sweeps, corrections):
        if len(p):
            added = m.add(p, o)
            assert added is not False
    return m


def exp_so3(w):
    """the rotation matrix of the rotation vector w (float64)"""
    w = np.asarray(w, np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * (K @ K)


def rigid(w, t, centre=(0.0, 0.0, 0.0)):
    """the 3x4 correction that turns by the rotation vector w about `centre` and then shifts by t"""
    R = exp_so3(w)
    c = np.asarray(centre, np.float64)
    return np.concatenate([R, (c - R @ c + np.asarray(t, np.float64)).reshape(3, 1)], axis=1)


def attempts(initial_slots, voxels_before, voxels_after):
    """the table sizes a rebuild tries: from the smallest, by doubling from initial_slots, that holds the voxels before at a load of
    one half; an attempt fails iff the rebuilt map has more voxels than half its slots, and is repeated with twice the slots"""
    slots = initial_slots
    while voxels_before > slots // 2:
        slots *= 2
    tried = [slots]
    while voxels_after > slots // 2:
        slots *= 2
        tried.append(slots)
    return tried
