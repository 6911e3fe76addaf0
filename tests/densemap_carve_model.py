"""numpy / Python model of the dense map's free-space carving (include/loamx.h, loamx_densemap_enable_carving and what follows it), exact
to the bit: the voxel walk in f32 scalars with the library's roundings (no fused multiply-add, correctly rounded division), one plain
Python loop per ray, integer miss counts and stamps per voxel.  Built on tests/densemap_model.py, which stays the model of the map
itself.  The checker of tests/test_densemap_carve_cpu.py and tests/test_gpu_densemap_carve.py."""
import numpy as np

import densemap_model as dm

F = np.float32
IMAX = 1 << dm.QBITS


def key_of(cell):
    """the voxel key of an integer cell (ix, iy, iz)"""
    return (cell[0] + IMAX) | ((cell[1] + IMAX) << dm.KBITS) | ((cell[2] + IMAX) << (2 * dm.KBITS))


def added_mask(points, origin, leaf, min_range=0.0, max_range=0.0):
    """(which points the map adds, d2 per point): the range and key filters of densemap_model.keys_of, per input point"""
    p = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    o = np.asarray(origin, np.float32)
    d = p - o
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = d2 >= F(min_range) * F(min_range)
    if max_range > 0:
        keep &= d2 <= F(max_range) * F(max_range)
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        keep &= np.all(np.abs(np.floor(p * inv)) < F(IMAX), axis=1)
    return keep, d2


def trace(origin, point, leaf):
    """the walk from the origin's cell to the point's cell: (cells, n_steps) with cells[k] the cell after k steps, k = 0 .. n_steps
    (so cells[-1] is the point's cell), or (None, None) when the origin's cell fails the key rule.  The point is one the map adds."""
    inv = F(1.0) / F(leaf)
    c, s, rem, tmax, tdelta = [0] * 3, [0] * 3, [0] * 3, [F(0)] * 3, [F(0)] * 3
    for a in range(3):
        so, sp = F(origin[a]) * inv, F(point[a]) * inv
        fo = np.floor(so)
        if not abs(fo) < F(IMAX):   # (NaN too)
            return None, None
        c0, c1 = int(fo), int(np.floor(sp))
        c[a], rem[a] = c0, abs(c1 - c0)
        s[a] = (c1 > c0) - (c1 < c0)
        if rem[a] > 0:
            d = sp - so
            b = F(c0 + (1 if s[a] > 0 else 0))
            tmax[a] = (b - so) / d
            tdelta[a] = F(1.0) / abs(d)
    n_steps = rem[0] + rem[1] + rem[2]
    cells = [tuple(c)]
    for _ in range(n_steps):
        ax = -1
        for a in range(3):   # the smallest tmax among the axes with cells left; ties to the lower axis
            if rem[a] > 0 and (ax < 0 or tmax[a] < tmax[ax]):
                ax = a
        c[ax] += s[ax]
        rem[ax] -= 1
        tmax[ax] = tmax[ax] + tdelta[ax]
        cells.append(tuple(c))
    return cells, n_steps


def visited(cells, n_steps, end_margin):
    """the cells a traced ray looks up: k = 0 .. n_steps - 1 - end_margin"""
    return cells[:max(n_steps - end_margin, 0)]


def is_dynamic(rule, n, miss):
    """rule = (min_misses, num, den), in 64-bit unsigned arithmetic as the library's"""
    mn, num, den = rule
    return miss >= mn and (miss * den) % (1 << 64) > (n * num) % (1 << 64)


DEFAULT_RULE = (3, 1, 1)
CARVE_KEYS = ("traced", "skipped_stride", "skipped_range", "skipped_steps", "cells_visited", "misses")


class CarveModel(dm.Model):
    """densemap_model.Model with carving enabled from the start"""

    def __init__(self, leaf=0.1, min_range=0.0, max_range=0.0, max_voxels=0, carve_max_range=0.0, ray_stride=1, end_margin=1,
                 max_steps=4096):
        super().__init__(leaf, min_range, max_range, max_voxels)
        self.carve_max_range, self.ray_stride, self.end_margin, self.max_steps = carve_max_range, ray_stride, end_margin, max_steps
        self.seq = 0
        self.miss, self.stamp = {}, {}   # per key
        self.cstats = dict.fromkeys(CARVE_KEYS, 0)

    def add(self, points, origin):
        points = np.asarray(points, np.float32)
        if self.would_refuse(len(points)):
            return False
        self.seq += 1
        keep, d2 = added_mask(points, origin, self.leaf, self.min_range, self.max_range)
        keys, _, _, _ = dm.keys_of(points, origin, self.leaf, self.min_range, self.max_range)
        assert len(keys) == int(keep.sum())
        super().add(points, origin)
        for k in keys.tolist():
            self.stamp[k] = self.seq
        present = set(self.keys.tolist())
        max2 = F(self.carve_max_range) * F(self.carve_max_range)
        st = self.cstats
        for i in np.flatnonzero(keep).tolist():
            if i % self.ray_stride != 0:
                st["skipped_stride"] += 1
                continue
            if self.carve_max_range > 0 and not d2[i] <= max2:
                st["skipped_range"] += 1
                continue
            cells, n_steps = trace(origin, points[i, :3], self.leaf)
            if cells is None or n_steps > self.max_steps:
                st["skipped_steps"] += 1
                continue
            st["traced"] += 1
            for cell in visited(cells, n_steps, self.end_margin):
                st["cells_visited"] += 1
                k = key_of(cell)
                if k in present and self.stamp[k] != self.seq:
                    self.miss[k] = self.miss.get(k, 0) + 1
                    st["misses"] += 1
        return True

    def carve_stats(self):
        return dict(self.cstats)

    def misses(self):
        """the miss count per voxel in the order of points()"""
        return np.array([self.miss.get(k, 0) for k in self.keys.tolist()], np.uint32)

    def dynamic_mask(self, rule=DEFAULT_RULE):
        return np.array([is_dynamic(rule, int(n), self.miss.get(k, 0)) for k, n in zip(self.keys.tolist(), self.vals[:, 0].tolist())], bool)

    def points(self, axes="loam", static=None):
        if static is None:
            return super().points(axes)
        keep = ~self.dynamic_mask(static)
        return dm.export(self.keys[keep], self.vals[keep], self.leaf, axes)

    def prune(self, rule=DEFAULT_RULE):
        """the dynamic voxels leave; returns how many"""
        dyn = self.dynamic_mask(rule)
        for k in self.keys[dyn].tolist():
            self.miss.pop(k, None)
            self.stamp.pop(k, None)
        self.keys, self.vals = self.keys[~dyn], self.vals[~dyn]
        return int(dyn.sum())
