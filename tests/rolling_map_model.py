"""Executable specification of the rolling map's update (loam_velodyne_amd/csrc/mapping.hip) in NumPy: what k_map_split, k_map_insert,
k_map_append_filtered, k_map_hist, the surround kernels and the host bookkeeping around them (Mapper::make_plan, shift_counts,
load_cubes) are DESIGNED to leave, word for word and in STORAGE ORDER, from what loamx_map_load_cubes / loamx_map_insert /
loamx_map_process take.

Zero pose angles only (asserted): sinf(0) / cosf(0) are exact, so every float32 operation of the update can be repeated here with one
rounding per operation.  The sweep's stack round trip and down-sizing is tests/voxbucket_model.py's run(); pcl::VoxelGrid per cube is
the oracle's restatement (orc.voxel_grid), on the input order this model states: the cube's old points in storage order, then its new
features in feature order.

Storage order after an update, per feature type:   rest ++ inserted-rest ++ filtered
  rest           old points of in-window cubes that are not valid, order kept
  inserted-rest  down-sized features that land in such cubes, in feature order
  filtered       per valid cube (slot order = the 5x5x5 neighbourhood in i, j, k order, field-of-view cubes only) the voxel grid's output
"""
import numpy as np

import voxbucket_model as vm

MW, MH, MD = 21, 11, 21
DIMS = (MW, MH, MD)
MCUBES = MW * MH * MD
MS_TILE, INS_BLOCK = 2048, 256
DROPPED, REST, VALID = 0, 1, 2
F32 = np.float32


def cube_abs(v):
    """cube index of a map coordinate relative to the map origin: double arithmetic, truncation, negative fix-up"""
    d = np.asarray(v, np.float32).astype(np.float64) + 25.0
    c = np.trunc(d / 50.0).astype(np.int64)
    return c - (d < 0)


def to_map_zero_angles(pts, pos):
    """to_map (dev_math.hpp) with sine 0 / cosine 1: rot_z, rot_x, rot_y, then the translation — every product and sum in float32"""
    one, zero = np.float32(1), np.float32(0)
    x, y, z = (np.ascontiguousarray(pts[:, k], np.float32) for k in range(3))
    x, y = vm._rot(x, y, one, zero)
    y, z = vm._rot(y, z, one, zero)
    x, z = vm._rot_y(x, z, one, zero)
    out = np.empty((len(pts), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = x + pos[0], y + pos[1], z + pos[2], pts[:, 3]
    return out


def window_index(cube, cen):
    """(window cube index, inside the window) of absolute cube triples"""
    w = np.asarray(cube, np.int64).reshape(-1, 3) + np.asarray(cen, np.int64)
    inside = np.all((w >= 0) & (w < np.array(DIMS)), axis=1)
    return np.where(inside, w[:, 0] + MW * w[:, 1] + MW * MH * w[:, 2], -1), inside


def neighbourhood(pos, cen, cc):
    """Mapper::make_plan behind the window shift: the 5x5x5 neighbourhood of window cube cc in i, j, k order, clipped to the window;
    the field-of-view test on the eight cube corners in float32.  Returns (window indices, in_fov flags, smallest |check1|, |check2|)"""
    pos = np.asarray(pos, np.float32)
    py = to_map_zero_angles(np.array([[0, 10, 0, 0]], np.float32), pos)[0, :3]
    idx, fov, m1, m2 = [], [], np.inf, np.inf
    sgn = np.array([[ii, jj, kk] for ii in (-1, 1) for jj in (-1, 1) for kk in (-1, 1)], np.float32)
    k103 = F32(10.0) * np.sqrt(F32(3.0))
    for i in range(cc[0] - 2, cc[0] + 3):
        for j in range(cc[1] - 2, cc[1] + 3):
            for k in range(cc[2] - 2, cc[2] + 3):
                if not (0 <= i < MW and 0 <= j < MH and 0 <= k < MD):
                    continue
                centre = F32(50.0) * np.array([i - cen[0], j - cen[1], k - cen[2]], np.float32)
                c = centre[None, :] + F32(25.0) * sgn
                a, b = pos[None, :] - c, py[None, :] - c
                s1 = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2]
                s2 = b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1] + b[:, 2] * b[:, 2]
                r = k103 * np.sqrt(s1)
                check1, check2 = F32(100.0) + s1 - s2 - r, F32(100.0) + s1 - s2 + r
                m1, m2 = min(m1, float(np.abs(check1).min())), min(m2, float(np.abs(check2).min()))
                idx.append(i + MW * j + MW * MH * k)
                fov.append(bool(((check1 < 0) & (check2 > 0)).any()))
    return np.array(idx, np.int64), np.array(fov, bool), m1, m2


def _tile_totals(cls, tile):
    """per tile of `tile` consecutive positions: how many dropped, rest, valid"""
    n = len(cls)
    nt = -(-n // tile)
    out = np.zeros((nt, 3), np.int64)
    if n:
        np.add.at(out, (np.arange(n) // tile, cls), 1)
    return out


class RollingMap:
    def __init__(self, orc, corner_leaf=0.2, surf_leaf=0.4):
        self.orc = orc
        self.leaf = (corner_leaf, surf_leaf)
        self.cen = [10, 5, 10]
        self.pts = [np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)]      # storage order
        self.cube = [np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)]         # absolute (ia, ja, ka) of every point
        self.cnt = [np.zeros(MCUBES, np.int64), np.zeros(MCUBES, np.int64)]          # the host directory, window coordinates
        self.sur = np.zeros(MCUBES, bool)                                            # the clipped 5x5x5 neighbourhood of the last update
        self.stats = dict(corner_from_map=0, surf_from_map=0, corner_ds=0, surf_ds=0)

    # ---- loamx_map_load_cubes: by coordinate, against the current window; input order kept
    def load_cubes(self, corner, surf):
        for t, p in enumerate((corner, surf)):
            p = np.ascontiguousarray(p, np.float32).reshape(-1, 4)
            cube = np.stack([cube_abs(p[:, a]) for a in range(3)], axis=1).reshape(-1, 3)
            idx, inside = window_index(cube, self.cen)
            self.pts[t] = np.concatenate([self.pts[t], p[inside]])
            self.cube[t] = np.concatenate([self.cube[t], cube[inside]])
            self.cnt[t] += np.bincount(idx[inside], minlength=MCUBES)

    def _shift(self, axis, direction):
        """shift_counts: contents move by one cube along `axis`, the vacated layer is cleared; returns the populated cubes pushed out"""
        lost = 0
        for t in range(2):
            c = self.cnt[t].reshape(MD, MH, MW)
            ax = 2 - axis
            leaving = np.take(c, DIMS[axis] - 1 if direction > 0 else 0, axis=ax)
            lost += int((leaving > 0).sum())
            c = np.roll(c, direction, axis=ax)
            sl = [slice(None)] * 3
            sl[ax] = 0 if direction > 0 else DIMS[axis] - 1
            c[tuple(sl)] = 0
            self.cnt[t] = c.reshape(-1).copy()
        return lost

    # ---- one sweep with a GIVEN pose (loamx_map_insert; loamx_map_process when no row is selected)
    def update(self, pose6, corner_last, surf_last):
        pose = np.asarray(pose6, np.float32)
        assert pose.shape == (6,) and not pose[:3].any(), "the model covers zero pose angles only"
        pos = pose[3:]
        facts = {}
        # 1. the window shift of Mapper::make_plan
        cc = [int(cube_abs(pos[a])) + self.cen[a] for a in range(3)]
        shifts, lost = [0, 0, 0], 0
        for a in range(3):
            while cc[a] < 3:
                lost += self._shift(a, +1); cc[a] += 1; self.cen[a] += 1; shifts[a] += 1
            while cc[a] >= DIMS[a] - 3:
                lost += self._shift(a, -1); cc[a] -= 1; self.cen[a] -= 1; shifts[a] -= 1
        facts["shifts"], facts["cubes_pushed_out"], facts["cen"], facts["cc"] = tuple(shifts), lost, tuple(self.cen), tuple(cc)
        # 2. the valid list and its slots
        nb, fov, m1, m2 = neighbourhood(pos, self.cen, cc)
        facts["min_check1"], facts["min_check2"] = m1, m2
        valid = nb[fov]
        lut = np.full(MCUBES, -1, np.int64)
        lut[valid] = np.arange(len(valid))
        self.sur = np.zeros(MCUBES, bool)
        self.sur[nb] = True
        facts["nvalid"], facts["valid"] = len(valid), valid
        # 4. the stack round trip and the down-sizing: what the registrar leaves in ds_pts
        feats = [np.ascontiguousarray(corner_last, np.float32).reshape(-1, 4), np.ascontiguousarray(surf_last, np.float32).reshape(-1, 4)]
        nin = [len(f) for f in feats]
        if sum(nin):
            R = vm.run(np.concatenate(feats), [0, nin[0], nin[0] + nin[1]], vm.pose_words(0, 0, 0, *pos)[None], self.leaf[0], self.leaf[1])
            assert not R.gave_up, "a case must stay inside what the bucketed voxel grid takes"
            ds = [R.out[int(R.out_off[t]):int(R.out_off[t + 1])] for t in range(2)]
        else:
            ds = [np.zeros((0, 4), np.float32)] * 2
        per_type = []
        for t in range(2):
            f = {}
            # 3. the split of the old map, in storage order
            idx, inside = window_index(self.cube[t], self.cen)
            slot = np.where(inside, lut[np.maximum(idx, 0)], -1)
            cls = np.where(slot >= 0, VALID, np.where(inside, REST, DROPPED))
            n_sub = int(self.cnt[t][valid].sum())
            assert n_sub == int((cls == VALID).sum()), "the host directory and the split disagree about the sub-map's size"
            f["n_old"], f["n_sub"] = len(cls), n_sub
            f["split"] = tuple(int((cls == c).sum()) for c in (DROPPED, REST, VALID))
            f["split_tiles"] = _tile_totals(cls, MS_TILE)
            rest_p, rest_c = self.pts[t][cls == REST], self.cube[t][cls == REST]
            sub_p, sub_slot = self.pts[t][cls == VALID], slot[cls == VALID]
            # 5. every down-sized feature into the map frame, one rounding per operation, and into its cube
            new = to_map_zero_angles(ds[t], pos)
            ncube = np.stack([cube_abs(new[:, a]) for a in range(3)], axis=1).reshape(-1, 3)
            nidx, ninside = window_index(ncube, self.cen)
            nslot = np.where(ninside, lut[np.maximum(nidx, 0)], -1)
            ncls = np.where(nslot >= 0, VALID, np.where(ninside, REST, DROPPED))
            f["n_in"], f["n_ds"] = nin[t], len(new)
            f["insert"] = tuple(int((ncls == c).sum()) for c in (DROPPED, REST, VALID))
            f["insert_blocks"] = _tile_totals(ncls, INS_BLOCK)
            # 6. pcl::VoxelGrid per valid slot: the cube's old points in storage order, then its new features in feature order
            filt, filt_cube, filt_n = [], [], np.zeros(len(valid), np.int64)
            for s in range(len(valid)):
                inp = np.concatenate([sub_p[sub_slot == s], new[nslot == s]])
                if not len(inp):
                    continue
                out = self.orc.voxel_grid(inp, self.leaf[t])
                filt_n[s] = len(out)
                w = int(valid[s])
                filt.append(out)
                filt_cube.append(np.tile(np.array([w % MW - self.cen[0], (w // MW) % MH - self.cen[1], w // (MW * MH) - self.cen[2]], np.int64), (len(out), 1)))
            f["filtered_per_slot"], f["empty_slots"] = filt_n, np.flatnonzero(filt_n == 0)
            # 7. the new storage order and the new directory
            self.pts[t] = np.concatenate([rest_p, new[ncls == REST]] + filt)
            self.cube[t] = np.concatenate([rest_c, ncube[ncls == REST]] + filt_cube)
            widx, winside = window_index(self.cube[t], self.cen)
            assert winside.all()
            self.cnt[t] = np.bincount(widx, minlength=MCUBES)
            f["n_new"], f["populated_cubes"] = len(self.pts[t]), int((self.cnt[t] > 0).sum())
            per_type.append(f)
        facts["corner"], facts["surf"] = per_type
        self.stats = dict(corner_from_map=per_type[0]["n_sub"], surf_from_map=per_type[1]["n_sub"], corner_ds=per_type[0]["n_ds"], surf_ds=per_type[1]["n_ds"])
        return facts

    # ---- createDownsizedMap as the product cuts it: flagged corners in storage order, then flagged surfs, ONE grid at the corner leaf
    def surround(self):
        parts = []
        for t in range(2):
            idx, inside = window_index(self.cube[t], self.cen)
            parts.append(self.pts[t][inside & self.sur[np.maximum(idx, 0)]])
        cat = np.concatenate(parts)
        return self.orc.voxel_grid(cat, self.leaf[0]) if len(cat) else cat

    def grouped(self, t):
        """the map of one type stably grouped by window cube: the order in which the oracle dumps its cube arrays"""
        idx, inside = window_index(self.cube[t], self.cen)
        keep = np.flatnonzero(inside)
        return self.pts[t][keep[np.argsort(idx[keep], kind="stable")]]
