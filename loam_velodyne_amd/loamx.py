"""ctypes binding of libloamx.so (the C-ABI of include/loamx.h) for the Python harness (tests/, bench.py, smoke()).

This is plumbing over the C-ABI, not a second implementation: every method is one `loamx_*` call.  There is no CPU
fallback — if the shared library is missing or no GPU is visible, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOAMX_LIB") or os.path.join(_HERE, "libloamx.so")   # LOAMX_LIB: a diagnostic build (time stamps inside kernels)

OK, SKIPPED, E_INVALID, E_CAPACITY, E_HIP, E_NOGPU, E_UNSUPPORTED, E_INTERNAL = 0, 1, -1, -2, -3, -4, -5, -6


class Cloud(C.Structure):
    _fields_ = [("data", C.c_void_p), ("count", C.c_uint32), ("stride", C.c_uint32),
                ("intensity_offset", C.c_uint32), ("reserved", C.c_uint32)]


class ScanRegConfig(C.Structure):
    _fields_ = [("scan_period", C.c_float), ("n_feature_regions", C.c_int), ("curvature_region", C.c_int),
                ("max_corner_sharp", C.c_int), ("max_surface_flat", C.c_int), ("less_flat_filter_size", C.c_float),
                ("surface_curvature_threshold", C.c_float), ("device", C.c_int), ("max_corner_less_sharp", C.c_int),
                ("imu_history_size", C.c_int)]


class OdomConfig(C.Structure):
    _fields_ = [("scan_period", C.c_float), ("max_iterations", C.c_int), ("delta_t_abort", C.c_float),
                ("delta_r_abort", C.c_float), ("device", C.c_int)]


class MapConfig(C.Structure):
    _fields_ = [("scan_period", C.c_float), ("max_iterations", C.c_int), ("delta_t_abort", C.c_float),
                ("delta_r_abort", C.c_float), ("corner_filter_size", C.c_float), ("surf_filter_size", C.c_float),
                ("map_filter_size", C.c_float), ("device", C.c_int)]


class LoamxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"loamx error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    """Load libloamx.so (built in-tree by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                    "(no CPU fallback exists)")
        L = C.CDLL(LIB_PATH)
        L.loamx_last_error.restype = C.c_char_p
        if hasattr(L, "loamx_build_info"):
            L.loamx_build_info.restype = C.c_char_p
        if hasattr(L, "loamx_dist_pack_clouds"):   # (64-bit sizes and more than six arguments: spelled out rather than left to ctypes' defaults)
            L.loamx_dist_pack_clouds.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            L.loamx_dist_unpack_clouds_header.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
            L.loamx_dist_unpack_clouds_stream.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.loamx_dist_gatherv.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p]
        for n in ("loamx_scanreg_create", "loamx_odom_create", "loamx_map_create", "loamx_batch_create",
                  "loamx_batch_stream"):
            if hasattr(L, n):
                getattr(L, n).restype = C.c_void_p
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise LoamxError(rc, lib().loamx_last_error().decode())
    return rc


def device_count() -> int:
    return int(lib().loamx_device_count())


def pinned_empty(shape, dtype=np.float32):
    """numpy array in host memory pinned by the library's HIP runtime (loamx_host_alloc): the entry points copy straight from / to such
    arrays (DMA) instead of through their staging blocks.  Freed when the array and every view of it are gone."""
    import weakref
    L = lib()
    L.loamx_host_alloc.restype = C.c_void_p
    L.loamx_host_alloc.argtypes = [C.c_size_t]
    L.loamx_host_free.argtypes = [C.c_void_p]
    shape = tuple(int(x) for x in (shape if hasattr(shape, "__len__") else (shape,)))
    nbytes = max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 1)
    ptr = L.loamx_host_alloc(nbytes)
    if not ptr:
        raise LoamxError(E_HIP, "loamx_host_alloc failed")
    buf = (C.c_char * nbytes).from_address(ptr)
    weakref.finalize(buf, L.loamx_host_free, C.c_void_p(ptr))
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def pinned_copy(a, dtype=np.float32):
    out = pinned_empty(np.shape(a), dtype)
    out[...] = a
    return out


def build_info() -> dict:
    """loamx_build_info() as a dict: abi, diag (1: a diagnostic build that reads the result-changing LOAMX_* switches), rccl, roctx."""
    return dict(kv.split("=", 1) for kv in lib().loamx_build_info().decode().split(";") if kv)


def as_points(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.ndim == 1:
        a = a.reshape(-1, 4)
    assert a.ndim == 2 and a.shape[1] in (4, 8), "points must be (N,4) packed xyzi or (N,8) PCL PointXYZI records"
    return a


def cloud_of(a: np.ndarray) -> Cloud:
    """Describe a (N,4) packed or (N,8) PCL-layout float32 array."""
    stride = a.shape[1] * 4
    return Cloud(a.ctypes.data if a.size else None, a.shape[0], stride, 12 if stride == 16 else 16, 0)


def to_pcl_layout(a: np.ndarray) -> np.ndarray:
    """(N,4) xyzi -> (N,8) pcl::PointXYZI records {x,y,z,1, intensity,0,0,0}."""
    out = np.zeros((len(a), 8), np.float32)
    out[:, :3] = a[:, :3]
    out[:, 3] = 1.0
    out[:, 4] = a[:, 3]
    return out


def _cfg(struct_t, default_fn, **kw):
    c = struct_t()
    getattr(lib(), default_fn)(C.byref(c))
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


class Batch:
    """loamx_batch_*: B independent sweeps registered against one frozen sub-map."""

    def __init__(self, max_sweeps: int, **cfg):
        self._c = _cfg(MapConfig, "loamx_map_default_config", **cfg)
        self.h = C.c_void_p(lib().loamx_batch_create(C.byref(self._c), max_sweeps))
        if not self.h:
            raise LoamxError(E_INVALID, lib().loamx_last_error().decode())
        self.n = 0
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_batch_destroy(self.h)
            self.h = None

    __del__ = close

    def set_frozen(self, corner_map, surf_map):
        c, s = as_points(corner_map), as_points(surf_map)
        cc, sc = cloud_of(c), cloud_of(s)
        _check(lib().loamx_batch_set_frozen(self.h, C.byref(cc), C.byref(sc)))

    def set_frozen_device(self, d_corner_ptr: int, n_corner: int, d_surf_ptr: int, n_surf: int):
        _check(lib().loamx_batch_set_frozen_device(self.h, C.c_void_p(d_corner_ptr), n_corner, C.c_void_p(d_surf_ptr), n_surf))

    def stage_frozen_device(self, d_corner_ptr: int, n_corner: int, d_surf_ptr: int, n_surf: int, wait_event: int = 0):
        """index the NEXT epoch's sub-map in the background (double-buffered map epochs); wait_event = raw hipEvent_t"""
        _check(lib().loamx_batch_stage_frozen_device(self.h, C.c_void_p(d_corner_ptr), n_corner, C.c_void_p(d_surf_ptr), n_surf,
                                                     C.c_void_p(wait_event or None)))

    def stage_frozen(self, corner_map, surf_map):
        cm, sm = as_points(corner_map), as_points(surf_map)
        cc, sc = cloud_of(cm), cloud_of(sm)
        _check(lib().loamx_batch_stage_frozen(self.h, C.byref(cc), C.byref(sc)))

    def swap_frozen(self) -> bool:
        return _check(lib().loamx_batch_swap_frozen(self.h)) == OK

    def upload(self, corner_last, surf_last, guesses, full_res=None):
        n = len(corner_last)
        assert len(surf_last) == n and len(guesses) == n
        cl = [as_points(a) for a in corner_last]
        sl = [as_points(a) for a in surf_last]
        fr = [as_points(a) for a in full_res] if full_res is not None else None
        CA = (Cloud * n)(*[cloud_of(a) for a in cl])
        SA = (Cloud * n)(*[cloud_of(a) for a in sl])
        FA = (Cloud * n)(*[cloud_of(a) for a in fr]) if fr is not None else None
        g = np.ascontiguousarray(guesses, np.float32).reshape(n, 6)
        _check(lib().loamx_batch_upload(self.h, n, CA, SA, FA, g.ctypes.data_as(C.c_void_p)))
        self.n = n
        self._full_sizes = [len(a) for a in fr] if fr is not None else None

    def run(self):
        return _check(lib().loamx_batch_run(self.h))

    def run_async(self):
        _check(lib().loamx_batch_run_async(self.h))

    def sync(self):
        _check(lib().loamx_batch_sync(self.h))

    def download(self):
        poses = np.zeros((self.n, 6), np.float32)
        stats = np.zeros((self.n, 4), np.int32)
        _check(lib().loamx_batch_download(self.h, poses.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p)))
        return poses, stats

    def download_full_res(self, sweep: int):
        out = np.zeros((self._full_sizes[sweep], 4), np.float32)
        c = cloud_of(out)
        _check(lib().loamx_batch_download_full_res(self.h, sweep, C.byref(c)))
        return out[:c.count]

    def download_ds(self, sweep: int, cap: int = 1 << 17):
        """the down-sampled stack clouds (corner, surf) of one sweep of the last run — the Gauss-Newton query points"""
        co, so = np.zeros((cap, 4), np.float32), np.zeros((cap, 4), np.float32)
        cc, sc = cloud_of(co), cloud_of(so)
        _check(lib().loamx_batch_download_ds(self.h, sweep, C.byref(cc), C.byref(sc)))
        return co[:cc.count].copy(), so[:sc.count].copy()

    def qr6_probe(self, ata, atb):
        """parity hook: n 6x6 systems through the kernels' wave-cooperative solve and through the scalar routine -> (x_coop, x_scalar)"""
        A = np.ascontiguousarray(ata, np.float32).reshape(-1, 36)
        b = np.ascontiguousarray(atb, np.float32).reshape(-1, 6)
        assert len(A) == len(b)
        xc, xs = np.zeros_like(b), np.zeros_like(b)
        _check(lib().loamx_batch_qr6_probe(self.h, A.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), len(A),
                                           xc.ctypes.data_as(C.c_void_p), xs.ctypes.data_as(C.c_void_p)))
        return xc, xs

    def xrec_stress(self, pairs: int = 64, rounds: int = 20000):
        """stress probe of k_odom_lm's tagged-record exchange -> dict(accepted, torn, inconsistent, timed_out)"""
        out = (C.c_uint64 * 4)()
        _check(lib().loamx_batch_xrec_stress(self.h, pairs, rounds, out))
        return dict(accepted=int(out[0]), torn=int(out[1]), inconsistent=int(out[2]), timed_out=int(out[3]))

    def knn_probe(self, which: int, queries_xyz):
        """the library's own 5-NN search for map-frame points: (indices into the cloud given to set_frozen, squared distances)"""
        q = np.ascontiguousarray(np.asarray(queries_xyz, np.float32)[:, :3])
        idx = np.zeros((len(q), 5), np.uint32)
        d2 = np.zeros((len(q), 5), np.float32)
        _check(lib().loamx_batch_knn_probe(self.h, which, q.ctypes.data_as(C.c_void_p), len(q), idx.ctypes.data_as(C.c_void_p),
                                           d2.ctypes.data_as(C.c_void_p)))
        return idx, d2

    def set_timing(self, on: bool):
        _check(lib().loamx_batch_set_timing(self.h, 1 if on else 0))

    def timing(self):
        ms = (C.c_float * 4)()
        cnt = (C.c_uint64 * 4)()
        _check(lib().loamx_batch_get_timing(self.h, ms, cnt))
        return dict(run_ms=ms[0], residual_ms=ms[1], residual_launches=int(cnt[0]), query_iterations=int(cnt[1]),
                    queries=int(cnt[2]))

    @property
    def stream(self) -> int:
        return int(lib().loamx_batch_stream(self.h) or 0)


SCAN_COUNT_ON_DEVICE, SCAN_IN_PLACE, SCAN_ZERO_IN = 1, 2, 4


def voxel_probe(points, nseg, leaf_even, leaf_odd=None, seg_off=None, seg_ids=None, valid=None):
    """parity hook: the segmented voxel grid on its own (loamx_voxel_probe) -> (voxel means of all segments back to back, out_off[nseg + 1]).
    Exactly one of seg_off (contiguous ranges, nseg + 1 offsets) / seg_ids (one id per point); valid: optional mask, 0 = ignored."""
    p = as_points(np.asarray(points, np.float32).reshape(-1, 4))
    n = len(p)
    off = None if seg_off is None else np.ascontiguousarray(seg_off, np.uint32)
    ids = None if seg_ids is None else np.ascontiguousarray(seg_ids, np.uint32)
    val = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    assert off is None or len(off) == nseg + 1
    assert ids is None or len(ids) == n
    assert val is None or len(val) == n
    out = np.zeros((max(n, 1), 4), np.float32)
    out_off = np.zeros(nseg + 1, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _check(lib().loamx_voxel_probe(ptr(p), C.c_uint32(n), ptr(off), ptr(ids), ptr(val), C.c_uint32(nseg), C.c_float(leaf_even),
                                   C.c_float(leaf_even if leaf_odd is None else leaf_odd), ptr(out), ptr(out_off)))
    return out[:int(out_off[-1])].copy(), out_off


def scan_probe(values, n, max_n=0, flags=0, out_fill=0, want_out2=False):
    """parity hook: the chained exclusive scan on the process's state buffer (loamx_scan_probe).  values: the whole input buffer,
    max(n, max_n) words.  The result buffers start filled with out_fill.  Returns dict(rc, out, total, out2, input_after): rc is the
    call's code (E_HIP after a cut count: the buffers are returned all the same), input_after the input buffer as the scan left it
    (with SCAN_ZERO_IN)."""
    length = max(n, max_n)
    v = np.ascontiguousarray(values, np.uint32).copy()
    assert v.shape == (length,)
    out = np.full(length + 1, out_fill, np.uint32)
    out2 = np.full(length + 1, out_fill, np.uint32) if want_out2 else None
    total = np.zeros(1, np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib().loamx_scan_probe(ptr(v), C.c_uint32(n), C.c_uint32(max_n), C.c_uint32(flags), ptr(out), ptr(total), ptr(out2))
    if rc < 0 and rc != E_HIP:
        _check(rc)
    return dict(rc=rc, out=out, total=int(total[0]), out2=out2, input_after=v if flags & SCAN_ZERO_IN else None)


INDEX_SINGLE, INDEX_PACK_RING, INDEX_FOLD_BOUNDS = 1, 2, 4
INDEX_MAX_CELLS = 16 * 1024 * 1024 - 2048
INDEX_DESC = np.dtype([("ox", "<f4"), ("oy", "<f4"), ("oz", "<f4"), ("inv_h", "<f4"), ("nx", "<i4"), ("ny", "<i4"), ("nz", "<i4"),
                       ("ncell", "<u4"), ("cell_base", "<u4"), ("pt_base", "<u4")])
_index_table = None


def index_probe(points, off, cell_edge=1.05, flags=0):
    """parity hook: the counting-sorted grid index on its own (loamx_index_probe) on the process's single / batch index ->
    dict(desc: K records of INDEX_DESC, table: total cells + 1 entries, sorted: (n, 4) float32 whose .w words are indices)."""
    global _index_table
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    off = np.ascontiguousarray(off, np.uint32)
    n, K = len(p), len(off) - 1
    if _index_table is None:
        _index_table = np.empty(INDEX_MAX_CELLS + 2, np.uint32)   # (the largest table there is; pages are touched as far as a build writes)
    desc = np.zeros(max(K, 1), INDEX_DESC)
    out = np.zeros((max(n, 1), 4), np.float32)
    tlen = np.zeros(1, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().loamx_index_probe(ptr(p), C.c_uint32(n), ptr(off), C.c_uint32(K), C.c_float(cell_edge), C.c_uint32(flags), ptr(desc),
                                   ptr(_index_table), C.c_uint32(len(_index_table)), ptr(tlen), ptr(out)))
    return dict(desc=desc[:K], table=_index_table[:int(tlen[0])].copy(), sorted=out[:n])


VOXBUCKET_SRC_POINTERS = 1
VOXBUCKET_SEG = np.dtype([("bucket0", "<u4"), ("nbuckets", "<u4"), ("pos_bits", "<u4"), ("pad", "<u4")])


def voxbucket_probe(points, seg_off, poses12, leaf_even, leaf_odd=None, flags=0):
    """parity hook: the bucketed voxel grid of the stack clouds on its own (loamx_voxbucket_probe), on the process's one object ->
    dict(stack, out (the rows out_off counts), out_off, gave_up, why, buckets, segs: VOXBUCKET_SEG records, lo, cnt).  poses12: one row
    of 12 float32 words per sweep (two segments): rx ry rz tx ty tz and the sine / cosine words as the kernels are to use them."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    off = np.ascontiguousarray(seg_off, np.uint32)
    poses = np.ascontiguousarray(np.asarray(poses12, np.float32).reshape(-1, 12))
    n, nseg = len(p), len(off) - 1
    assert len(poses) == (nseg + 1) // 2
    m = np.diff(off.astype(np.int64))
    cap = int(np.maximum(1, -(-m // 2048)).sum()) if nseg >= 1 and (m >= 0).all() else 1
    stack = np.zeros((max(n, 1), 4), np.float32)
    out = np.zeros((max(n, 1), 4), np.float32)
    out_off = np.zeros(nseg + 1, np.uint32)
    status = np.zeros(4, np.uint32)
    segs = np.zeros(max(nseg, 1), VOXBUCKET_SEG)
    lo = np.zeros(cap, np.uint64)
    cnt = np.zeros(cap, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().loamx_voxbucket_probe(ptr(p), C.c_uint32(n), ptr(off), C.c_uint32(nseg), ptr(poses), C.c_float(leaf_even),
                                       C.c_float(leaf_even if leaf_odd is None else leaf_odd), C.c_uint32(flags), ptr(stack), ptr(out),
                                       ptr(out_off), ptr(status), ptr(segs), ptr(lo), ptr(cnt), C.c_uint32(cap)))
    return dict(stack=stack[:n], out=out[:min(int(out_off[-1]), n)].copy(), out_off=out_off, gave_up=int(status[0]), why=int(status[1]),
                buckets=int(status[2]), segs=segs[:nseg], lo=lo, cnt=cnt)


REPROJECT_BATCH, REPROJECT_FUSED, REPROJECT_SINGLE, REPROJECT_COPY, REPROJECT_GATHER, REPROJECT_TO_START = 0, 1, 2, 3, 4, 5
REPROJECT_NO_RING_TABLE, REPROJECT_NO_BOUNDS = 8, 16
REPROJECT_RF_N = 320
REPROJECT_PARAMS = np.dtype([("T", "<f4", 6), ("sT", "<f4", 3), ("cT", "<f4", 3), ("shift", "<f4", 3), ("s_start", "<f4", 3),
                             ("c_start", "<f4", 3), ("s_end", "<f4", 3), ("c_end", "<f4", 3), ("scan_period", "<f4"), ("enabled", "<i4")])


def reproject_probe(points, off, params, epoch=1, n_corner_all=0, flags=0, ring_first=None, bounds=None):
    """parity hook: the sweep re-projection kernels on their own (loamx_reproject_probe), on the process's one object ->
    dict(out: (n, 4) float32, ring_first: (K, 320) uint32, bounds: (K, 6) uint32 encoded words).  params: ns records of
    REPROJECT_PARAMS, used word for word.  ring_first / bounds: what the arrays hold before the call (default: zeros / the reset
    words, all ones for a minimum and zero for a maximum); they come back as the kernel left them."""
    p = np.ascontiguousarray(np.asarray(points, np.float32).reshape(-1, 4))
    off = np.ascontiguousarray(off, np.uint32)
    par = np.ascontiguousarray(params, REPROJECT_PARAMS).reshape(-1)
    n, K = len(p), len(off) - 1
    rf = np.zeros((max(K, 1), REPROJECT_RF_N), np.uint32) if ring_first is None else np.array(ring_first, np.uint32).reshape(max(K, 1), REPROJECT_RF_N)
    bb = np.tile(np.array([0xffffffff] * 3 + [0] * 3, np.uint32), (max(K, 1), 1)) if bounds is None else np.array(bounds, np.uint32).reshape(max(K, 1), 6)
    out = np.zeros((max(n, 1), 4), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(lib().loamx_reproject_probe(ptr(p), C.c_uint32(n), ptr(off), C.c_uint32(K), ptr(par), C.c_uint32(len(par)), C.c_uint32(epoch),
                                       C.c_uint32(n_corner_all), C.c_uint32(flags), ptr(out), ptr(rf), ptr(bb)))
    return dict(out=out[:n], ring_first=rf, bounds=bb)


class TransformMaintenance:
    """loamx_tm_*: BasicTransformMaintenance (host arithmetic, no device)."""

    def __init__(self):
        lib().loamx_tm_create.restype = C.c_void_p
        self.h = C.c_void_p(lib().loamx_tm_create())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_tm_destroy(self.h)
            self.h = None

    __del__ = close

    def update_odometry(self, transform_sum):
        t = np.ascontiguousarray(transform_sum, np.float32)
        _check(lib().loamx_tm_update_odometry(self.h, t.ctypes.data_as(C.c_void_p)))

    def update_mapping_transform(self, aft_mapped, bef_mapped):
        a, b = np.ascontiguousarray(aft_mapped, np.float32), np.ascontiguousarray(bef_mapped, np.float32)
        _check(lib().loamx_tm_update_mapping_transform(self.h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))

    def associate_to_map(self):
        _check(lib().loamx_tm_associate_to_map(self.h))
        out = np.zeros(6, np.float32)
        _check(lib().loamx_tm_get_mapped(self.h, out.ctypes.data_as(C.c_void_p)))
        return out


def wire_pose_to_quat(rot_xyz):
    r = np.ascontiguousarray(rot_xyz, np.float32)
    q = np.zeros(4, np.float64)
    _check(lib().loamx_wire_pose_to_quat(r.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p)))
    return q


def wire_quat_to_pose(quat_xyzw):
    q = np.ascontiguousarray(quat_xyzw, np.float64)
    r = np.zeros(3, np.float32)
    _check(lib().loamx_wire_quat_to_pose(q.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p)))
    return r


class MultiScanMapper(C.Structure):
    """loamx_multiscan_mapper (loam::MultiScanMapper)."""
    _fields_ = [("lower_bound_deg", C.c_float), ("upper_bound_deg", C.c_float), ("n_scan_rings", C.c_uint32)]


RING_FROM_BOUNDS, RING_FROM_TABLE, RING_FROM_FIELD = 0, 1, 2
TIME_FROM_AZIMUTH, TIME_FROM_FIELD = 0, 1
FIELD_U8, FIELD_U16, FIELD_U32, FIELD_F32, FIELD_F64 = 1, 2, 3, 4, 5
_FIELD_TYPES = {"u1": FIELD_U8, "u2": FIELD_U16, "u4": FIELD_U32, "f4": FIELD_F32, "f8": FIELD_F64}


class SensorModel(C.Structure):
    """loamx_sensor_model (include/loamx.h): where a raw record's ring and its time within the sweep come from."""
    _fields_ = [("n_scan_rings", C.c_uint32), ("ring_source", C.c_uint32), ("time_source", C.c_uint32),
                ("lower_bound_deg", C.c_float), ("upper_bound_deg", C.c_float), ("ring_angles_deg", C.c_void_p),
                ("max_angle_error_deg", C.c_float), ("ring_offset", C.c_uint32), ("ring_type", C.c_uint32),
                ("time_offset", C.c_uint32), ("time_type", C.c_uint32), ("time_scale", C.c_double)]

    @classmethod
    def from_mapper(cls, sensor="VLP-16", mapper=None):
        """BOUNDS + AZIMUTH: a preset by name, or mapper = (lower_deg, upper_deg, n_rings)"""
        out = cls()
        _check(lib().loamx_sensor_model_from_mapper(C.byref(_mapper(sensor, mapper)), C.byref(out)))
        return out

    def set_table(self, angles_deg, max_error_deg):
        """RING_FROM_TABLE: laser elevations in degrees, strictly increasing (ring 0 = lowest); kept referenced by the model"""
        self._table = np.ascontiguousarray(angles_deg, np.float32)
        self.ring_source = RING_FROM_TABLE
        self.n_scan_rings = len(self._table)
        self.ring_angles_deg = self._table.ctypes.data if len(self._table) else None
        self.max_angle_error_deg = float(max_error_deg)
        return self

    @classmethod
    def from_dtype(cls, dtype, ring="ring", time=None, time_scale=1.0, n_rings=None, table=None, max_error_deg=None, mapper=None):
        """Fill the model from a numpy structured dtype (a PointCloud2 field list: name -> offset, type).  ring: the name of the
        ring field (FIELD), or None for table= (TABLE, with max_error_deg) or mapper= (BOUNDS: a preset name or (lower, upper,
        n)).  time: the name of the time field (FIELD, time_scale = seconds per unit), or None (AZIMUTH: firing order only)."""
        dtype = np.dtype(dtype)
        if ring is not None:
            m = cls()
            off, kind = _field(dtype, ring, (FIELD_U8, FIELD_U16, FIELD_U32))
            assert n_rings is not None, "a ring field needs n_rings"
            m.ring_source, m.ring_offset, m.ring_type, m.n_scan_rings = RING_FROM_FIELD, off, kind, int(n_rings)
        elif table is not None:
            m = cls().set_table(table, max_error_deg)
        else:
            m = cls.from_mapper(mapper) if isinstance(mapper, str) else cls.from_mapper(mapper=mapper)
        m.time_scale = float(time_scale)
        if time is not None:
            m.time_offset, m.time_type = _field(dtype, time, (FIELD_U32, FIELD_F32, FIELD_F64))
            m.time_source = TIME_FROM_FIELD
        return m

    def check(self, stride):
        """loamx_sensor_model_check: raises LoamxError for an invalid model (no device needed)"""
        _check(lib().loamx_sensor_model_check(C.byref(self), int(stride)))


def _field(dtype, name, kinds):
    ft, off = dtype.fields[name][:2]
    kind = _FIELD_TYPES.get(f"{ft.kind}{ft.itemsize}") if ft.byteorder != ">" else None
    assert kind in kinds, f"field {name!r} has type {ft}, the model reads {kinds}"
    return off, kind


def _mapper(sensor, mapper):
    m = MultiScanMapper()
    if mapper is None:
        _check(lib().loamx_multiscan_mapper_preset(sensor.encode(), C.byref(m)))
    else:
        m.lower_bound_deg, m.upper_bound_deg, m.n_scan_rings = float(mapper[0]), float(mapper[1]), int(mapper[2])
    return m


def as_records(records):
    """(bytes as uint8 array, count, stride) of a structured record array (itemsize = stride) or an (n, 3) float32 array"""
    a = np.asarray(records)
    if a.dtype.fields is None:
        a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    else:
        a = np.ascontiguousarray(a).reshape(-1)
        names = list(a.dtype.fields)
        assert a.dtype.fields[names[0]][1] == 0 and all(a.dtype.fields[k][0] == np.float32 for k in names[:3]), "x, y, z float32 at 0 / 4 / 8"
    return a, len(a), a.dtype.itemsize * (3 if a.dtype.fields is None else 1)


class ScanRegistration:
    """loamx_scanreg_*: BasicScanRegistration::processScanlines / extractFeatures on the GPU."""
    NAMES = ("sharp", "less_sharp", "flat", "less_flat")

    def __init__(self, **cfg):
        self._c = _cfg(ScanRegConfig, "loamx_scanreg_default_config", **cfg)
        self.h = C.c_void_p(lib().loamx_scanreg_create(C.byref(self._c)))
        if not self.h:
            raise LoamxError(E_INVALID, lib().loamx_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_scanreg_destroy(self.h)
            self.h = None

    __del__ = close

    def configure(self, **cfg):
        """loamx_scanreg_configure: new parameters, the handle's IMU history and sweep state are kept"""
        for k, v in cfg.items():
            assert hasattr(self._c, k), k
            setattr(self._c, k, v)
        _check(lib().loamx_scanreg_configure(self.h, C.byref(self._c)))

    def process(self, points, ring_sizes, pcl_layout=False):
        pts = as_points(points)
        rs = np.ascontiguousarray(ring_sizes, np.uint32)
        n = len(pts)
        width = 8 if pcl_layout else 4
        key = (max(n, 1), width)
        if getattr(self, "_out_key", None) != key:   # landing buffers are kept between calls (the results below are copies)
            self._outs = [np.zeros(key, np.float32) for _ in range(4)]
            self._out_key = key
        outs = self._outs
        cl = [cloud_of(o) for o in outs]
        cin = cloud_of(pts)
        _check(lib().loamx_scanreg_process(self.h, C.byref(cin), rs.ctypes.data_as(C.c_void_p), len(rs), C.byref(cl[0]),
                                           C.byref(cl[1]), C.byref(cl[2]), C.byref(cl[3])))
        res = {name: outs[k][:cl[k].count].copy() for k, name in enumerate(self.NAMES)}
        res["full"] = pts   # laserCloud(): THE CALLER'S ARRAY, not a copy (binned rings already): a consumer that registers it in place
        # (LaserMapping.process(inplace=True)) rewrites the caller's sweep — pass a copy where the sweep is needed again
        return res

    def process_linked(self, points, ring_sizes):
        """loamx_scanreg_process_linked: enqueue the extraction and leave the clouds in HBM for LaserOdometry.process_linked"""
        pts = as_points(points)
        rs = np.ascontiguousarray(ring_sizes, np.uint32)
        cin = cloud_of(pts)
        self._linked_n = len(pts)
        return _check(lib().loamx_scanreg_process_linked(self.h, C.byref(cin), rs.ctypes.data_as(C.c_void_p), len(rs)))

    def update_imu(self, stamp, roll, pitch, yaw, acc):
        """loamx_scanreg_update_imu (updateIMUData); stamp in seconds"""
        a = np.ascontiguousarray(acc, np.float32)
        _check(lib().loamx_scanreg_update_imu(self.h, C.c_double(stamp), C.c_float(roll), C.c_float(pitch), C.c_float(yaw),
                                              a.ctypes.data_as(C.c_void_p)))

    def set_time(self, t):
        """the scanTime of the next process call"""
        _check(lib().loamx_scanreg_set_time(self.h, C.c_double(t)))

    def imu_trans(self):
        out = np.zeros(12, np.float32)
        _check(lib().loamx_scanreg_get_imu_trans(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def process_raw(self, raw_xyz, sensor="VLP-16", mapper=None):
        """loamx_scanreg_process_raw: MultiScanRegistration::process on a raw (n,3) firing-order cloud in sensor axes.
        mapper = (lower_deg, upper_deg, n_rings) overrides the sensor preset.  Adds "full" and "ring_sizes"."""
        raw = np.ascontiguousarray(raw_xyz, np.float32).reshape(-1, 3)
        return self._process_records(lib().loamx_scanreg_process_raw, _mapper(sensor, mapper), raw.ctypes.data_as(C.c_void_p), len(raw), 12)

    def process_sensor(self, records, model: SensorModel):
        """loamx_scanreg_process_sensor: process_raw with a sensor model.  records: a structured array (itemsize = stride, x, y, z
        float32 first) or an (n, 3) float32 array.  Same results as process_raw."""
        a, n, stride = as_records(records)
        return self._process_records(lib().loamx_scanreg_process_sensor, model, a.ctypes.data_as(C.c_void_p) if n else None, n, stride)

    def _process_records(self, entry, model, data, n, stride):
        """entry(handle, mapper or model, records, ...): landing buffers for n points, the call, the results as copies"""
        outs = [np.zeros((max(n, 1), 4), np.float32) for _ in range(5)]
        cl = [cloud_of(o) for o in outs]
        rs = np.zeros(max(int(model.n_scan_rings), 1), np.uint32)
        _check(entry(self.h, C.byref(model), data, n, stride, C.byref(cl[4]), rs.ctypes.data_as(C.c_void_p), C.byref(cl[0]), C.byref(cl[1]),
                     C.byref(cl[2]), C.byref(cl[3])))
        res = {name: outs[k][:cl[k].count].copy() for k, name in enumerate(self.NAMES)}
        res["full"] = outs[4][:cl[4].count].copy()
        res["ring_sizes"] = rs.astype(np.int32)
        return res


class LaserOdometry:
    """loamx_odom_*: BasicLaserOdometry on the GPU."""

    def __init__(self, **cfg):
        self._c = _cfg(OdomConfig, "loamx_odom_default_config", **cfg)
        self.h = C.c_void_p(lib().loamx_odom_create(C.byref(self._c)))
        if not self.h:
            raise LoamxError(E_INVALID, lib().loamx_last_error().decode())
        self._sizes = (0, 0)

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_odom_destroy(self.h)
            self.h = None

    __del__ = close

    def update_imu(self, t12):
        t = np.ascontiguousarray(t12, np.float32)
        _check(lib().loamx_odom_update_imu(self.h, t.ctypes.data_as(C.c_void_p)))

    def process(self, feats):
        arrs = [as_points(feats[n]) for n in ("sharp", "less_sharp", "flat", "less_flat")]
        cl = [cloud_of(a) for a in arrs]
        rc = _check(lib().loamx_odom_process(self.h, C.byref(cl[0]), C.byref(cl[1]), C.byref(cl[2]), C.byref(cl[3])))
        self._sizes = (len(arrs[1]), len(arrs[3]))
        return rc

    def process_linked(self, scanreg):
        """loamx_odom_process_linked: the sweep `scanreg` has just extracted, taken from its device buffers"""
        rc = _check(lib().loamx_odom_process_linked(self.h, scanreg.h))
        self._sizes = (scanreg._linked_n, scanreg._linked_n)   # (capacities for last_clouds(): each cloud is a subset of the sweep)
        return rc

    def link_wait(self):
        return _check(lib().loamx_odom_link_wait(self.h))

    def _t(self, fn):
        t = np.zeros(6, np.float32)
        _check(fn(self.h, t.ctypes.data_as(C.c_void_p)))
        return t

    @property
    def transform(self):
        return self._t(lib().loamx_odom_get_transform)

    @property
    def transform_sum(self):
        return self._t(lib().loamx_odom_get_transform_sum)

    def set_transform(self, t6):
        t = np.ascontiguousarray(t6, np.float32)
        _check(lib().loamx_odom_set_transform(self.h, t.ctypes.data_as(C.c_void_p)))

    def set_transform_sum(self, t6):
        t = np.ascontiguousarray(t6, np.float32)
        _check(lib().loamx_odom_set_transform_sum(self.h, t.ctypes.data_as(C.c_void_p)))

    def last_clouds(self):
        c = np.zeros((max(self._sizes[0], 1), 4), np.float32)
        s = np.zeros((max(self._sizes[1], 1), 4), np.float32)
        cc, sc = cloud_of(c), cloud_of(s)
        _check(lib().loamx_odom_get_last_clouds(self.h, C.byref(cc), C.byref(sc)))
        return c[:cc.count].copy(), s[:sc.count].copy()

    def transform_to_end(self, cloud):
        a = as_points(cloud).copy()
        c = cloud_of(a)
        _check(lib().loamx_odom_transform_to_end(self.h, C.byref(c)))
        return a

    def stats(self):
        s = (C.c_int * 4)()
        _check(lib().loamx_odom_get_stats(self.h, s))
        return dict(iterations=s[0], sel=s[1], frame=s[2], degenerate=s[3])


class LaserMapping:
    """loamx_map_*: BasicLaserMapping (live rolling map) on the GPU."""

    def __init__(self, **cfg):
        self._c = _cfg(MapConfig, "loamx_map_default_config", **cfg)
        self.h = C.c_void_p(lib().loamx_map_create(C.byref(self._c)))
        if not self.h:
            raise LoamxError(E_INVALID, lib().loamx_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_map_destroy(self.h)
            self.h = None

    __del__ = close

    def update_odometry(self, t6):
        t = np.ascontiguousarray(t6, np.float32)
        _check(lib().loamx_map_update_odometry(self.h, t.ctypes.data_as(C.c_void_p)))

    def update_imu(self, stamp, roll, pitch):
        """updateIMU(IMUState2); stamp in seconds"""
        _check(lib().loamx_map_update_imu(self.h, C.c_double(stamp), C.c_float(roll), C.c_float(pitch)))

    def set_time(self, t):
        """the laserOdometryTime argument of process()"""
        _check(lib().loamx_map_set_time(self.h, C.c_double(t)))

    def process(self, corner_last, surf_last, full_res=None, inplace=False):
        """inplace: register full_res where it lies (what the C entry point does) instead of in a copy"""
        c, s = as_points(corner_last), as_points(surf_last)
        cc, sc = cloud_of(c), cloud_of(s)
        if full_res is not None:
            f = as_points(full_res) if inplace else as_points(full_res).copy()
            fc = cloud_of(f)
            rc = _check(lib().loamx_map_process(self.h, C.byref(cc), C.byref(sc), C.byref(fc)))
            return rc, f
        rc = _check(lib().loamx_map_process(self.h, C.byref(cc), C.byref(sc), None))
        return rc, None

    def process_linked(self, odometry, full_out=None):
        """loamx_map_process_linked: the sweep `odometry` has just handed on (device to device); full_out: an (n, 4) / (n, 8) float32
        array with room for the sweep — receives the registered full-resolution cloud (returned trimmed, a view)"""
        if full_out is None:
            return _check(lib().loamx_map_process_linked(self.h, odometry.h, None)), None
        fc = cloud_of(full_out)
        rc = _check(lib().loamx_map_process_linked(self.h, odometry.h, C.byref(fc)))
        return rc, full_out[:fc.count]

    def speculation(self):
        """(sweeps that adopted the partition prepared for the predicted pose, sweeps whose prediction missed)"""
        c = (C.c_uint64 * 2)()
        _check(lib().loamx_map_get_speculation(self.h, c))
        return int(c[0]), int(c[1])

    def insert(self, corner_last, surf_last, pose6):
        """loamx_map_insert: the epoch merge step — stack, down-size and insert a sweep registered elsewhere with the given pose"""
        c, s = as_points(corner_last), as_points(surf_last)
        cc, sc = cloud_of(c), cloud_of(s)
        p = np.ascontiguousarray(pose6, np.float32)
        assert p.shape == (6,)
        return _check(lib().loamx_map_insert(self.h, C.byref(cc), C.byref(sc), p.ctypes.data_as(C.c_void_p)))

    def transform(self, which="aft"):
        t = np.zeros(6, np.float32)
        _check(lib().loamx_map_get_transform(self.h, ("aft", "bef", "tobe", "sum").index(which), t.ctypes.data_as(C.c_void_p)))
        return t

    def set_transform(self, which, t6):
        t = np.ascontiguousarray(t6, np.float32)
        _check(lib().loamx_map_set_transform(self.h, ("aft", "bef", "tobe", "sum").index(which), t.ctypes.data_as(C.c_void_p)))

    def set_timing(self, on: bool):
        _check(lib().loamx_map_set_timing(self.h, 1 if on else 0))

    def timing(self):
        ms = (C.c_float * 4)()
        cnt = (C.c_uint64 * 4)()
        _check(lib().loamx_map_get_timing(self.h, ms, cnt))
        return dict(run_ms=ms[0], residual_ms=ms[1], residual_launches=int(cnt[0]), query_iterations=int(cnt[1]), queries=int(cnt[2]))

    def has_fresh_map(self):
        return bool(lib().loamx_map_has_fresh_map(self.h))

    def _get(self, fn, *args, cap=1 << 16):
        while True:
            out = np.zeros((cap, 4), np.float32)
            c = cloud_of(out)
            rc = fn(self.h, *args, C.byref(c))
            if rc == E_CAPACITY:
                cap = int(c.count) + 16
                continue
            _check(rc)
            return out[:c.count].copy()

    def save_snapshot(self, path: str):
        _check(lib().loamx_map_save_snapshot(self.h, path.encode()))

    def load_snapshot(self, path: str):
        _check(lib().loamx_map_load_snapshot(self.h, path.encode()))

    def surround(self):
        return self._get(lib().loamx_map_get_surround)

    def cubes(self, which):
        return self._get(lib().loamx_map_get_cubes, 0 if which == "corner" else 1)

    def load_cubes(self, corner, surf):
        c, s = as_points(corner), as_points(surf)
        cc, sc = cloud_of(c), cloud_of(s)
        _check(lib().loamx_map_load_cubes(self.h, C.byref(cc), C.byref(sc)))

    def stats(self):
        s = (C.c_int * 8)()
        _check(lib().loamx_map_get_stats(self.h, s))
        keys = ("iterations", "sel", "corner_ds", "surf_ds", "corner_from_map", "surf_from_map", "degenerate", "optimized")
        return dict(zip(keys, (int(v) for v in s)))


class Pipeline:
    """loamx_pipeline_*: n independent streams, one sweep per stream per step, features -> odometry -> registration
    against a frozen sub-map."""

    def __init__(self, n_streams: int, scanreg=None, odom=None, mapping=None):
        self._f = _cfg(ScanRegConfig, "loamx_scanreg_default_config", **(scanreg or {}))
        self._o = _cfg(OdomConfig, "loamx_odom_default_config", **(odom or {}))
        self._m = _cfg(MapConfig, "loamx_map_default_config", **(mapping or {}))
        L = lib()
        L.loamx_pipeline_create.restype = C.c_void_p
        L.loamx_pipeline_stream.restype = C.c_void_p
        self.h = C.c_void_p(L.loamx_pipeline_create(C.byref(self._f), C.byref(self._o), C.byref(self._m), n_streams))
        if not self.h:
            raise LoamxError(E_INVALID, L.loamx_last_error().decode())
        self.n_streams = n_streams
        self._sizes = None

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_pipeline_destroy(self.h)
            self.h = None

    __del__ = close

    def set_frozen(self, corner_map, surf_map):
        c, s = as_points(corner_map), as_points(surf_map)
        cc, sc = cloud_of(c), cloud_of(s)
        _check(lib().loamx_pipeline_set_frozen(self.h, C.byref(cc), C.byref(sc)))

    def set_frozen_device(self, d_corner_ptr, n_corner, d_surf_ptr, n_surf):
        _check(lib().loamx_pipeline_set_frozen_device(self.h, C.c_void_p(d_corner_ptr), n_corner, C.c_void_p(d_surf_ptr), n_surf))

    def stage_frozen_device(self, d_corner_ptr, n_corner, d_surf_ptr, n_surf, wait_event: int = 0):
        """index the NEXT epoch's sub-map in the background (double-buffered map epochs); wait_event = raw hipEvent_t"""
        _check(lib().loamx_pipeline_stage_frozen_device(self.h, C.c_void_p(d_corner_ptr), n_corner, C.c_void_p(d_surf_ptr), n_surf,
                                                        C.c_void_p(wait_event or None)))

    def stage_frozen(self, corner_map, surf_map):
        cm, sm = as_points(corner_map), as_points(surf_map)
        cc, sc = cloud_of(cm), cloud_of(sm)
        _check(lib().loamx_pipeline_stage_frozen(self.h, C.byref(cc), C.byref(sc)))

    def swap_frozen(self) -> bool:
        return _check(lib().loamx_pipeline_swap_frozen(self.h)) == OK

    def set_state(self, stream, transform=None, transform_sum=None, bef=None, aft=None):
        def p(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)
        keep = []
        _check(lib().loamx_pipeline_set_state(self.h, stream, p(transform), p(transform_sum), p(bef), p(aft)))

    def upload(self, sweeps):
        """sweeps[t][s] = (points (N,4), ring_sizes)"""
        n_steps = len(sweeps)
        ns = self.n_streams
        pts, rings = [], []
        for t in range(n_steps):
            assert len(sweeps[t]) == ns
            for s in range(ns):
                pts.append(as_points(sweeps[t][s][0]))
                rings.append(np.ascontiguousarray(sweeps[t][s][1], np.uint32))
        CA = (Cloud * len(pts))(*[cloud_of(a) for a in pts])
        RP = (C.c_void_p * len(pts))(*[r.ctypes.data for r in rings])
        NR = (C.c_uint32 * len(pts))(*[len(r) for r in rings])
        _check(lib().loamx_pipeline_upload(self.h, n_steps, CA, RP, NR))
        self._sizes = [len(a) for a in pts]

    def stage_step(self, t: int, sweeps_t):
        """streaming input: stage step t (sweeps_t[s] = (points (N,4) float32 C-contiguous, ring_sizes)) without blocking.
        The arrays must stay alive until step(t) has returned (kept referenced here); pinned memory makes the copy a DMA."""
        ns = self.n_streams
        assert len(sweeps_t) == ns
        pts = [as_points(sweeps_t[s][0]) for s in range(ns)]
        rings = [np.ascontiguousarray(sweeps_t[s][1], np.uint32) for s in range(ns)]
        CA = (Cloud * ns)(*[cloud_of(a) for a in pts])
        RP = (C.c_void_p * ns)(*[r.ctypes.data for r in rings])
        NR = (C.c_uint32 * ns)(*[len(r) for r in rings])
        _check(lib().loamx_pipeline_stage_step(self.h, t, CA, RP, NR))
        if not hasattr(self, "_staged"):
            self._staged = {}
        self._staged[t % 8] = (pts, rings, CA, RP, NR)

    def stage_step_raw(self, t: int, raws, sensor="VLP-16", mapper=None, scan_times=None):
        """streaming raw input: raws[s] = (N,3) float32 C-contiguous sensor-frame points in firing order (kept alive here)"""
        ns = self.n_streams
        assert len(raws) == ns
        arrs = [np.ascontiguousarray(r, np.float32).reshape(-1, 3) for r in raws]
        m = MultiScanMapper()
        if mapper is None:
            _check(lib().loamx_multiscan_mapper_preset(sensor.encode(), C.byref(m)))
        else:
            m.lower_bound_deg, m.upper_bound_deg, m.n_scan_rings = float(mapper[0]), float(mapper[1]), int(mapper[2])
        PP = (C.c_void_p * ns)(*[a.ctypes.data if len(a) else None for a in arrs])
        CN = (C.c_uint32 * ns)(*[len(a) for a in arrs])
        st = (C.c_double * ns)(*[float(x) for x in scan_times]) if scan_times is not None else None
        _check(lib().loamx_pipeline_stage_step_raw(self.h, t, PP, CN, 12, C.byref(m), st))
        if not hasattr(self, "_staged"):
            self._staged = {}
        self._staged[t % 8] = (arrs, PP, CN, st)

    def stage_step_sensor(self, t: int, records_list, model: SensorModel, scan_times=None):
        """stage_step_raw with a sensor model: records_list[s] = structured records (one dtype for every stream) or (n, 3) float32"""
        ns = self.n_streams
        assert len(records_list) == ns
        recs = [as_records(r) for r in records_list]
        strides = {r[2] for r in recs if r[1]}
        assert len(strides) <= 1, "every stream's records must have the same stride"
        stride = strides.pop() if strides else recs[0][2]
        PP = (C.c_void_p * ns)(*[r[0].ctypes.data if r[1] else None for r in recs])
        CN = (C.c_uint32 * ns)(*[r[1] for r in recs])
        st = (C.c_double * ns)(*[float(x) for x in scan_times]) if scan_times is not None else None
        _check(lib().loamx_pipeline_stage_step_sensor(self.h, t, PP, CN, stride, C.byref(model), st))
        if not hasattr(self, "_staged"):
            self._staged = {}
        self._staged[t % 8] = (recs, PP, CN, st, model)

    def update_imu(self, stream: int, stamp, roll, pitch, yaw, acc):
        a = np.ascontiguousarray(acc, np.float32)
        _check(lib().loamx_pipeline_update_imu(self.h, stream, C.c_double(stamp), C.c_float(roll), C.c_float(pitch), C.c_float(yaw),
                                               a.ctypes.data_as(C.c_void_p)))

    def enable_async_downloads(self):
        _check(lib().loamx_pipeline_enable_async_downloads(self.h))

    def download_step_async(self, outs):
        """outs: list of (N,4) float32 C-contiguous arrays (capacity); returns the point counts (the data is valid after wait_downloads())"""
        CA = (Cloud * len(outs))(*[cloud_of(a) for a in outs])
        _check(lib().loamx_pipeline_download_step_async(self.h, CA, len(outs)))
        self._dl_keep = (outs, CA)
        return [int(CA[k].count) for k in range(len(outs))]

    def wait_downloads(self):
        _check(lib().loamx_pipeline_wait_downloads(self.h))

    def download_counts(self):
        """(downloads handed to the SDMA engine directly, downloads through hipMemcpyAsync)"""
        c = (C.c_uint64 * 2)()
        _check(lib().loamx_pipeline_download_counts(self.h, c))
        return int(c[0]), int(c[1])

    def step(self, t: int):
        return _check(lib().loamx_pipeline_step(self.h, t))

    def get(self, stream: int):
        tr, ts, aft = (np.zeros(6, np.float32) for _ in range(3))
        st = (C.c_int * 8)()
        _check(lib().loamx_pipeline_get(self.h, stream, tr.ctypes.data_as(C.c_void_p), ts.ctypes.data_as(C.c_void_p),
                                        aft.ctypes.data_as(C.c_void_p), st))
        keys = ("odom_iterations", "odom_sel", "map_iterations", "map_sel", "corner_ds", "surf_ds", "degenerate", "mapped")
        return tr, ts, aft, dict(zip(keys, (int(v) for v in st)))

    def download_full_res(self, slot: int, n: int):
        out = np.zeros((n, 4), np.float32)
        c = cloud_of(out)
        _check(lib().loamx_pipeline_download_full_res(self.h, slot, C.byref(c)))
        return out[:c.count]

    def last_clouds(self, stream: int, capacity: int):
        """loamx_pipeline_download_last_clouds: (corner_last, surf_last) of the stream's sweep of the last step"""
        c, s = np.zeros((max(capacity, 1), 4), np.float32), np.zeros((max(capacity, 1), 4), np.float32)
        cc, sc = cloud_of(c), cloud_of(s)
        _check(lib().loamx_pipeline_download_last_clouds(self.h, stream, C.byref(cc), C.byref(sc)))
        return c[:cc.count].copy(), s[:sc.count].copy()

    def set_lookahead(self, on: bool):
        _check(lib().loamx_pipeline_set_lookahead(self.h, 1 if on else 0))

    def lookahead_depth(self) -> int:
        """steps the odometry may run ahead of the registration (0: look-ahead off)"""
        return int(lib().loamx_pipeline_lookahead_depth(self.h))

    def drain_lookahead(self):
        """wait until the look-ahead has run as far as it may; returns the last step whose odometry is complete (-1: none)"""
        last = C.c_int(-1)
        _check(lib().loamx_pipeline_drain_lookahead(self.h, C.byref(last)))
        return int(last.value)

    def set_timing(self, on, per_launch: bool = True):
        """on: stage events; per_launch: also an event pair around every Gauss-Newton launch (costs ~3 % of a step)."""
        _check(lib().loamx_pipeline_set_timing(self.h, (1 if per_launch else 2) if on else 0))

    def timing(self):
        ms = (C.c_float * 4)()
        rms = (C.c_float * 4)()
        cnt = (C.c_uint64 * 4)()
        _check(lib().loamx_pipeline_get_timing(self.h, ms, rms, cnt))
        return dict(features_ms=ms[0], odometry_ms=ms[1], registration_ms=ms[2], step_ms=ms[3], reg_run_ms=rms[0],
                    residual_ms=rms[1], residual_launches=int(cnt[0]), query_iterations=int(cnt[1]), queries=int(cnt[2]))

    def odom_launch_timing(self):
        """running totals of the odometry chains' timed launch pairs (loamx_pipeline_get_odom_launch_timing)"""
        ms = (C.c_double * 4)()
        cnt = (C.c_uint64 * 7)()
        _check(lib().loamx_pipeline_get_odom_launch_timing(self.h, ms, cnt))
        return dict(lm_ms=ms[0], lm_noop_ms=ms[1], corr_ms=ms[2], corr_noop_ms=ms[3], lm_launches=int(cnt[0]), lm_noop_launches=int(cnt[1]),
                    lm_iterations=int(cnt[2]), corr_launches=int(cnt[3]), corr_noop_launches=int(cnt[4]), lm_bytes=int(cnt[5]),
                    corr_features=int(cnt[6]))

    @property
    def stream(self) -> int:
        return int(lib().loamx_pipeline_stream(self.h) or 0)


class DenseMapConfig(C.Structure):
    _fields_ = [("leaf", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float), ("max_voxels", C.c_uint64),
                ("initial_slots", C.c_uint32), ("device", C.c_int)]


class DenseMapCarveConfig(C.Structure):
    _fields_ = [("max_range", C.c_float), ("ray_stride", C.c_uint32), ("end_margin", C.c_uint32), ("max_steps", C.c_uint32)]


class DenseMapFileInfo(C.Structure):
    """struct loamx_densemap_file_info: the header of a dense map file (flags: 1 carving, 2 moments)"""
    _fields_ = [("version", C.c_uint32), ("flags", C.c_uint32), ("leaf", C.c_float), ("voxels", C.c_uint64), ("offered", C.c_uint64),
                ("dropped_range", C.c_uint64), ("dropped_key", C.c_uint64), ("carve_stats", C.c_uint64 * 6), ("carve", DenseMapCarveConfig)]


def densemap_file_info(path: str, deep: bool = False) -> dict:
    """loamx_densemap_file_info (host only): the header of a dense map file as a dict.  The header and the exact size of the file
    are checked; deep=True also validates every record.  LoamxError E_INVALID names the offending field."""
    i = DenseMapFileInfo()
    _check(lib().loamx_densemap_file_info(os.fsencode(path), C.byref(i), 1 if deep else 0))
    carving = bool(i.flags & 1)
    return dict(version=int(i.version), flags=int(i.flags), carving=carving, moments=bool(i.flags & 2), leaf=float(i.leaf),
                voxels=int(i.voxels), offered=int(i.offered), dropped_range=int(i.dropped_range), dropped_key=int(i.dropped_key),
                carve_stats=[int(v) for v in i.carve_stats],
                carve=dict(max_range=float(i.carve.max_range), ray_stride=int(i.carve.ray_stride), end_margin=int(i.carve.end_margin),
                           max_steps=int(i.carve.max_steps)) if carving else None)


REGION_INSIDE, REGION_OUTSIDE = 0, 1


class DenseMapRegion(C.Structure):
    """loamx_densemap_region: an inclusive window of voxel indices and a side (REGION_INSIDE: the voxels inside it, REGION_OUTSIDE:
    the others).  DenseMapRegion() selects everything; lo / hi: three indices each"""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("side", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, lo=None, hi=None, side=None):
        super().__init__()
        lib().loamx_densemap_region_default(C.byref(self))
        if lo is not None:
            self.lo[:] = [int(v) for v in lo]
        if hi is not None:
            self.hi[:] = [int(v) for v in hi]
        if side is not None:
            self.side = side

    def check(self):
        """loamx_densemap_region_check (host only): LoamxError E_INVALID names the offending field"""
        _check(lib().loamx_densemap_region_check(C.byref(self)))
        return self

    def outside(self) -> "DenseMapRegion":
        """the same window with the other side"""
        return DenseMapRegion(list(self.lo), list(self.hi), REGION_OUTSIDE if self.side == REGION_INSIDE else REGION_INSIDE)

    def as_dict(self) -> dict:
        return dict(lo=list(self.lo), hi=list(self.hi), side=int(self.side))


class DenseMapPageConfig(C.Structure):
    """loamx_densemap_page_config: the tile directory, the voxels per tile edge and the tiles kept around the centre tile per axis"""
    _fields_ = [("dir", C.c_char_p), ("tile_voxels", C.c_uint32), ("radius", C.c_uint32 * 3)]

    def __init__(self, dir=None, tile_voxels=64, radius=(1, 1, 1)):
        super().__init__()
        self.dir = os.fsencode(dir) if dir is not None else None
        self.tile_voxels = tile_voxels
        self.radius[:] = [int(v) for v in radius]


def _f3(v):
    a = np.ascontiguousarray(v, np.float32)
    assert a.shape == (3,)
    return a


def _i3(v):
    return (C.c_int32 * 3)(*[int(x) for x in v])


def densemap_region_about(leaf: float, centre, half) -> DenseMapRegion:
    """loamx_densemap_region_about (host only): the window of the box centre +- half (metres) in a map of this leaf"""
    r, c, h = DenseMapRegion(), _f3(centre), _f3(half)
    _check(lib().loamx_densemap_region_about(C.c_float(leaf), c.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), C.byref(r)))
    return r


def densemap_tile_of(idx, tile_voxels: int):
    """loamx_densemap_tile_of (host only): the tile of a voxel, floor(i / tile_voxels) per axis"""
    t = (C.c_int32 * 3)()
    _check(lib().loamx_densemap_tile_of(_i3(idx), C.c_uint32(tile_voxels), t))
    return tuple(int(v) for v in t)


def densemap_tile_region(tile, tile_voxels: int) -> DenseMapRegion:
    """loamx_densemap_tile_region (host only): the voxels of a tile as a window"""
    r = DenseMapRegion()
    _check(lib().loamx_densemap_tile_region(_i3(tile), C.c_uint32(tile_voxels), C.byref(r)))
    return r


def densemap_tile_name(tile) -> str:
    """loamx_densemap_tile_name (host only): tile_<tx>_<ty>_<tz>.lxdm"""
    buf = C.create_string_buffer(64)
    _check(lib().loamx_densemap_tile_name(_i3(tile), buf, C.c_uint64(64)))
    return buf.value.decode()


def densemap_file_merge(path_a: str, path_b: str, path_out: str):
    """loamx_densemap_file_merge (host only): the records of two dense map files added per key, as DenseMap.merge adds"""
    _check(lib().loamx_densemap_file_merge(os.fsencode(path_a), os.fsencode(path_b), os.fsencode(path_out)))


class StaticRule(C.Structure):
    """loamx_densemap_static_rule: a voxel is dynamic iff miss >= min_misses and miss * den > n * num.  StaticRule() is the default
    rule (3, 1, 1)."""
    _fields_ = [("min_misses", C.c_uint32), ("num", C.c_uint32), ("den", C.c_uint32)]

    def __init__(self, min_misses=None, num=None, den=None):
        super().__init__()
        lib().loamx_densemap_static_rule_default(C.byref(self))
        for k, v in (("min_misses", min_misses), ("num", num), ("den", den)):
            if v is not None:
                setattr(self, k, v)

    def is_dynamic(self, n: int, miss: int) -> bool:
        """the rule on one voxel (host only)"""
        return bool(_check(lib().loamx_densemap_rule_is_dynamic(C.byref(self), C.c_uint64(n), C.c_uint32(miss))))


class SurfelConfig(C.Structure):
    """loamx_densemap_surfel_config: a voxel has a surfel iff n >= min_points, its points are not all equal, and the middle
    eigenvalue of their covariance is at least min_planar_ratio times the largest.  SurfelConfig() holds the defaults (5, 0.01)."""
    _fields_ = [("min_points", C.c_uint32), ("min_planar_ratio", C.c_float)]

    def __init__(self, min_points=None, min_planar_ratio=None):
        super().__init__()
        lib().loamx_densemap_surfel_default_config(C.byref(self))
        for k, v in (("min_points", min_points), ("min_planar_ratio", min_planar_ratio)):
            if v is not None:
                setattr(self, k, v)


SURFEL_FIELDS = ("x", "y", "z", "intensity", "normal_x", "normal_y", "normal_z", "curvature")   # loamx_surfel, PCL PointXYZINormal order

_AXES = {"loam": 0, "sensor": 1}


def _axes(axes) -> int:
    assert axes in _AXES, f"axes must be one of {tuple(_AXES)}"
    return _AXES[axes]


def surfel_of(leaf, idx, vals, mom, axes="loam", min_points=None, min_planar_ratio=None) -> np.ndarray:
    """loamx_densemap_surfel_of (host only): the surfel of one voxel from its integer words — idx = (ix, iy, iz), vals = (n, Sx, Sy,
    Sz), mom = the nine moment words (Python integers are taken modulo 2^64).  Returns (8,) float32 in the order of SURFEL_FIELDS."""
    i = (C.c_int32 * 3)(*[int(v) for v in idx])
    v = (C.c_uint64 * 4)(*[int(x) % (1 << 64) for x in vals])
    m = (C.c_uint64 * 9)(*[int(x) % (1 << 64) for x in mom])
    c = SurfelConfig(min_points, min_planar_ratio)
    out = np.zeros(8, np.float32)
    _check(lib().loamx_densemap_surfel_of(C.c_float(leaf), i, v, m, C.byref(c), _axes(axes), out.ctypes.data_as(C.c_void_p)))
    return out


class AlignConfig(C.Structure):
    """loamx_densemap_align_config; AlignConfig() holds the defaults (20 iterations, neighbourhood 1, max_residual 0 = the leaf, 50
    matches, 1e-5 rad / 1e-5 m, degenerate_ratio 1e-4)."""
    _fields_ = [("max_iterations", C.c_uint32), ("neighbourhood", C.c_uint32), ("max_residual", C.c_float), ("min_matched", C.c_uint32),
                ("eps_rot", C.c_float), ("eps_trans", C.c_float), ("degenerate_ratio", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        lib().loamx_densemap_align_default_config(C.byref(self))
        for k, v in kw.items():
            assert hasattr(self, k), k
            if v is not None:
                setattr(self, k, v)


class AlignResult(C.Structure):
    """loamx_densemap_align_result: pose (row-major 3x4, map <- cloud), iterations, degenerate_dims, status (0 converged, 1
    max_iterations reached, 2 fewer than min_matched matches), rms and counts of the last step"""
    _fields_ = [("pose", C.c_double * 12), ("iterations", C.c_uint32), ("degenerate_dims", C.c_uint32), ("status", C.c_int),
                ("rms", C.c_double), ("counts", C.c_uint64 * 5)]

    def as_dict(self) -> dict:
        return dict(pose=np.array(self.pose[:], np.float64).reshape(3, 4), iterations=int(self.iterations),
                    degenerate_dims=int(self.degenerate_dims), status=int(self.status), rms=float(self.rms),
                    counts=dict(zip(ALIGN_COUNTS, (int(v) for v in self.counts))))


ALIGN_COUNTS = ("far", "outside", "unmatched", "rejected", "matched")   # counts[5] of loamx_densemap_align_step


def align_solve(sums, degenerate_ratio=1e-4):
    """loamx_densemap_align_solve (host only): (x (6,) float64, dropped) from the 28 integer sums of an align_step"""
    s = np.ascontiguousarray(sums, np.int64)
    assert s.shape == (28,)
    x = np.zeros(6, np.float64)
    dropped = C.c_uint32(0)
    _check(lib().loamx_densemap_align_solve(s.ctypes.data_as(C.c_void_p), C.c_float(degenerate_ratio), x.ctypes.data_as(C.c_void_p),
                                            C.byref(dropped)))
    return x, int(dropped.value)


ALIGN_MAX_POSES = 4096   # LOAMX_ALIGN_MAX_POSES
PYRAMID_MAX_LEVELS = 6   # LOAMX_PYRAMID_MAX_LEVELS


class PyramidConfig(C.Structure):
    """loamx_densemap_pyramid_config: levels (1 .. PYRAMID_MAX_LEVELS, default 3) and max_curvature (levels >= 1: a surfel with a larger
    curvature gets no entry; 0 = no limit, the default)"""
    _fields_ = [("levels", C.c_uint32), ("max_curvature", C.c_float)]


def align_best(results):
    """loamx_densemap_align_best (host only): the index of the best of a list of AlignResult / an (n,) ctypes array of them — status
    != 2, most matched, then the smallest rms, then the smallest index — or None when there is no candidate.  A converged status is
    not evidence of a correct pose: judge the winner by its matched count and rms"""
    arr = results if isinstance(results, C.Array) else (AlignResult * max(len(results), 1))(*results)
    n = len(results)
    best = C.c_uint32(0)
    _check(lib().loamx_densemap_align_best(arr, C.c_uint32(n), C.byref(best)))
    return None if best.value == 0xFFFFFFFF else int(best.value)


def pose_grid(base, centre=None, yaws=(0,), offsets=((0, 0, 0),)) -> np.ndarray:
    """Start poses for DenseMap.align_many around base (3x4, map <- cloud): for each yaw a (rad; rot_y of the pose convention, about
    the image of centre, default 0) and each map-frame offset o, R = Ry(a) R_base and t' = (R_base c + t_base + o) - R c, so the image
    of centre moves by exactly o.  Returns (len(yaws) * len(offsets), 3, 4) float64, yaw-major.  numpy only.
    For a loamx_place match pass the stored entry's pose as base, its sensor origin as centre and the match's yaw_hint as it is
    (yaws = yaw_hint + a few steps of 2 pi / n_sectors either side): shift k means the query sensor has turned by +k 2 pi / S."""
    P = np.asarray(base, np.float64).reshape(3, 4)
    c = np.zeros(3) if centre is None else np.asarray(centre, np.float64).reshape(3)
    ys = np.asarray(yaws, np.float64).reshape(-1)
    os_ = np.asarray(offsets, np.float64).reshape(-1, 3)
    anchor = P[:, :3] @ c + P[:, 3]
    out = np.zeros((len(ys) * len(os_), 3, 4), np.float64)
    for i, a in enumerate(ys):
        if a == 0.0:
            R = P[:, :3].copy()   # (bit for bit the base)
        else:
            ca, sa = np.cos(a), np.sin(a)
            R = np.array([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]]) @ P[:, :3]
        for j, o in enumerate(os_):
            out[i * len(os_) + j, :, :3] = R
            out[i * len(os_) + j, :, 3] = P[:, 3] if a == 0.0 and not o.any() else (anchor + o) - R @ c
    return out


def _pose12(pose):
    p = np.ascontiguousarray(pose, np.float64)
    assert p.shape == (3, 4) or p.shape == (12,), "a pose is a row-major 3x4 matrix"
    return p.reshape(12)


class RayHit(C.Structure):
    """loamx_ray_hit, 40 bytes: the first voxel a ray meets — its key, its exported position (the bytes of points()), the range along
    the ray to the foot of that position, its point count and miss word, steps (k of the hit cell; without a hit the cells looked up)
    and status (RAY_NOT_TRACED, RAY_MISS, RAY_HIT, RAY_HIT_END)"""
    _fields_ = [("key", C.c_uint64), ("x", C.c_float), ("y", C.c_float), ("z", C.c_float), ("range", C.c_float), ("n", C.c_uint32),
                ("miss", C.c_uint32), ("steps", C.c_uint32), ("status", C.c_uint32)]


class RaycastConfig(C.Structure):
    """loamx_densemap_raycast_config; the defaults are 4096, 0, 1"""
    _fields_ = [("max_steps", C.c_uint32), ("skip_steps", C.c_uint32), ("min_points", C.c_uint32)]


RAY_NOT_TRACED, RAY_MISS, RAY_HIT, RAY_HIT_END = range(4)                         # loamx_ray_hit.status
RAY_COUNTS = ("not_traced", "miss", "hit", "hit_end", "cells")                    # counts[5] of loamx_densemap_raycast
RAY_DTYPE = np.dtype([(n, np.dtype(t)) for n, t in RayHit._fields_])              # the records as a structured numpy array


def range_image_ends(pose, elevations_deg, n_azimuth: int, max_range: float) -> np.ndarray:
    """the end points of the rays of a lidar at pose (3x4, map <- sensor, LOAM axes: x left, y up, z forward): one ring per
    elevation, n_azimuth rays per ring at the azimuths 2 pi j / n_azimuth from +z towards +x, each max_range long.  Returns
    (rings * n_azimuth, 4) float32, ring-major, intensity = the ring's index; computed in float64 and rounded once.  numpy only.
    A rendered range image is DenseMap.raycast(ends, origin=pose[:, 3])[0]["range"].reshape(rings, n_azimuth)."""
    P = np.asarray(pose, np.float64).reshape(3, 4)
    el = np.deg2rad(np.asarray(elevations_deg, np.float64).reshape(-1))
    az = 2.0 * np.pi * np.arange(int(n_azimuth)) / int(n_azimuth)
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    d = np.stack([ce * np.sin(az)[None, :], se * np.ones_like(az)[None, :], ce * np.cos(az)[None, :]], axis=2).reshape(-1, 3)
    out = np.zeros((len(d), 4), np.float32)
    out[:, :3] = (d * float(max_range)) @ P[:, :3].T + P[:, 3]
    out[:, 3] = np.repeat(np.arange(len(el)), int(n_azimuth))
    return out


class _DefaultedConfig:
    """what GridConfig, RouteConfig, FrontierConfig and SegmentConfig share, beside C.Structure: construction from the library's defaults (the
    function named by _default) with keyword arguments on top, update, copy, and check by the function named by _checker"""
    _default = _checker = None

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)

        def check(self):
            _check(getattr(lib(), cls._checker)(C.byref(self)))
            return self
        check.__doc__ = cls._checker + " (host only): LoamxError E_INVALID names the first field out of its bounds"
        cls.check = check

    def __init__(self, **fields):
        super().__init__()
        getattr(lib(), self._default)(C.byref(self))
        self.update(**fields)

    def update(self, **fields):
        for k, v in fields.items():
            assert hasattr(self, k), k
            setattr(self, k, v)
        return self

    def copy(self, **fields):
        c = type(self)()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(c))
        return c.update(**fields)


class GridConfig(_DefaultedConfig, C.Structure):
    """loamx_densemap_grid_config: the window (cell_leaves, x0, z0, nx, nz) and the rules of the navigation grid.  GridConfig() holds
    the defaults (2; 0, 0; 256 x 256; min_points 2; y in [-2^20, 2^20]; band 3..20; 1 obstacle voxel; max_step 2; clear_max 10);
    keyword arguments replace them."""
    _fields_ = [("cell_leaves", C.c_uint32), ("x0", C.c_int32), ("z0", C.c_int32), ("nx", C.c_uint32), ("nz", C.c_uint32),
                ("min_points", C.c_uint32), ("y_min", C.c_int32), ("y_max", C.c_int32), ("band_lo", C.c_uint32), ("band_hi", C.c_uint32),
                ("min_obstacle_voxels", C.c_uint32), ("max_step", C.c_uint32), ("clear_max", C.c_uint32)]

    _default, _checker = "loamx_densemap_grid_default_config", "loamx_densemap_grid_check"


class GridCell(C.Structure):
    """loamx_grid_cell, 24 bytes: ground (iy of the lowest qualifying voxel; GRID_NONE: none), elevation (metres), obstacles (voxels in
    the body band), overhead (lowest iy above the band; GRID_NONE: none), clear2 (capped squared distance in cells to the nearest
    OBSTACLE or STEP cell) and cls (GRID_UNKNOWN, GRID_FREE, GRID_OBSTACLE, GRID_STEP)"""
    _fields_ = [("ground", C.c_int32), ("elevation", C.c_float), ("obstacles", C.c_uint32), ("overhead", C.c_int32),
                ("clear2", C.c_uint32), ("cls", C.c_uint32)]


GRID_UNKNOWN, GRID_FREE, GRID_OBSTACLE, GRID_STEP = range(4)                      # loamx_grid_cell.cls
GRID_NONE = 0x7fffffff                                                            # ground / overhead of a cell without one
GRID_CELL = np.dtype([(n, np.dtype(t)) for n, t in GridCell._fields_])            # the records as a structured numpy array


def grid_window(leaf, centre_x, centre_z, half_extent, cell_leaves=2) -> GridConfig:
    """loamx_densemap_grid_window (host only): a GridConfig (defaults otherwise) whose window covers centre +- half_extent metres in
    x and z (LOAM frame) with cells of cell_leaves voxels.  LoamxError E_INVALID when the window breaks a bound of the check."""
    c = GridConfig(cell_leaves=cell_leaves)
    _check(lib().loamx_densemap_grid_window(C.c_float(leaf), C.c_float(centre_x), C.c_float(centre_z), C.c_float(half_extent), C.byref(c)))
    return c


def _grid_cells(cells) -> np.ndarray:
    a = np.ascontiguousarray(cells)
    assert a.dtype == GRID_CELL, "cells must be an array of GRID_CELL records"
    return a


def grid_occupancy(cells) -> np.ndarray:
    """loamx_grid_occupancy (host only): int8 of the cells' shape, -1 UNKNOWN, 0 FREE, 100 OBSTACLE or STEP (nav_msgs/OccupancyGrid)"""
    a = _grid_cells(cells)
    out = np.zeros(a.shape, np.int8)
    _check(lib().loamx_grid_occupancy(a.ctypes.data_as(C.c_void_p), C.c_uint64(a.size), out.ctypes.data_as(C.c_void_p)))
    return out


def write_grid_pgm(stem: str, cells, cfg: GridConfig, leaf: float):
    """loamx_write_grid_pgm (host only): stem.pgm and stem.yaml as ROS map_server reads them, in the sensor axes (image columns run
    along LOAM z = x_s, image rows against LOAM x = y_s).  cells: the (nz, nx) array of DenseMap.grid(cfg)."""
    a = _grid_cells(cells)
    assert a.size == cfg.nx * cfg.nz, "cells does not have the configuration's nx * nz records"
    _check(lib().loamx_write_grid_pgm(os.fsencode(stem), a.ctypes.data_as(C.c_void_p), C.byref(cfg), C.c_float(leaf)))


class RouteConfig(_DefaultedConfig, C.Structure):
    """loamx_grid_route_config: how the cells of a navigation grid are weighted and joined for routing.  RouteConfig() holds the
    defaults (connectivity 8, min_clear2 1, soft_clear2 0, soft_weight 0, unknown_weight 0); keyword arguments replace them."""
    _fields_ = [("connectivity", C.c_uint32), ("min_clear2", C.c_uint32), ("soft_clear2", C.c_uint32), ("soft_weight", C.c_uint32),
                ("unknown_weight", C.c_uint32)]

    _default, _checker = "loamx_grid_route_default_config", "loamx_grid_route_check"


class RouteCell(C.Structure):
    """loamx_route_cell, 8 bytes: cost (the smallest sum of move costs to a goal; ROUTE_UNREACHABLE) and next (the direction 0..7 of
    the next step, (dx, dz) = ROUTE_MOVES[next]; ROUTE_GOAL; ROUTE_NONE)"""
    _fields_ = [("cost", C.c_uint32), ("next", C.c_uint32)]


ROUTE_UNREACHABLE, ROUTE_GOAL, ROUTE_NONE = 0xffffffff, 8, 9
ROUTE_MOVES = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))   # (dx, dz) of direction d
ROUTE_CELL = np.dtype([(n, np.dtype(t)) for n, t in RouteCell._fields_])              # the field as a structured numpy array


def _tuples(cells, dim) -> np.ndarray:
    """(n, dim) uint32, C order, of a list of cells, each a tuple of dim window-relative indices"""
    return np.ascontiguousarray(np.asarray(cells, np.uint32).reshape(-1, dim))


def _xz_pairs(pairs) -> np.ndarray:
    """(n, 2) uint32, C order, of a list of (rx, rz) pairs"""
    return _tuples(pairs, 2)


def _route_field(field) -> np.ndarray:
    a = np.ascontiguousarray(field)
    assert a.dtype == ROUTE_CELL and a.ndim == 2, "field must be an (nz, nx) array of ROUTE_CELL records"
    return a


def _host_trace(fn, f, dims, start, dim, capacity):
    """route_trace and route3_trace: fn(field, *dims, *start, out, capacity, &n) walks on the host; capacity None: asked for the
    length first"""
    n = C.c_uint32(0)
    if capacity is None:
        _check(fn(f.ctypes.data_as(C.c_void_p), *dims, *start, None, 0, C.byref(n)))
        capacity = n.value
    out = np.zeros((capacity, dim), np.uint32)
    _check(fn(f.ctypes.data_as(C.c_void_p), *dims, *start, out.ctypes.data_as(C.c_void_p), C.c_uint32(capacity), C.byref(n)))
    return out[:min(n.value, capacity)], n.value


def route_weight(cells, cfg: RouteConfig = None) -> np.ndarray:
    """loamx_grid_route_weight (host only): the weight of every cell of a GRID_CELL array under cfg, uint8 of the cells' shape: 0
    blocked, otherwise 1..32"""
    a = _grid_cells(cells)
    c = RouteConfig() if cfg is None else cfg
    flat = a.reshape(-1)
    out = np.zeros(flat.shape, np.uint8)
    L, p, step = lib(), flat.ctypes.data, GRID_CELL.itemsize
    for i in range(flat.size):
        out[i] = _check(L.loamx_grid_route_weight(C.c_void_p(p + i * step), C.byref(c)))
    return out.reshape(a.shape)


def route_trace(field, start, capacity=None):
    """loamx_grid_route_trace (host only): the route from start = (rx, rz) over an (nz, nx) field -> ((min(n, capacity), 2) uint32 of
    (rx, rz) pairs up to and including the goal cell, n = the full length; 0 for a start outside the window or unreachable).
    capacity None: the whole route.  LoamxError E_INVALID on a field that is not a route field"""
    f = _route_field(field)
    nz, nx = f.shape
    return _host_trace(lib().loamx_grid_route_trace, f, (nx, nz), (C.c_uint32(start[0]), C.c_uint32(start[1])), 2, capacity)


def route_points(cfg: GridConfig, leaf: float, route, cells=None) -> np.ndarray:
    """loamx_grid_route_points (host only): (n, 3) float32 metres in the LOAM frame for the (rx, rz) pairs of a route, the cell
    centres in x and z and the cells' elevation in y (cells None: 0)"""
    r = _xz_pairs(route)
    a = None if cells is None else _grid_cells(cells)
    assert a is None or a.size == cfg.nx * cfg.nz, "cells does not have the configuration's nx * nz records"
    out = np.zeros((len(r), 3), np.float32)
    _check(lib().loamx_grid_route_points(C.byref(cfg), C.c_float(leaf), a.ctypes.data_as(C.c_void_p) if a is not None else None,
                                         r.ctypes.data_as(C.c_void_p), C.c_uint32(len(r)), out.ctypes.data_as(C.c_void_p)))
    return out


def grid_cell_of(cfg: GridConfig, leaf: float, x: float, z: float):
    """loamx_densemap_grid_cell_of (host only): the window-relative cell (rx, rz) of a position in metres (LOAM x and z), or None
    when it lies outside the window"""
    rx, rz, inside = C.c_uint32(0), C.c_uint32(0), C.c_int(0)
    _check(lib().loamx_densemap_grid_cell_of(C.byref(cfg), C.c_float(leaf), C.c_float(x), C.c_float(z), C.byref(rx), C.byref(rz),
                                             C.byref(inside)))
    return (rx.value, rz.value) if inside.value else None


class FrontierConfig(_DefaultedConfig, C.Structure):
    """loamx_grid_frontier_config: which FREE cells of a navigation grid are frontier cells (min_unknown of the eight neighbours
    UNKNOWN, clear2 >= min_clear2), how they join (connectivity 4 or 8) and which frontiers are kept (min_cells).  FrontierConfig()
    holds the defaults (8, 1, 1, 1); keyword arguments replace them."""
    _fields_ = [("connectivity", C.c_uint32), ("min_unknown", C.c_uint32), ("min_clear2", C.c_uint32), ("min_cells", C.c_uint32)]

    _default, _checker = "loamx_grid_frontier_default_config", "loamx_grid_frontier_check"


FRONTIER_NONE = 0xffffffff                                                        # label of a cell in no kept frontier; no best_cell
# loamx_frontier, 64 bytes: min_cell (the smallest record index of its cells, its identity), cells, the inclusive box lo .. hi in
# (rx, rz), the sums of rx and rz, unknown_links (the sum of unknown8), and from the field reachable, best_cost and best_cell
FRONTIER = np.dtype([("min_cell", "<u4"), ("cells", "<u4"), ("lo", "<u4", 2), ("hi", "<u4", 2), ("sum_rx", "<u8"), ("sum_rz", "<u8"),
                     ("unknown_links", "<u8"), ("reachable", "<u4"), ("best_cost", "<u4"), ("best_cell", "<u4"), ("reserved", "<u4")])
FRONTIER_STATS = ("cells", "frontiers", "kept", "kept_cells", "kept_reachable", "hooks_lost")   # stats[6] of loamx_densemap_frontiers


def frontiers_best(frontiers, min_cost=0) -> int:
    """loamx_frontiers_best (host only): the index of the FRONTIER record with the smallest best_cost among those with
    min_cost <= best_cost < ROUTE_UNREACHABLE, ties to the smaller index; FRONTIER_NONE when there is none"""
    a = np.ascontiguousarray(frontiers, FRONTIER).reshape(-1)
    best = C.c_uint32(0)
    _check(lib().loamx_frontiers_best(a.ctypes.data_as(C.c_void_p) if len(a) else None, C.c_uint64(len(a)), C.c_uint32(min_cost),
                                      C.byref(best)))
    return int(best.value)


class DistConfig(_DefaultedConfig, C.Structure):
    """loamx_densemap_dist_config: the 3-D window (cell_leaves, x0, y0, z0, nx, ny, nz), which voxels count (min_points) and the cap
    d_max of the distance field.  DistConfig() holds the defaults (2; 0, 0, 0; 128 x 32 x 128; min_points 2; d_max 16); keyword
    arguments replace them."""
    _fields_ = [("cell_leaves", C.c_uint32), ("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32), ("nx", C.c_uint32),
                ("ny", C.c_uint32), ("nz", C.c_uint32), ("min_points", C.c_uint32), ("d_max", C.c_uint32)]

    _default, _checker = "loamx_densemap_dist_default_config", "loamx_densemap_dist_check"


DIST_NONE = 0xffffffff                                                            # near of a capped cell, and of a point outside
DIST_OUTSIDE = 0xffffffff                                                         # d2 of a point that has no cell in the window
DIST_SAMPLE = np.dtype([("d2", "<u4"), ("near", "<u4")])                          # loamx_dist_sample, 8 bytes
DIST_STATS = ("voxels", "occupied", "within", "max_d2")                           # stats[4] of loamx_densemap_dist
DIST_QUERY_STATS = ("inside", "outside", "capped", "below", "best")               # stats[5] of loamx_densemap_dist_query


def dist_window(leaf, x, y, z, half_extent_xyz, cell_leaves=2) -> DistConfig:
    """loamx_densemap_dist_window (host only): a DistConfig (defaults otherwise) whose window covers (x, y, z) +- half_extent_xyz
    metres (LOAM frame; one number serves the three axes) with cells of cell_leaves voxels.  LoamxError E_INVALID when the window
    breaks a bound of the check."""
    c = DistConfig(cell_leaves=cell_leaves)
    centre = (C.c_float * 3)(x, y, z)
    half = (C.c_float * 3)(*np.broadcast_to(np.asarray(half_extent_xyz, np.float32), (3,)).tolist())
    _check(lib().loamx_densemap_dist_window(C.c_float(leaf), centre, half, C.byref(c)))
    return c


def dist_near_unpack(near):
    """loamx_dist_near_unpack (host only): the window-relative cell (rx, ry, rz) of a near word; LoamxError E_INVALID for DIST_NONE"""
    rx, ry, rz = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    _check(lib().loamx_dist_near_unpack(C.c_uint32(int(near)), C.byref(rx), C.byref(ry), C.byref(rz)))
    return rx.value, ry.value, rz.value


def dist_metres(d2, leaf: float, cell_leaves: int) -> float:
    """loamx_dist_metres (host only): sqrt(d2) * leaf * cell_leaves in double, the distance between the cell centres"""
    fn = lib().loamx_dist_metres
    fn.restype = C.c_double
    return float(fn(C.c_uint32(int(d2)), C.c_float(leaf), C.c_uint32(cell_leaves)))


class Route3Config(_DefaultedConfig, C.Structure):
    """loamx_route3_config: how the cells of a distance field are weighted and joined for routing in 3-D.  Route3Config() holds the
    defaults (connectivity 26, min_d2 1, soft_d2 0, soft_weight 0); keyword arguments replace them."""
    _fields_ = [("connectivity", C.c_uint32), ("min_d2", C.c_uint32), ("soft_d2", C.c_uint32), ("soft_weight", C.c_uint32)]

    _default, _checker = "loamx_route3_default_config", "loamx_route3_check"


ROUTE3_GOAL, ROUTE3_NONE = 26, 27
# (dx, dy, dz) of direction d: six axial, twelve face diagonals, eight space diagonals (include/loamx.h; loamx_route3_move)
ROUTE3_MOVES = (((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
                + tuple((a, b, 0) for b in (1, -1) for a in (1, -1)) + tuple((a, 0, b) for b in (1, -1) for a in (1, -1))
                + tuple((0, a, b) for b in (1, -1) for a in (1, -1)) + tuple((a, b, c) for c in (1, -1) for b in (1, -1) for a in (1, -1)))
ROUTE3_STATS = ("traversable", "reachable", "goals_used", "max_cost", "rounds", "brick_runs")   # stats[6] of loamx_densemap_route3


def _xyz_triples(triples) -> np.ndarray:
    """(n, 3) uint32, C order, of a list of (rx, ry, rz) triples"""
    return _tuples(triples, 3)


def _route3_field(field) -> np.ndarray:
    a = np.ascontiguousarray(field)
    assert a.dtype == ROUTE_CELL and a.ndim == 3, "field must be an (nz, ny, nx) array of ROUTE_CELL records"
    return a


def route3_weight(d2, cfg: Route3Config = None) -> np.ndarray:
    """loamx_route3_weight (host only): the weight of every cell of a d2 array under cfg, uint8 of its shape: 0 blocked, otherwise
    1..16"""
    a = np.asarray(d2)
    c = Route3Config() if cfg is None else cfg
    L = lib()
    return np.array([_check(L.loamx_route3_weight(C.c_uint32(int(v)), C.byref(c))) for v in a.reshape(-1)], np.uint8).reshape(a.shape)


def route3_move(d: int):
    """loamx_route3_move (host only): (dx, dy, dz) of direction d = 0..25"""
    out = (C.c_int32 * 3)()
    _check(lib().loamx_route3_move(C.c_uint32(d), out))
    return tuple(out)


def route3_trace(field, start, capacity=None):
    """loamx_route3_trace (host only): the route from start = (rx, ry, rz) over an (nz, ny, nx) field -> ((min(n, capacity), 3)
    uint32 of (rx, ry, rz) triples up to and including the goal cell, n = the full length; 0 for a start outside the window or
    unreachable).  capacity None: the whole route.  LoamxError E_INVALID on a field that is not a route3 field"""
    f = _route3_field(field)
    nz, ny, nx = f.shape
    return _host_trace(lib().loamx_route3_trace, f, (nx, ny, nz), ((C.c_uint32 * 3)(*[int(v) for v in start]),), 3, capacity)


def route3_points(cfg: DistConfig, leaf: float, route) -> np.ndarray:
    """loamx_route3_points (host only): (n, 3) float32 metres in the LOAM frame, the cell centres of the (rx, ry, rz) triples of a
    route"""
    r = _xyz_triples(route)
    out = np.zeros((len(r), 3), np.float32)
    _check(lib().loamx_route3_points(C.byref(cfg), C.c_float(leaf), r.ctypes.data_as(C.c_void_p), C.c_uint32(len(r)),
                                     out.ctypes.data_as(C.c_void_p)))
    return out


def dist_cell_of(cfg: DistConfig, leaf: float, x: float, y: float, z: float):
    """loamx_densemap_dist_cell_of (host only): the window-relative cell (rx, ry, rz) of a position in metres (LOAM frame), or None
    when it lies outside the window"""
    r, inside = (C.c_uint32 * 3)(), C.c_int(0)
    _check(lib().loamx_densemap_dist_cell_of(C.byref(cfg), C.c_float(leaf), C.c_float(x), C.c_float(y), C.c_float(z), r, C.byref(inside)))
    return tuple(r) if inside.value else None


class TsdfConfig(_DefaultedConfig, C.Structure):
    """loamx_densemap_tsdf_config: the window of one-voxel cells (x0, y0, z0, nx, ny, nz), the truncation in leaves, whether the
    whole ray is integrated (free_space), the ray stride, the step limit and the range filter of the signed distance field.
    TsdfConfig() holds the defaults (-64, -64, -64; 128^3; 3 leaves; band only; stride 1; 4096 steps; no range limits); keyword
    arguments replace them."""
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("z0", C.c_int32), ("nx", C.c_uint32), ("ny", C.c_uint32), ("nz", C.c_uint32),
                ("trunc_leaves", C.c_float), ("free_space", C.c_uint32), ("ray_stride", C.c_uint32), ("max_steps", C.c_uint32),
                ("min_range", C.c_float), ("max_range", C.c_float)]

    _default, _checker = "loamx_densemap_tsdf_default_config", "loamx_densemap_tsdf_check"


class MeshConfig(C.Structure):
    """loamx_densemap_mesh_config: min_weight (a cell is valid when W >= min_weight) and axes (0: LOAM frame, 1: sensor axes)"""
    _fields_ = [("min_weight", C.c_uint32), ("axes", C.c_int32)]


TSDF_STATS = ("traced", "skipped_stride", "skipped_filter", "skipped_steps", "zero_length", "cells_visited", "cells_set", "max_weight")
MESH_STATS = ("valid", "inside", "tetrahedra", "holes", "vertices", "triangles")     # stats[6] of loamx_densemap_mesh


def tsdf_window(leaf, x, y, z, half_extent_xyz, **fields) -> TsdfConfig:
    """loamx_densemap_tsdf_window (host only): a TsdfConfig (defaults and fields otherwise) whose window covers (x, y, z) +-
    half_extent_xyz metres (LOAM frame; one number serves the three axes).  LoamxError E_INVALID when it breaks a bound of the check."""
    c = TsdfConfig(**fields)
    centre = (C.c_float * 3)(x, y, z)
    half = (C.c_float * 3)(*np.broadcast_to(np.asarray(half_extent_xyz, np.float32), (3,)).tolist())
    _check(lib().loamx_densemap_tsdf_window(C.c_float(leaf), centre, half, C.byref(c)))
    return c


def write_ply(path: str, verts, tris):
    """loamx_write_ply (host only): (V, 3) float32 vertices and (T, 3) uint32 indices as a binary little-endian PLY file"""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris, np.uint32).reshape(-1, 3)
    _check(lib().loamx_write_ply(os.fsencode(path), v.ctypes.data_as(C.c_void_p) if len(v) else None, C.c_uint64(len(v)),
                                 t.ctypes.data_as(C.c_void_p) if len(t) else None, C.c_uint64(len(t))))


SEGMENT_NONE = 0xffffffff                                                         # label of a voxel in no kept component
SEGMENT_ALL, SEGMENT_STATIC, SEGMENT_DYNAMIC = range(3)                           # loamx_densemap_segment_config.which


class SegmentConfig(_DefaultedConfig, C.Structure):
    """loamx_densemap_segment_config: which voxels are selected (which, min_points, the inclusive window lo .. hi in voxel indices),
    how they join (connectivity 6, 18 or 26) and which components are kept (min_voxels).  SegmentConfig() holds the defaults (ALL,
    26, 1, 1, the whole key range); keyword arguments replace them, lo and hi as triples."""
    _fields_ = [("which", C.c_uint32), ("connectivity", C.c_uint32), ("min_points", C.c_uint32), ("min_voxels", C.c_uint32),
                ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    _default, _checker = "loamx_densemap_segment_default_config", "loamx_densemap_segment_check"

    def update(self, **fields):
        return super().update(**{k: (C.c_int32 * 3)(*v) if k in ("lo", "hi") else v for k, v in fields.items()})


class Segment(C.Structure):
    """loamx_segment, 72 bytes: min_key (the smallest voxel key of the component, its identity), voxels, points (the sum of their n),
    the inclusive box lo .. hi in voxel indices and sum_idx, the sum of the indices per axis"""
    _fields_ = [("min_key", C.c_uint64), ("voxels", C.c_uint64), ("points", C.c_uint64), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3),
                ("sum_idx", C.c_int64 * 3)]


SEGMENT = np.dtype([("min_key", "<u8"), ("voxels", "<u8"), ("points", "<u8"), ("lo", "<i4", 3), ("hi", "<i4", 3), ("sum_idx", "<i8", 3)])
SEGMENT_STATS = ("selected", "components", "kept", "kept_voxels", "largest", "hooks_lost")   # stats[6] of loamx_densemap_segment


def segment_box(seg, leaf: float):
    """loamx_segment_box (host only): (lo_m, hi_m, centre), three float32 triples in metres, LOAM frame, of one SEGMENT record: the
    box of its voxels and the mean of their centres.  LoamxError E_INVALID for a record without voxels."""
    a = np.ascontiguousarray(seg, SEGMENT).reshape(1)
    out = np.zeros((3, 3), np.float32)
    _check(lib().loamx_segment_box(a.ctypes.data_as(C.c_void_p), C.c_float(leaf), out[0].ctypes.data_as(C.c_void_p),
                                   out[1].ctypes.data_as(C.c_void_p), out[2].ctypes.data_as(C.c_void_p)))
    return out[0], out[1], out[2]


CLOUD_ALL, CLOUD_NEW, CLOUD_KNOWN = range(3)                                      # loamx_densemap_segment_cloud_config.which


class SegmentCloudConfig(_DefaultedConfig, C.Structure):
    """loamx_densemap_segment_cloud_config: which admitted points of a cloud enter (which: CLOUD_ALL, CLOUD_NEW = no mapped voxel
    within margin cells, CLOUD_KNOWN = one; a map voxel is mapped with n >= map_min_points) and how the voxels they fill are grouped
    (connectivity, min_points, min_voxels, the window lo .. hi, as in SegmentConfig).  SegmentCloudConfig() holds the defaults (NEW,
    margin 1, 1, 26, 1, 1, the whole key range); keyword arguments replace them, lo and hi as triples."""
    _fields_ = [("which", C.c_uint32), ("margin", C.c_uint32), ("map_min_points", C.c_uint32), ("connectivity", C.c_uint32),
                ("min_points", C.c_uint32), ("min_voxels", C.c_uint32), ("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]

    _default, _checker = "loamx_densemap_segment_cloud_default_config", "loamx_densemap_segment_cloud_check"

    def update(self, **fields):
        return super().update(**{k: (C.c_int32 * 3)(*v) if k in ("lo", "hi") else v for k, v in fields.items()})


# stats[13] of loamx_densemap_segment_cloud
SEGMENT_CLOUD_STATS = ("offered", "dropped_range", "dropped_key", "rejected", "entered", "voxels", "selected", "components", "kept",
                       "kept_voxels", "largest", "labelled", "hooks_lost")


def segments_match(prev, cur, gap=0) -> np.ndarray:
    """loamx_segments_match (host only): for each SEGMENT record of cur the index of the record of prev whose box, grown by gap
    voxels on every side, shares the most cells with it (ties to the smaller min_key), SEGMENT_NONE when none overlaps; uint32"""
    a, b = np.ascontiguousarray(prev, SEGMENT).reshape(-1), np.ascontiguousarray(cur, SEGMENT).reshape(-1)
    out = np.full(max(len(b), 1), SEGMENT_NONE, np.uint32)
    _check(lib().loamx_segments_match(a.ctypes.data_as(C.c_void_p) if len(a) else None, C.c_uint64(len(a)),
                                      b.ctypes.data_as(C.c_void_p) if len(b) else None, C.c_uint64(len(b)), C.c_uint32(gap),
                                      out.ctypes.data_as(C.c_void_p)))
    return out[:len(b)]


def write_pcd(path: str, points, axes="loam"):
    """loamx_write_pcd: an (N, 4) / (N, 8) float32 cloud as a binary PCD v0.7 file (x y z intensity); axes="sensor" writes the sensor
    axes ingestion started from (x_s = z, y_s = x, z_s = y).  Host only."""
    a = as_points(points)
    c = cloud_of(a)
    _check(lib().loamx_write_pcd(os.fsencode(path), C.byref(c), _axes(axes)))


class DenseMapHistoryConfig(C.Structure):
    _fields_ = [("max_bytes", C.c_uint64), ("initial_points", C.c_uint64)]


def correct(correction, xyz) -> np.ndarray:
    """loamx_densemap_correct (host only): the rigid correction (row-major 3x4 or 4x4, float64) applied to (N, 3) points, or to the
    x, y, z of (N, 4) points (w untouched), in f32 exactly as rebuild() applies it on the device"""
    m = np.ascontiguousarray(np.asarray(correction, np.float64)[:3, :4])
    assert m.shape == (3, 4)
    a = np.array(xyz, np.float32, ndmin=2)
    assert a.ndim == 2 and a.shape[1] in (3, 4), "xyz must be (N, 3) or (N, 4)"
    src = np.ascontiguousarray(a[:, :3])
    dst = np.empty_like(src)
    _check(lib().loamx_densemap_correct(m.ctypes.data_as(C.c_void_p), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                        C.c_uint64(len(src))))
    out = a.copy()
    out[:, :3] = dst
    return out


class DenseMap:
    """loamx_densemap_*: a sparse voxel map of the whole run in device memory, fed with registered sweeps where they lie (add_from: a
    LaserMapping's last process; add_from_pipeline: a Pipeline's last step) or with map-frame points from the host (add)."""

    def __init__(self, leaf=0.1, min_range=0.0, max_range=0.0, max_voxels=0, initial_slots=1 << 20, device=0):
        L = lib()
        L.loamx_densemap_create.restype = C.c_void_p
        L.loamx_densemap_rehashes.restype = C.c_uint64
        L.loamx_densemap_route_active_rounds.restype = C.c_uint64
        L.loamx_densemap_route3_active_rounds.restype = C.c_uint64
        self.route_stats = None
        self.route3_stats = None
        self._dist_shape = None   # (nz, ny, nx) of the distance field that stands, for route3_last
        self.frontier_stats = None
        self._level = 0   # the level select_level chose (loamx_densemap_align_select_level)
        self._c = _cfg(DenseMapConfig, "loamx_densemap_default_config", leaf=leaf, min_range=min_range, max_range=max_range,
                       max_voxels=max_voxels, initial_slots=initial_slots, device=device)
        self.h = C.c_void_p(L.loamx_densemap_create(C.byref(self._c)))
        if not self.h:
            raise LoamxError(E_INVALID, L.loamx_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_densemap_destroy(self.h)
            self.h = None

    __del__ = close

    def add(self, points, origin=(0.0, 0.0, 0.0)):
        """map-frame points (N, 4) / (N, 8); origin = the sensor position the range filter measures from.  Returns the status (OK);
        LoamxError E_CAPACITY when max_voxels would be passed (the map is then unchanged)"""
        a = as_points(points)
        c = cloud_of(a)
        o = np.ascontiguousarray(origin, np.float32)
        assert o.shape == (3,)
        return _check(lib().loamx_densemap_add(self.h, C.byref(c), o.ctypes.data_as(C.c_void_p)))

    def add_from(self, mapping):
        """the registered full-resolution cloud of mapping's last process / process_linked (SKIPPED when it produced none)"""
        return _check(lib().loamx_densemap_add_from_map(self.h, mapping.h))

    def add_from_pipeline(self, pipeline, slot: int):
        """the registered cloud of the slot-th stream registered in pipeline's last step (SKIPPED when that step registered none)"""
        return _check(lib().loamx_densemap_add_from_pipeline(self.h, pipeline.h, slot))

    def stats(self):
        s = (C.c_uint64 * 6)()
        _check(lib().loamx_densemap_get_stats(self.h, s))
        keys = ("voxels", "slots", "offered", "added", "dropped_range", "dropped_key")
        return dict(zip(keys, (int(v) for v in s)))

    def __len__(self):
        return self.stats()["voxels"]

    def points(self, axes="loam", static=None):
        """(n, 4) float32: one record per voxel in ascending key order — the mean position, intensity = the voxel's point count.
        static (a StaticRule; needs carving): without the voxels the rule calls dynamic"""
        n = len(self)
        while True:
            out = np.zeros((max(n, 1), 4), np.float32)
            c = cloud_of(out)
            c.count = n
            if static is None:
                rc = lib().loamx_densemap_download(self.h, C.byref(c), _axes(axes))
            else:
                rc = lib().loamx_densemap_download_static(self.h, C.byref(c), _axes(axes), C.byref(static))
            if rc == E_CAPACITY:
                n = int(c.count)
                continue
            _check(rc)
            return out[:c.count]

    def save_pcd(self, path: str, axes="loam", static=None, surfels=False, min_points=None, min_planar_ratio=None):
        """the map as a binary PCD v0.7 file: x y z intensity, or with surfels=True (needs moments) the eight fields of surfels()"""
        if surfels:
            c = SurfelConfig(min_points, min_planar_ratio)
            _check(lib().loamx_densemap_save_pcd_surfels(self.h, os.fsencode(path), _axes(axes), C.byref(c),
                                                         C.byref(static) if static is not None else None))
        elif static is None:
            _check(lib().loamx_densemap_save_pcd(self.h, os.fsencode(path), _axes(axes)))
        else:
            _check(lib().loamx_densemap_save_pcd_static(self.h, os.fsencode(path), _axes(axes), C.byref(static)))

    def enable_carving(self, max_range=0.0, ray_stride=1, end_margin=1, max_steps=4096):
        """free-space carving (include/loamx.h): from now on every add also traces its rays from the origin and counts, per voxel, the
        rays that crossed it.  Only on an empty map (fresh, or right after reset); ray_stride is the cost knob."""
        c = _cfg(DenseMapCarveConfig, "loamx_densemap_carve_default_config", max_range=max_range, ray_stride=ray_stride,
                 end_margin=end_margin, max_steps=max_steps)
        _check(lib().loamx_densemap_enable_carving(self.h, C.byref(c)))

    def carve_stats(self):
        s = (C.c_uint64 * 6)()
        _check(lib().loamx_densemap_get_carve_stats(self.h, s))
        keys = ("traced", "skipped_stride", "skipped_range", "skipped_steps", "cells_visited", "misses")
        return dict(zip(keys, (int(v) for v in s)))

    def misses(self):
        """(n,) uint32: the miss count per voxel, in the order of points()"""
        n = C.c_uint64(len(self))
        while True:
            out = np.zeros(max(int(n.value), 1), np.uint32)
            rc = lib().loamx_densemap_download_misses(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(int(n.value)), C.byref(n))
            if rc == E_CAPACITY:
                continue
            _check(rc)
            return out[:int(n.value)]

    def prune(self, rule=None) -> int:
        """remove the voxels the rule (default: StaticRule()) calls dynamic from the table; returns how many left"""
        rule = StaticRule() if rule is None else rule
        removed = C.c_uint64(0)
        _check(lib().loamx_densemap_prune(self.h, C.byref(rule), C.byref(removed)))
        return int(removed.value)

    def enable_moments(self):
        """second moments (include/loamx.h): from now on every add also accumulates, per voxel, the sums of the products of the offsets
        and the vector from the sensor — nine 64-bit words, 72 bytes per slot.  Only on an empty map (fresh, or right after reset)."""
        _check(lib().loamx_densemap_enable_moments(self.h))

    def moments(self):
        """(n, 9) uint64: Mxx, Myy, Mzz, Mxy, Mxz, Myz, Vx, Vy, Vz per voxel (V as two's complement), in the order of points()"""
        n = C.c_uint64(len(self))
        while True:
            out = np.zeros((max(int(n.value), 1), 9), np.uint64)
            rc = lib().loamx_densemap_download_moments(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(int(n.value)), C.byref(n))
            if rc == E_CAPACITY:
                continue
            _check(rc)
            return out[:int(n.value)]

    def surfels(self, axes="loam", min_points=None, min_planar_ratio=None, static=None):
        """(n, 8) float32 in the order of SURFEL_FIELDS: the record of points() plus the unit normal facing the sensors and the
        curvature, zeros where the voxel has no surfel.  static (a StaticRule; needs carving): without the dynamic voxels"""
        c = SurfelConfig(min_points, min_planar_ratio)
        n = C.c_uint64(len(self))
        while True:
            out = np.zeros((max(int(n.value), 1), 8), np.float32)
            rc = lib().loamx_densemap_download_surfels(self.h, out.ctypes.data_as(C.c_void_p), C.c_uint64(int(n.value)), C.byref(n),
                                                       _axes(axes), C.byref(c), C.byref(static) if static is not None else None)
            if rc == E_CAPACITY:
                continue
            _check(rc)
            return out[:int(n.value)]

    def freeze(self, min_points=None, min_planar_ratio=None, static=None) -> int:
        """loamx_densemap_freeze: the surfels of surfels(min_points, min_planar_ratio, static) that have a normal, frozen into a
        table of their own on the device for align*; replaces an earlier snapshot.  Returns their number.  Needs moments."""
        c = SurfelConfig(min_points, min_planar_ratio)
        n = C.c_uint64(0)
        _check(lib().loamx_densemap_freeze(self.h, C.byref(c), C.byref(static) if static is not None else None, C.byref(n)))
        self._level = 0
        return int(n.value)

    @property
    def frozen_size(self) -> int:
        n = C.c_uint64(0)
        _check(lib().loamx_densemap_frozen_size(self.h, C.byref(n)))
        return int(n.value)

    def align_step(self, points, rtc, neighbourhood=1, max_residual=None):
        """loamx_densemap_align_step: one linearisation about rtc = (R row-major, t, c), 15 float32.  Returns (sums (28,) int64,
        counts (5,) uint64 in the order of ALIGN_COUNTS); max_residual None: the leaf"""
        a = as_points(points)
        c = cloud_of(a)
        r = np.ascontiguousarray(rtc, np.float32)
        assert r.shape == (15,)
        sums, counts = np.zeros(28, np.int64), np.zeros(5, np.uint64)
        mr = self.level_leaf() if max_residual is None else max_residual
        _check(lib().loamx_densemap_align_step(self.h, C.byref(c), r.ctypes.data_as(C.c_void_p), C.c_uint32(neighbourhood), C.c_float(mr),
                                               sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return sums, counts

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    @staticmethod
    def _host_cloud(points, centre):
        """what the host forms of align* pass before and behind the pose: (the cloud,) and (the centre or NULL,), and in front of
        both the arrays they point into, for the caller to hold during the call"""
        a = as_points(points)
        ctr = None if centre is None else np.ascontiguousarray(centre, np.float32)
        assert ctr is None or ctr.shape == (3,)
        return (a, ctr), (C.byref(cloud_of(a)),), (DenseMap._ptr(ctr),)

    def _align(self, fn, head, pose, mid, cfg):
        # the marshalling every form of align shares: head and mid are the arguments before and behind the pose
        p = None if pose is None else _pose12(pose)
        k, out = AlignConfig(**cfg), AlignResult()
        rc = _check(fn(self.h, *head, self._ptr(p), *mid, C.byref(k), C.byref(out)))
        return rc, out.as_dict()

    def align(self, points, pose=np.eye(3, 4), centre=None, **cfg) -> dict:
        """loamx_densemap_align: Gauss-Newton point-to-plane alignment of (N, 4) / (N, 8) points to the frozen snapshot from pose
        (3x4, map <- cloud), rotating about centre (default 0).  cfg: the fields of AlignConfig.  Blocks; returns AlignResult.as_dict()"""
        keep, head, mid = self._host_cloud(points, centre)
        return self._align(lib().loamx_densemap_align, head, pose, mid, cfg)[1]

    def align_from(self, mapping, pose=None, **cfg):
        """loamx_densemap_align_from_map: the registered cloud of mapping's last process, where it lies, about its origin; pose None:
        identity.  Returns (status code OK / SKIPPED, AlignResult.as_dict())"""
        return self._align(lib().loamx_densemap_align_from_map, (mapping.h,), pose, (), cfg)

    def align_from_pipeline(self, pipeline, slot: int, pose=None, **cfg):
        """loamx_densemap_align_from_pipeline: the same for the slot-th stream registered in pipeline's last step"""
        return self._align(lib().loamx_densemap_align_from_pipeline, (pipeline.h, C.c_uint32(slot)), pose, (), cfg)

    def align_step_many(self, points, rtc, neighbourhood=1, max_residual=None):
        """loamx_densemap_align_step_many: the linearisation of align_step about the K poses rtc (K, 15) float32 in one launch.
        Returns (sums (K, 28) int64, counts (K, 5) uint64): row k holds the words of align_step(points, rtc[k])"""
        a = as_points(points)
        c = cloud_of(a)
        r = np.ascontiguousarray(rtc, np.float32)
        assert r.ndim == 2 and r.shape[1] == 15
        k = len(r)
        sums, counts = np.zeros((max(k, 1), 28), np.int64), np.zeros((max(k, 1), 5), np.uint64)
        mr = self.level_leaf() if max_residual is None else max_residual
        _check(lib().loamx_densemap_align_step_many(self.h, C.byref(c), r.ctypes.data_as(C.c_void_p), C.c_uint32(k), C.c_uint32(neighbourhood),
                                                    C.c_float(mr), sums.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)))
        return sums[:k], counts[:k]

    @staticmethod
    def _poses(poses):
        p = np.ascontiguousarray(poses, np.float64)
        assert p.ndim >= 2 and p.size == len(p) * 12, "start poses are (K, 3, 4) or (K, 12)"
        return p.reshape(len(p), 12)

    def _align_many(self, fn, head, poses, mid, raw, cfg):
        # the marshalling every form of align_many shares: head and mid are the arguments before the poses and behind their count
        p = None if poses is None else self._poses(poses)
        n = 1 if p is None else len(p)
        k, out, best = AlignConfig(**cfg), (AlignResult * max(n, 1))(), C.c_uint32(0xFFFFFFFF)
        rc = _check(fn(self.h, *head, self._ptr(p), C.c_uint32(n), *mid, C.byref(k), out, C.byref(best)))
        return rc, (out if raw else [out[i].as_dict() for i in range(n)]), (None if best.value == 0xFFFFFFFF else int(best.value))

    def align_many(self, points, poses, centre=None, raw=False, **cfg):
        """loamx_densemap_align_many: align() from each of the K start poses (K, 3, 4), their Gauss-Newton loops in lockstep: one
        launch and one readback per iteration for all of them.  Returns (results, best): results[k] is what align(points, poses[k],
        centre, **cfg) returns (raw=True: the ctypes array of AlignResult instead of dicts), best the index align_best picks or None"""
        keep, head, mid = self._host_cloud(points, centre)
        return self._align_many(lib().loamx_densemap_align_many, head, poses, mid, raw, cfg)[1:]

    def align_many_from(self, mapping, poses=None, raw=False, **cfg):
        """loamx_densemap_align_many_from_map: the same for the registered cloud of mapping's last process, where it lies, about its
        origin; poses None: the identity alone.  Returns (status code OK / SKIPPED, results, best)"""
        return self._align_many(lib().loamx_densemap_align_many_from_map, (mapping.h,), poses, (), raw, cfg)

    def align_many_from_pipeline(self, pipeline, slot: int, poses=None, raw=False, **cfg):
        """loamx_densemap_align_many_from_pipeline: the same for the slot-th stream registered in pipeline's last step"""
        return self._align_many(lib().loamx_densemap_align_many_from_pipeline, (pipeline.h, C.c_uint32(slot)), poses, (), raw, cfg)

    def align_stats(self) -> dict:
        """loamx_densemap_get_align_stats: launches of either step kernel, readbacks of accumulator words and pose-steps (the sum of
        the poses linearised over the launches) since the handle was created"""
        s = (C.c_uint64 * 3)()
        _check(lib().loamx_densemap_get_align_stats(self.h, s))
        return dict(launches=int(s[0]), readbacks=int(s[1]), pose_steps=int(s[2]))

    def coarsen(self, level: int, static=None):
        """loamx_densemap_coarsen: the voxels of level `level` (1 .. PYRAMID_MAX_LEVELS - 1; leaf * 2^level) in ascending key order as
        (keys (n,) uint64, vals (n, 4) uint64, mom (n, 9) uint64), computed on the device from the map's table; static (a StaticRule;
        needs carving): without the voxels the rule calls dynamic.  Needs moments.  With surfel_of(leaf * 2^level, ...) a coarser
        surfel export"""
        n, cap = C.c_uint64(0), 0
        while True:
            keys, vals, mom = np.zeros(max(cap, 1), np.uint64), np.zeros((max(cap, 1), 4), np.uint64), np.zeros((max(cap, 1), 9), np.uint64)
            rc = lib().loamx_densemap_coarsen(self.h, C.c_uint32(level), C.byref(static) if static is not None else None,
                                              keys.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), mom.ctypes.data_as(C.c_void_p),
                                              C.c_uint64(cap), C.byref(n))
            if rc == E_CAPACITY:
                cap = int(n.value)
                continue
            _check(rc)
            return keys[:int(n.value)], vals[:int(n.value)], mom[:int(n.value)]

    def freeze_pyramid(self, levels=None, max_curvature=None, min_points=None, min_planar_ratio=None, static=None):
        """loamx_densemap_freeze_pyramid: freeze() as level 0 and, for l = 1 .. levels - 1, a snapshot of the voxels of level l (leaf *
        2^l) that have a surfel, without those whose curvature exceeds max_curvature (0: no limit).  levels None: 3.  Returns the
        entry counts per level.  The selected level returns to 0"""
        c = SurfelConfig(min_points, min_planar_ratio)
        pc = _cfg(PyramidConfig, "loamx_densemap_pyramid_default_config",
                  **{k: v for k, v in (("levels", levels), ("max_curvature", max_curvature)) if v is not None})
        n = (C.c_uint64 * PYRAMID_MAX_LEVELS)()
        _check(lib().loamx_densemap_freeze_pyramid(self.h, C.byref(c), C.byref(static) if static is not None else None, C.byref(pc), n))
        self._level = 0
        return [int(v) for v in n[:pc.levels]]

    @property
    def frozen_levels(self) -> int:
        """loamx_densemap_frozen_levels: 0 = nothing frozen, 1 after freeze(), the pyramid's levels after freeze_pyramid()"""
        n = C.c_uint32(0)
        _check(lib().loamx_densemap_frozen_levels(self.h, C.byref(n)))
        return int(n.value)

    def select_level(self, level: int):
        """loamx_densemap_align_select_level: align_step, align_step_many, align, align_many and their from forms read the snapshot of
        `level` from now on (max_residual None / 0: that level's leaf); every freeze and reset select level 0 again"""
        _check(lib().loamx_densemap_align_select_level(self.h, C.c_uint32(level)))
        self._level = int(level)

    def level_leaf(self, level=None) -> float:
        """the leaf of a level (default: the selected one) as the library computes it: one f32 multiply by a power of two"""
        return float(np.float32(self._c.leaf) * np.float32(1 << (self._level if level is None else level)))

    def _align_pyramid(self, fn, head, pose, mid, first_level, cfg):
        # the marshalling every form of align_pyramid shares: head and mid are the arguments before and behind the pose
        p = None if pose is None else _pose12(pose)
        first = max(self.frozen_levels - 1, 0) if first_level is None else int(first_level)
        k, out = AlignConfig(**cfg), (AlignResult * PYRAMID_MAX_LEVELS)()
        rc = _check(fn(self.h, *head, self._ptr(p), *mid, C.byref(k), C.c_uint32(first), out))
        return rc, [out[i].as_dict() for i in range(first + 1)]

    def align_pyramid(self, points, pose=np.eye(3, 4), centre=None, first_level=None, **cfg):
        """loamx_densemap_align_pyramid: align() against level first_level (default: the coarsest that stands), then against each
        finer level from the pose the level before reported.  Returns first_level + 1 result dicts, coarsest first; the last one is
        level 0's.  Each is what select_level(level) + align() returns from the same start; the selected level is left alone"""
        keep, head, mid = self._host_cloud(points, centre)
        return self._align_pyramid(lib().loamx_densemap_align_pyramid, head, pose, mid, first_level, cfg)[1]

    def align_pyramid_from(self, mapping, pose=None, first_level=None, **cfg):
        """loamx_densemap_align_pyramid_from_map: the same for the registered cloud of mapping's last process, where it lies, about its
        origin; pose None: identity.  Returns (status code OK / SKIPPED, results)"""
        return self._align_pyramid(lib().loamx_densemap_align_pyramid_from_map, (mapping.h,), pose, (), first_level, cfg)

    def align_pyramid_from_pipeline(self, pipeline, slot: int, pose=None, first_level=None, **cfg):
        """loamx_densemap_align_pyramid_from_pipeline: the same for the slot-th stream registered in pipeline's last step"""
        return self._align_pyramid(lib().loamx_densemap_align_pyramid_from_pipeline, (pipeline.h, C.c_uint32(slot)), pose, (), first_level,
                                   cfg)

    def _raycast(self, fn, head, n, max_steps, skip_steps, min_points, static, records):
        k = _cfg(RaycastConfig, "loamx_densemap_raycast_default_config", max_steps=max_steps, skip_steps=skip_steps, min_points=min_points)
        out = np.zeros(max(n, 1), RAY_DTYPE) if records else None
        counts = np.zeros(5, np.uint64)
        rc = _check(fn(self.h, *head, C.byref(k), C.byref(static) if static is not None else None,
                       out.ctypes.data_as(C.c_void_p) if records else None, C.c_uint64(n), counts.ctypes.data_as(C.c_void_p)))
        return rc, (out[:n] if records else None), dict(zip(RAY_COUNTS, (int(v) for v in counts)))

    def raycast(self, ends, origin=(0.0, 0.0, 0.0), max_steps=4096, skip_steps=0, min_points=1, static=None, records=True):
        """loamx_densemap_raycast: ray i from origin to ends[i] ((N, 4) / (N, 8), map frame) through the live map, to the first voxel
        with at least min_points points that static (a StaticRule; needs carving) does not call dynamic; the cells before skip_steps
        are not looked up.  Returns (records, counts): a structured array of RAY_DTYPE, one record per ray (None with
        records=False), and a dict in the order of RAY_COUNTS.  Blocks."""
        a = as_points(ends)
        c = cloud_of(a)
        o = np.ascontiguousarray(origin, np.float32)
        assert o.shape == (3,)
        _, out, counts = self._raycast(lib().loamx_densemap_raycast, (C.byref(c), o.ctypes.data_as(C.c_void_p)), len(a), max_steps,
                                       skip_steps, min_points, static, records)
        return out, counts

    def _raycast_device(self, fn, head, capacity, max_steps, skip_steps, min_points, static, records):
        # (the registered cloud's count is the device's to know: the room for the records doubles until they fit, each refusal
        # coming before anything is launched; the first four counts add up to the count)
        while True:
            try:
                rc, out, counts = self._raycast(fn, head, int(capacity), max_steps, skip_steps, min_points, static, records)
            except LoamxError as e:
                if e.code != E_CAPACITY:
                    raise
                capacity = 2 * int(capacity)
                continue
            n = sum(counts[k] for k in RAY_COUNTS[:4])
            return rc, (out[:n] if records else None), counts

    def raycast_from(self, mapping, max_steps=4096, skip_steps=0, min_points=1, static=None, records=True, capacity=1 << 17):
        """loamx_densemap_raycast_from_map: the rays of the registered cloud of mapping's last process, where it lies, from its
        origin; capacity = the room for the records to start with.  Returns (status code OK / SKIPPED, records, counts)"""
        return self._raycast_device(lib().loamx_densemap_raycast_from_map, (mapping.h,), capacity, max_steps, skip_steps, min_points,
                                    static, records)

    def raycast_from_pipeline(self, pipeline, slot: int, max_steps=4096, skip_steps=0, min_points=1, static=None, records=True,
                              capacity=1 << 17):
        """loamx_densemap_raycast_from_pipeline: the same for the slot-th stream registered in pipeline's last step"""
        return self._raycast_device(lib().loamx_densemap_raycast_from_pipeline, (pipeline.h, C.c_uint32(slot)), capacity, max_steps,
                                    skip_steps, min_points, static, records)

    def grid(self, cfg=None, static=None, **fields):
        """loamx_densemap_grid: the navigation grid of a window of the map, computed on the device — an (nz, nx) array of GRID_CELL
        records, [cz - z0, cx - x0].  cfg: a GridConfig (None: the defaults; grid_window() makes one around a position); fields
        replace members of a copy of it.  static (a StaticRule; needs carving): without the voxels the rule calls dynamic."""
        c = (GridConfig() if cfg is None else cfg).copy(**fields).check()
        out = np.zeros((c.nz, c.nx), GRID_CELL)
        _check(lib().loamx_densemap_grid(self.h, C.byref(c), C.byref(static) if static is not None else None,
                                         out.ctypes.data_as(C.c_void_p)))
        return out

    def dist(self, cfg=None, static=None, want_d2=True, want_near=False, **fields):
        """loamx_densemap_dist: the exact squared distance, in cells, from every cell of a 3-D window to the nearest occupied cell
        of the window, capped at d_max, computed on the device.  cfg: a DistConfig (None: the defaults; dist_window() makes one
        around a position); fields replace members of a copy of it.  static (a StaticRule; needs carving): without the voxels the
        rule calls dynamic.  Returns (d2, near): (nz, ny, nx) arrays, [cz - z0, cy - y0, cx - x0], uint16 and uint32 (DIST_NONE:
        capped), None for a plane not wanted.  With neither only the stats cross; the field stays on the device for dist_query()
        either way.  The four stats of the call are left in dist_stats."""
        c = (DistConfig() if cfg is None else cfg).copy(**fields).check()
        d2 = np.zeros((c.nz, c.ny, c.nx), np.uint16) if want_d2 else None
        near = np.zeros((c.nz, c.ny, c.nx), np.uint32) if want_near else None
        st = (C.c_uint64 * 4)()
        _check(lib().loamx_densemap_dist(self.h, C.byref(c), C.byref(static) if static is not None else None,
                                         d2.ctypes.data_as(C.c_void_p) if want_d2 else None,
                                         near.ctypes.data_as(C.c_void_p) if want_near else None, st))
        self.dist_stats = dict(zip(DIST_STATS, (int(v) for v in st)))
        self._dist_shape = (c.nz, c.ny, c.nx)
        return d2, near

    def dist_query(self, points, min_d2=0, records=True):
        """loamx_densemap_dist_query: the d2 and near of the cell of every point ((N, 4) / (N, 8), map frame) in the field of the
        last dist() call, looked up on the device.  Returns (samples, stats): DIST_SAMPLE records, d2 = DIST_OUTSIDE for a point
        without a cell in the window (None with records=False), and a dict in the order of DIST_QUERY_STATS: points inside,
        outside, inside and capped, inside with d2 < min_d2, and best = (the smallest d2) << 32 | the smallest index with it,
        2^64 - 1 when no point is inside.  Blocks."""
        a = as_points(points)
        c = cloud_of(a)
        out = np.zeros(max(len(a), 1), DIST_SAMPLE) if records else None
        st = (C.c_uint64 * 5)()
        _check(lib().loamx_densemap_dist_query(self.h, C.byref(c), C.c_uint32(min_d2), out.ctypes.data_as(C.c_void_p) if records else None,
                                               C.c_uint64(len(a)), st))
        return (out[:len(a)] if records else None), dict(zip(DIST_QUERY_STATS, (int(v) for v in st)))

    def tsdf_begin(self, cfg=None, **fields):
        """loamx_densemap_tsdf_begin: a zeroed signed distance field over the window of cfg (a TsdfConfig, None: the defaults;
        tsdf_window() makes one around a position; fields replace members of a copy of it), kept in the handle.  Returns the
        configuration used"""
        c = (TsdfConfig() if cfg is None else cfg).copy(**fields).check()
        _check(lib().loamx_densemap_tsdf_begin(self.h, C.byref(c)))
        return c

    def tsdf_add(self, points, origin=(0.0, 0.0, 0.0)):
        """loamx_densemap_tsdf_add: the rays from origin to map-frame points (N, 4) / (N, 8) into the field; does not wait"""
        a = as_points(points)
        c = cloud_of(a)
        o = np.ascontiguousarray(origin, np.float32)
        assert o.shape == (3,)
        return _check(lib().loamx_densemap_tsdf_add(self.h, C.byref(c), o.ctypes.data_as(C.c_void_p)))

    def tsdf_add_from(self, mapping):
        """loamx_densemap_tsdf_add_from_map: the registered cloud of mapping's last process (SKIPPED when it produced none)"""
        return _check(lib().loamx_densemap_tsdf_add_from_map(self.h, mapping.h))

    def tsdf_add_from_pipeline(self, pipeline, slot: int):
        """loamx_densemap_tsdf_add_from_pipeline: the registered cloud of the slot-th stream of pipeline's last step"""
        return _check(lib().loamx_densemap_tsdf_add_from_pipeline(self.h, pipeline.h, slot))

    def tsdf_add_history(self, first: int, n: int, corrections=None):
        """loamx_densemap_tsdf_add_from_history: the logged calls first .. first + n - 1 where they lie in the log, in one launch,
        call k of the window moved by corrections[k] (row-major 3x4 or 4x4, map <- map, float64; None: where they were)"""
        p = None
        if corrections is not None:
            a = np.asarray(corrections, np.float64)
            a = np.ascontiguousarray(a.reshape(-1, *a.shape[-2:])[:, :3, :4] if a.size else a.reshape(0, 3, 4))
            assert a.ndim == 3 and a.shape[1:] == (3, 4) and a.shape[0] == n, "corrections must be (n, 3, 4) or (n, 4, 4)"
            p = a.ctypes.data_as(C.c_void_p)
        return _check(lib().loamx_densemap_tsdf_add_from_history(self.h, C.c_uint64(first), C.c_uint64(n), p))

    def tsdf(self, cfg: TsdfConfig, want_w=True, want_d=True):
        """loamx_densemap_tsdf_download: waits; (W, D, stats) with W uint32 and D int64 as (nz, ny, nx) arrays of the window of cfg
        (what tsdf_begin returned; None for a plane not wanted) and a dict in the order of TSDF_STATS"""
        w = np.zeros((cfg.nz, cfg.ny, cfg.nx), np.uint32) if want_w else None
        d = np.zeros((cfg.nz, cfg.ny, cfg.nx), np.int64) if want_d else None
        st = (C.c_uint64 * 8)()
        _check(lib().loamx_densemap_tsdf_download(self.h, w.ctypes.data_as(C.c_void_p) if want_w else None,
                                                  d.ctypes.data_as(C.c_void_p) if want_d else None, st))
        return w, d, dict(zip(TSDF_STATS, (int(v) for v in st)))

    def mesh(self, min_weight=None, axes="loam", count_only=False):
        """loamx_densemap_mesh: the zero crossing of the field as an indexed triangle mesh, extracted on the device: (verts (V, 3)
        float32, tris (T, 3) uint32, stats in the order of MESH_STATS); count_only: (V, T, stats), nothing else crosses"""
        c = _cfg(MeshConfig, "loamx_densemap_mesh_default_config", axes=_axes(axes), **({} if min_weight is None else dict(min_weight=min_weight)))
        nv, nt, st = C.c_uint64(0), C.c_uint64(0), (C.c_uint64 * 6)()
        _check(lib().loamx_densemap_mesh(self.h, C.byref(c), None, C.c_uint64(0), None, C.c_uint64(0), C.byref(nv), C.byref(nt), st))
        if count_only:
            return int(nv.value), int(nt.value), dict(zip(MESH_STATS, (int(v) for v in st)))
        v, t = np.zeros((max(nv.value, 1), 3), np.float32), np.zeros((max(nt.value, 1), 3), np.uint32)
        _check(lib().loamx_densemap_mesh(self.h, C.byref(c), v.ctypes.data_as(C.c_void_p), C.c_uint64(nv.value), t.ctypes.data_as(C.c_void_p),
                                         C.c_uint64(nt.value), C.byref(nv), C.byref(nt), st))
        return v[:nv.value], t[:nt.value], dict(zip(MESH_STATS, (int(v) for v in st)))

    def save_ply(self, path: str, min_weight=None, axes="loam") -> dict:
        """loamx_densemap_save_ply: mesh(), written as a binary little-endian PLY file; returns the stats"""
        c = _cfg(MeshConfig, "loamx_densemap_mesh_default_config", axes=_axes(axes), **({} if min_weight is None else dict(min_weight=min_weight)))
        st = (C.c_uint64 * 6)()
        _check(lib().loamx_densemap_save_ply(self.h, C.byref(c), os.fsencode(path), st))
        return dict(zip(MESH_STATS, (int(v) for v in st)))

    ROUTE_STATS = ("traversable", "reachable", "goals_used", "max_cost", "rounds", "tile_runs")

    def _route(self, dim, fn, head, mid, shape, goals, cfg, want_field, fields):
        """the 2-D (dim 2) and 3-D (dim 3) route calls: fn(h, *head, cfg, goals, n_goals, *mid, field, stats); the stats are left in
        route_stats or route3_stats"""
        Config, names, attr = (RouteConfig, self.ROUTE_STATS, "route_stats") if dim == 2 else (Route3Config, ROUTE3_STATS, "route3_stats")
        c = (Config() if cfg is None else cfg).copy(**fields).check()
        t = _tuples(goals, dim)
        field = np.zeros(shape, ROUTE_CELL) if want_field else None
        st = (C.c_uint64 * 6)()
        _check(fn(self.h, *head, C.byref(c), t.ctypes.data_as(C.c_void_p), C.c_uint32(len(t)), *mid,
                  field.ctypes.data_as(C.c_void_p) if want_field else None, st))
        setattr(self, attr, dict(zip(names, (int(v) for v in st))))
        return field

    def _route_trace(self, dim, fn, starts, capacity):
        """route_trace (dim 2) and route3_trace (dim 3): fn(h, starts, n_starts, out, capacity, lengths) traces on the device"""
        t = _tuples(starts, dim)
        out = np.zeros((len(t), capacity, dim), np.uint32)
        lengths = np.zeros(len(t), np.uint32)
        _check(fn(self.h, t.ctypes.data_as(C.c_void_p), C.c_uint32(len(t)), out.ctypes.data_as(C.c_void_p), C.c_uint32(capacity),
                  lengths.ctypes.data_as(C.c_void_p)))
        return [out[i, :min(int(n), capacity)] for i, n in enumerate(lengths)], lengths

    def route(self, goals, cfg=None, grid=None, static=None, want_cells=False, want_field=True, **fields):
        """loamx_densemap_route: the navigation grid of a window (grid: a GridConfig, None: the defaults; static: a StaticRule)
        and, on it where it lies on the device, the cost-to-go field towards goals, a list of window-relative (rx, rz) pairs, under
        cfg (a RouteConfig, None: the defaults; fields replace members of a copy of it).  Returns the (nz, nx) array of ROUTE_CELL
        records, or (field, cells) with want_cells; want_field=False leaves the field on the device for route_trace() and returns
        None in its place.  The six stats of the call are left in route_stats."""
        g = (GridConfig() if grid is None else grid).copy().check()
        cells = np.zeros((g.nz, g.nx), GRID_CELL) if want_cells else None
        head = (C.byref(g), C.byref(static) if static is not None else None)
        field = self._route(2, lib().loamx_densemap_route, head, (cells.ctypes.data_as(C.c_void_p) if want_cells else None,), (g.nz, g.nx),
                            goals, cfg, want_field, fields)
        return (field, cells) if want_cells else field

    def route_cells(self, cells, goals, cfg=None, want_field=True, **fields):
        """loamx_densemap_route_cells: the same on an (nz, nx) array of GRID_CELL records of the caller's (edited, painted with
        keep-out zones, or hand-made), uploaded to a buffer of the route's own"""
        a = _grid_cells(cells)
        assert a.ndim == 2, "cells must be an (nz, nx) array"
        head = (a.ctypes.data_as(C.c_void_p), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0]))
        return self._route(2, lib().loamx_densemap_route_cells, head, (), a.shape, goals, cfg, want_field, fields)

    def route_trace(self, starts, capacity):
        """loamx_densemap_route_trace: the routes from starts, a list of 1..4096 (rx, rz) pairs, over the field of the last route /
        route_cells call, traced on the device -> (a list of (min(n_i, capacity), 2) uint32 arrays of (rx, rz) pairs up to and
        including the goal cell, the full lengths n_i as uint32; 0: the start is outside the window or unreachable)"""
        return self._route_trace(2, lib().loamx_densemap_route_trace, starts, capacity)

    @property
    def route_active_rounds(self) -> int:
        """test hook: the relaxation rounds of the last route call in which a tile ran"""
        return int(lib().loamx_densemap_route_active_rounds(self.h))

    def route_set_batch(self, batch: int):
        """bench hook: the relaxation rounds launched per look at the counters (1..64)"""
        _check(lib().loamx_densemap_route_set_batch(self.h, C.c_uint32(batch)))

    def route3(self, goals, cfg=None, dist=None, static=None, want_field=True, **fields):
        """loamx_densemap_route3: the distance field of a 3-D window (dist: a DistConfig, None: the defaults; static: a StaticRule),
        which replaces the standing one and stays for dist_query(), and on its d2 where it lies on the device the cost-to-go field
        towards goals, a list of window-relative (rx, ry, rz) triples, under cfg (a Route3Config, None: the defaults; fields
        replace members of a copy of it).  Returns the (nz, ny, nx) array of ROUTE_CELL records; want_field=False leaves the field
        on the device for route3_trace() and returns None.  The six stats of the call are left in route3_stats."""
        g = (DistConfig() if dist is None else dist).copy().check()
        head = (C.byref(g), C.byref(static) if static is not None else None)
        out = self._route(3, lib().loamx_densemap_route3, head, (), (g.nz, g.ny, g.nx), goals, cfg, want_field, fields)
        self._dist_shape = (g.nz, g.ny, g.nx)
        return out

    def route3_last(self, goals, cfg=None, want_field=True, **fields):
        """loamx_densemap_route3_last: the same on the distance field that stands (dist() or route3()); LoamxError E_INVALID when
        there is none"""
        return self._route(3, lib().loamx_densemap_route3_last, (), (), self._dist_shape or (1, 1, 1), goals, cfg, want_field, fields)

    def route3_cells(self, d2, goals, cfg=None, want_field=True, **fields):
        """loamx_densemap_route3_cells: the same on an (nz, ny, nx) uint16 array of d2 values of the caller's (an earlier field
        painted with no-fly zones, or a hand-made one), uploaded to a buffer of the route's own; the standing distance field is
        left alone"""
        a = np.ascontiguousarray(d2, np.uint16)
        assert a.ndim == 3, "d2 must be an (nz, ny, nx) array"
        head = (a.ctypes.data_as(C.c_void_p), C.c_uint32(a.shape[2]), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0]))
        return self._route(3, lib().loamx_densemap_route3_cells, head, (), a.shape, goals, cfg, want_field, fields)

    def route3_trace(self, starts, capacity):
        """loamx_densemap_route3_trace: the routes from starts, a list of 1..4096 (rx, ry, rz) triples, over the field of the last
        route3 / route3_last / route3_cells call, traced on the device -> (a list of (min(n_i, capacity), 3) uint32 arrays of
        triples up to and including the goal cell, the full lengths n_i as uint32; 0: the start is outside the window or
        unreachable)"""
        return self._route_trace(3, lib().loamx_densemap_route3_trace, starts, capacity)

    @property
    def route3_active_rounds(self) -> int:
        """test hook: the relaxation rounds of the last route3 call in which a brick ran"""
        return int(lib().loamx_densemap_route3_active_rounds(self.h))

    def route3_set_batch(self, batch: int):
        """bench hook: the relaxation rounds launched per look at the counters (1..64)"""
        _check(lib().loamx_densemap_route3_set_batch(self.h, C.c_uint32(batch)))

    def _frontiers(self, fn, head, shape, cfg, route, start, labels, fields):
        # (as segment(): a refusal by capacity leaves the needed count, and the call is made again with that room)
        c = (FrontierConfig() if cfg is None else cfg).copy(**fields).check()
        rc = (RouteConfig() if route is None else route).copy().check()
        xz = None if start is None else _xz_pairs([start])
        n_fr = C.c_uint64(256)
        st = (C.c_uint64 * 6)()
        while True:
            lab = np.full(shape, FRONTIER_NONE, np.uint32) if labels else None
            out = np.zeros(max(int(n_fr.value), 1), FRONTIER)
            code = fn(self.h, *head, C.byref(rc), C.byref(c), xz.ctypes.data_as(C.c_void_p) if xz is not None else None,
                      lab.ctypes.data_as(C.c_void_p) if labels else None, out.ctypes.data_as(C.c_void_p), C.c_uint64(int(n_fr.value)),
                      C.byref(n_fr), st)
            if code == E_CAPACITY:
                continue
            _check(code)
            self.frontier_stats = dict(zip(FRONTIER_STATS, (int(v) for v in st)))
            return lab, out[:int(n_fr.value)]

    def frontiers(self, cfg=None, grid=None, static=None, route=None, start=None, labels=True, **fields):
        """loamx_densemap_frontiers: the navigation grid of a window (grid: a GridConfig, None: the defaults; static: a StaticRule)
        and, on it where it lies on the device, its frontiers: the FREE cells that touch UNKNOWN ones, grouped under cfg (a
        FrontierConfig, None: the defaults; fields replace members of a copy of it).  start = (rx, rz), the vehicle's cell: the call
        routes towards it under route (a RouteConfig, None: the defaults), every frontier gets reachable, best_cost and best_cell,
        and the field stays on the device, so that route_trace([best_cell's (rx, rz)], ...) walks from the frontier to the vehicle.
        start None: nothing is routed and the handle's field is left alone.  Returns (labels, frontiers): an (nz, nx) uint32 array,
        the number of each cell's frontier or FRONTIER_NONE (None with labels=False), and the kept frontiers as FRONTIER records in
        ascending min_cell.  The six stats of the call are left in frontier_stats.  Blocks; the map is only read."""
        g = (GridConfig() if grid is None else grid).copy().check()
        head = (C.byref(g), C.byref(static) if static is not None else None)
        return self._frontiers(lib().loamx_densemap_frontiers, head, (g.nz, g.nx), cfg, route, start, labels, fields)

    def frontiers_cells(self, cells, cfg=None, route=None, start=None, labels=True, **fields):
        """loamx_densemap_frontiers_cells: the same on an (nz, nx) array of GRID_CELL records of the caller's, uploaded as
        route_cells() uploads"""
        a = _grid_cells(cells)
        assert a.ndim == 2, "cells must be an (nz, nx) array"
        head = (a.ctypes.data_as(C.c_void_p), C.c_uint32(a.shape[1]), C.c_uint32(a.shape[0]))
        return self._frontiers(lib().loamx_densemap_frontiers_cells, head, a.shape, cfg, route, start, labels, fields)

    def segment(self, cfg=None, static=None, labels=True, **fields):
        """loamx_densemap_segment: the connected components of the selected voxels, labelled on the device.  cfg: a SegmentConfig
        (None: the defaults: every voxel, connectivity 26); fields replace members of a copy of it.  static: the StaticRule that
        which=SEGMENT_STATIC / SEGMENT_DYNAMIC select by (None: the default rule; needs carving).  Returns (labels, segments,
        stats): labels one uint32 per voxel in the order of points(), the number of its component or SEGMENT_NONE (None with
        labels=False); segments the kept components as SEGMENT records in ascending min_key; stats a dict in the order of
        SEGMENT_STATS.  Blocks; the map is only read."""
        c = (SegmentConfig() if cfg is None else cfg).copy(**fields).check()
        n_vox, n_seg = C.c_uint64(len(self) if labels else 0), C.c_uint64(4096)
        st = (C.c_uint64 * 6)()
        while True:
            lab = np.full(max(int(n_vox.value), 1), SEGMENT_NONE, np.uint32) if labels else None
            segs = np.zeros(max(int(n_seg.value), 1), SEGMENT)
            rc = lib().loamx_densemap_segment(self.h, C.byref(c), C.byref(static) if static is not None else None,
                                              lab.ctypes.data_as(C.c_void_p) if labels else None, C.c_uint64(int(n_vox.value)), C.byref(n_vox),
                                              segs.ctypes.data_as(C.c_void_p), C.c_uint64(int(n_seg.value)), C.byref(n_seg), st)
            if rc == E_CAPACITY:   # (the counts now hold what is needed)
                continue
            _check(rc)
            return (lab[:int(n_vox.value)] if labels else None), segs[:int(n_seg.value)], dict(zip(SEGMENT_STATS, (int(v) for v in st)))

    def _segment_cloud(self, fn, head, n_pts, cfg, static, labels, fields):
        # (as segment(): a refusal by capacity leaves the needed counts, and the call is made again with that room)
        c = (SegmentCloudConfig() if cfg is None else cfg).copy(**fields).check()
        n_pts, n_seg = C.c_uint64(n_pts if labels else 0), C.c_uint64(max(4096, getattr(self, "_cloud_segs", 0)))   # (room as the last call needed)
        st = (C.c_uint64 * 13)()
        while True:
            lab = np.full(max(int(n_pts.value), 1), SEGMENT_NONE, np.uint32) if labels else None
            segs = np.zeros(max(int(n_seg.value), 1), SEGMENT)
            rc = fn(self.h, *head, C.byref(c), C.byref(static) if static is not None else None,
                    lab.ctypes.data_as(C.c_void_p) if labels else None, C.c_uint64(int(n_pts.value)), C.byref(n_pts),
                    segs.ctypes.data_as(C.c_void_p), C.c_uint64(int(n_seg.value)), C.byref(n_seg), st)
            if rc == E_CAPACITY:
                continue
            _check(rc)
            self._cloud_segs = int(n_seg.value) if rc == OK else 0
            if rc == SKIPPED:
                return rc, (np.zeros(0, np.uint32) if labels else None), segs[:0], dict.fromkeys(SEGMENT_CLOUD_STATS, 0)
            return (rc, (lab[:int(n_pts.value)] if labels else None), segs[:int(n_seg.value)],
                    dict(zip(SEGMENT_CLOUD_STATS, (int(v) for v in st))))

    def segment_cloud(self, points, origin=(0.0, 0.0, 0.0), cfg=None, static=None, labels=True, **fields):
        """loamx_densemap_segment_cloud: the objects of a cloud that is not in the map ((N, 4) / (N, 8), map frame, about origin as
        add() takes them).  The points that add() would admit are tested against the live map (cfg.which: CLOUD_NEW keeps those with
        no mapped voxel within cfg.margin cells, CLOUD_KNOWN those with one, CLOUD_ALL all of them; static, a StaticRule that needs
        carving: the voxels it calls dynamic are not mapped), the kept ones are clustered as segment() clusters a map's voxels.  cfg:
        a SegmentCloudConfig (None: the defaults); fields replace members of a copy of it.  Returns (labels, segments, stats): one
        uint32 per point, the number of its object or SEGMENT_NONE (None with labels=False); SEGMENT records in ascending min_key;
        a dict in the order of SEGMENT_CLOUD_STATS.  Blocks; the map is only read."""
        a = as_points(points)
        c = cloud_of(a)
        o = np.ascontiguousarray(origin, np.float32)
        assert o.shape == (3,)
        return self._segment_cloud(lib().loamx_densemap_segment_cloud, (C.byref(c), o.ctypes.data_as(C.c_void_p)), len(a), cfg, static,
                                   labels, fields)[1:]

    def segment_cloud_from(self, mapping, cfg=None, static=None, labels=True, capacity=1 << 17, **fields):
        """loamx_densemap_segment_cloud_from_map: the same for the registered cloud of mapping's last process, where it lies, about
        its origin; capacity = the room for the labels to start with.  Returns (status code OK / SKIPPED, labels, segments, stats)"""
        return self._segment_cloud(lib().loamx_densemap_segment_cloud_from_map, (mapping.h,), int(capacity), cfg, static, labels, fields)

    def segment_cloud_from_pipeline(self, pipeline, slot: int, cfg=None, static=None, labels=True, capacity=1 << 17, **fields):
        """loamx_densemap_segment_cloud_from_pipeline: the same for the slot-th stream registered in pipeline's last step"""
        return self._segment_cloud(lib().loamx_densemap_segment_cloud_from_pipeline, (pipeline.h, C.c_uint32(slot)), int(capacity), cfg,
                                   static, labels, fields)

    def save(self, path: str):
        """loamx_densemap_save: every word of the map as an 'LXDM' file (include/loamx.h), written beside path and renamed.  The
        bytes depend on neither the order of the points nor the table behind the map"""
        _check(lib().loamx_densemap_save(self.h, os.fsencode(path)))

    def load(self, path: str):
        """loamx_densemap_load: the file's map into this empty handle (same leaf); enables the carving / moments the file has.
        Afterwards every export, freeze and align give what the saving handle gave"""
        _check(lib().loamx_densemap_load(self.h, os.fsencode(path)))

    def merge(self, other: "DenseMap"):
        """loamx_densemap_merge: other's voxels added into this map on the device, word for word (same leaf, device and features).
        n, S and the moments become those of one map fed with both maps' sweeps; the miss counts are summed, not re-carved"""
        _check(lib().loamx_densemap_merge(self.h, other.h))

    def merge_file(self, path: str):
        """loamx_densemap_merge_file: the same with a saved map as the source"""
        _check(lib().loamx_densemap_merge_file(self.h, os.fsencode(path)))

    def count_region(self, region: DenseMapRegion):
        """loamx_densemap_count_region: (voxels, points) the region selects, counted on the device"""
        c = (C.c_uint64 * 2)()
        _check(lib().loamx_densemap_count_region(self.h, C.byref(region), c))
        return int(c[0]), int(c[1])

    def region_points(self, region: DenseMapRegion, axes="loam"):
        """loamx_densemap_download_region: the records of points() for the voxels the region selects only, in ascending key order;
        only those cross to the host"""
        n = 0
        while True:
            out = np.zeros((max(n, 1), 4), np.float32)
            c = cloud_of(out)
            c.count = n
            rc = lib().loamx_densemap_download_region(self.h, C.byref(region), C.byref(c), _axes(axes))
            if rc == E_CAPACITY:
                n = int(c.count)
                continue
            _check(rc)
            return out[:c.count]

    def save_region(self, region: DenseMapRegion, path: str):
        """loamx_densemap_save_region: the voxels the region selects as an 'LXDM' file that load and merge_file accept"""
        _check(lib().loamx_densemap_save_region(self.h, C.byref(region), os.fsencode(path)))

    def evict(self, region: DenseMapRegion, path=None):
        """loamx_densemap_evict: the voxels the region selects leave the map — into the file `path` (merge_file brings them back bit
        for bit), or discarded with path None — and the table shrinks to what stays.  Returns (voxels, points) removed"""
        r = (C.c_uint64 * 2)()
        _check(lib().loamx_densemap_evict(self.h, C.byref(region), os.fsencode(path) if path is not None else None, r))
        return int(r[0]), int(r[1])

    def page(self, cfg: DenseMapPageConfig, centre) -> dict:
        """loamx_densemap_page: the tiles of cfg.dir around `centre` merged in, everything outside the keep box moved out to tile files"""
        s, c = (C.c_uint64 * 6)(), _f3(centre)
        _check(lib().loamx_densemap_page(self.h, C.byref(cfg), c.ctypes.data_as(C.c_void_p), s))
        keys = ("tiles_in", "voxels_in", "files_written", "voxels_out", "files_merged", "resident")
        return dict(zip(keys, (int(v) for v in s)))

    def enable_history(self, max_bytes=0, initial_points=1 << 20):
        """the sweep log (include/loamx.h): from now on every add also appends its whole cloud, as offered, to a block in device
        memory that rebuild() replays.  Only on an empty map (fresh, or right after reset); max_bytes caps the block (an add past it
        raises E_CAPACITY), initial_points is its first capacity"""
        c = _cfg(DenseMapHistoryConfig, "loamx_densemap_history_default_config", max_bytes=max_bytes, initial_points=initial_points)
        _check(lib().loamx_densemap_enable_history(self.h, C.byref(c)))

    def history_size(self):
        """(logged calls, logged points)"""
        calls, points = C.c_uint64(0), C.c_uint64(0)
        _check(lib().loamx_densemap_history_size(self.h, C.byref(calls), C.byref(points)))
        return int(calls.value), int(points.value)

    def history(self, k: int):
        """logged call k: ((n, 4) float32, the bytes that were added; (3,) float32, the origin it was added with)"""
        n = 0
        origin = np.zeros(3, np.float32)
        while True:
            out = np.zeros((max(n, 1), 4), np.float32)
            c = cloud_of(out)
            c.count = n
            rc = lib().loamx_densemap_history_download(self.h, C.c_uint64(k), C.byref(c), origin.ctypes.data_as(C.c_void_p))
            if rc == E_CAPACITY:
                n = int(c.count)
                continue
            _check(rc)
            return out[:c.count], origin

    def rebuild(self, corrections=None):
        """loamx_densemap_rebuild: the map becomes what a fresh handle fed with the logged sweeps would hold, sweep k moved by
        corrections[k] (row-major 3x4 or 4x4, map <- map, float64; None: every sweep where it was) — on the device, from the log.
        Blocks until the new map stands; freeze() again afterwards"""
        if corrections is None:
            calls, _ = self.history_size()
            return _check(lib().loamx_densemap_rebuild(self.h, None, C.c_uint64(calls)))
        a = np.asarray(corrections, np.float64)
        a = np.ascontiguousarray(a.reshape(-1, *a.shape[-2:])[:, :3, :4] if a.size else a.reshape(0, 3, 4))
        assert a.ndim == 3 and a.shape[1:] == (3, 4), "corrections must be (n_calls, 3, 4) or (n_calls, 4, 4)"
        return _check(lib().loamx_densemap_rebuild(self.h, a.ctypes.data_as(C.c_void_p), C.c_uint64(a.shape[0])))

    def freeze_device(self, min_points=None, min_planar_ratio=None, static=None) -> int:
        """loamx_densemap_freeze_device: freeze() with the surfels computed on the device, from the table where it lies — the same
        set of entries byte for byte, no voxel crosses to the host.  Returns their number.  Needs moments."""
        c = SurfelConfig(min_points, min_planar_ratio)
        n = C.c_uint64(0)
        _check(lib().loamx_densemap_freeze_device(self.h, C.byref(c), C.byref(static) if static is not None else None, C.byref(n)))
        self._level = 0
        return int(n.value)

    def freeze_pyramid_device(self, levels=None, max_curvature=None, min_points=None, min_planar_ratio=None, static=None):
        """loamx_densemap_freeze_pyramid_device: freeze_pyramid() with every level's surfels computed on the device; the same
        entries per level.  Returns the entry counts per level.  The selected level returns to 0"""
        c = SurfelConfig(min_points, min_planar_ratio)
        pc = _cfg(PyramidConfig, "loamx_densemap_pyramid_default_config",
                  **{k: v for k, v in (("levels", levels), ("max_curvature", max_curvature)) if v is not None})
        n = (C.c_uint64 * PYRAMID_MAX_LEVELS)()
        _check(lib().loamx_densemap_freeze_pyramid_device(self.h, C.byref(c), C.byref(static) if static is not None else None, C.byref(pc), n))
        self._level = 0
        return [int(v) for v in n[:pc.levels]]

    def freeze_history(self, first: int, n: int, corrections=None, min_points=None, min_planar_ratio=None) -> int:
        """loamx_densemap_freeze_history: level 0 becomes the snapshot of the logged calls first .. first + n - 1 alone, call k of the
        window moved by corrections[k] (row-major 3x4 or 4x4, map <- map, float64; None: every sweep where it was): what a fresh map
        fed with those sweeps would freeze.  On the device, from the log; the live map is only read.  Returns the entries"""
        c = SurfelConfig(min_points, min_planar_ratio)
        out = C.c_uint64(0)
        p = None
        if corrections is not None:
            a = np.asarray(corrections, np.float64)
            a = np.ascontiguousarray(a.reshape(-1, *a.shape[-2:])[:, :3, :4] if a.size else a.reshape(0, 3, 4))
            assert a.ndim == 3 and a.shape[1:] == (3, 4) and a.shape[0] == n, "corrections must be (n, 3, 4) or (n, 4, 4)"
            p = a.ctypes.data_as(C.c_void_p)
        _check(lib().loamx_densemap_freeze_history(self.h, C.c_uint64(first), C.c_uint64(n), p, C.byref(c), C.byref(out)))
        self._level = 0
        return int(out.value)

    def download_frozen(self, level=0):
        """loamx_densemap_download_frozen: the entries of snapshot level `level` in ascending key order as (keys (n,) uint64,
        rec (n, 6) float32: mean x, y, z, normal x, y, z)"""
        n, cap = C.c_uint64(0), 0
        while True:
            keys, rec = np.zeros(max(cap, 1), np.uint64), np.zeros((max(cap, 1), 6), np.float32)
            rc = lib().loamx_densemap_download_frozen(self.h, C.c_uint32(level), keys.ctypes.data_as(C.c_void_p),
                                                      rec.ctypes.data_as(C.c_void_p), C.c_uint64(cap), C.byref(n))
            if rc == E_CAPACITY:
                cap = int(n.value)
                continue
            _check(rc)
            return keys[:int(n.value)], rec[:int(n.value)]

    def align_from_history(self, call: int, pose=None, **cfg) -> dict:
        """loamx_densemap_align_from_history: align() of logged call `call` where it lies in the log, about its logged origin; pose
        None: identity.  Byte for byte align(*history(call)'s cloud, pose, centre=its origin)"""
        return self._align(lib().loamx_densemap_align_from_history, (C.c_uint64(call),), pose, (), cfg)[1]

    def align_many_from_history(self, call: int, poses=None, raw=False, **cfg):
        """loamx_densemap_align_many_from_history: align_many() of logged call `call` where it lies, about its logged origin; poses
        None: the identity alone.  Returns (results, best)"""
        return self._align_many(lib().loamx_densemap_align_many_from_history, (C.c_uint64(call),), poses, (), raw, cfg)[1:]

    def align_pyramid_from_history(self, call: int, pose=None, first_level=None, **cfg):
        """loamx_densemap_align_pyramid_from_history: align_pyramid() of logged call `call` where it lies, about its logged origin"""
        return self._align_pyramid(lib().loamx_densemap_align_pyramid_from_history, (C.c_uint64(call),), pose, (), first_level, cfg)[1]

    def rebuild_stats(self) -> dict:
        s = (C.c_uint64 * 4)()
        _check(lib().loamx_densemap_get_rebuild_stats(self.h, s))
        return dict(zip(("rebuilds", "tables_tried", "launches", "points_replayed"), (int(v) for v in s)))

    def reset(self):
        _check(lib().loamx_densemap_reset(self.h))
        self._level = 0

    def set_combine(self, on: bool):
        """bench hook: the in-wave combining of equal keys before the table is touched (default on; results are the same)"""
        _check(lib().loamx_densemap_set_combine(self.h, 1 if on else 0))

    @property
    def rehashes(self) -> int:
        return int(lib().loamx_densemap_rehashes(self.h))


class PlaceConfig(C.Structure):
    _fields_ = [("n_rings", C.c_int), ("n_sectors", C.c_int), ("max_range", C.c_float), ("min_range", C.c_float),
                ("height_offset", C.c_float), ("n_candidates", C.c_int), ("exclude_recent", C.c_uint32), ("max_entries", C.c_uint32),
                ("initial_entries", C.c_uint32), ("device", C.c_int)]


class PlaceMatch(C.Structure):
    _fields_ = [("id", C.c_uint32), ("shift", C.c_uint32), ("distance", C.c_float), ("ring_key_distance", C.c_float)]


PLACE_MAX_RESULTS = 64


def place_sector_table(n_sectors: int) -> np.ndarray:
    """loamx_place_sector_table: (S, 2) float32 boundary directions (cos, sin)(2 pi k / S) of the sectors.  Host only."""
    out = np.zeros((max(int(n_sectors), 1), 2), np.float32)
    _check(lib().loamx_place_sector_table(int(n_sectors), out.ctypes.data_as(C.c_void_p)))
    return out


class PlaceViewConfig(C.Structure):
    """loamx_place_view_config: how loamx_place_add_views sees the map from a view origin; the defaults are PLACE_VIEW_CAST, 4096, 0, 1"""
    _fields_ = [("mode", C.c_uint32), ("max_steps", C.c_uint32), ("skip_steps", C.c_uint32), ("min_points", C.c_uint32)]


PLACE_VIEW_CAST, PLACE_VIEW_VOXELS = 0, 1                                        # loamx_place_view_config.mode
PLACE_VIEW_MAX_ORIGINS, PLACE_VIEW_MAX_RAYS = 4096, 65536
PLACE_VIEW_STATS = ("entries", "not_traced", "miss", "hit", "hit_end", "cells")   # stats[6] of loamx_place_add_views (CAST mode)


def _triples(a, what) -> np.ndarray:
    t = np.ascontiguousarray(a, np.float32)
    assert t.ndim == 2 and t.shape[1] == 3, what + " must be (n, 3)"
    return t


def view_rays(n_azimuth: int, elevations, range_m: float) -> np.ndarray:
    """loamx_place_view_rays (host only): (len(elevations) * n_azimuth, 3) float32 offsets of a lidar's rays, ring-major, each range_m
    long; elevations in radians, azimuth 2 pi a / n_azimuth from +z towards +x.  The offsets argument of PlaceDB.add_views."""
    el = np.ascontiguousarray(elevations, np.float32).reshape(-1)
    out = np.zeros((max(len(el) * int(n_azimuth), 1), 3), np.float32)
    _check(lib().loamx_place_view_rays(C.c_uint32(n_azimuth), el.ctypes.data_as(C.c_void_p), C.c_uint32(len(el)), C.c_float(range_m),
                                       out.ctypes.data_as(C.c_void_p)))
    return out[:len(el) * int(n_azimuth)]


def grid_view_origins(cells, cfg: GridConfig, leaf: float, stride=1, min_clear2=1, sensor_height=0.0, capacity=None) -> np.ndarray:
    """loamx_grid_view_origins (host only): (n, 3) float32 view origins, one per FREE cell (rx, rz) of a navigation grid with
    rx % stride == rz % stride == 0 and clear2 >= min_clear2, in ascending record order: the cell's centre in x and z, its elevation
    + sensor_height in y.  capacity None: all of them; otherwise the first `capacity`."""
    a = _grid_cells(cells)
    assert a.size == cfg.nx * cfg.nz, "cells does not have the configuration's nx * nz records"
    n = C.c_uint64(0)
    args = (a.ctypes.data_as(C.c_void_p), C.byref(cfg), C.c_float(leaf), C.c_uint32(stride), C.c_uint32(min_clear2), C.c_float(sensor_height))
    if capacity is None:
        _check(lib().loamx_grid_view_origins(*args, None, C.c_uint64(0), C.byref(n)))
        capacity = n.value
    out = np.zeros((max(int(capacity), 1), 3), np.float32)
    _check(lib().loamx_grid_view_origins(*args, out.ctypes.data_as(C.c_void_p), C.c_uint64(capacity), C.byref(n)))
    return out[:min(int(capacity), n.value)]


def view_pose(view_origin, shift: int, n_sectors: int, query_origin=None) -> np.ndarray:
    """loamx_place_view_pose (host only): the (3, 4) float64 start pose, map <- query frame, that the match (id, shift) of a query
    described about query_origin (None: 0) implies for the view at view_origin: R = rot_y(shift * 2 pi / n_sectors),
    t = view_origin - R query_origin.  The pose argument of DenseMap.align_many / align_pyramid."""
    v = np.ascontiguousarray(view_origin, np.float32)
    q = None if query_origin is None else np.ascontiguousarray(query_origin, np.float32)
    assert v.shape == (3,) and (q is None or q.shape == (3,))
    out = np.zeros(12, np.float64)
    _check(lib().loamx_place_view_pose(v.ctypes.data_as(C.c_void_p), C.c_uint32(shift), C.c_int(n_sectors),
                                       q.ctypes.data_as(C.c_void_p) if q is not None else None, out.ctypes.data_as(C.c_void_p)))
    return out.reshape(3, 4)


class PlaceDB:
    """loamx_place_*: scan-context descriptors of sweeps in device memory and the search for earlier entries that look like a query.
    add: a cloud from the host; add_from: a LaserMapping's last registered cloud; add_from_pipeline: a Pipeline's; add_views: a
    DenseMap seen from many view origins.  A match is (id, shift, distance, ring_key_distance); yaw_hint(shift) = shift * 2 pi /
    n_sectors (include/loamx.h has the convention)."""

    def __init__(self, n_rings=20, n_sectors=60, max_range=80.0, min_range=0.0, height_offset=2.0, n_candidates=0, exclude_recent=50,
                 max_entries=0, initial_entries=1024, device=0):
        L = lib()
        L.loamx_place_create.restype = C.c_void_p
        L.loamx_place_size.restype = C.c_uint32
        L.loamx_place_growths.restype = C.c_uint64
        self._c = _cfg(PlaceConfig, "loamx_place_default_config", n_rings=n_rings, n_sectors=n_sectors, max_range=max_range,
                       min_range=min_range, height_offset=height_offset, n_candidates=n_candidates, exclude_recent=exclude_recent,
                       max_entries=max_entries, initial_entries=initial_entries, device=device)
        self.n_rings, self.n_sectors = n_rings, n_sectors
        self.h = C.c_void_p(L.loamx_place_create(C.byref(self._c)))
        if not self.h:
            raise LoamxError(E_INVALID, L.loamx_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_place_destroy(self.h)
            self.h = None

    __del__ = close

    def __len__(self):
        return int(lib().loamx_place_size(self.h))

    @staticmethod
    def _origin(origin):
        o = np.ascontiguousarray(origin, np.float32)
        assert o.shape == (3,)
        return o

    def _add(self, fn, *head):
        # the new entry's id, or None when the source had no cloud
        i = C.c_uint32(0)
        rc = _check(fn(self.h, *head, C.byref(i)))
        return int(i.value) if rc == OK else None

    def add(self, points, origin=(0.0, 0.0, 0.0)) -> int:
        """describe an (N, 4) / (N, 8) cloud about origin and store it; returns the new entry's id.  LoamxError E_CAPACITY when
        max_entries would be passed (the database is then unchanged)"""
        a = as_points(points)
        o = self._origin(origin)
        return self._add(lib().loamx_place_add, C.byref(cloud_of(a)), o.ctypes.data_as(C.c_void_p))

    def add_from(self, mapping):
        """the registered full-resolution cloud of mapping's last process / process_linked: the new id, or None when it produced none"""
        return self._add(lib().loamx_place_add_from_map, mapping.h)

    def add_from_pipeline(self, pipeline, slot: int):
        """the registered cloud of the slot-th stream registered in pipeline's last step: the new id, or None when it registered none"""
        return self._add(lib().loamx_place_add_from_pipeline, pipeline.h, slot)

    def add_views(self, densemap, origins, offsets=None, mode=None, max_steps=4096, skip_steps=0, min_points=1, static=None):
        """loamx_place_add_views: one entry per view origin ((n, 3), map frame), described from densemap on the device.  With offsets
        ((n_rays, 3), e.g. view_rays()) a view is what the rays origin -> origin + offset hit (PLACE_VIEW_CAST; max_steps, skip_steps
        and min_points as DenseMap.raycast takes them); without, every voxel of the map (PLACE_VIEW_VOXELS).  mode None: by whether
        offsets are given.  static (a StaticRule; needs carving): without the voxels the rule calls dynamic.  Returns (first_id,
        stats): entry first_id + i belongs to origins[i]; stats is a dict in the order of PLACE_VIEW_STATS (in VOXELS mode
        "not_traced" holds the number of qualifying voxels).  Blocks.  LoamxError E_CAPACITY when max_entries would be passed."""
        o = _triples(origins, "origins")
        f = None if offsets is None else _triples(offsets, "offsets")
        if mode is None:
            mode = PLACE_VIEW_VOXELS if f is None else PLACE_VIEW_CAST
        k = _cfg(PlaceViewConfig, "loamx_place_view_default_config", mode=mode, max_steps=max_steps, skip_steps=skip_steps,
                 min_points=min_points)
        first, stats = C.c_uint32(0), np.zeros(6, np.uint64)
        _check(lib().loamx_place_add_views(self.h, densemap.h, o.ctypes.data_as(C.c_void_p), C.c_uint32(len(o)),
                                           f.ctypes.data_as(C.c_void_p) if f is not None else None, C.c_uint32(0 if f is None else len(f)),
                                           C.byref(k), C.byref(static) if static is not None else None, C.byref(first),
                                           stats.ctypes.data_as(C.c_void_p)))
        return int(first.value), dict(zip(PLACE_VIEW_STATS, (int(v) for v in stats)))

    @staticmethod
    def _matches(m, n):
        return [(int(m[i].id), int(m[i].shift), np.float32(m[i].distance), np.float32(m[i].ring_key_distance)) for i in range(n)]

    def query_entry(self, entry: int, n_results=5):
        """the best earlier entries for a stored one (the configuration's exclude_recent): [(id, shift, distance, ring_key_distance)]"""
        m = (PlaceMatch * PLACE_MAX_RESULTS)()
        n = C.c_uint32(0)
        _check(lib().loamx_place_query_entry(self.h, C.c_uint32(entry), m, C.c_uint32(n_results), C.byref(n)))
        return self._matches(m, n.value)

    def query(self, points, origin=(0.0, 0.0, 0.0), exclude_recent=0, n_results=5):
        """the best entries for a cloud that is not stored (exclude_recent 0: every entry is a candidate)"""
        a = as_points(points)
        c = cloud_of(a)
        o = self._origin(origin)
        m = (PlaceMatch * PLACE_MAX_RESULTS)()
        n = C.c_uint32(0)
        _check(lib().loamx_place_query(self.h, C.byref(c), o.ctypes.data_as(C.c_void_p), C.c_uint32(exclude_recent), m, C.c_uint32(n_results),
                                       C.byref(n)))
        return self._matches(m, n.value)

    def yaw_hint(self, shift: int) -> float:
        return float(shift) * 2.0 * np.pi / self.n_sectors

    def descriptor(self, entry: int):
        """(desc (R, S), ring_key (R,)) float32 of a stored entry"""
        d = np.zeros((self.n_rings, self.n_sectors), np.float32)
        k = np.zeros(self.n_rings, np.float32)
        _check(lib().loamx_place_get_descriptor(self.h, C.c_uint32(entry), d.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)))
        return d, k

    def save(self, path: str):
        _check(lib().loamx_place_save(self.h, os.fsencode(path)))

    def load(self, path: str):
        _check(lib().loamx_place_load(self.h, os.fsencode(path)))

    def reset(self):
        _check(lib().loamx_place_reset(self.h))

    @property
    def growths(self) -> int:
        """test hook: how often the table of entries has doubled"""
        return int(lib().loamx_place_growths(self.h))


class PoseGraphConfig(_DefaultedConfig, C.Structure):
    """loamx_posegraph_config.  PoseGraphConfig() holds the defaults (50 LM steps, 500 CG iterations per step in batches of 16, room for
    1024 nodes and 2048 edges, cg_tolerance 1e-8, eps_step 1e-9, eps_cost 1e-12, lambda_init 1e-6, huber_delta 0); keyword arguments
    replace them."""
    _fields_ = [("max_iterations", C.c_uint32), ("max_cg_iterations", C.c_uint32), ("cg_batch", C.c_uint32), ("initial_nodes", C.c_uint32),
                ("initial_edges", C.c_uint32), ("cg_tolerance", C.c_double), ("eps_step", C.c_double), ("eps_cost", C.c_double),
                ("lambda_init", C.c_double), ("huber_delta", C.c_double), ("device", C.c_int)]

    _default, _checker = "loamx_posegraph_default_config", "loamx_posegraph_check"


class PoseGraphEdge(C.Structure):
    _fields_ = [("i", C.c_uint32), ("j", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32), ("z", C.c_double * 12),
                ("info", C.c_double * 21)]


class PoseGraphResult(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("accepted", C.c_uint32), ("cg_iterations", C.c_uint32), ("looks", C.c_uint32),
                ("status", C.c_int), ("cost_initial", C.c_double), ("cost_final", C.c_double), ("last_step", C.c_double),
                ("lambda_final", C.c_double)]


PG_EDGE_ROBUST = 1                                                               # LOAMX_PG_EDGE_ROBUST
POSEGRAPH_EDGE = np.dtype([("i", "<u4"), ("j", "<u4"), ("flags", "<u4"), ("reserved", "<u4"), ("z", "<f8", 12), ("info", "<f8", 21)])
POSEGRAPH_STATS = ("launches", "looks", "cg_iterations", "linearisations")      # stats[4] of loamx_posegraph_get_stats
POSEGRAPH_STATUS = ("converged", "max_iterations", "lambda_cap")                 # loamx_posegraph_result.status


def _poses12(poses) -> np.ndarray:
    """(N, 12) float64 from (N, 12), (N, 3, 4) or (N, 4, 4); a single pose becomes N = 1"""
    a = np.asarray(poses, np.float64)
    if a.ndim == 1 or (a.ndim == 2 and a.shape[-1] == 4):
        a = a[None]
    if a.ndim == 3:
        a = a[:, :3, :4].reshape(len(a), 12)
    assert a.ndim == 2 and a.shape[1] == 12, "poses must be (N, 12), (N, 3, 4) or (N, 4, 4)"
    return np.ascontiguousarray(a)


def posegraph_edges(i, j, z, info, flags=0) -> np.ndarray:
    """POSEGRAPH_EDGE records from arrays: i, j (M,), z (M, 12) / (M, 3, 4) / (M, 4, 4), info (M, 21) or one (21,) for all"""
    i = np.atleast_1d(np.asarray(i, np.uint32))
    e = np.zeros(len(i), POSEGRAPH_EDGE)
    e["i"], e["j"], e["flags"] = i, np.asarray(j, np.uint32), flags
    e["z"] = _poses12(z)
    e["info"] = np.asarray(info, np.float64)
    return e


def posegraph_between(Ti, Tj) -> np.ndarray:
    """loamx_posegraph_between (host only): z = Ti^-1 Tj as (12,) float64, the odometry edge between two registered sweeps"""
    a, b, z = _poses12(Ti), _poses12(Tj), np.zeros(12)
    _check(lib().loamx_posegraph_between(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p)))
    return z


def posegraph_residual(Ti, Tj, z) -> np.ndarray:
    """loamx_posegraph_residual (host only): r = [t_E ; Log(R_E)] of the edge z between the poses Ti and Tj, (6,) float64"""
    a, b, m, r = _poses12(Ti), _poses12(Tj), _poses12(z), np.zeros(6)
    _check(lib().loamx_posegraph_residual(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p),
                                          r.ctypes.data_as(C.c_void_p)))
    return r


def posegraph_info_diagonal(sigma_t: float, sigma_r: float) -> np.ndarray:
    """loamx_posegraph_info_diagonal (host only): the 21 upper-triangle entries of diag(1 / sigma_t^2 x 3, 1 / sigma_r^2 x 3)"""
    info = np.zeros(21)
    _check(lib().loamx_posegraph_info_diagonal(C.c_double(sigma_t), C.c_double(sigma_r), info.ctypes.data_as(C.c_void_p)))
    return info


def posegraph_check_gauge(fixed, edges):
    """loamx_posegraph_check_gauge (host only): None when every connected component has a fixed node, else the smallest node id of a
    component without one.  fixed: (N,) flags; edges: POSEGRAPH_EDGE records (only i and j are read)"""
    f = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
    e = np.ascontiguousarray(edges, POSEGRAPH_EDGE)
    bad = C.c_uint32(0)
    L = lib()
    rc = L.loamx_posegraph_check_gauge(C.c_uint32(len(f)), f.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.c_uint64(len(e)),
                                       C.byref(bad))
    if rc == OK:
        return None
    if "gauge" not in L.loamx_last_error().decode():
        _check(rc)
    return int(bad.value)


def posegraph_corrections(before, after) -> np.ndarray:
    """loamx_posegraph_corrections (host only): C_k = after_k * before_k^-1 as (N, 12) float64, what DenseMap.rebuild takes"""
    b, a = _poses12(before), _poses12(after)
    assert a.shape == b.shape
    out = np.zeros_like(a)
    _check(lib().loamx_posegraph_corrections(b.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.c_uint32(len(a)),
                                             out.ctypes.data_as(C.c_void_p)))
    return out


class PoseGraph:
    """loamx_posegraph_*: SE(3) poses (double[12], row-major 3x4) and relative-pose edges in device memory, optimised there by
    Levenberg-Marquardt with a block-Jacobi PCG (include/loamx.h has every definition).  config: a PoseGraphConfig, or keyword
    arguments on top of the defaults."""

    def __init__(self, config: PoseGraphConfig = None, **fields):
        L = lib()
        L.loamx_posegraph_create.restype = C.c_void_p
        L.loamx_posegraph_bad_pivots.restype = C.c_uint32
        self.config = (config.copy(**fields) if config is not None else PoseGraphConfig(**fields))
        self.h = C.c_void_p(L.loamx_posegraph_create(C.byref(self.config)))
        if not self.h:
            raise LoamxError(E_INVALID, L.loamx_last_error().decode())

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_posegraph_destroy(self.h)
            self.h = None

    __del__ = close

    def reset(self):
        _check(lib().loamx_posegraph_reset(self.h))

    @property
    def size(self):
        """(nodes, edges)"""
        n, e = C.c_uint32(0), C.c_uint64(0)
        _check(lib().loamx_posegraph_size(self.h, C.byref(n), C.byref(e)))
        return int(n.value), int(e.value)

    def add_nodes(self, poses) -> int:
        """new free nodes with these poses; returns the id of the first"""
        a = _poses12(poses)
        first = C.c_uint32(0)
        _check(lib().loamx_posegraph_add_nodes(self.h, a.ctypes.data_as(C.c_void_p), C.c_uint32(len(a)), C.byref(first)))
        return int(first.value)

    def set_fixed(self, node: int, fixed=True):
        _check(lib().loamx_posegraph_set_fixed(self.h, C.c_uint32(node), C.c_int(1 if fixed else 0)))

    def set_poses(self, first: int, poses):
        a = _poses12(poses)
        _check(lib().loamx_posegraph_set_poses(self.h, C.c_uint32(first), C.c_uint32(len(a)), a.ctypes.data_as(C.c_void_p)))

    def poses(self, first=0, n=None) -> np.ndarray:
        """(n, 12) float64: the poses of the nodes first .. first + n - 1 (n None: to the last node)"""
        if n is None:
            n = self.size[0] - first
        out = np.zeros((max(int(n), 0), 12))
        _check(lib().loamx_posegraph_get_poses(self.h, C.c_uint32(first), C.c_uint32(n), out.ctypes.data_as(C.c_void_p)))
        return out

    def add_edges(self, edges):
        """POSEGRAPH_EDGE records (posegraph_edges builds them from arrays)"""
        e = np.ascontiguousarray(edges, POSEGRAPH_EDGE)
        _check(lib().loamx_posegraph_add_edges(self.h, e.ctypes.data_as(C.c_void_p), C.c_uint64(len(e))))

    def linearise(self) -> dict:
        """the probe: chi2 (E,), grad (N, 6), diag (N, 6, 6) and cost at the current poses, weights at lambda = 0"""
        n, m = self.size
        chi2, grad, diag, cost = np.zeros(m), np.zeros((n, 6)), np.zeros((n, 6, 6)), C.c_double(0.0)
        _check(lib().loamx_posegraph_linearise(self.h, chi2.ctypes.data_as(C.c_void_p), grad.ctypes.data_as(C.c_void_p),
                                               diag.ctypes.data_as(C.c_void_p), C.byref(cost)))
        return dict(chi2=chi2, grad=grad, diag=diag, cost=float(cost.value))

    def optimize(self) -> dict:
        """loamx_posegraph_optimize: the result record as a dict (status 0 converged, 1 max_iterations, 2 lambda at its cap)"""
        r = PoseGraphResult()
        _check(lib().loamx_posegraph_optimize(self.h, C.byref(r)))
        out = {f: getattr(r, f) for f, _ in PoseGraphResult._fields_}
        out["bad_pivots"] = int(lib().loamx_posegraph_bad_pivots(self.h))
        return out

    def stats(self) -> dict:
        s = (C.c_uint64 * 4)()
        _check(lib().loamx_posegraph_get_stats(self.h, s))
        return dict(zip(POSEGRAPH_STATS, (int(v) for v in s)))


def dist_shard_of(rank: int, world: int, batch: int):
    b, e = C.c_uint32(0), C.c_uint32(0)
    _check(lib().loamx_dist_shard_of(rank, world, batch, C.byref(b), C.byref(e)))
    return int(b.value), int(e.value)


def dist_pack_results(poses6, iters_flags, n_pad: int) -> np.ndarray:
    """a rank's padded send block of the result exchange (n_pad x 8 floats)"""
    p = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
    f = np.ascontiguousarray(iters_flags, np.int32).reshape(len(p), 2) if iters_flags is not None else None
    out = np.zeros((n_pad, 8), np.float32)
    _check(lib().loamx_dist_pack_results(p.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p) if f is not None else None, len(p), n_pad,
                                         out.ctypes.data_as(C.c_void_p)))
    return out


def dist_unpack_results(recv, counts, n_pad: int):
    """inverse of dist_pack_results for the gathered blocks recv[world][n_pad][8]"""
    r = np.ascontiguousarray(recv, np.float32)
    c = np.ascontiguousarray(counts, np.uint32)
    tot = int(c.sum())
    pa, fa = np.zeros((max(tot, 1), 6), np.float32), np.zeros((max(tot, 1), 2), np.int32)
    _check(lib().loamx_dist_unpack_results(r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), len(c), n_pad, pa.ctypes.data_as(C.c_void_p),
                                           fa.ctypes.data_as(C.c_void_p)))
    return pa[:tot], fa[:tot]


def dist_pack_clouds(corners, surfs, poses6) -> np.ndarray:
    """one rank's message of the epoch merge step (loamx_dist_pack_clouds): per stream its re-projected corner / surf clouds and its
    transformAftMapped -> uint32 words"""
    cs = [as_points(c) for c in corners]
    ss = [as_points(c) for c in surfs]
    n = len(cs)
    assert len(ss) == n
    p = np.ascontiguousarray(poses6, np.float32).reshape(n, 6) if n else np.zeros((0, 6), np.float32)
    CA = Cloud * max(n, 1)
    ca, sa = CA(*[cloud_of(c) for c in cs]), CA(*[cloud_of(c) for c in ss])
    nw = C.c_uint64(0)
    _check(lib().loamx_dist_pack_clouds(n, C.addressof(ca), C.addressof(sa), p.ctypes.data, None, 0, C.addressof(nw)))
    out = np.zeros(int(nw.value), np.uint32)
    _check(lib().loamx_dist_pack_clouds(n, C.addressof(ca), C.addressof(sa), p.ctypes.data, out.ctypes.data, len(out), C.addressof(nw)))
    return out


def dist_unpack_clouds(words):
    """inverse of dist_pack_clouds -> [(pose6, corner, surf)] per stream"""
    w = np.ascontiguousarray(words, np.uint32)
    ns = C.c_uint32(0)
    _check(lib().loamx_dist_unpack_clouds_header(w.ctypes.data, len(w), C.addressof(ns), None, None, 0))
    n = int(ns.value)
    nc, nsf = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    _check(lib().loamx_dist_unpack_clouds_header(w.ctypes.data, len(w), C.addressof(ns), nc.ctypes.data, nsf.ctypes.data, max(n, 1)))
    out = []
    for s in range(n):
        pose = np.zeros(6, np.float32)
        co, so = np.zeros((max(int(nc[s]), 1), 4), np.float32), np.zeros((max(int(nsf[s]), 1), 4), np.float32)
        cc, sc = cloud_of(co), cloud_of(so)
        _check(lib().loamx_dist_unpack_clouds_stream(w.ctypes.data, len(w), s, pose.ctypes.data, C.addressof(cc), C.addressof(sc)))
        out.append((pose, co[:cc.count].copy(), so[:sc.count].copy()))
    return out


def dist_split_messages(words, counts):
    """the root's receive buffer of a gatherv -> one message per rank (rank order; an empty rank -> None)"""
    out, o = [], 0
    for c in counts:
        c = int(c)
        out.append(np.ascontiguousarray(words[o:o + c]) if c else None)
        o += c
    return out


class Dist:
    """loamx_dist_*: the multi-GPU exchanges of the batched mode over RCCL (one process per GPU)."""
    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_ubyte * Dist.ID_BYTES)()
        _check(lib().loamx_dist_get_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id: bytes, rank: int, world_size: int, device: int = 0):
        assert len(unique_id) == self.ID_BYTES
        L = lib()
        L.loamx_dist_create.restype = C.c_void_p
        L.loamx_dist_stream.restype = C.c_void_p
        buf = (C.c_ubyte * self.ID_BYTES).from_buffer_copy(unique_id)
        self.h = C.c_void_p(L.loamx_dist_create(buf, rank, world_size, device))
        if not self.h:
            raise LoamxError(E_INVALID, L.loamx_last_error().decode())
        self.rank, self.world = rank, world_size

    def close(self):
        if getattr(self, "h", None):
            lib().loamx_dist_destroy(self.h)
            self.h = None

    __del__ = close

    def shard(self, batch: int):
        b, e = C.c_uint32(), C.c_uint32()
        _check(lib().loamx_dist_shard(self.h, batch, C.byref(b), C.byref(e)))
        return int(b.value), int(e.value)

    def broadcast_map(self, d_corner_ptr: int, n_corner: int, d_surf_ptr: int, n_surf: int, root: int = 0, wait_event: int = 0) -> int:
        """asynchronous; returns the raw hipEvent_t recorded behind the broadcast (for stage_frozen_device)"""
        ev = C.c_void_p()
        _check(lib().loamx_dist_broadcast_map(self.h, C.c_void_p(d_corner_ptr), n_corner, C.c_void_p(d_surf_ptr), n_surf, root,
                                              C.c_void_p(wait_event or None), C.byref(ev)))
        return int(ev.value or 0)

    def allgather_results(self, poses6, iters_flags=None, batch=None):
        """every rank's records in rank order; shards may be unequal, also empty.  The counts are gathered first
        (loamx_dist_allgather_counts) and the receive arrays sized by them; batch (optional) = the total the caller expects.  The C call is told the
        capacity either way and answers LOAMX_E_CAPACITY instead of writing beyond it.  Returns (poses, flags, counts per rank)"""
        p = np.ascontiguousarray(poses6, np.float32).reshape(-1, 6)
        n = len(p)
        f = np.ascontiguousarray(iters_flags, np.int32).reshape(n, 2) if iters_flags is not None else None
        cnt = np.zeros(self.world, np.uint32)
        # the counts are ALWAYS gathered: whether a rank passes `batch` must not decide which collectives it takes part in (ranks that
        # disagreed would hang in mismatched collectives); `batch` is only checked against them
        _check(lib().loamx_dist_allgather_counts(self.h, n, cnt.ctypes.data_as(C.c_void_p)))
        cap = int(cnt.sum())
        # (a `batch` that disagrees is reported AFTER the results collective: a rank that left the protocol between the two collectives
        # would leave the others blocked inside the second one)
        pa = np.zeros((max(cap, 1), 6), np.float32)
        fa = np.zeros((max(cap, 1), 2), np.int32)
        _check(lib().loamx_dist_allgather_results_cap(self.h, p.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p) if f is not None else None,
                                                      n, pa.ctypes.data_as(C.c_void_p), fa.ctypes.data_as(C.c_void_p), cap, cnt.ctypes.data_as(C.c_void_p)))
        tot = int(cnt.sum())
        if batch is not None and int(batch) != cap:
            raise ValueError(f"allgather_results: batch = {batch} but the ranks hold {cap} records")
        return pa[:tot], fa[:tot], cnt

    def allgather_counts(self, n: int) -> np.ndarray:
        """every rank's n (loamx_dist_allgather_counts): also the way a root tells the others a size"""
        cnt = np.zeros(self.world, np.uint32)
        _check(lib().loamx_dist_allgather_counts(self.h, int(n), cnt.ctypes.data_as(C.c_void_p)))
        return cnt

    def gatherv(self, words, root: int = 0):
        """variable-size gather of uint32 words to `root` (loamx_dist_gatherv): returns (messages per rank | None off the root, counts)"""
        w = np.ascontiguousarray(words if words is not None else np.zeros(0, np.uint32), np.uint32)
        cnt = np.zeros(self.world, np.uint32)
        # the root cannot size its buffer before it knows the counts: they are gathered by a first call with nothing to receive into
        _check(lib().loamx_dist_allgather_counts(self.h, len(w), cnt.ctypes.data_as(C.c_void_p)))
        tot = int(cnt.sum())
        recv = np.zeros(max(tot, 1), np.uint32) if self.rank == root else None
        _check(lib().loamx_dist_gatherv(self.h, w.ctypes.data, len(w), root, recv.ctypes.data if recv is not None else None,
                                        tot if recv is not None else 0, cnt.ctypes.data))
        return (dist_split_messages(recv[:tot], cnt) if recv is not None else None), cnt

    def comm_count(self) -> int:
        return int(lib().loamx_dist_comm_count(self.h))

    def barrier(self):
        _check(lib().loamx_dist_barrier(self.h))

    @property
    def stream(self) -> int:
        return int(lib().loamx_dist_stream(self.h) or 0)
