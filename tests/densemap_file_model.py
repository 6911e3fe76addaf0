"""numpy model of the dense map's file and of the merge of two maps (include/loamx.h, loamx_densemap_save and what follows it), exact:
every compared quantity is an integer word or a byte string.  A map is described by its records — a dict with flags, leaf (float32),
keys (ascending uint64), vals (n, 4) uint64, miss (n,) uint32 or None, mom (n, 9) uint64 or None, stats (offered, dropped by range,
dropped by key), carve_stats (six) and carve (max_range, ray_stride, end_margin, max_steps) — taken from one of the models of
tests/densemap_model.py, densemap_carve_model.py and densemap_moments_model.py, which stay the models of the map itself, or read from
a file.  The checker of tests/test_densemap_file_cpu.py and tests/test_gpu_densemap_file.py."""
import struct

import numpy as np

import densemap_carve_model as cm
import densemap_moments_model as mm

CARVING, MOMENTS = 1, 2
HEADER_BYTES = 128
MAX_COUNT = 1 << 30


def records_of(m):
    """the records of a model (or records, returned as they are)"""
    if isinstance(m, dict):
        return m
    carving, moments = isinstance(m, cm.CarveModel), hasattr(m, "moments")
    cs = m.carve_stats() if carving else None
    return dict(flags=(CARVING if carving else 0) | (MOMENTS if moments else 0), leaf=np.float32(m.leaf),
                keys=np.asarray(m.keys, np.uint64), vals=np.asarray(m.vals, np.uint64).reshape(-1, 4),
                miss=m.misses() if carving else None, mom=np.asarray(m.moments(), np.uint64).reshape(-1, 9) if moments else None,
                stats=(m.offered, m.dropped_range, m.dropped_key),
                carve_stats=tuple(cs[k] for k in cm.CARVE_KEYS) if carving else (0,) * 6,
                carve=(m.carve_max_range, m.ray_stride, m.end_margin, m.max_steps) if carving else (0.0, 0, 0, 0))


def to_bytes(m):
    """the file of a model or of records"""
    r = records_of(m)
    n = len(r["keys"])
    hdr = struct.pack("<4sIIf4Q6QfIII16x", b"LXDM", 1, r["flags"], float(np.float32(r["leaf"])), n, *r["stats"], *r["carve_stats"],
                      float(np.float32(r["carve"][0])), *r["carve"][1:])
    assert len(hdr) == HEADER_BYTES
    body = [np.asarray(r["keys"], "<u8").tobytes(), np.asarray(r["vals"], "<u8").tobytes()]
    if r["flags"] & CARVING:
        body.append(np.asarray(r["miss"], "<u4").tobytes() + b"\0" * (4 * (n % 2)))
    if r["flags"] & MOMENTS:
        body.append(np.asarray(r["mom"], "<u8").tobytes())
    return hdr + b"".join(body)


def write(path, m):
    with open(path, "wb") as f:
        f.write(to_bytes(m))


def file_size(flags, n):
    return HEADER_BYTES + 40 * n + (4 * (n + n % 2) if flags & CARVING else 0) + (72 * n if flags & MOMENTS else 0)


def read(path):
    """the records of a file, with the checks of the deep validation (AssertionError)"""
    raw = open(path, "rb").read()
    assert len(raw) >= HEADER_BYTES
    f = struct.unpack("<4sIIf4Q6QfIII16s", raw[:HEADER_BYTES])
    magic, version, flags, leaf, n = f[:5]
    assert magic == b"LXDM" and version == 1 and flags & ~3 == 0 and np.isfinite(leaf) and leaf > 0 and f[-1] == b"\0" * 16
    assert n <= MAX_COUNT and len(raw) == file_size(flags, n)
    pos = HEADER_BYTES
    keys = np.frombuffer(raw, "<u8", n, pos)
    vals = np.frombuffer(raw, "<u8", 4 * n, pos + 8 * n).reshape(n, 4)
    pos += 40 * n
    miss = mom = None
    if flags & CARVING:
        miss = np.frombuffer(raw, "<u4", n, pos)
        pos += 4 * (n + n % 2)
    else:
        assert raw[48:112] == b"\0" * 64
    if flags & MOMENTS:
        mom = np.frombuffer(raw, "<u8", 9 * n, pos).reshape(n, 9)
    assert np.all(keys[1:] > keys[:-1]) and np.all(keys < np.uint64(1 << 63)) and np.all(vals[:, 0] >= 1)
    for a in range(3):
        assert np.all((keys >> np.uint64(21 * a)) & np.uint64((1 << 21) - 1) >= 1)
    return dict(flags=flags, leaf=np.float32(leaf), keys=keys, vals=vals, miss=miss, mom=mom, stats=tuple(f[5:8]),
                carve_stats=tuple(f[8:14]), carve=tuple(f[14:18]))


def merge(a, b):
    """the records of loamx_densemap_merge(a, b) (models or records): words added per key modulo 2^64 (miss: 2^32), statistics
    summed; leaf, flags and the carve configuration are a's"""
    a, b = records_of(a), records_of(b)
    assert a["flags"] == b["flags"] and np.float32(a["leaf"]).tobytes() == np.float32(b["leaf"]).tobytes()
    keys, inv = np.unique(np.concatenate([a["keys"], b["keys"]]), return_inverse=True)
    inv = inv.reshape(-1)

    def summed(x, y, width, dtype):
        acc = np.zeros((len(keys), width), dtype)
        np.add.at(acc, inv, np.concatenate([np.asarray(x, dtype).reshape(-1, width), np.asarray(y, dtype).reshape(-1, width)]))   # (wraps)
        return acc

    return dict(flags=a["flags"], leaf=a["leaf"], keys=keys, vals=summed(a["vals"], b["vals"], 4, np.uint64),
                miss=summed(a["miss"], b["miss"], 1, np.uint32).reshape(-1) if a["flags"] & CARVING else None,
                mom=summed(a["mom"], b["mom"], 9, np.uint64) if a["flags"] & MOMENTS else None,
                stats=tuple(x + y for x, y in zip(a["stats"], b["stats"])),
                carve_stats=tuple(x + y for x, y in zip(a["carve_stats"], b["carve_stats"])), carve=a["carve"])


MODELS = {0: None, CARVING: cm.CarveModel, MOMENTS: mm.MomentsModel, CARVING | MOMENTS: mm.CarveMomentsModel}


def model_of(flags, leaf, **carve):
    """a fresh model with the features of flags; carve: ray_stride, end_margin, max_steps, carve_max_range"""
    import densemap_model as dm
    return dm.Model(leaf=leaf) if flags == 0 else (MODELS[flags](leaf=leaf, **carve) if flags & CARVING else MODELS[flags](leaf=leaf))
