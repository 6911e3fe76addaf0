"""GPU: the chained exclusive scan (csrc/scan.hip: k_scan_chained, the look-back of scan.hpp) on its own through loamx_scan_probe,
against np.cumsum in uint64 reduced mod 2^32 — exactly.  The probe's state buffer is cleared once per process and never again, so
every launch here continues the epochs of the ones before it: tile counts around the 64-tile look-back window (64, 65, 128, 129+),
the count as a kernel argument and read from device memory with idle tiles behind it, in place and out of place with the input
cleared behind the scan, empty launches in between, and a count beyond the launch (the kernel's designed cut)."""
import numpy as np
import pytest

from loam_velodyne_amd import loamx

pytestmark = pytest.mark.gpu

TILE = 2048
NS = (0, 1, 2047, 2048, 2049, 131072, 131073, 133120, 262145, 264199)
FILL = 0xA5A5A5A5


def _inputs(n, length, seed):
    rng = np.random.default_rng(seed)
    wrap = rng.integers(2**30, 2**32, length, dtype=np.uint64).astype(np.uint32)   # a handful of these already pass 2^32
    return dict(ones=np.ones(length, np.uint32), random16=rng.integers(1, 2**16, length, dtype=np.uint64).astype(np.uint32), wraps=wrap)


def _expected(values, n):
    c = np.concatenate([np.zeros(1, np.uint64), np.cumsum(values[:n].astype(np.uint64), dtype=np.uint64)])
    return (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _check(values, n, max_n, flags, what):
    length, in_place = max(n, max_n), bool(flags & loamx.SCAN_IN_PLACE)
    r = loamx.scan_probe(values, n, max_n, flags, out_fill=FILL, want_out2=True)
    assert r["rc"] == loamx.OK, what
    want = _expected(values, n)
    for name in ("out", "out2"):
        got = r[name]
        if got is None:
            continue
        assert np.array_equal(got[:n + 1], want), f"{what}: {name}[0..n], first difference at {int(np.flatnonzero(got[:n + 1] != want)[0])}"
        # behind [n] nothing is written: the fill pattern, or — in place — the rest of the input buffer and the fill word at its end
        tail = np.concatenate([values[n + 1:], [FILL]]).astype(np.uint32)[:length - n] if in_place and name == "out" else np.full(length - n, FILL, np.uint32)
        assert np.array_equal(got[n + 1:], tail), f"{what}: {name} written beyond [n]"
    assert r["total"] == int(want[n]), what
    if flags & loamx.SCAN_ZERO_IN:
        after = r["input_after"]
        assert not after[:n].any(), f"{what}: input not cleared"
        assert np.array_equal(after[n:], values[n:]), f"{what}: input cleared beyond the scanned range"


@pytest.mark.parametrize("on_device", [False, True], ids=["count_as_argument", "count_on_device"])
@pytest.mark.parametrize("n", NS)
def test_scan_equals_cumsum(n, on_device):
    # on the device the launch covers five tiles more than the count: idle tiles that must return without being waited for;
    # as an argument max_n only sizes the buffers (a few guard words behind the scanned range)
    max_n = n + 5 * TILE if on_device else n + 9
    base = loamx.SCAN_COUNT_ON_DEVICE if on_device else 0
    for name, v in _inputs(n, max(n, max_n), 7 * n + on_device).items():
        if name == "wraps" and n >= 8:
            assert int(v[:n].astype(np.uint64).sum()) >= 2**32
        _check(v, n, max_n, base, f"{name} n={n} out of place")
        _check(v, n, max_n, base | loamx.SCAN_ZERO_IN, f"{name} n={n} out of place, input cleared")
        _check(v, n, max_n, base | loamx.SCAN_IN_PLACE, f"{name} n={n} in place")


def test_fixed_sequence_on_the_shared_state():
    """nothing is cleared between launches; an empty launch advances the epoch without touching the tile counter"""
    for on_device in (True, False):
        for step, n in enumerate((0, 264199, 1, 0, 0, 131073, 2048)):
            max_n = n + 5 * TILE if on_device else n
            v = _inputs(n, max(n, max_n), 100 + step)["random16"]
            _check(v, n, max_n, loamx.SCAN_COUNT_ON_DEVICE if on_device else 0, f"sequence step {step} n={n} on_device={on_device}")


def test_count_beyond_the_launch_is_cut_and_reported():
    """device count 5000, launch sized for 2048: the kernel cuts the count to its grid, raises the error word (LOAMX_E_HIP), writes
    nothing behind out[2048] and leaves the state usable"""
    n, max_n = 5000, 2048
    v = _inputs(n, n, 5)["random16"]
    r = loamx.scan_probe(v, n, max_n, loamx.SCAN_COUNT_ON_DEVICE, out_fill=FILL, want_out2=True)
    assert r["rc"] == loamx.E_HIP
    want = _expected(v, max_n)
    for name in ("out", "out2"):
        assert np.array_equal(r[name][:max_n + 1], want), name
        assert np.all(r[name][max_n + 1:] == FILL), f"{name}: written behind the cut"
    assert r["total"] == int(want[max_n])
    for m in (2049, 131073, 0, 1):   # the next ordinary scans on the same state
        w = _inputs(m, m + 5 * TILE, 6)["random16"]
        _check(w, m, m + 5 * TILE, loamx.SCAN_COUNT_ON_DEVICE, f"after the cut, n={m}")


def test_invalid_arguments_are_refused():
    v = np.ones(8, np.uint32)
    with pytest.raises(loamx.LoamxError) as e:
        loamx.scan_probe(v, 8, 8, loamx.SCAN_IN_PLACE | loamx.SCAN_ZERO_IN)
    assert e.value.code == loamx.E_INVALID
    with pytest.raises(loamx.LoamxError) as e:
        loamx.scan_probe(v, 8, 8, 64)
    assert e.value.code == loamx.E_INVALID
