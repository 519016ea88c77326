"""device primitives (scan, radix sort) against numpy -- through the C ABI test hooks"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from reveal_amd import _lib
    L = _lib.get(False)
    assert L.dll.rv_device_count() > 0, "no HIP device"
    return L


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 100000, 2048 * 2048 + 17])
def test_exclusive_sum(lib, n):
    rng = np.random.default_rng(n)
    a = rng.integers(0, 5, size=n, dtype=np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    assert lib.dll.rv_test_exclusive_sum_u32(a.ctypes.data, out.ctypes.data, n) == 0, lib.err()
    ref = np.concatenate([[0], np.cumsum(a, dtype=np.uint64)[:-1]]).astype(np.uint32)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("n", [1, 7, 64, 2049, 300000])
def test_inclusive_max(lib, n):
    rng = np.random.default_rng(n)
    a = np.where(rng.random(n) < 0.05, np.arange(n), 0).astype(np.uint32)
    out = np.zeros(n, dtype=np.uint32)
    assert lib.dll.rv_test_inclusive_max_u32(a.ctypes.data, out.ctypes.data, n) == 0, lib.err()
    assert np.array_equal(out, np.maximum.accumulate(a))


# ---- the 64-bit scans (rv_glocal.hip is their only caller; their wavefront step shuffles a value as two 32-bit words) and all four scans in place
# (in == out: one device buffer, as rv_glocal.hip and rv_blocks.hip scan): 2047 / 2048 / 2049 = one scan tile and two, 2048 * 2048 + 17 = three levels
SCAN_N = [1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 100000, 2048 * 2048 + 17]


def scan_both(lib, fn, a):
    """out of place, then in place on a copy: -> the out-of-place result, after asserting that the in-place one equals it and the input is untouched"""
    keep = a.copy()
    out = np.zeros_like(a)
    assert fn(a.ctypes.data, out.ctypes.data, len(a)) == 0, lib.err()
    assert np.array_equal(a, keep)
    buf = a.copy()
    assert fn(buf.ctypes.data, buf.ctypes.data, len(a)) == 0, lib.err()
    assert np.array_equal(buf, out)
    return out


def exclusive(a):
    return np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(a, dtype=np.uint64)[:-1]])


@pytest.mark.parametrize("n", SCAN_N)
def test_exclusive_sum_u64(lib, n):
    """values below 2^40: every prefix of up to 2^22 + 17 of them stays below 2^63, np.cumsum on uint64 is exact; nearly every value is above 2^32, so
    the high word of a shuffled value matters wherever a thread takes its prefix from another lane (n > 8)"""
    rng = np.random.default_rng(1000 + n)
    a = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    assert n * ((1 << 40) - 1) < 1 << 63
    assert np.array_equal(scan_both(lib, lib.dll.rv_test_exclusive_sum_u64, a), exclusive(a))


@pytest.mark.parametrize("kind", ["high_words_decide", "low_words_decide"])
@pytest.mark.parametrize("n", SCAN_N)
def test_inclusive_max_u64(lib, n, kind):
    rng = np.random.default_rng(2000 + n)
    if kind == "high_words_decide":      # sparse values up to 2^61 among zeros
        a = np.where(rng.random(n) < 0.05, rng.integers(0, 1 << 61, size=n, dtype=np.uint64), np.uint64(0)).astype(np.uint64)
    else:                                  # one high word everywhere: the running maximum moves in the low words only
        a = (np.uint64(0x12345678) << np.uint64(32)) | np.where(rng.random(n) < 0.05, rng.integers(0, 1 << 32, size=n, dtype=np.uint64), np.uint64(0)).astype(np.uint64)
    assert np.array_equal(scan_both(lib, lib.dll.rv_test_inclusive_max_u64, a), np.maximum.accumulate(a))


@pytest.mark.parametrize("n", SCAN_N)
def test_scans_u32_in_place(lib, n):
    rng = np.random.default_rng(3000 + n)
    a = rng.integers(0, 5, size=n, dtype=np.uint32)
    assert np.array_equal(scan_both(lib, lib.dll.rv_test_exclusive_sum_u32, a), exclusive(a).astype(np.uint32))
    b = np.where(rng.random(n) < 0.05, rng.integers(0, 1 << 32, size=n, dtype=np.uint64), 0).astype(np.uint32)
    assert np.array_equal(scan_both(lib, lib.dll.rv_test_inclusive_max_u32, b), np.maximum.accumulate(b))


@pytest.mark.parametrize("n,lo,hi", [(1, 0, 64), (2, 0, 8), (1000, 0, 64), (4096, 0, 16), (4097, 8, 40),
                                      (123457, 0, 64), (1 << 20, 0, 24), (3000001, 32, 56), (70001, 3, 40), (5000, 0, 5)])
def test_radix_sort_stable(lib, n, lo, hi):
    rng = np.random.default_rng(n + lo)
    keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    if n > 1000:                       # many duplicates in the sorted bit range: stability matters
        keys[: n // 2] &= np.uint64(0xFFFF00FF00FF00FF)
    vals = np.arange(n, dtype=np.uint32)
    k, v = keys.copy(), vals.copy()
    assert lib.dll.rv_test_radix_sort(k.ctypes.data, v.ctypes.data, n, lo, hi) == 0, lib.err()
    width = hi - lo
    mask = np.uint64((1 << width) - 1) if width < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    # (the last pass masks its digit: exactly the bits [lo, hi) take part)
    sub = (keys >> np.uint64(lo)) & mask
    order = np.argsort(sub, kind="stable")
    assert np.array_equal(v, vals[order])
    assert np.array_equal(k, keys[order])


@pytest.mark.parametrize("flags", range(16))
@pytest.mark.parametrize("n,bits,dist", [(100_000, 40, 1), (4096 * 9 + 5, 37, 0), (300_000, 16, 2), (1_200_000, 40, 1), (1_050_001, 35, 0)])
def test_radix_sort_variants(lib, flags, n, bits, dist):
    """every variant of the sort (10-bit digits, XCD-aware tile order, 16-bit wave counters, flag 8: histograms from the keys instead of the
    digit bytes the pass before left -- those only above 2^20 keys: rv_prims.hip) sorts device-made
    keys stably -- checked on the device: no adjacent pair out of order by (key bits, original index)"""
    import ctypes
    ms = (ctypes.c_double * 2)()
    bad = ctypes.c_int64(-1)
    assert lib.dll.rv_test_radix_time(n, bits, dist, flags, 2, ms, ctypes.byref(bad)) == 0, lib.err()
    assert bad.value == 0
