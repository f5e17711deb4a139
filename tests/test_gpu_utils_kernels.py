"""The kernels of csrc/zk_utils.hip through the C ABI: order statistics against np.sort, exactly, at the sizes where the radix
select changes path (one lane, one wave, one workgroup, one vector, one sweep of the whole grid) and on inputs that put all the
work into one digit; the statistics against math.fsum."""
import math
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

from mtflearn_amd import _native, utils

pytestmark = pytest.mark.gpu

# 1 + 1024 * 1024: the grid sweeps 1024 workgroups x 256 lanes x 4 float32 per step, so only a larger image makes a lane loop
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 4099, 70001, 1024 * 1024 + 4099]
FLT_MAX = np.finfo(np.float32).max


def order_stats(x, ranks, center=None):
    """zk_image_order_stats (the host-buffer form) on a flat array."""
    x = np.ascontiguousarray(x)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    values = np.empty(len(ranks), np.float32)
    mode = _native.ORDER_VALUES if center is None else _native.ORDER_DEVIATIONS
    _native.check(_native.load().zk_image_order_stats(0, x.ctypes.data_as(c_void_p), _native.dtype_code(x.dtype), x.size, mode,
                                                      0.0 if center is None else float(center), ranks.ctypes.data_as(c_void_p),
                                                      len(ranks), values.ctypes.data_as(c_void_p)), "zk_image_order_stats")
    return values


def image_stats(x, center=None, wide=False):
    x = np.ascontiguousarray(x)
    minmax, sums, bad = np.empty(2, np.float32), np.empty(3, np.float64), c_int64()
    mode = (_native.STATS_CENTERED if center is not None else 0) | (_native.STATS_WIDE if wide else 0)
    _native.check(_native.load().zk_image_stats(0, x.ctypes.data_as(c_void_p), _native.dtype_code(x.dtype), x.size, mode,
                                                0.0 if center is None else float(center), minmax.ctypes.data_as(c_void_p), byref(bad),
                                                sums.ctypes.data_as(c_void_p)), "zk_image_stats")
    return minmax[0], minmax[1], bad.value, sums


def make_input(kind, n, seed=0):
    rng = np.random.default_rng([seed, n])
    if kind == "normal":
        return rng.normal(size=n).astype(np.float32)
    if kind == "ties":                                      # four values: every rank lies inside a run of equal elements
        return rng.integers(0, 4, size=n).astype(np.float32)
    if kind == "constant":
        return np.full(n, -2.5, np.float32)
    if kind == "last_digit":                                # keys that differ in the last radix digit only
        return (1.0 + rng.integers(0, 256, size=n) * 2.0 ** -23).astype(np.float32)
    if kind == "first_digit":                               # +-2^e over the whole exponent range
        return (rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.integers(-126, 128, size=n)).astype(np.float32)
    if kind == "edges":                                     # signed zeros, denormals, the largest finite values
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, FLT_MAX, -FLT_MAX, 1.0, -1.0], np.float32)
        return rng.choice(pool, size=n)
    raise KeyError(kind)


KINDS = ["normal", "ties", "constant", "last_digit", "first_digit", "edges"]


def rank_batches(n, seed=0):
    if n <= 257:
        every = np.arange(n)
        return [every[i:i + 16] for i in range(0, n, 16)]
    rng = np.random.default_rng([seed, n, 1])
    return [np.concatenate([[0, n - 1, (n - 1) // 2, n // 2], rng.integers(0, n, size=12)])]


@pytest.mark.parametrize("n", SIZES)
def test_order_statistics_equal_the_sort(n):
    for kind in KINDS if n <= 70001 else ["normal", "ties", "constant"]:
        x = make_input(kind, n)
        want = np.sort(x)
        for ranks in rank_batches(n):
            got = order_stats(x, ranks)
            assert np.all(got == want[ranks]), (kind, n, ranks[got != want[ranks]], got[got != want[ranks]])


@pytest.mark.parametrize("n", [1, 2, 65, 257, 4099, 70001])
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_deviation_mode_equals_the_sorted_deviations(n, kind):
    x = make_input(kind, n, seed=5)
    c = np.median(x)
    assert c.dtype == np.float32
    want = np.sort(np.abs(x - c))
    for ranks in rank_batches(n):
        got = order_stats(x, ranks, center=c)
        assert np.all(got == want[ranks]), (kind, n)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float64])
def test_other_element_types_are_sorted_as_float32(dtype):
    rng = np.random.default_rng(257)
    if dtype == np.float64:
        x = rng.normal(size=257) * 1e3                      # rounds on conversion
        x[:3] = [1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24]   # a tie, just above it, an odd tie
    else:
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max + 1, size=257).astype(dtype)
    want = np.sort(x.astype(np.float32))
    for ranks in rank_batches(257):
        assert np.all(order_stats(x, ranks) == want[ranks])


@pytest.mark.parametrize("dtype,offsets", [(np.float32, (1, 2, 3)), (np.uint8, (1, 7, 15)), (np.float64, (1,))])
def test_images_off_the_16_byte_grid(dtype, offsets):
    """A view that starts inside a 16-byte vector: the loose elements at both ends are read one by one."""
    rng = np.random.default_rng(9)
    full = (rng.normal(size=4099 + 16) * 50 + 100).clip(0, 255).astype(dtype)
    dev = _native.DeviceArray.from_numpy(full)
    for off in offsets:
        for n in (1, 5, 4099):
            x = full[off:off + n]
            op = utils._Operand(dev[off:off + n])
            ranks = rank_batches(n)[0]
            assert np.all(utils._order_stats(op, ranks) == np.sort(x.astype(np.float32))[ranks])
            mn, mx, bad, sums = utils._stats(op)
            x32 = x.astype(np.float32)
            assert (mn, mx, bad) == (x32.min(), x32.max(), 0)
            assert abs(sums[0] - math.fsum(x32.astype(np.float64))) <= n * 2.0 ** -53 * math.fsum(np.abs(x32).astype(np.float64))


def test_rank_and_size_checks():
    x = np.zeros(10, np.float32)
    for ranks in ([10], [-1], list(range(10)) + list(range(7))):
        with pytest.raises(RuntimeError, match="rank"):
            order_stats(x, ranks)


# ------------------------------------------------------------------------------------------------ stats
def check_sum(got, terms):
    """Within n 2^-53 sum |terms| of the exact sum: the bound of a float64 summation in any order."""
    terms = np.asarray(terms, dtype=np.float64)
    exact, bound = math.fsum(terms), terms.size * 2.0 ** -53 * math.fsum(np.abs(terms))
    print(f"sum {got!r} exact {exact!r} |difference| {abs(got - exact):.3e} bound {bound:.3e}")
    assert abs(got - exact) <= bound


@pytest.mark.parametrize("n", [1, 65, 257, 4099, 70001, 1024 * 1024 + 4099])
def test_stats_of_float32(n):
    rng = np.random.default_rng([3, n])
    x = (rng.normal(size=n) * 100 + 7).astype(np.float32)
    if n >= 65:
        x[rng.choice(n, size=6, replace=False)] = [np.nan, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX]
    finite = x[np.isfinite(x)].astype(np.float64)
    mn, mx, bad, sums = image_stats(x)
    assert (mn, mx, bad) == (finite.min(), finite.max(), n - finite.size) and mn.dtype == np.float32
    check_sum(sums[0], finite)
    check_sum(sums[1], np.abs(finite))
    check_sum(sums[2], finite * finite)
    c = sums[0] / finite.size
    _, _, bad2, centred = image_stats(x, center=c)
    assert bad2 == bad and centred[1] == 0 and centred[2] == 0
    check_sum(centred[0], (finite - c) ** 2)
    again = image_stats(x)
    assert (again[0], again[1], again[2]) == (mn, mx, bad) and again[3].tobytes() == sums.tobytes()   # bit-identical
    assert image_stats(x, center=c)[3].tobytes() == centred.tobytes()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16, np.float64])
@pytest.mark.parametrize("n", [257, 4099])
def test_stats_of_other_element_types(dtype, n):
    rng = np.random.default_rng([4, n])
    if dtype == np.float64:
        x = rng.normal(size=n) * 1e3 + 1.0 / 3.0
    else:
        info = np.iinfo(dtype)
        x = rng.integers(info.min, info.max + 1, size=n).astype(dtype)
    x32 = x.astype(np.float32).astype(np.float64)
    mn, mx, bad, sums = image_stats(x)
    assert (mn, mx, bad) == (np.float32(x32.min()), np.float32(x32.max()), 0)
    check_sum(sums[0], x32)
    check_sum(sums[2], x32 * x32)
    if dtype == np.float64:                                 # ZK_STATS_WIDE: the elements as stored
        wide = image_stats(x, wide=True)[3]
        check_sum(wide[0], x)
        check_sum(wide[1], np.abs(x))
        assert wide[0] != sums[0]
        c = wide[0] / n
        check_sum(image_stats(x, center=c, wide=True)[3][0], (x - c) ** 2)


def test_stats_with_no_finite_element():
    mn, mx, bad, sums = image_stats(np.array([np.nan, np.inf, -np.inf], np.float32))
    assert (mn, mx, bad) == (np.inf, -np.inf, 3) and not sums.any()
