"""The kernels of csrc/zk_background.hip at their own thresholds (case tables: tests/background_cases.py): the rolling ball
across its 16 x 256 tile, its 64-column lane stride and its staging trips, at the radius cap and below one pixel; NaN and inf
pixels in all three estimators and the residual; axes long enough for more than 65,535 row blocks; the residual's second sweep;
the baseline past one 64-column block; the opening at whole segments and at windows around one and two frame lengths.

Every comparison is array equality over the whole frame, against SciPy (opening, baseline) or the restatements of
tests/background_oracle.py (rolling ball), whose forms used here are licensed on the CPU by tests/test_background_cpu.py.

Measured on the MI355X (gfx950), recorded here because two of the groups hinge on it:

* radius 1536 asks for 53,248 bytes of dynamic LDS per workgroup: the launch is accepted (hipDeviceProp_t::sharedMemPerBlock is
  163,840) and exact, so the cap stays at 1536;
* hipDeviceProp_t::maxGridSize is {2147483647, 65536, 65536}.  The launches of group D would need 65,537 blocks along y, one
  more than that, so the kernels that put rows on grid.y stride over it (grid_y in the .hip, at most 65,535 blocks) and such a
  launch is never sent; with the stride all five cases are exact.
"""
import functools
from ctypes import c_double, c_void_p

import numpy as np
import pytest
from scipy import ndimage

import background_cases as bc
import background_oracle as bo
from mtflearn_amd import _native
from mtflearn_amd.background import (estimate_background_baseline, estimate_background_opening,
                                     estimate_background_rolling_ball, remove_background_baseline,
                                     remove_background_opening, remove_background_rolling_ball)

pytestmark = pytest.mark.gpu

HOST_REMOVE = {"opening": remove_background_opening, "rolling_ball": remove_background_rolling_ball,
               "baseline": remove_background_baseline}


def _on_device(method, image, parameter, clip=True, **kw):
    """``(residual, background)`` of ``remove_background_device`` on a device copy of ``image``, back as NumPy arrays."""
    from mtflearn_amd.distributed import remove_background_device
    res, bg = remove_background_device(_native.DeviceArray.from_numpy(image), method, parameter, clip=clip, **kw)
    return res.numpy(), bg.numpy()


def _frozen(array):
    array.setflags(write=False)
    return array


def _scipy_baseline(image, sigma, num_iters):
    """The reference's loop on SciPy, as in tests/test_gpu_background.py."""
    with np.errstate(invalid="ignore"):
        return bo.baseline(image, sigma, num_iters, gauss=ndimage.gaussian_filter)


def _residual(image, background, clip):
    with np.errstate(invalid="ignore"):                                   # inf - inf
        res = image.astype(background.dtype) - background
        return np.clip(res, 0, None) if clip else res


def _assert_same(got, want):
    """Array equality, NaN positions and the signs of infinities included, and the dtype."""
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want))
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ A: rolling-ball seams
@functools.lru_cache(maxsize=None)
def _seam_case(shape, dtype, radius):
    img = bc.frame(shape, dtype, seed=20 + shape[1])
    return _frozen(img), _frozen(bo.rolling_ball(img, radius))


@pytest.mark.parametrize("shape,dtype,radius", bc.SEAM_CASES)
def test_rolling_ball_across_tiles_and_lane_strides(shape, dtype, radius):
    img, want = _seam_case(shape, dtype, radius)
    _assert_same(estimate_background_rolling_ball(img, radius), want)


@pytest.mark.parametrize("shape,dtype,radius", bc.SEAM_DEVICE_CASES)
def test_rolling_ball_across_tiles_on_the_device_entry(shape, dtype, radius):
    img, want = _seam_case(shape, dtype, radius)
    res, bg = _on_device("rolling_ball", img, radius, clip=False)
    _assert_same(bg, want)
    _assert_same(res, img - want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_rolling_ball_planted_pixels_reach_across_every_seam(dtype):
    level, radius = bc.PLANTED_LEVEL, bc.PLANTED_RADIUS
    every = [(y, x) for y in bc.PLANTED_ROWS for x in bc.PLANTED_COLS]
    for pixels in [[p] for p in every] + [every]:
        img = bc.planted_frame(pixels, dtype)
        want = bo.rolling_ball(img, radius)
        if len(pixels) == 1:
            # the case's own conditioning: one low pixel only, so every output below the level is below it because of that
            # pixel -- and the outputs across the row seam, across the column seam and across both are
            (y, x), = pixels
            ya, xa = sum(bc.PLANTED_ROWS) - y, bc.PLANTED_ACROSS[x]
            assert y // bc.RB_TH != ya // bc.RB_TH
            assert x in (0, 512) or x // bc.RB_LANES != xa // bc.RB_LANES
            assert want[ya, x] < level and want[y, xa] < level and want[ya, xa] < level
        _assert_same(estimate_background_rolling_ball(img, radius), want)
    res, bg = _on_device("rolling_ball", img, radius)
    _assert_same(bg, want)
    _assert_same(res, _residual(img, want, True))


def test_rolling_ball_uint16_truncates_past_the_first_lane_stride():
    img = bc.frame((17, 257), np.uint16, seed=21)
    want = bo.rolling_ball(img, 6)
    exact = bo.rolling_ball(img.astype(np.float64), 6)
    for lo in (64, 128, 192, 256):                      # the lane's outputs u = 1, 2, 3 and the second tile had fractions to drop
        assert np.any(exact[:, lo:lo + 64] != np.trunc(exact[:, lo:lo + 64]))
    residual, background = remove_background_rolling_ball(img, 6)
    _assert_same(background, want)
    _assert_same(residual, np.clip(img - want, 0, None))
    res, bg = _on_device("rolling_ball", img, 6)
    _assert_same(bg, want)
    _assert_same(res, residual)


# ------------------------------------------------------------------------------------------------ B: radius limits
@functools.lru_cache(maxsize=None)
def _cap_case(dtype, radius, planted):
    img = (np.random.default_rng(22).random(bc.CAP_SHAPE) * bc.CAP_SCALE).astype(dtype)
    if planted:
        img[bc.CAP_PLANTED_AT] = -bc.CAP_SCALE / 50        # below every pixel by twice the table's largest difference
    want, source = bo.rolling_ball_dense(img, radius, return_source=True)
    return _frozen(img), _frozen(want), _frozen(source)


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("radius", bc.CAP_RADII)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rolling_ball_at_the_radius_cap(dtype, radius, planted):
    img, want, source = _cap_case(dtype, radius, planted)
    assert np.ptp(img) > 50 * (bc.RB_MAX_R - np.sqrt(bc.RB_MAX_R ** 2 - 299 ** 2))
    # far pixels win: outputs take their minimum from beyond the lane stride and from the other tile, a few low pixels between
    # them on the random frame; on the planted one the far corner's pixel wins everywhere, each offset's difference on show
    columns = np.arange(bc.CAP_SHAPE[1])[None, :]
    reach = np.abs(source % bc.CAP_SHAPE[1] - columns)
    assert np.any(source % bc.CAP_SHAPE[1] // bc.RB_TW != columns // bc.RB_TW)
    if planted:
        assert reach.max() > bc.RB_TW and len(np.unique(source)) == 1 and len(np.unique(want)) > want.size // 2
    else:
        assert reach.max() > bc.RB_LANES and len(np.unique(source)) > 1 and np.count_nonzero(reach > bc.RB_LANES) > reach.size // 4
    _assert_same(estimate_background_rolling_ball(img, radius), want)
    if radius == bc.RB_MAX_R:
        res, bg = _on_device("rolling_ball", img, radius)
        _assert_same(bg, want)
        _assert_same(res, _residual(img, want, True))


@pytest.mark.parametrize("radius", bc.TINY_RADII)
@pytest.mark.parametrize("dtype", [np.float64, np.float32, np.uint8])
def test_rolling_ball_below_one_pixel_is_the_image(dtype, radius):
    img = bc.frame((15, 255), dtype, seed=23)
    _assert_same(bo.rolling_ball(img, radius), img)      # so says the restatement: the ball holds its centre only
    residual, background = remove_background_rolling_ball(img, radius)
    _assert_same(background, img)
    _assert_same(residual, np.zeros_like(img))
    res, bg = _on_device("rolling_ball", img, radius)
    _assert_same(bg, img)
    _assert_same(res, np.zeros_like(img))


def test_rolling_ball_radii_beyond_the_cap_are_refused():
    from mtflearn_amd.distributed import remove_background_device
    lib = _native.load()
    img = bc.frame((9, 20), np.float32, seed=24)
    dev = _native.DeviceArray.from_numpy(img)
    want = bo.rolling_ball(img, 3)
    for radius in bc.REFUSED_RADII:
        for call in (lambda: estimate_background_rolling_ball(img, radius), lambda: remove_background_rolling_ball(img, radius),
                     lambda: remove_background_device(dev, "rolling_ball", radius)):
            with pytest.raises(ValueError, match="radius must be finite and at most 1536 pixels on the device"):
                call()
        out = np.full(img.shape, 7, np.float32)
        code = lib.zk_background_rolling_ball(_native.default_device(), img.ctypes.data_as(c_void_p), _native.ZK_F32, 9, 20,
                                              c_double(radius), 0, out.ctypes.data_as(c_void_p), None)
        assert code == _native.ZK_E_BADARG and "radius must be in (0, 1536]" in _native.last_error()
        assert np.all(out == 7)
        # the next valid call is served
        _assert_same(estimate_background_rolling_ball(img, 3), want)
        _assert_same(remove_background_device(dev, "rolling_ball", 3)[1].numpy(), want)


# ------------------------------------------------------------------------------------------------ C: non-finite pixels
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rolling_ball_skips_nan_sums(dtype):
    radius = bc.NONFINITE_RADIUS
    img = bc.rolling_ball_nonfinite_frame(dtype)
    want = bo.rolling_ball(img, radius, skip_nan=True)
    # conditioning: the output that sees the -inf pixel off the ball but inside its wave's widest chord stays finite, the output
    # three rows down in the same wave takes it; the +inf pixel and the lone NaN are passed over; the NaN patch's centre has no sum
    assert np.isfinite(want[bc.OFF_BALL_OUTPUT]) and want[bc.ON_BALL_OUTPUT] == -np.inf
    assert bc.OFF_BALL_OUTPUT[0] // 4 == bc.ON_BALL_OUTPUT[0] // 4
    assert np.isfinite(want[bc.PLUS_INF_AT]) and np.isfinite(want[bc.NAN_AT]) and want[bc.NAN_PATCH_CENTRE] == np.inf
    assert np.count_nonzero(want == np.inf) == 1 and not np.isnan(want).any()
    assert np.isnan(bo.rolling_ball(img, radius)).sum() > 100            # np.minimum would have spread the NaN
    _assert_same(estimate_background_rolling_ball(img, radius), want)
    for clip in (True, False):
        residual, background = remove_background_rolling_ball(img, radius, clip=clip)
        _assert_same(background, want)
        _assert_same(residual, _residual(img, want, clip))
        res, bg = _on_device("rolling_ball", img, radius, clip=clip)
        _assert_same(bg, want)
        _assert_same(res, residual)
    assert np.isnan(residual).sum() >= 170                               # the NaN pixels, and inf - inf at the patch's centre


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rolling_ball_all_nan_frame_is_plus_inf(dtype):
    img = np.full((5, 5), np.nan, dtype=dtype)
    want = np.full((5, 5), np.inf, dtype=dtype)
    _assert_same(bo.rolling_ball(img, bc.NONFINITE_RADIUS, skip_nan=True), want)
    residual, background = remove_background_rolling_ball(img, bc.NONFINITE_RADIUS)
    _assert_same(background, want)
    _assert_same(residual, img)
    _assert_same(_on_device("rolling_ball", img, bc.NONFINITE_RADIUS)[1], want)


@pytest.mark.parametrize("size", bc.OPENING_INF_SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_opening_infinite_pixels(dtype, size):
    img = bc.opening_inf_frame(dtype)
    want = ndimage.grey_opening(img, size=size)
    assert np.isposinf(want).any() and np.isneginf(want).any() and not np.isnan(want).any()
    for clip in (True, False):
        residual, background = remove_background_opening(img, size, clip=clip)
        _assert_same(background, want)
        _assert_same(residual, _residual(img, want, clip))
    res, bg = _on_device("opening", img, size, clip=False)
    _assert_same(bg, want)
    _assert_same(res, residual)


@pytest.mark.parametrize("num_iters", bc.BASELINE_NONFINITE_ITERS)
@pytest.mark.parametrize("sigma", bc.BASELINE_NONFINITE_SIGMAS)
@pytest.mark.parametrize("kind", list(bc.BASELINE_NONFINITE_PIXELS))
def test_baseline_non_finite_pixels(kind, sigma, num_iters):
    img = bc.baseline_nonfinite_frame(kind)
    want = _scipy_baseline(img, sigma, num_iters)
    assert not np.isfinite(want).all()
    if sigma == 3 and kind in ("nan", "together"):
        # np.minimum keeps a NaN from either side: finite pixels under a NaN filter value come out NaN
        assert np.count_nonzero(np.isnan(want) & np.isfinite(img)) > 100
    _assert_same(estimate_background_baseline(img, sigma=sigma, num_iters=num_iters), want)
    for clip in (True, False):
        residual, background = remove_background_baseline(img, sigma=sigma, num_iters=num_iters, clip=clip)
        _assert_same(background, want)
        _assert_same(residual, _residual(img, want, clip))
    res, bg = _on_device("baseline", img, sigma, clip=False, num_iters=num_iters)
    _assert_same(bg, want)
    _assert_same(res, residual)


# ------------------------------------------------------------------------------------------------ D: long axes
@pytest.mark.parametrize("name,method,parameter,shape,dtype,axis,rows_per_block", bc.LONG_AXIS_CASES,
                         ids=[c[0] for c in bc.LONG_AXIS_CASES])
def test_axes_of_more_than_65535_row_blocks(name, method, parameter, shape, dtype, axis, rows_per_block):
    assert -(-shape[axis] // rows_per_block) == bc.GRID_Y_BLOCKS
    img = bc.frame(shape, dtype, seed=25)
    kw = {"num_iters": 2} if method == "baseline" else {}
    if method == "baseline":
        want = _scipy_baseline(img, parameter, 2)
    elif method == "opening":
        want = ndimage.grey_opening(img, size=(parameter, parameter) if np.isscalar(parameter) else parameter)
    else:
        want = bo.rolling_ball(img, parameter)
    assert name == "opening_transpose" or np.any(want != img)     # a window of 2 on an axis of 1 pixel: the whole period
    residual, background = HOST_REMOVE[method](img, parameter, clip=False, **kw)
    _assert_same(background, want)
    _assert_same(residual, _residual(img, want, False))
    res, bg = _on_device(method, img, parameter, clip=False, **kw)
    _assert_same(bg, want)
    _assert_same(res, residual)


# ------------------------------------------------------------------------------------------------ E: residual second sweep
@pytest.mark.parametrize("dtype", bc.RESIDUAL_DTYPES)
def test_residual_second_sweep(dtype):
    img = bc.residual_frame(dtype)
    assert img.size > bc.RESIDUAL_THREADS
    want = ndimage.grey_opening(img, size=(3, 3))
    wrapped = img - want
    assert np.any(wrapped.ravel()[bc.RESIDUAL_THREADS:] != 0)                     # the second sweep has something to write
    if dtype == "int16":
        assert np.any(wrapped < 0) and np.all(img.astype(np.int64) - want >= 0)   # the difference wraps as NumPy's does
    for clip, want_res in ((True, np.clip(wrapped, 0, None)), (False, wrapped)):
        residual, background = remove_background_opening(img, size=3, clip=clip)
        _assert_same(background, want)
        _assert_same(residual, want_res)
    res, bg = _on_device("opening", img, 3, clip=False)
    _assert_same(bg, want)
    _assert_same(res, wrapped)
    base = _scipy_baseline(img, 1, 1)
    residual, background = remove_background_baseline(img, sigma=1, num_iters=1)
    _assert_same(background, base)
    _assert_same(residual, np.clip(img.astype(np.float64) - base, 0, None))
    assert np.any(residual[-1] > 0) and np.any(residual[0] > 0)


# ------------------------------------------------------------------------------------------------ F: baseline blocks and folds
@pytest.mark.parametrize("shape,sigma", bc.BASELINE_BLOCK_CASES)
def test_baseline_past_one_block_and_folded_twice(shape, sigma):
    img = bc.frame(shape, np.float64, seed=26)
    want = _scipy_baseline(img, sigma, 2)
    residual, background = remove_background_baseline(img, sigma=sigma, num_iters=2)
    _assert_same(background, want)
    _assert_same(residual, np.clip(img - want, 0, None))
    res, bg = _on_device("baseline", img, sigma, num_iters=2)
    _assert_same(bg, want)
    _assert_same(res, residual)


# ------------------------------------------------------------------------------------------------ G: opening segments
@pytest.mark.parametrize("dtype", [np.float64, np.uint8])
@pytest.mark.parametrize("shape", bc.OPENING_SEGMENT_SHAPES)
def test_opening_whole_segments_past_one_block(shape, dtype):
    img = bc.frame(shape, dtype, seed=27)
    for size in bc.OPENING_SEGMENT_SIZES:
        want = ndimage.grey_opening(img, size=size)
        _assert_same(estimate_background_opening(img, size), want)
    res, bg = _on_device("opening", img, size)
    _assert_same(bg, want)
    _assert_same(res, np.clip(img - want, 0, None))


@pytest.mark.parametrize("dtype", [np.float64, np.uint8])
@pytest.mark.parametrize("n", bc.OPENING_FOLD_LENGTHS)
@pytest.mark.parametrize("axis", [0, 1])
def test_opening_windows_around_one_and_two_frame_lengths(axis, n, dtype):
    shape = (n, 70) if axis == 0 else (70, n)
    img = bc.frame(shape, dtype, seed=28)
    for k in bc.fold_windows(n):
        size = (k, 3) if axis == 0 else (3, k)
        want = ndimage.grey_opening(img, size=size)
        _assert_same(estimate_background_opening(img, size), want)
    _assert_same(_on_device("opening", img, size)[1], want)
