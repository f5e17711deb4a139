"""mtflearn_amd.background on the GPU: the opening against scipy.ndimage.grey_opening and the baseline against the
reference's loop on SciPy, both exactly; the rolling ball against the test-local restatement of scikit-image's algorithm
(tests/background_oracle.py), exactly; residuals, dtypes, and the device-resident chain into local_max."""
import numpy as np
import pytest
from scipy import ndimage

import background_oracle as bo
from mtflearn_amd import ZPs, _native
from mtflearn_amd.background import (estimate_background_baseline, estimate_background_opening,
                                     estimate_background_rolling_ball, remove_background_baseline,
                                     remove_background_opening, remove_background_rolling_ball)
from mtflearn_amd.features import local_max
from mtflearn_amd.synthetic import honeycomb_frame

pytestmark = pytest.mark.gpu

DEVICE_DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)


def _frame(shape, dtype, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.random(shape)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (x * 4 - 1).astype(dtype)
    if dtype == np.int16:
        return (x * 60000 - 30000).astype(dtype)
    return (x * np.iinfo(dtype).max).astype(dtype)


def _ramped(h, w, seed=3):
    frame = honeycomb_frame(h, w, seed=seed).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    return (frame + 1.5 * xx / w + 0.5 * yy / h).astype(np.float32)


# ------------------------------------------------------------------------------------------------ opening
@pytest.mark.parametrize("size", [1, 2, 3, 4, 15, 41, (15, 6), (60, 7), (3, 1), (1, 5)])
def test_opening_matches_scipy(size):
    img = _frame((37, 29), np.float64, seed=1)
    sz = (size, size) if np.isscalar(size) else size
    np.testing.assert_array_equal(estimate_background_opening(img, size), ndimage.grey_opening(img, size=sz))


@pytest.mark.parametrize("shape", [(1, 40), (40, 1), (37, 29), (5, 3)])
@pytest.mark.parametrize("size", [3, 4, (7, 2), 99])
def test_opening_shapes_and_windows_larger_than_the_frame(shape, size):
    img = _frame(shape, np.float32, seed=2)
    sz = (size, size) if np.isscalar(size) else size
    np.testing.assert_array_equal(estimate_background_opening(img, size), ndimage.grey_opening(img, size=sz))


@pytest.mark.parametrize("dtype", DEVICE_DTYPES)
def test_opening_dtypes_and_residual(dtype):
    img = _frame((64, 71), dtype, seed=3)
    residual, background = remove_background_opening(img, size=(9, 6))
    want_bg = ndimage.grey_opening(img, size=(9, 6))
    want_res = np.clip(img - want_bg, 0, None)
    assert background.dtype == img.dtype and residual.dtype == want_res.dtype
    np.testing.assert_array_equal(background, want_bg)
    np.testing.assert_array_equal(residual, want_res)
    res_nc, _ = remove_background_opening(img, size=5, clip=False)
    np.testing.assert_array_equal(res_nc, img - ndimage.grey_opening(img, size=(5, 5)))


def test_opening_strided_view_and_widened_dtypes():
    base = _frame((90, 120), np.float64, seed=4)
    view = base[::2, 1::3]
    np.testing.assert_array_equal(estimate_background_opening(view, 7), ndimage.grey_opening(view, size=(7, 7)))
    for dtype in (np.int32, np.int8, np.int64):
        img = _frame((33, 40), np.int16, seed=5).astype(dtype)
        got_res, got = remove_background_opening(img, size=5)
        want = ndimage.grey_opening(img, size=(5, 5))
        assert got.dtype == img.dtype and got_res.dtype == img.dtype
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got_res, np.clip(img - want, 0, None))


@pytest.mark.parametrize("n", [2048, 4096])
def test_opening_full_frames(n):
    img = _ramped(n, n, seed=n)
    np.testing.assert_array_equal(estimate_background_opening(img, 41), ndimage.grey_opening(img, size=(41, 41)))
    if n == 2048:
        np.testing.assert_array_equal(estimate_background_opening(img, (25, 8)), ndimage.grey_opening(img, size=(25, 8)))


# ------------------------------------------------------------------------------------------------ baseline
def _reference_baseline(image, sigma, num_iters):
    image = np.asarray(image, dtype=float)
    out = np.minimum(ndimage.gaussian_filter(image, sigma=sigma), image)
    for _ in range(num_iters - 1):
        out = np.minimum(ndimage.gaussian_filter(out, sigma=sigma), image)
    return out


@pytest.mark.parametrize("sigma", [0.5, 3, 20, (2.5, 7), (0, 5), (4, 0), 0])
@pytest.mark.parametrize("num_iters", [1, 4, 10])
def test_baseline_matches_scipy_bit_for_bit(sigma, num_iters):
    img = _frame((40, 53), np.float64, seed=6)
    got = estimate_background_baseline(img, sigma=sigma, num_iters=num_iters)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, _reference_baseline(img, sigma, num_iters))


@pytest.mark.parametrize("dtype", DEVICE_DTYPES)
def test_baseline_dtypes_small_frames_and_residual(dtype):
    img = _frame((32, 32), dtype, seed=7)
    residual, background = remove_background_baseline(img, sigma=20, num_iters=3)   # radius 80 > the frame
    want = _reference_baseline(img, 20, 3)
    np.testing.assert_array_equal(background, want)
    assert residual.dtype == np.float64
    np.testing.assert_array_equal(residual, np.clip(img.astype(np.float64) - want, 0, None))
    res_nc, _ = remove_background_baseline(img[::3, ::2], sigma=(1.5, 4), num_iters=2, clip=False)
    np.testing.assert_array_equal(res_nc, img[::3, ::2].astype(np.float64) - _reference_baseline(img[::3, ::2], (1.5, 4), 2))


def test_baseline_full_frame():
    img = _ramped(2048, 2048, seed=9)
    np.testing.assert_array_equal(estimate_background_baseline(img, sigma=30, num_iters=2), _reference_baseline(img, 30, 2))


# ------------------------------------------------------------------------------------------------ rolling ball
@pytest.mark.parametrize("radius", [1, 2.5, 6, 20, 60])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rolling_ball_matches_the_restatement(radius, dtype):
    img = _frame((70, 90), dtype, seed=10)
    got = estimate_background_rolling_ball(img, radius=radius)
    assert got.dtype == img.dtype
    np.testing.assert_array_equal(got, bo.rolling_ball(img, radius))


def test_rolling_ball_float32_stays_float32():
    # float64 sums would round differently from float32 ones on some pixels of this frame
    rng = np.random.default_rng(11)
    img = (rng.random((48, 40)) * 1000).astype(np.float32)
    got = estimate_background_rolling_ball(img, radius=7.3)
    want32 = bo.rolling_ball(img, 7.3)
    want64 = bo.rolling_ball(img.astype(np.float64), 7.3).astype(np.float32)
    np.testing.assert_array_equal(got, want32)
    assert not np.array_equal(want32, want64)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int16])
def test_rolling_ball_integer_types_truncate(dtype):
    img = _frame((50, 61), dtype, seed=12)
    residual, background = remove_background_rolling_ball(img, radius=6)
    want = bo.rolling_ball(img, 6)
    assert background.dtype == img.dtype and residual.dtype == img.dtype
    np.testing.assert_array_equal(background, want)
    np.testing.assert_array_equal(residual, np.clip(img - want, 0, None))
    # the float64 result had fractions: the cast back truncated them
    exact = bo.rolling_ball(img.astype(np.float64), 6)
    assert np.any(exact != np.trunc(exact))


@pytest.mark.parametrize("shape", [(40, 50), (1, 33), (33, 1)])
def test_rolling_ball_larger_than_the_frame(shape):
    img = _frame(shape, np.float64, seed=13)
    np.testing.assert_array_equal(estimate_background_rolling_ball(img, radius=60), bo.rolling_ball(img, 60))


def test_rolling_ball_strided_view():
    base = _frame((80, 99), np.float32, seed=14)
    view = base[1::2, ::3]
    np.testing.assert_array_equal(estimate_background_rolling_ball(view, 5.5), bo.rolling_ball(view, 5.5))


def test_rolling_ball_full_frame_sampled():
    img = _ramped(2048, 2048, seed=15).astype(np.float64)
    got = estimate_background_rolling_ball(img, radius=60)
    rng = np.random.default_rng(16)
    pts = np.concatenate([rng.integers(0, 2048, (248, 2)), [[0, 0], [0, 2047], [2047, 0], [2047, 2047], [5, 1000],
                                                             [1000, 5], [2042, 1000], [1000, 2042]]])
    np.testing.assert_array_equal(got[pts[:, 0], pts[:, 1]], bo.rolling_ball_at(img, 60, pts))


# ------------------------------------------------------------------------------------------------ all three
@pytest.mark.parametrize("dtype", DEVICE_DTYPES)
def test_constant_image_is_preserved(dtype):
    img = np.full((16, 16), 0.25 if np.dtype(dtype).kind == "f" else 7, dtype=dtype)
    for residual, background in (remove_background_opening(img, size=5), remove_background_rolling_ball(img, radius=4),
                                 remove_background_baseline(img, sigma=2, num_iters=3)):
        np.testing.assert_array_equal(background, img)
        np.testing.assert_array_equal(residual, np.zeros_like(residual))
        assert np.all(residual >= 0) and np.all(background <= img)


# ------------------------------------------------------------------------------------------------ device chain
@pytest.mark.parametrize("method,param", [("opening", 25), ("rolling_ball", 24), ("baseline", 8)])
@pytest.mark.parametrize("kind", ["native", "torch"])
def test_device_chain_matches_the_host_chain(method, param, kind):
    from mtflearn_amd.distributed import local_max_device, points_moments_device, remove_background_device
    remove = {"opening": remove_background_opening, "rolling_ball": remove_background_rolling_ball,
              "baseline": remove_background_baseline}[method]
    frame = _ramped(384, 320, seed=17)
    kw = {"num_iters": 3} if method == "baseline" else {}
    want_res, want_bg = remove(frame, param, **kw)
    want_pts = local_max(want_res, 5, threshold=0.3)
    z = ZPs(8, 24)
    plan = z._device_plan()
    want = z.transform_at(want_res, want_pts).data
    if kind == "native":
        img = _native.DeviceArray.from_numpy(frame, device=plan.device)
        res, bg = remove_background_device(img, method, param, **kw)
        pts = local_max_device(res, 5, threshold=0.3)
        mom = points_moments_device(plan, res, pts).numpy()
        res, bg, pts = res.numpy(), bg.numpy(), pts.numpy()
    else:
        torch = pytest.importorskip("torch")
        img = torch.from_numpy(frame).to(f"cuda:{plan.device}")
        res, bg = remove_background_device(img, method, param, **kw)
        assert res.is_cuda and bg.is_cuda
        pts = local_max_device(res, 5, threshold=0.3)
        mom = points_moments_device(plan, res, pts)
        torch.cuda.synchronize()
        res, bg, mom, pts = res.cpu().numpy(), bg.cpu().numpy(), mom.cpu().numpy(), pts.cpu().numpy()
    np.testing.assert_array_equal(bg, want_bg)
    np.testing.assert_array_equal(res, want_res)
    np.testing.assert_array_equal(pts, want_pts)
    np.testing.assert_allclose(mom, want, rtol=1e-12, atol=1e-15 * np.abs(want).max())
    # the background decides which columns are found: removing it changes the key points
    raw = local_max(frame, 5, threshold=0.3)
    assert len(want_pts) > 0 and (len(raw) != len(want_pts) or not np.array_equal(raw, want_pts))


def test_device_entry_checks():
    from mtflearn_amd.distributed import remove_background_device
    img = _native.DeviceArray.from_numpy(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match="method must be one of"):
        remove_background_device(img, "tophat", 3)
    with pytest.raises(ValueError, match="size must be a positive integer."):
        remove_background_device(img, "opening", 0)
    with pytest.raises(ValueError, match="num_iters must be positive."):
        remove_background_device(img, "baseline", 2, num_iters=0)
    with pytest.raises(TypeError):
        remove_background_device(img, "opening", 3, num_iters=2)
