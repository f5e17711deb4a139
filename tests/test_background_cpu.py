"""mtflearn_amd.background without a GPU: the public names, the reference's argument checks and parameter picker, and the
test-local restatements (tests/background_oracle.py) against SciPy, the oracles the GPU tests lean on."""
import numpy as np
import pytest
from scipy import ndimage

import background_oracle as bo
import mtflearn_amd.background as bg
from mtflearn_amd.background import (estimate_background_baseline, estimate_background_opening,
                                     estimate_background_rolling_ball, estimate_characteristic_spacing,
                                     remove_background_baseline, remove_background_opening, remove_background_rolling_ball,
                                     select_background_parameter, suggest_background_parameters)


@pytest.fixture
def synthetic_image():
    image = np.zeros((32, 32), dtype=float)
    image += np.linspace(0.0, 0.5, 32)[None, :]
    image[10, 10] = 2.0
    image[21, 18] = 1.5
    return image


def test_public_names():
    expected = {"estimate_background_opening", "remove_background_opening", "estimate_background_rolling_ball",
                "remove_background_rolling_ball", "estimate_background_baseline", "remove_background_baseline",
                "estimate_characteristic_spacing", "suggest_background_parameters", "select_background_parameter"}
    assert expected <= set(dir(bg))
    assert expected == set(bg.__all__)
    from mtflearn_amd.distributed import remove_background_device
    assert callable(remove_background_device)


def test_non_2d_input_is_rejected():
    for fn in (estimate_background_opening, remove_background_opening, estimate_background_rolling_ball,
               remove_background_rolling_ball, estimate_background_baseline, remove_background_baseline,
               estimate_characteristic_spacing):
        with pytest.raises(ValueError, match="image must be a 2D array."):
            fn(np.ones((4, 4, 2)))
    with pytest.raises(ValueError, match="image must be a 2D array."):
        suggest_background_parameters(np.ones(5), spacing=3)


def test_invalid_parameters_raise_the_reference_messages(synthetic_image):
    with pytest.raises(ValueError, match="size must be a positive integer."):
        estimate_background_opening(synthetic_image, size=0)
    with pytest.raises(ValueError, match="size must be a positive int or a length-2 tuple."):
        estimate_background_opening(synthetic_image, size=(3, 0))
    with pytest.raises(ValueError, match="size must be a positive int or a length-2 tuple."):
        remove_background_opening(synthetic_image, size=(3, 3, 3))
    for r in (0, -2.5):
        with pytest.raises(ValueError, match="radius must be positive."):
            estimate_background_rolling_ball(synthetic_image, radius=r)
        with pytest.raises(ValueError, match="radius must be positive."):
            remove_background_rolling_ball(synthetic_image, radius=r)
    for n in (0, -1):
        with pytest.raises(ValueError, match="num_iters must be positive."):
            estimate_background_baseline(synthetic_image, sigma=3, num_iters=n)
        with pytest.raises(ValueError, match="num_iters must be positive."):
            remove_background_baseline(synthetic_image, sigma=3, num_iters=n)


def test_suggest_background_parameters(synthetic_image):
    assert suggest_background_parameters(synthetic_image, spacing=20) == {
        "spacing": 20.0, "opening_size": 41, "rolling_ball_radius": 60, "baseline_sigma": 30.0}
    # an even opening size goes up to the next odd number
    assert suggest_background_parameters(synthetic_image, spacing=12.25)["opening_size"] == 25
    assert suggest_background_parameters(synthetic_image, spacing=12)["opening_size"] == 25
    # the floors: 3, 3 and 1.0
    small = suggest_background_parameters(synthetic_image, spacing=0.2)
    assert small == {"spacing": 0.2, "opening_size": 3, "rolling_ball_radius": 3, "baseline_sigma": 1.0}
    with pytest.raises(ValueError, match="spacing must be positive"):
        suggest_background_parameters(synthetic_image, spacing=0)
    custom = suggest_background_parameters(synthetic_image, spacing=10, opening_factor=1.0, rolling_ball_factor=2.0,
                                           baseline_factor=0.5)
    assert custom == {"spacing": 10.0, "opening_size": 11, "rolling_ball_radius": 20, "baseline_sigma": 5.0}


def test_select_background_parameter(synthetic_image):
    assert select_background_parameter("opening", synthetic_image, spacing=20) == 41
    assert select_background_parameter("rolling_ball", synthetic_image, spacing=20) == 60
    assert select_background_parameter("baseline", synthetic_image, spacing=20) == 30.0
    assert select_background_parameter("Rolling_Ball", synthetic_image, spacing=20) == 60
    with pytest.raises(ValueError, match="method must be one of"):
        select_background_parameter("unknown", synthetic_image, spacing=20)


def test_characteristic_spacing_restores_the_global_random_state(monkeypatch):
    import mtflearn_amd.features.pickers as pickers
    draws = []

    def fake(image, window_size=None, n_samples=None, **kw):
        draws.append(np.random.randint(0, 1 << 30))
        return 12
    monkeypatch.setattr(pickers, "estimate_patch_size", fake)
    np.random.seed(123)
    before = np.random.get_state()[1].copy()
    assert estimate_characteristic_spacing(np.zeros((64, 64)), random_state=7) == 12
    assert estimate_characteristic_spacing(np.zeros((64, 64)), random_state=7) == 12
    assert draws[0] == draws[1]                             # seeded the same way both times
    np.testing.assert_array_equal(np.random.get_state()[1], before)
    assert suggest_background_parameters(np.zeros((64, 64)))["spacing"] == 12.0


def test_gaussian_weights_are_scipys():
    from scipy.ndimage._filters import _gaussian_kernel1d
    for sigma in (0.5, 1.0, 3, 7, 20, 30.0, 2.5):
        r = int(4.0 * float(sigma) + 0.5)
        full = _gaussian_kernel1d(sigma, 0, r)
        np.testing.assert_array_equal(bg._gaussian_weights(sigma), full[r:])
        np.testing.assert_array_equal(bo.gaussian_weights(sigma), full)
    np.testing.assert_array_equal(bg._gaussian_weights(0), [1.0])
    np.testing.assert_array_equal(bg._gaussian_weights(1e-16), [1.0])


@pytest.mark.parametrize("sigma,shape", [(3, (40, 53)), (20, (40, 53)), ((2.5, 7), (40, 53)), (0.5, (17, 9)),
                                         ((0, 5), (23, 31)), (20, (32, 32)), (4, (1, 30)), (4, (30, 1))])
def test_gaussian_restatement_is_scipy_bit_for_bit(sigma, shape):
    rng = np.random.default_rng(5)
    img = rng.random(shape) * 3 - 1
    np.testing.assert_array_equal(bo.gaussian_filter(img, sigma), ndimage.gaussian_filter(img, sigma))


def test_baseline_restatement_is_the_reference_loop():
    rng = np.random.default_rng(6)
    img = rng.random((29, 41))
    for sigma, iters in ((3, 4), ((2.5, 7), 2), (20, 10)):
        want = np.minimum(ndimage.gaussian_filter(img, sigma), img)
        for _ in range(iters - 1):
            want = np.minimum(ndimage.gaussian_filter(want, sigma), img)
        np.testing.assert_array_equal(bo.baseline(img, sigma, iters), want)


@pytest.mark.parametrize("radius", [1, 2.5, 3, 6, 7.5, 20])
def test_rolling_ball_restatement_is_a_grey_erosion(radius):
    rng = np.random.default_rng(7)
    img = rng.random((45, 38)) * 10
    diff = bo.ball_diff(radius)
    want = ndimage.grey_erosion(img, footprint=np.isfinite(diff), structure=-np.where(np.isfinite(diff), diff, 0),
                                mode="constant", cval=np.inf)
    np.testing.assert_array_equal(bo.rolling_ball(img, radius), want)
    # the brute-force form agrees with the offset-at-a-time form
    pts = [(0, 0), (44, 37), (20, 5), (3, 30)]
    np.testing.assert_array_equal(bo.rolling_ball_at(img, radius, pts), [want[y, x] for y, x in pts])


def test_rolling_ball_restatement_types():
    rng = np.random.default_rng(8)
    img = (rng.random((20, 24)) * 200).astype(np.uint8)
    out = bo.rolling_ball(img, 4)
    assert out.dtype == np.uint8 and np.all(out <= img)
    f32 = rng.random((20, 24)).astype(np.float32)
    assert bo.rolling_ball(f32, 4).dtype == np.float32
    assert bo.ball_diff(4, np.float32).dtype == np.float32
    diff = bo.ball_diff(2.5)
    assert diff.shape == (7, 7) and diff[3, 3] == 0 and np.isinf(diff[0, 0]) and np.isinf(diff[3, 0])


# ------------------------------------------------------------------------------------------------ licences of the oracle forms
# that tests/test_gpu_background_kernels.py leans on
def _finite_frames():
    """The finite frames the rolling-ball restatement is checked on above."""
    rng = np.random.default_rng(7)
    yield rng.random((45, 38)) * 10
    rng = np.random.default_rng(8)
    yield (rng.random((20, 24)) * 200).astype(np.uint8)
    yield rng.random((20, 24)).astype(np.float32)


@pytest.mark.parametrize("radius", [1, 2.5, 3, 6, 7.5, 20])
def test_rolling_ball_skip_nan_is_the_restatement_on_finite_frames(radius):
    for img in _finite_frames():
        got, want = bo.rolling_ball(img, radius, skip_nan=True), bo.rolling_ball(img, radius)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


def test_rolling_ball_skip_nan_by_hand():
    # radius 1: the pixel itself (diff 0) and its four neighbours (diff 1); a NaN sum is skipped
    inf, nan = np.inf, np.nan
    img = np.array([[1.0, 5.0, -inf],
                    [nan, 2.0, 9.0],
                    [7.0, inf, 4.0]])
    want = np.array([[1.0, -inf, -inf],
                     [2.0, 2.0, -inf],
                     [7.0, 3.0, 4.0]])
    for dtype in (np.float64, np.float32):
        got = bo.rolling_ball(img.astype(dtype), 1, skip_nan=True)
        assert got.dtype == dtype
        np.testing.assert_array_equal(got, want.astype(dtype))
    # np.minimum keeps the NaN wherever the ball touches it: the two rules differ exactly there
    np.testing.assert_array_equal(np.isnan(bo.rolling_ball(img, 1)),
                                  [[True, False, False], [True, True, False], [True, False, False]])
    # nothing but NaN sums: +inf
    np.testing.assert_array_equal(bo.rolling_ball(np.full((3, 3), nan), 1, skip_nan=True), np.full((3, 3), inf))


@pytest.mark.parametrize("radius", [1, 2.5, 6, 20])
def test_rolling_ball_dense_is_the_restatement(radius):
    rng = np.random.default_rng(7)
    img = rng.random((45, 38)) * 10
    for frame in (img, img.astype(np.float32), (img * 25).astype(np.uint8)):
        got, want = bo.rolling_ball_dense(frame, radius), bo.rolling_ball(frame, radius)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    got, source = bo.rolling_ball_dense(img, radius, return_source=True)
    np.testing.assert_array_equal(got, bo.rolling_ball(img, radius))
    # the source named for every output gives that output's value, and lies on the ball
    sy, sx = np.divmod(source, img.shape[1])
    yy, xx = np.mgrid[0:45, 0:38]
    assert np.all(np.hypot(sy - yy, sx - xx) <= radius)
    R = int(np.ceil(radius))
    np.testing.assert_array_equal(img[sy, sx] + bo.ball_diff(radius)[sy - yy + R, sx - xx + R], got)


def test_ball_diff_window_is_a_window_of_ball_diff():
    for radius in (0.5, 1, 2.5, 6, 20, 33.5):
        R = int(np.ceil(radius))
        for dtype in (np.float64, np.float32):
            full = bo.ball_diff(radius, dtype)
            for ry, rx in ((R, R), (0, R), (R, 0), (2, 1), (R + 3, R + 5)):
                win = bo.ball_diff_window(radius, dtype, ry, rx)
                assert win.dtype == dtype and win.shape == (2 * ry + 1, 2 * rx + 1)
                padded = np.pad(full, ((max(ry - R, 0),) * 2, (max(rx - R, 0),) * 2), constant_values=np.inf)
                cy, cx = padded.shape[0] // 2, padded.shape[1] // 2
                np.testing.assert_array_equal(win, padded[cy - ry:cy + ry + 1, cx - rx:cx + rx + 1])
