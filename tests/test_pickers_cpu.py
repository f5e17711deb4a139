"""Parameter pickers, CPU side: the oracle restatement (oracle/pickers_oracle.py) against goldens captured from the
reference's own code, and the product's host-only pieces (peak search, noise model, wavelet noise estimate)."""
import os

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def pg():
    with np.load(os.path.join(ROOT, "tests", "golden", "pickers_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def po():
    from oracle import pickers_oracle
    return pickers_oracle


def test_oracle_autocorrelation_matches_reference(pg, po):
    np.testing.assert_allclose(po.standardize_image(pg["win_64"]), pg["std_win_64"], rtol=1e-12, atol=1e-12)
    for key_in, key_out, std in (("win_64", "autocorr_64", True), ("win_64", "autocorr_64_raw", False), ("win_33", "autocorr_33", True)):
        got = po.autocorrelation(pg[key_in], standardize=std)
        np.testing.assert_allclose(got, pg[key_out], rtol=1e-10, atol=1e-9 * np.abs(pg[key_out]).max())
    got = po.autocorr_mean(pg["noisy_192"], 96, pg["origins_96"])
    np.testing.assert_allclose(got, pg["autocorr_mean_96"], rtol=1e-10, atol=1e-9 * np.abs(got).max())
    with pytest.raises(ValueError, match="Standard deviation is zero"):
        po.standardize_image(np.ones((4, 4)))


def test_oracle_and_product_peak_search_match_reference(pg, po):
    from mtflearn_amd.features import pickers
    for impl in (po.find_highest_peak, pickers.find_highest_peak):
        peak, peaks, props = impl(pg["profile_a"], max_distance=len(pg["profile_a"]))
        assert peak == int(pg["profile_a_peak"])
        np.testing.assert_array_equal(peaks, pg["profile_a_all"])
        np.testing.assert_allclose(props["prominences"], pg["profile_a_prominences"], rtol=1e-12)
        np.testing.assert_allclose(props["widths"], pg["profile_a_widths"], rtol=1e-12)
        peak, peaks, _ = impl(pg["profile_flat"], max_distance=len(pg["profile_flat"]))
        assert (peak is None) == (int(pg["profile_flat_found"]) == 0) and (peaks is None) == (peak is None)
        peak, peaks, _ = impl(pg["profile_c"], min_distance=5, max_distance=len(pg["profile_c"]))
        assert (-1 if peak is None else peak) == int(pg["profile_c_peak"])
        np.testing.assert_array_equal([] if peaks is None else peaks, pg["profile_c_all"])


def test_oracle_denoise_fft_matches_reference(pg, po):
    for k in ("", "_f32"):
        got = po.denoise_fft(pg["denoise_in" + k], float(pg["denoise_p" + k]))
        np.testing.assert_allclose(got, pg["denoise_out" + k], rtol=1e-9, atol=1e-9 * np.abs(pg["denoise_out" + k]).max())


def test_noise_model_matches_reference(pg, po):
    from mtflearn_amd.features import pickers
    for impl in (po.add_gaussian_noise, pickers.add_gaussian_noise):
        got = impl(pg["lattice_192"], sigma=0.2, seed=5)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, pg["noisy_192"])
    with pytest.raises(ValueError, match="non-negative"):
        pickers.add_gaussian_noise(pg["lattice_192"], sigma=-1)


def test_oracle_wavelet_noise_estimate_tracks_sigma(pg, po):
    """estimate_sigma is restated from scikit-image / PyWavelets (parity unpinned): on white noise of known sigma the
    estimate is the sigma, and it separates the clean lattice from its noisy twin."""
    rng = np.random.default_rng(1)
    noise = 0.37 * rng.standard_normal((512, 512))
    assert abs(po.estimate_sigma(noise) - 0.37) < 0.01
    assert po.estimate_sigma(pg["lattice_192"]) < 0.01 < po.estimate_sigma(pg["noisy_192"])


POLAR_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (257, 131), (181, 181), (182, 182), (1024, 1024)]


@pytest.mark.parametrize("shape", POLAR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_scipy_warp_polar_agrees_with_restated_warp_polar(po, shape):
    """tests/pickers_reference.py resamples with scipy.ndimage.map_coordinates, the oracle with its own floor / ceil
    bilinear code; neither is scikit-image (not installed), but an error would have to be made twice, differently.
    Measured: at most 1e-13 up to 64 x 64 (|data| 1.5 to 3), 5e-13 at 257 x 131, 2.3e-12 at 1024 x 1024."""
    import pickers_reference as pr
    rng = np.random.default_rng(21)
    h, w = shape
    tol = 1e-11 if h * w > 257 * 257 else 1e-12
    for data in (rng.random(shape) + 0.5, rng.standard_normal(shape)):        # fill value 0 outside / inside the range
        for center in (None, (0, 0), (h - 1, w - 1), (h // 3, (w // 2 + 1) % w)):
            got = pr.warp_polar_ref(data, center)
            ref = po.warp_polar_linear(data, (h // 2, w // 2) if center is None else center)
            assert got.shape == ref.shape == (360, pr.polar_radii(h, w))
            np.testing.assert_allclose(got, ref, rtol=0, atol=tol)


def test_direct_lag_sum_agrees_with_oracle_autocorrelation(po):
    import pickers_reference as pr
    rng = np.random.default_rng(22)
    img = rng.standard_normal((131, 260))
    for ws in (1, 2, 3, 8, 31, 33, 50):
        origins = [(0, 0), (131 - ws, 260 - ws), (0, 260 - ws), (131 - ws, 0), (17, 101)]
        for standardize in (True, False) if ws > 1 else (False,):
            got = pr.autocorr_mean_ref(img, ws, origins, standardize)
            ref = po.autocorr_mean(img, ws, origins, standardize)
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    flat = img.copy()
    flat[40:48, 60:68] = 3.0
    with pytest.raises(ValueError, match="Standard deviation is zero"):
        pr.autocorr_mean_ref(flat, 8, [(0, 0), (40, 60)], True)


def test_extended_precision_power_spectrum_agrees_with_oracle(po):
    import pickers_reference as pr
    rng = np.random.default_rng(23)
    img = rng.standard_normal((260, 300))
    for size in (1, 2, 3, 8, 31, 33, 48, 64, 97, 100, 255):
        y, x = 260 - size, 7 if size < 255 else 0
        patch = img[y:y + size, x:x + size]
        for name in ("hann", None):
            ref = po.cumulative_energy(patch, window_type=name)[2]
            got = pr.power_spectra_ref(img, size, [(y, x)], pr.window_ref(name, size))[0]
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12 * max(ref.max(), np.finfo(float).tiny))
    for name, fn in (("hanning", np.hanning), ("hamming", np.hamming), ("blackman", np.blackman)):   # the reference's calls
        for size in (1, 2, 8, 33, 64):
            np.testing.assert_allclose(pr.window_ref(name, size), fn(size), rtol=0, atol=1e-15)
    from scipy.signal import windows
    for size in (1, 2, 8, 33, 64):
        np.testing.assert_allclose(pr.window_ref("tukey", size), windows.tukey(size, alpha=0.5), rtol=0, atol=1e-15)


def test_picker_argument_errors_need_no_device():
    from mtflearn_amd.features import pickers
    with pytest.raises(ValueError, match="Invalid method 'median'"):
        pickers.radial_profile(np.zeros((8, 8)), method="median")
    with pytest.raises(TypeError, match="numpy array"):
        pickers.denoise_fft([[1.0, 2.0]], 0.5)
    with pytest.raises(ValueError, match="2D array"):
        pickers.denoise_fft(np.zeros(4), 0.5)
    with pytest.raises(ValueError, match="between 0 and 1"):
        pickers.denoise_fft(np.zeros((4, 4)), 0.0)
    with pytest.raises(ValueError, match="too large for image"):
        pickers.estimate_patch_size(np.zeros((16, 16)), window_size=32)
    with pytest.raises(ValueError, match="Unknown window type"):
        pickers._window_1d("kaiser", 8)
