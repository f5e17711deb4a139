"""The Fourier window-size estimators and the angular spectrum average on the GPU against the goldens captured from the
reference (tests/make_golden_window_size.py; tests/test_window_size_cpu.py is their licence).

Tolerances.  Maps (``compute_autocorrelation``, ``fft_power_spectrum``): 1e-9 of max|ref| for float64 inputs, 1e-6 for float32
inputs -- the rule and the reasoning of tests/test_gpu_pickers.py (``close``, ``F32_TOL``).  Cut profiles and ``y2``: 1e-9 of
max|ref| for every float64 input (they inherit the FFT's error; the profile kernel alone is held to 1e-12 there).  The one
float32 input takes 1e-6 there too, for the reason it does on the maps: the reference transforms a float32 image in single
precision (NumPy keeps complex64; the golden maps are float32, asserted in tests/test_window_size_cpu.py), so its own profile
carries ~1e-7 of its maximum in rounding noise, while the device computes in float64.  Angular counts: exact; angular means:
``n_bin * 2^-52 * mean|x|`` per bin, the bound of any summation order over n_bin terms, from the recorded count; angles:
bit-equal.  Centres, ``ind``, ``peaks[0]``, the lengths, and stack against per-frame calls: equal."""
import os

import numpy as np
import pytest

import window_size_cases as wc
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32_TOL = 1e-6


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "window_size_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def ws():
    from mtflearn_amd.features import window_size
    return window_size


def close(got, ref, tol=1e-9):
    np.testing.assert_allclose(got, ref, rtol=0, atol=tol * np.abs(ref).max())


def tol_of(name):
    return F32_TOL if wc.IMAGES[name][2] == np.float32 else 1e-9


@pytest.mark.parametrize("name", list(wc.IMAGES))
def test_maps_match_the_reference(golden, ws, name):
    img = golden[f"{name}/image"]
    ac, raw, spec = ws.compute_autocorrelation(img), ws.compute_autocorrelation(img, standardize=False), ws.fft_power_spectrum(img)
    assert ac.shape == raw.shape == spec.shape == img.shape and ac.dtype == np.float64
    frames = wc.frames_of(name)
    for b, (key, _) in enumerate(frames):
        pick = (lambda a: a[b]) if img.ndim == 3 else (lambda a: a)
        close(pick(ac), golden[f"{key}/autocorr"], tol_of(name))
        close(pick(raw), golden[f"{key}/autocorr_raw"], tol_of(name))
        close(pick(spec), golden[f"{key}/spectrum"], tol_of(name))


@pytest.mark.parametrize("name", list(wc.IMAGES))
def test_characteristic_length_fft(golden, ws, name):
    img = golden[f"{name}/image"]
    centres, ys, y2s, inds, _ = ws._char_length_fft(img, 10, 9, True, True)
    lengths = np.atleast_1d(ws.get_characteristic_length_fft(img))
    lin_centres, lin_ys, _, _, _ = ws._char_length_fft(img, 10, 9, False, True)
    n4 = ws._char_length_fft(img, 4, 6, True, True)
    n4_len = np.atleast_1d(ws.get_characteristic_length_fft(img, niter=4, size=6))
    for b, (key, frame) in enumerate(wc.frames_of(name)):
        assert tuple(centres[b]) == tuple(golden[f"{key}/fft_log_centre"]) and tuple(lin_centres[b]) == tuple(golden[f"{key}/fft_lin_centre"])
        assert ys[b].shape == golden[f"{key}/fft_log_y"].shape
        close(ys[b], golden[f"{key}/fft_log_y"], tol_of(name))
        close(lin_ys[b], golden[f"{key}/fft_lin_y"], tol_of(name))
        close(y2s[b], golden[f"{key}/fft_log_y2"], tol_of(name))
        close(n4[2][b], golden[f"{key}/fft_n4s6_y2"], tol_of(name))
        assert inds[b] == int(golden[f"{key}/fft_log_ind"])
        assert lengths[b] == float(golden[f"{key}/fft_log_length"]) and n4_len[b] == float(golden[f"{key}/fft_n4s6_length"])
        if img.ndim == 3:                                                    # the stack call against the 2-D call of each frame
            assert ws.get_characteristic_length_fft(frame) == lengths[b]
    assert lengths.shape == ((img.shape[0],) if img.ndim == 3 else (1,))


@pytest.mark.parametrize("name", list(wc.IMAGES))
def test_characteristic_length(golden, ws, name):
    img = golden[f"{name}/image"]
    centres, lines, peaks, _ = ws._char_length(img, True, True)              # centres, profiles and the DEVICE's peak search
    got = np.atleast_1d(ws.get_characteristic_length(img))                   # 2-D: SciPy's find_peaks on the host
    for b, (key, frame) in enumerate(wc.frames_of(name)):
        assert tuple(centres[b]) == tuple(golden[f"{key}/cl_centre"])
        assert lines[b].shape == golden[f"{key}/cl_line"].shape
        close(lines[b], golden[f"{key}/cl_line"], tol_of(name))
        assert peaks[b] == got[b] == int(golden[f"{key}/cl_peak"])
        if img.ndim == 3:
            assert ws.get_characteristic_length(frame) == got[b]


def test_device_peak_search_is_find_peaks_plain_rule(ws):
    """Profiles without a peak (the pyramid of a constant frame, smooth ramps): the stack answers -1 where the 2-D call raises
    the reference's error, and both agree with SciPy's rule on the host."""
    flat = np.full((2, 24, 24), 2.0)
    flat[1, 5, 5] = 3.0
    got = ws.get_characteristic_length(flat, standardize=False)
    assert list(got) == [wc.get_characteristic_length(f, standardize=False)[0] for f in flat]
    ramp = np.add.outer(np.arange(20.0), np.arange(24.0))
    ref = wc.get_characteristic_length(ramp)[0]
    assert ws.get_characteristic_length(np.stack([ramp, ramp]))[1] == ref
    if ref < 0:
        with pytest.raises(ValueError, match="No peak detected in the radial profile."):
            ws.get_characteristic_length(ramp)
    one_row = wc.image("small33x40")[:1]                                      # H = 1: the centre is on row 0, the cut profile empty
    with pytest.raises(ValueError, match="No peak detected in the radial profile."):
        ws.get_characteristic_length(one_row)
    with pytest.raises(ValueError, match="attempt to get argmax of an empty sequence"):
        ws.get_characteristic_length_fft(one_row)
    assert np.isnan(ws.get_characteristic_length_fft(np.stack([one_row, one_row]))).all()      # a stack: nan for such a frame
    assert list(ws.get_characteristic_length(np.stack([one_row, one_row]))) == [-1, -1]


def test_a_constant_frame_of_a_stack_is_refused_on_the_device(ws):
    """0.1 is not a binary fraction: the mean of a constant frame rounds, the two-pass deviation need not be 0, the frame's
    min == max is.  The single image is refused on the host, the frame of a stack by the device's statistics."""
    img = wc.image("small33x40")
    for value in (0.1, 3.0, 1e-300):
        stack = np.stack([img, np.full_like(img, value), img])
        for fn in (ws.compute_autocorrelation, ws.get_characteristic_length):
            with pytest.raises(ValueError, match="Standard deviation is zero, can't standardize the image."):
                fn(stack)
            with pytest.raises(ValueError, match="Standard deviation is zero, can't standardize the image."):
                fn(stack.astype(np.float32))
    assert ws.compute_autocorrelation(np.stack([img, np.full_like(img, 0.1)]), standardize=False).shape == (2, 33, 40)


@pytest.mark.parametrize("shape", wc.ANGULAR_SHAPES + ["spikes"])
def test_angular_average(golden, ws, shape):
    sid = shape if shape == "spikes" else f"{shape[0]}x{shape[1]}"
    data = golden[f"angular/{sid}/input"]
    for nb in wc.ANGULAR_BINS:
        for use_mask in (True, False):
            key = f"angular/{sid}/{nb}/{int(use_mask)}"
            angles, sums, counts = ws._angular_sums(data, nb, use_mask)
            a2, profile = ws.angular_average(data, num_bins=nb, use_mask=use_mask)
            ref_counts = golden[f"{key}/counts"]
            np.testing.assert_array_equal(counts, ref_counts)               # a flipped edge pixel shows here
            np.testing.assert_array_equal(angles, golden[f"{key}/angles"])
            np.testing.assert_array_equal(a2, angles)
            bound = ref_counts * 2.0 ** -52 * np.abs(data).mean()
            err = np.abs(profile - golden[f"{key}/profile"])
            assert np.all(err <= bound), (key, (err - bound).max())
            assert np.all(profile[ref_counts == 0] == 0)


def test_angular_average_beyond_the_lds_table(ws):
    """More bins than the per-workgroup table holds: the global path, same membership."""
    data = wc.angular_input((31, 20))
    angles, sums, counts = ws._angular_sums(data, 5000, False)
    ref_angles, ref_profile, ref_counts = wc.angular_average(data, 5000, False)
    np.testing.assert_array_equal(counts, ref_counts)
    np.testing.assert_array_equal(angles, ref_angles)
    np.testing.assert_allclose(ws.angular_average(data, 5000, False)[1], ref_profile, rtol=1e-15, atol=0)


def test_radial_profile_is_unchanged(ws):
    """The polar kernel now reads a centre table: radial_profile on the existing golden inputs, through the comparisons of
    tests/test_gpu_pickers.py (the restated warp_polar at 1e-12, every method, default and explicit centre)."""
    from mtflearn_amd.features import pickers as pk
    from oracle import pickers_oracle as po
    with np.load(os.path.join(ROOT, "tests", "golden", "pickers_golden.npz")) as f:
        inputs = [f["autocorr_64"].astype(np.float64), f["autocorr_33"], f["autocorr_mean_96"].astype(np.float64),
                  f["denoise_in"][:40, :52]]
    for data in inputs:
        h, w = data.shape
        for method in ("max", "mean", "sum"):
            got, ref = pk.radial_profile(data, method=method), po.radial_profile(data, method=method)
            assert got.shape == ref.shape
            np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        centre = (h // 3, w // 2 + 1)
        np.testing.assert_allclose(pk.radial_profile(data, center=centre, method="mean"),
                                   po.radial_profile(data, center=centre, method="mean"), rtol=1e-12, atol=1e-12)
    stack = np.stack([inputs[0], inputs[0][::-1].copy()])
    np.testing.assert_array_equal(pk._radial_profiles(stack)[0], pk.radial_profile(inputs[0]))
