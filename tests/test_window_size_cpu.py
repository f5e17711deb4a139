"""CPU checks of mtflearn_amd.features.window_size: the goldens captured from the reference (tests/make_golden_window_size.py)
against the NumPy / SciPy restatement of tests/window_size_cases.py, the margins that keep the cases meaningful, the C ABI
table, and every refusal that comes before a device call.  The licence of tests/test_gpu_window_size.py."""
import os
import re

import numpy as np
import pytest

import window_size_cases as wc
from mtflearn_amd import _native, features
from mtflearn_amd.features import window_size as ws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["zk_circular_autocorr", "zk_shifted_magnitude", "zk_char_length", "zk_char_length_fft", "zk_angular_average"]
NAMES = ["compute_autocorrelation", "get_characteristic_length", "get_characteristic_length_fft", "fft_power_spectrum",
         "angular_average"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "window_size_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def test_the_notebook_import_and_the_exports():
    from mtflearn_amd.features import autocorrelation, radial_profile, get_characteristic_length, get_characteristic_length_fft
    assert all(callable(f) for f in (autocorrelation, radial_profile, get_characteristic_length, get_characteristic_length_fft))
    assert set(NAMES) <= set(features.__all__) and set(NAMES) == set(ws.__all__)
    assert "baseline_correction" in features.__all__
    import mtflearn_amd
    assert "get_characteristic_length_fft" in mtflearn_amd.__doc__ and "angular_average" in features.__doc__


def test_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = _native.load()
    for sym in SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym


@pytest.mark.parametrize("name", list(wc.IMAGES))
def test_restatement_equals_the_reference(golden, name):
    """NumPy on both sides: equal, except where the reference computed a float32 image in single precision."""
    f32 = wc.IMAGES[name][2] == np.float32
    np.testing.assert_array_equal(golden[f"{name}/image"], wc.image(name))
    for key, img in wc.frames_of(name):
        np.testing.assert_array_equal(wc.compute_autocorrelation(img), golden[f"{key}/autocorr"])
        np.testing.assert_array_equal(wc.compute_autocorrelation(img, False), golden[f"{key}/autocorr_raw"])
        np.testing.assert_array_equal(wc.fft_power_spectrum(img), golden[f"{key}/spectrum"])
        peak, centre, line = wc.get_characteristic_length(img)
        assert peak == int(golden[f"{key}/cl_peak"]) and centre == tuple(golden[f"{key}/cl_centre"])
        np.testing.assert_array_equal(line, golden[f"{key}/cl_line"])
        length, centre, y, y2, ind = wc.get_characteristic_length_fft(img)
        assert length == float(golden[f"{key}/fft_log_length"]) and ind == int(golden[f"{key}/fft_log_ind"])
        assert centre == tuple(golden[f"{key}/fft_log_centre"]) == (img.shape[0] // 2, img.shape[1] // 2)
        np.testing.assert_array_equal(y, golden[f"{key}/fft_log_y"])
        np.testing.assert_array_equal(y2, golden[f"{key}/fft_log_y2"])
        np.testing.assert_array_equal(wc.get_characteristic_length_fft(img, use_log=False)[2], golden[f"{key}/fft_lin_y"])
        np.testing.assert_array_equal(wc.get_characteristic_length_fft(img, 4, 6)[3], golden[f"{key}/fft_n4s6_y2"])
        assert golden[f"{key}/autocorr"].dtype == (np.float32 if f32 else np.float64)


def test_the_cases_keep_their_margins(golden):
    frames = [kv for name in wc.IMAGES for kv in wc.frames_of(name)]
    assert len(frames) == 9                                                 # six images and the three frames of the stack
    assert {wc.IMAGES[n][0] for n in wc.IMAGES} == {(64, 64), (48, 80), (80, 48), (63, 65), (33, 40), (3, 48, 80)}
    for key, img in frames:
        assert wc.dc_ratio(img) >= 2.0, key
        assert wc.argmax_margin(golden[f"{key}/fft_log_y2"]) >= 1e-6 and wc.argmax_margin(golden[f"{key}/fft_n4s6_y2"]) >= 1e-6, key
        assert wc.peak_margin(golden[f"{key}/cl_line"], int(golden[f"{key}/cl_peak"])) >= 1e-6, key
        assert int(golden[f"{key}/fft_log_ind"]) > 0 and int(golden[f"{key}/cl_peak"]) > 0
    stack = [int(golden[f"{wc.STACK}/{b}/fft_log_ind"]) for b in range(3)]
    assert len(set(stack)) == 3                                             # a shared profile would show


@pytest.mark.parametrize("shape", wc.ANGULAR_SHAPES + ["spikes"])
def test_angular_restatement_equals_the_reference(golden, shape):
    sid = shape if shape == "spikes" else f"{shape[0]}x{shape[1]}"
    data = golden[f"angular/{sid}/input"]
    np.testing.assert_array_equal(data, wc.angular_spikes() if shape == "spikes" else wc.angular_input(shape))
    for nb in wc.ANGULAR_BINS:
        for use_mask in (True, False):
            key = f"angular/{sid}/{nb}/{int(use_mask)}"
            angles, profile, counts = wc.angular_average(data, nb, use_mask)
            np.testing.assert_array_equal(angles, golden[f"{key}/angles"])
            np.testing.assert_array_equal(profile, golden[f"{key}/profile"])
            np.testing.assert_array_equal(counts, golden[f"{key}/counts"])
            if not use_mask:
                assert counts.sum() == data.size                            # every direction has a bin


def test_the_eight_directions_are_what_numpy_yields():
    """The exact angles the kernel assigns to dy == 0, dx == 0 and |dx| == |dy| (csrc/zk_window_size.hip)."""
    for r in (1, 3, 64, 1000, 8191):
        dy = np.array([0, r, r, r, 0, -r, -r, -r])
        dx = np.array([r, r, 0, -r, -r, -r, 0, r])
        np.testing.assert_array_equal(np.degrees(np.arctan2(dy, dx)) % 360, [0, 45, 90, 135, 180, 225, 270, 315])
    assert np.degrees(np.arctan2(0, 0)) % 360 == 0


def test_every_refusal_comes_before_any_device_call():
    img = wc.image("small33x40")
    for fn in (ws.compute_autocorrelation, ws.get_characteristic_length, ws.get_characteristic_length_fft, ws.fft_power_spectrum):
        with pytest.raises(ValueError, match="2-D image or a 3-D stack"):
            fn(img[0])
        with pytest.raises(ValueError, match="2-D image or a 3-D stack"):
            fn(img[None, None])
        with pytest.raises(TypeError, match="complex"):
            fn(img.astype(np.complex128))
    with pytest.raises(ValueError, match="2-D power spectrum"):
        ws.angular_average(img[None])
    with pytest.raises(TypeError, match="complex"):
        ws.angular_average(img.astype(np.complex64))
    for fn in (ws.compute_autocorrelation, ws.get_characteristic_length):
        with pytest.raises(ValueError, match="Standard deviation is zero, can't standardize the image."):
            fn(np.full((16, 20), 3.0))
    # a centre on row 0 leaves an empty profile: what the reference raises from find_peaks' empty answer and from argmax
    with pytest.raises(ValueError, match="No peak detected in the radial profile."):
        ws._first_peak(np.empty(0))
    with pytest.raises(ValueError, match="attempt to get argmax of an empty sequence"):
        ws._length_from_ind(64, np.int64(-1))
    with pytest.warns(RuntimeWarning):
        assert ws._length_from_ind(64, np.int64(0)) == np.inf              # ind == 0: inf with NumPy's warning, as in the reference
    np.testing.assert_array_equal(ws._length_from_ind(64, np.array([8, -1, 4])), [8.0, np.nan, 16.0])   # a stack: nan for that frame
    angles, profile = ws.angular_average(np.ones((4, 4)), num_bins=0)       # nothing to bin: the reference's empty answer
    assert angles.shape == profile.shape == (0,)
