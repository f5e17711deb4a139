"""mtflearn_amd.utils without a GPU: the host half (NumPy's percentile interpolation and median restated, the clip decision, the
argument checks and their messages) against NumPy and against goldens captured from the reference
(tests/make_golden_utils.py), with the device calls replaced by NumPy stand-ins."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mtflearn_amd import _native, utils
from utils_cases import CLIP_METHODS, golden_inputs, info_arrays


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "utils_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def images():
    return golden_inputs()


class HostOperand:
    """What the stand-ins below take for a device operand: the image converted to float32, on the host."""

    def __init__(self, array):
        self.host = np.asarray(array).astype(np.float32)
        self.shape, self.n = self.host.shape, self.host.size
        self.code = _native.dtype_code(np.asarray(array).dtype)


def sort_order_stats(operand, ranks, center=None):
    flat = operand.host.reshape(-1)
    if center is not None:
        flat = np.abs(flat - np.float32(center))
    return np.sort(flat)[np.asarray(ranks)]


def numpy_stats(operand, center=None, wide=False):
    flat = operand.host.reshape(-1)
    finite = flat[np.isfinite(flat)]
    return finite.min(), finite.max(), flat.size - finite.size, np.zeros(3)


def numpy_map(operand, op, params, keep_nonfinite=False):
    assert op == _native.MAP_CLIP
    return np.clip(operand.host, np.float32(params[0]), np.float32(params[1]))


@pytest.fixture
def host_device(monkeypatch):
    monkeypatch.setattr(utils, "_upload", HostOperand)
    monkeypatch.setattr(utils, "_stats", numpy_stats)
    monkeypatch.setattr(utils, "_order_stats", sort_order_stats)
    monkeypatch.setattr(utils, "_map", numpy_map)
    monkeypatch.setattr(utils, "_download", lambda a: a)


# ---------------------------------------------------------------- percentile_clip's decision against the reference
@pytest.mark.parametrize("name", ["hot", "clean", "u8", "f64", "const"])
@pytest.mark.parametrize("method", CLIP_METHODS)
def test_clip_decision_and_info_equal_the_reference(host_device, golden, images, name, method):
    out, did_clip, info = utils.percentile_clip(images[name], method=method)
    keys, values = info_arrays(info)
    assert list(keys) == list(golden[f"{name}/clip/{method}/keys"])             # the same entries in the same order
    assert info["method"] == method and did_clip == bool(golden[f"{name}/clip/{method}/values"][0])
    assert type(did_clip) is bool and type(info["ratio_flag"]) is bool and type(info["p_high"]) is float
    np.testing.assert_array_equal(values, golden[f"{name}/clip/{method}/values"])
    if did_clip:
        np.testing.assert_array_equal(out, golden[f"{name}/clip/out"])
    assert out.dtype == np.float32


def test_clip_percentiles_other_than_the_defaults(host_device, golden, images):
    out, did_clip, info = utils.percentile_clip(images["hot"], low=5.0, high=90.0, method="MAD")   # the method's case is folded
    assert did_clip and info["method"] == "mad"
    np.testing.assert_array_equal(info_arrays(info)[1], golden["hot/clip/low5_high90/values"])
    np.testing.assert_array_equal(out, golden["hot/clip/low5_high90/out"])


def test_the_hot_pixel_trips_every_test_and_its_absence_none(golden):
    for method in CLIP_METHODS:
        assert golden[f"hot/clip/{method}/values"][0] == 1.0 and golden[f"clean/clip/{method}/values"][0] == 0.0


# ---------------------------------------------------------------- NumPy's interpolation, restated
@pytest.mark.parametrize("n", [1, 2, 3, 5, 100, 257, 4099])
def test_interpolation_equals_numpy_bit_for_bit(n):
    a = np.sort(np.random.default_rng(n).normal(size=n).astype(np.float32))
    branches = set()
    for q in (0, 1, 25, 33.3, 50, 75, 99, 100):
        lo, hi, gamma = utils._quantile_neighbours(n, q)
        got, ref = utils._lerp(a[lo], a[hi], gamma), np.percentile(a, q)
        assert got.dtype == ref.dtype == np.float32 and got.tobytes() == ref.tobytes(), (n, q, got, ref)
        branches.add(bool(gamma >= 0.5))
    if n >= 100:
        assert branches == {False, True}                                         # both formulas of NumPy's lerp
    got, ref = utils._median_of(a[utils._median_ranks(n)]), np.median(a)
    assert got.dtype == ref.dtype == np.float32 and got.tobytes() == ref.tobytes()


def test_percentile_range_is_checked_as_numpy_checks_it():
    for q in (-0.1, 100.5):
        with pytest.raises(ValueError, match=re.escape("Percentiles must be in the range [0, 100]")):
            utils._quantile_neighbours(10, q)


# ---------------------------------------------------------------- messages, ahead of any device call
def test_argument_errors_match_the_reference(images):
    img = images["clean"]
    for fn in (utils.normalize_image, utils.normalize_image_robust):
        with pytest.raises(ValueError, match=re.escape("mode must be 'l1', 'l2', or 'minmax'.")):
            fn(img, mode="max")
    with pytest.raises(ValueError, match=re.escape("method must be 'ratio', 'mad', 'iqr', or 'auto'.")):
        utils.percentile_clip(img, method="sigma")
    with pytest.raises(ValueError, match=re.escape("Percentiles must be in the range [0, 100]")):
        utils.percentile_clip(img, high=101.0)
    with pytest.raises(TypeError):
        utils.normalize_image(img.astype(np.complex64))


def test_data_errors_match_the_reference(monkeypatch, images):
    monkeypatch.setattr(utils, "_upload", HostOperand)
    monkeypatch.setattr(utils, "_stats", numpy_stats)
    with pytest.raises(ValueError, match="Input contains NaN or inf values"):
        utils.normalize_image(images["nonfinite"])
    with pytest.raises(ValueError, match="Input contains NaN or inf values"):
        utils.percentile_clip(images["nonfinite"])
    monkeypatch.setattr(utils, "_stats", lambda op, center=None, wide=False: (np.float32(np.inf), np.float32(-np.inf), op.n, np.zeros(3)))
    with pytest.raises(ValueError, match=re.escape("All values are non-finite (NaN or inf)")):
        utils.normalize_image_robust(np.full((4, 4), np.nan, np.float32))
    monkeypatch.setattr(utils, "_stats", lambda op, center=None, wide=False: (np.float32(2), np.float32(2), 0, np.array([2.0 * op.n, 0, 0]) * (center is None)))
    with pytest.raises(ValueError, match=re.escape("Standard deviation is zero, can't standardize the image.")):
        utils.standardize_image(np.full((4, 4), 2.0, np.float32))


def test_helpers_are_plain_numpy():
    img = np.array([[1.0, np.nan], [3.0, np.inf], [-np.inf, 2.0]])
    np.testing.assert_array_equal(utils.ensure_finite(img), [[1, 0], [3, 3], [1, 2]])
    np.testing.assert_array_equal(utils.ensure_finite(img, nan_value=-1, inf_value=9), [[1, -1], [3, 9], [9, 2]])
    data, mask = utils.mask_nonfinite(img)
    np.testing.assert_array_equal(data, [1, 3, 2])
    np.testing.assert_array_equal(mask, [[True, False], [True, False], [False, True]])
    assert np.isnan(img[0, 1])                                                   # the input is left alone


# ---------------------------------------------------------------- surface
def test_exports_and_bindings():
    assert set(utils.__all__) == {"normalize_image", "normalize_image_robust", "standardize_image", "percentile_clip", "value_clip",
                                  "ensure_finite", "mask_nonfinite"}
    from mtflearn_amd import distributed
    assert {"normalize_image_device", "standardize_image_device", "percentile_clip_device"} <= set(distributed.__all__)
    names = ["zk_image_stats", "zk_image_order_stats", "zk_image_map"]
    header = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in names:
        for sym in (name, name + "_dev"):
            assert sym in _native.SYMBOLS and hasattr(lib, sym) and re.search(rf"\bint {sym}\(", header), sym
            n_args = len(_native.SYMBOLS[sym][1])
            decl = re.search(rf"\bint {sym}\(([^;]*)\);", header).group(1)
            assert n_args == decl.count(",") + 1, sym
    makefile = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "Makefile")).read()
    assert "zk_utils.hip" in makefile and re.search(r"zk_utils\.o: CXXFLAGS \+= -ffp-contract=off", makefile)
    assert "asm" not in open(os.path.join(ROOT, "motif-learn_amd", "csrc", "zk_utils.hip")).read()


def test_signatures_are_the_references():
    import inspect
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(utils.normalize_image) == sig(utils.normalize_image_robust) == [("img", E), ("mode", "minmax"), ("eps", 1e-8), ("vmin", 0.0), ("vmax", 1.0)]
    assert sig(utils.standardize_image) == [("image", E)]
    assert sig(utils.percentile_clip) == [("img", E), ("low", 1.0), ("high", 99.0), ("method", "auto"), ("high_ratio_thresh", 5.0),
                                          ("mad_k", 8.0), ("iqr_k", 3.0), ("eps", 1e-8), ("copy", True)]
    assert sig(utils.value_clip) == [("img", E), ("vmin", E), ("vmax", E), ("copy", True)]


def test_no_device_is_a_runtime_error(monkeypatch, images):
    """No CPU fallback: with no HIP device in sight every function that computes raises (the count is forced to zero, so the
    test says the same on a GPU machine)."""
    monkeypatch.setattr(_native, "device_count", lambda: 0)
    for call in (lambda: utils.normalize_image(images["clean"]), lambda: utils.standardize_image(images["clean"]),
                 lambda: utils.percentile_clip(images["clean"]), lambda: utils.value_clip(images["clean"], 0.1, 0.9),
                 lambda: utils.normalize_image_robust(images["nonfinite"])):
        with pytest.raises(RuntimeError, match="no HIP device"):
            call()
