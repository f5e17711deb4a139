"""mtflearn_amd.utils on the GPU: against goldens captured from the reference (tests/make_golden_utils.py) at the goldens' shape,
and against the same few lines of NumPy at shapes below one wave, off the vector width, past one workgroup and with a channel
axis; the device-resident chain into background removal and local_max."""
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from mtflearn_amd import _native, utils
from mtflearn_amd.synthetic import honeycomb_frame
from utils_cases import CLIP_METHODS, golden_inputs, info_arrays

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5), (33, 65), (64, 64), (257, 129), (12, 10, 3)]
DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "utils_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def images():
    return golden_inputs()


def frame(shape, dtype=np.float32, seed=0, hot=True):
    """A lattice frame of any shape (channels: scaled copies), optionally with one hot pixel, in ``dtype``."""
    rng = np.random.default_rng([seed, *shape])
    x = honeycomb_frame(shape[0], shape[1], l=6.0, seed=seed).astype(np.float64)
    if len(shape) == 3:
        x = x[:, :, None] * np.linspace(0.5, 1.5, shape[2])
    x = x + 0.01 * rng.random(shape)
    if hot:
        x[(shape[0] // 2, shape[1] // 3) + (0,) * (len(shape) - 2)] = 30.0
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return x.astype(dtype)
    return np.round(x * (8 if dtype == np.uint8 else 900)).astype(dtype)


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ bit-exact: goldens
@pytest.mark.parametrize("name", ["hot", "clean", "u8", "f64", "const"])
def test_minmax_and_clip_equal_the_reference(golden, images, name):
    img = images[name]
    got = utils.normalize_image(img)
    assert got.dtype == np.float32 and got.shape == img.shape
    np.testing.assert_array_equal(got, golden[f"{name}/normalize/minmax"])
    for method in CLIP_METHODS:
        out, did_clip, info = utils.percentile_clip(img, method=method)
        keys, values = info_arrays(info)
        assert list(keys) == list(golden[f"{name}/clip/{method}/keys"]) and info["method"] == method
        np.testing.assert_array_equal(values, golden[f"{name}/clip/{method}/values"])
        assert did_clip == bool(values[0]) and out.dtype == np.float32
        np.testing.assert_array_equal(out, golden[f"{name}/clip/out"] if did_clip else img.astype(np.float32))


def test_other_ranges_percentiles_and_value_clip_equal_the_reference(golden, images):
    np.testing.assert_array_equal(utils.normalize_image(images["clean"], "minmax", vmin=-1.0, vmax=2.0), golden["clean/normalize/minmax_-1_2"])
    out, did_clip, info = utils.percentile_clip(images["hot"], low=5.0, high=90.0, method="mad")
    np.testing.assert_array_equal(info_arrays(info)[1], golden["hot/clip/low5_high90/values"])
    np.testing.assert_array_equal(out, golden["hot/clip/low5_high90/out"])
    np.testing.assert_array_equal(utils.value_clip(images["clean"], 0.2, 0.7), golden["clean/value_clip"])


@pytest.mark.parametrize("name", ["nonfinite", "clean", "const"])
def test_robust_minmax_equals_the_reference_and_keeps_nonfinite_elements(golden, images, name):
    img = images[name]
    got = utils.normalize_image_robust(img)
    np.testing.assert_array_equal(got, golden[f"{name}/robust/minmax"])          # NaN == NaN here
    bad = ~np.isfinite(img)
    assert np.array_equal(got[bad], img[bad], equal_nan=True) and np.isfinite(got[~bad]).all()
    assert bad.sum() == (4 if name == "nonfinite" else 0)


# ------------------------------------------------------------------------------------------------ bit-exact: NumPy at other shapes
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_minmax_and_clips_equal_numpy(shape, dtype):
    img = frame(shape, dtype, seed=len(shape) + shape[0])
    x = img.astype(np.float32)
    mn, mx = x.min(), x.max()
    np.testing.assert_array_equal(utils.normalize_image(img, vmin=-0.5, vmax=3.0), -0.5 + (x - mn) * (3.0 - -0.5) / ((mx - mn) + 1e-8))
    lo, hi = float(np.percentile(x, 10)), float(np.percentile(x, 60))
    np.testing.assert_array_equal(utils.value_clip(img, lo, hi), np.clip(x, lo, hi))
    np.testing.assert_array_equal(utils.value_clip(img, 0.1, 0.05), np.clip(x, 0.1, 0.05))      # bounds that cross

    out, did_clip, info = utils.percentile_clip(img, low=2.0, high=98.5)
    flat = x.reshape(-1)
    med = np.median(flat)
    want = {"min": float(mn), "max": float(mx), "p_low": float(np.percentile(flat, 2.0)), "p_high": float(np.percentile(flat, 98.5)),
            "median": float(med), "mad": float(np.median(np.abs(flat - med))), "q1": float(np.percentile(flat, 25)),
            "q3": float(np.percentile(flat, 75))}
    assert {k: info[k] for k in want} == want
    assert did_clip and (info["vmin"], info["vmax"]) == (want["p_low"], want["p_high"])          # the hot pixel
    np.testing.assert_array_equal(out, np.clip(x, want["p_low"], want["p_high"]))
    quiet, did_clip, _ = utils.percentile_clip(frame(shape, dtype, seed=2, hot=False), method="ratio")
    assert not did_clip
    np.testing.assert_array_equal(quiet, frame(shape, dtype, seed=2, hot=False).astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES)
def test_robust_equals_numpy_with_nonfinite_elements(shape):
    img = frame(shape, np.float32, seed=4)
    rng = np.random.default_rng(shape[0])
    flat = img.reshape(-1)
    flat[rng.choice(flat.size, size=5, replace=False)] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    finite = np.isfinite(img)
    mn, mx = img[finite].min(), img[finite].max()
    with np.errstate(invalid="ignore"):
        want = 0.0 + (img - mn) * (1.0 - 0.0) / ((mx - mn) + 1e-8)
    want[~finite] = img[~finite]
    got = utils.normalize_image_robust(img)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(got[~finite], img[~finite], equal_nan=True)
    for mode in ("l1", "l2"):
        got = utils.normalize_image_robust(img, mode)
        assert np.array_equal(got[~finite], img[~finite], equal_nan=True) and np.isfinite(got[finite]).all()
    with pytest.raises(ValueError, match="Input contains NaN or inf values"):
        utils.normalize_image(img)
    with pytest.raises(ValueError, match="Input contains NaN or inf values"):
        utils.percentile_clip(img)
    assert np.isnan(utils.standardize_image(img)).all()                          # NumPy's mean and std are NaN


def test_constant_images(golden, images):
    got = utils.normalize_image(images["const"])
    np.testing.assert_array_equal(got, golden["const/normalize/minmax"])
    assert np.all(got == 0.5)
    for mode in ("l1", "l2"):
        got, want = utils.normalize_image(images["const"], mode), norm_statement(images["const"], mode)
        assert np.all(np.abs(got.astype(np.float64) - want) <= ulp32(want))
    const = images["const"].copy()
    const[2, 3] = np.nan
    got = utils.normalize_image_robust(const)
    np.testing.assert_array_equal(got, golden["const/robust/minmax"] * np.where(np.isnan(const), np.nan, 1))
    with pytest.raises(ValueError, match="Standard deviation is zero"):
        utils.standardize_image(images["const"])
    with pytest.raises(ValueError, match="All values are non-finite"):
        utils.normalize_image_robust(np.full((3, 3), np.inf, np.float32))


# ------------------------------------------------------------------------------------------------ float64 sums: one ulp
def norm_statement(x32, mode):
    """The float64 statement of l1 / l2 on the float32 image."""
    x = x32.astype(np.float64).reshape(-1)
    total = math.fsum(np.abs(x)) if mode == "l1" else math.fsum(x * x)
    return x32.astype(np.float64) / ((total + 1e-8) if mode == "l1" else math.sqrt(total + 1e-8))


def standard_statement(x):
    x = x.astype(np.float64)
    mean = math.fsum(x.reshape(-1)) / x.size
    return (x - mean) / math.sqrt(math.fsum(((x - mean) ** 2).reshape(-1)) / x.size)


def cases_for_sums(images):
    yield from ((f"golden {name}", images[name], name) for name in ("hot", "clean", "u8", "f64"))
    for shape in SHAPES:
        for dtype in DTYPES:
            yield f"{shape} {np.dtype(dtype).name}", frame(shape, dtype, seed=7), None


def test_l1_l2_within_one_float32_ulp_of_the_float64_statement(golden, images):
    for label, img, name in cases_for_sums(images):
        for mode in ("l1", "l2"):
            got = utils.normalize_image(img, mode)
            want = norm_statement(img.astype(np.float32), mode)
            assert got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= ulp32(want)), (label, mode, (err / ulp32(want)).max())
            if name:
                ref = golden[f"{name}/normalize/{mode}"]
                print(f"{mode} {name}: largest distance to the reference's float32 result "
                      f"{(np.abs(got.astype(np.float64) - ref) / ulp32(ref)).max():.2f} float32 ulp")


def test_standardize_within_one_rounding_of_the_float64_statement(golden, images):
    for label, img, name in cases_for_sums(images):
        got = utils.standardize_image(img)
        want = standard_statement(img)
        assert got.shape == img.shape
        if img.dtype == np.float32:
            assert got.dtype == np.float32
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= ulp32(want)), (label, (err / ulp32(want)).max())
        else:
            assert got.dtype == np.float64
            assert np.all(np.abs(got - want) <= 4 * 2.0 ** -53 * np.abs(want)), (label, np.abs(got / want - 1).max())
        if name in ("hot", "u8", "f64"):
            ref = golden[f"{name}/standardize"]
            assert ref.dtype == got.dtype
            scale = ulp32(ref) if ref.dtype == np.float32 else np.spacing(np.abs(ref))
            print(f"standardize {name}: largest distance to the reference's result "
                  f"{(np.abs(got.astype(np.float64) - ref) / scale).max():.2f} {ref.dtype} ulp")


def test_wide_integers_and_float16_follow_numpy():
    img = frame((33, 65), np.uint16, seed=5).astype(np.int64) * 70000
    np.testing.assert_array_equal(utils.normalize_image(img), utils.normalize_image(img.astype(np.float32)))
    half = frame((33, 65), np.float32, seed=5).astype(np.float16)
    np.testing.assert_array_equal(utils.value_clip(half, 0.1, 0.6), np.clip(half.astype(np.float32), 0.1, 0.6))
    assert utils.standardize_image(img).dtype == np.float64 and utils.standardize_image(half).dtype == np.float32


# ------------------------------------------------------------------------------------------------ device chain
@pytest.mark.parametrize("kind", ["native", "torch"])
def test_device_chain_matches_the_host_chain(kind):
    from mtflearn_amd.background import remove_background_opening
    from mtflearn_amd.distributed import (local_max_device, normalize_image_device, percentile_clip_device,
                                          remove_background_device, standardize_image_device)
    from mtflearn_amd.features import local_max
    img = frame((257, 129), np.float32, seed=21)
    clipped, did_clip, info = utils.percentile_clip(img)
    normal = utils.normalize_image(clipped)
    want_res, _ = remove_background_opening(normal, 15)
    want_pts = local_max(want_res, 3, threshold=0.2)
    assert did_clip and len(want_pts) > 50
    if kind == "native":
        dev = _native.DeviceArray.from_numpy(img)
        host = lambda a: a.numpy()
    else:
        torch = pytest.importorskip("torch")
        dev = torch.from_numpy(img).to("cuda:0")
        host = lambda a: a.cpu().numpy()
    d_clipped, d_did, d_info = percentile_clip_device(dev)
    d_normal = normalize_image_device(d_clipped)
    d_res, _ = remove_background_device(d_normal, "opening", 15)
    d_pts = local_max_device(d_res, 3, threshold=0.2)
    assert type(d_clipped) is type(dev) and d_did is True and d_info == info
    np.testing.assert_array_equal(host(d_clipped), clipped)
    np.testing.assert_array_equal(host(d_normal), normal)
    np.testing.assert_array_equal(host(d_res), want_res)
    np.testing.assert_array_equal(host(d_pts), want_pts)
    np.testing.assert_array_equal(host(standardize_image_device(dev)), utils.standardize_image(img))
    np.testing.assert_array_equal(host(normalize_image_device(dev, "l2")), utils.normalize_image(img, "l2"))
    raw = local_max(utils.normalize_image(img), 3, threshold=0.2)                # without the clip the hot pixel sets the scale
    assert len(raw) != len(want_pts)


def test_device_entry_checks():
    from mtflearn_amd.distributed import normalize_image_device, percentile_clip_device
    dev = _native.DeviceArray.from_numpy(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError, match="mode must be"):
        normalize_image_device(dev, mode="max")
    with pytest.raises(ValueError, match="method must be"):
        percentile_clip_device(dev, method="sigma")
    with pytest.raises(TypeError, match="device images must be"):
        normalize_image_device(_native.DeviceArray.from_numpy(np.zeros((8, 8), np.int32)))


def test_device_entry_refuses_a_host_tensor():
    torch = pytest.importorskip("torch")
    from mtflearn_amd.distributed import normalize_image_device
    with pytest.raises(ValueError, match="must live on the GPU"):
        normalize_image_device(torch.zeros(4, 4))
