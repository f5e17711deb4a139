"""local_max without a GPU: the fixture against the test-local tie-rule oracle and scipy, input validation, and the
threshold promotion helper (tests/golden/local_max_golden.npz, made by tests/make_golden_local_max.py)."""
import os

import numpy as np
import pytest
from scipy import ndimage

import local_max_oracle as lmo
from mtflearn_amd.features import local_max
from mtflearn_amd.features.peaks import _comparison_threshold

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_max_golden.npz")


def golden_cases():
    with np.load(GOLDEN) as f:
        g = {k: f[k] for k in f.files}
    images = {}
    for name in lmo.GOLDEN_IMAGES:               # regenerated from their recipe, checked against the stored digest
        images[name] = lmo.golden_image(name)
        assert lmo.image_digest(images[name]) == str(g[f"{name}_sha256"]), f"{name} no longer regenerates exactly"
    for k in range(int(g["n_cases"])):
        c = {name: g[f"case{k}_{name}"] for name in ("r", "has_threshold", "threshold", "distinct")}
        c["image"] = images[str(g[f"case{k}_image"])]
        cand = g[str(g[f"case{k}_candidates"])].astype(np.int64)       # raster indices
        c["candidates"] = np.stack(np.unravel_index(cand, c["image"].shape), axis=1).reshape(-1, 2)   # (row, col)
        c["expected"] = g[f"case{k}_expected"].astype(np.int64).reshape(-1, 2)
        c["name"] = f"case{k}_{g[f'case{k}_image']}_r{float(c['r']):.3f}"
        # thresholds are stored as float64; the NEP 50 case is a Python float against float32, as the reference saw it
        c["t"] = float(c["threshold"]) if c["has_threshold"] else None
        yield c


CASES = list(golden_cases())


def test_fixture_covers_the_contract():
    radii = {round(float(c["r"]), 6) for c in CASES}
    assert {1.0, 1.5, round(np.sqrt(2), 6), round(np.sqrt(5), 6), 3.0, 5.0, 8.0} <= radii
    assert {c["image"].dtype for c in CASES} >= {np.dtype(np.float32), np.dtype(np.float64)}
    assert any(c["image"].shape == (3, 1021) and len(c["expected"]) == 255 for c in CASES)          # the ramp
    assert any(c["image"].shape[0] == 2 for c in CASES) and any(c["image"].shape[1] == 2 for c in CASES)
    assert sum(len(c["expected"]) == 0 for c in CASES) >= 4


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_reproduces_reference(case):
    got = lmo.local_max_raster(case["image"], float(case["r"]), case["t"])
    ref = case["expected"]
    if case["distinct"]:
        np.testing.assert_array_equal(got, ref)
    else:
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, ref.tolist()))
        vals = case["image"][got[:, 1], got[:, 0]]
        assert (np.diff(vals.astype(np.float64)) <= 0).all()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stored_candidates_are_scipy_maxima(case):
    img = case["image"]
    if img.shape[0] < 3 or img.shape[1] < 3 or (img == img.flat[0]).all():
        assert len(case["candidates"]) == 0
        return
    mask = img == ndimage.maximum_filter(img, size=3, mode="nearest")
    mask &= img > (img.min() if case["t"] is None else case["t"])
    mask[[0, -1], :] = False
    mask[:, [0, -1]] = False
    np.testing.assert_array_equal(np.stack(np.nonzero(mask), axis=1), case["candidates"])


def test_nep50_case_compares_in_float32():
    case = [c for c in CASES if c["image"].shape == (256, 240) and c["t"] not in (None, 0.45)][0]
    img, t = case["image"], case["t"]
    assert (img > t).sum() < (img.astype(np.float64) > t).sum()
    assert (img.astype(np.float64) > _comparison_threshold(img.dtype, t)).sum() == (img > t).sum()


def test_rejects_other_ranks():
    with pytest.raises(ValueError):
        local_max(np.zeros((4, 5, 6), dtype=np.float32), 3)
    with pytest.raises(ValueError):
        local_max(np.zeros(16, dtype=np.float32), 3)
    with pytest.raises(ValueError):
        local_max(np.zeros((8, 8), dtype=np.float32), -1.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.uint16, np.int16, np.int32, np.float16, np.bool_])
def test_threshold_promotion_matches_numpy(dtype):
    rng = np.random.default_rng(7)
    info = np.finfo(dtype) if np.dtype(dtype).kind == "f" else None
    if np.dtype(dtype) == np.bool_:
        v = np.array([False, True])
    elif info is not None:
        base = rng.standard_normal(200).astype(dtype)
        v = np.concatenate([base, np.nextafter(base, np.inf, dtype=dtype), np.array([0.3, 0.1, 1 / 3], dtype=dtype)])
    else:
        ii = np.iinfo(dtype)
        v = np.concatenate([rng.integers(max(ii.min, -40000), min(ii.max, 70000), 300), [0, 1, 2, 99, 100, 101]]).astype(dtype)
    thresholds = [0.3, 0.1, 1 / 3, 100, 100.5, -2, 2.000000001, 0.30000001192092896, np.float32(0.1), np.float64(0.1),
                  np.float16(0.3), np.int64(100), np.uint8(99), True, 70000, -70000.25]
    for t in thresholds:
        with np.errstate(over="ignore"):
            want = v > t
        got = v.astype(np.float64) > _comparison_threshold(v.dtype, t)
        np.testing.assert_array_equal(got, want, err_msg=f"{np.dtype(dtype)} > {t!r} ({type(t).__name__})")


def test_fails_loudly_without_device():
    from mtflearn_amd import _native
    if _native.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(RuntimeError, match="no HIP device"):
        local_max(np.random.default_rng(0).random((32, 32)), 3)
