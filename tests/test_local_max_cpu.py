"""local_max without a GPU: the fixture against the test-local tie-rule oracle and scipy, input validation, and the
threshold promotion helper (tests/golden/local_max_golden.npz, made by tests/make_golden_local_max.py)."""
import os

import numpy as np
import pytest
from scipy import ndimage

import local_max_cases as lmc
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


# ---- the oracle's additions (NaN rule, tile_lds_bytes) and the inputs of tests/test_gpu_local_max_kernels.py
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_candidate_mask_still_gives_the_stored_candidates(case):
    mask = lmo.candidate_mask(case["image"], case["t"])
    np.testing.assert_array_equal(np.stack(np.nonzero(mask), axis=1).reshape(-1, 2), case["candidates"])


def test_candidate_mask_nan_rule():
    nan = np.nan
    img = np.array([[0, 0, 0, 0, 0, 0, 0],
                    [0, 3, nan, 1, 0, 2, 0],          # a NaN neighbour exceeds neither the 3 nor the 1; the 2 has one below
                    [0, 0, 0, 0, 0, nan, 0],
                    [0, nan, 0, 0, 0, 0, 0],
                    [nan, 0, 0, 0, 0, 0, nan]], dtype=np.float64)
    for dtype in (np.float32, np.float64):
        mask = lmo.candidate_mask(img.astype(dtype))
        assert sorted(zip(*np.nonzero(mask))) == [(1, 1), (1, 3), (1, 5)]
        assert sorted(zip(*np.nonzero(lmo.candidate_mask(img.astype(dtype), 1)))) == [(1, 1), (1, 5)]
        assert sorted(zip(*np.nonzero(lmo.candidate_mask(img.astype(dtype), -1)))) == [(1, 1), (1, 3), (1, 5), (3, 2), (3, 3), (3, 4), (3, 5)]
    low = np.where(np.isnan(img), nan, -img - 1)      # negative everywhere: the default threshold is the non-NaN minimum, -4
    assert sorted(zip(*np.nonzero(lmo.candidate_mask(low)))) == [(1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4), (3, 5)]
    assert not lmo.candidate_mask(np.full((5, 6), nan)).any()
    const = np.full((5, 6), 0.5)
    const[2, 2] = const[0, 3] = nan
    assert not lmo.candidate_mask(const).any() and not lmo.candidate_mask(const, 0.0).any()
    with np.errstate(all="raise"):                    # the NaN path raises no floating-point warning
        lmo.candidate_mask(img)
    assert lmo.local_max_raster(img, 2.0).tolist() == [[1, 1], [5, 1]]       # 1 at (3, 1) falls to the 3 two pixels away
    assert lmo.local_max_raster(np.full((5, 6), nan), 2.0).shape == (0, 2)


def test_tile_lds_bytes_restates_the_host_formula():
    assert lmo.tile_lds_bytes(31, 96, 160) == 61140 == 126 * 78 * 5 + 4 * 3000
    assert lmo.tile_lds_bytes(31, 96, 160) <= lmo.TILE_LDS_MAX == 61440 < lmo.tile_lds_bytes(31.4, 96, 160)
    assert lmo.tile_lds_bytes(0, 96, 160) == 64 * 16 * 5
    assert lmo.tile_lds_bytes(1, 96, 160) == 66 * 18 * 5 + 4 * 4
    assert lmo.tile_lds_bytes(np.sqrt(2), 96, 160) == 66 * 18 * 5 + 4 * 8
    assert lmo.tile_lds_bytes(8, 240, 256) == 80 * 32 * 5 + 4 * 196      # 197 lattice points in the closed disk of radius 8
    for r in lmc.WIDE_RADII:
        assert lmo.tile_lds_bytes(r, *lmc.FRAME) <= lmo.TILE_LDS_MAX
    for r in lmc.CROSSOVER_RADII[1:] + (33.0, 45.5):
        assert lmo.tile_lds_bytes(r, *lmc.FRAME) > lmo.TILE_LDS_MAX
    for name, shape, r, tiled in lmc.CLIPPED:
        assert (lmo.tile_lds_bytes(r, *shape) <= lmo.TILE_LDS_MAX) == tiled, name
    assert lmo.tile_lds_bytes(40, 150, 20) == 60904 == (64 + 38) * (16 + 80) * 5 + 4 * lmc.disk_offsets(40, 19, 40)
    assert lmo.tile_lds_bytes(40, 20, 150) == (64 + 80) * (16 + 38) * 5 + 4 * lmc.disk_offsets(40, 40, 19)
    assert lmo.tile_lds_bytes(1000, 20, 20) == (64 + 38) * (16 + 38) * 5 + 4 * (39 * 39 - 1)
    assert lmo.tile_lds_bytes(1e6, 40, 40) == (64 + 78) * (16 + 78) * 5 + 4 * (79 * 79 - 1)
    assert lmo.tile_lds_bytes(17, 3, 200) == (64 + 34) * (16 + 4) * 5 + 4 * (34 + 4 * 33)


FAMILIES = list(lmc.cpu_families())


@pytest.mark.parametrize("k", range(len(FAMILIES)), ids=[f"{f[0]}_r{f[2]:g}_t{f[3]}_{f[1].dtype}" for f in FAMILIES])
def test_both_checkers_agree_on_the_kernel_test_inputs(k):
    _, img, r, t = FAMILIES[k]
    pts = lmo.local_max_raster(img, r, t)
    assert lmo.check_greedy(img, r, pts, t)
    assert pts.dtype == np.int64 and pts.shape == (len(pts), 2)


def test_kernel_test_inputs_hold_what_they_are_for():
    for dtype in (np.float32, np.float64):
        img = lmc.signed_zeros(dtype)
        pts, vals = lmo.candidates_by_priority(img, -1.0)
        zeros = pts[vals == 0]
        assert len(zeros) > 1000 and np.signbit(img[zeros[:, 1], zeros[:, 0]]).any()
        assert (np.diff(zeros[:, 1] * img.shape[1] + zeros[:, 0]) > 0).all()       # the tied zeros: raster order
        assert len(lmo.candidates_by_priority(img)[0]) == 7
    img, pairs = lmc.ulp_pairs()
    for r in lmc.EDGE_RADII:
        kept = set(map(tuple, lmo.local_max_raster(img, r).tolist()))
        for big, small, apart in pairs:
            assert big in kept and ((small in kept) == (apart > r)), (big, small, r)
    frame = lmc.chain_frame("boustrophedon")
    assert lmo.candidate_mask(frame).sum() == 23 * 64 == np.count_nonzero(frame)
    assert frame[1, 127] + 1 == frame[3, 127] and frame[3, 1] + 1 == frame[5, 1]
    assert sorted(lmc.chain_frame("permutation")[1:-1:2, 1:-1:2].ravel()) == list(range(1, 23 * 64 + 1))
    for img in (lmc.all_negative(np.float32), lmc.all_negative(np.int16)):
        assert img.max() < 0 and len(lmo.local_max_raster(img, 5)) > 10
