"""local_max on the GPU (zk_local_max / zk_local_max_dev, csrc/zk_peaks.hip) against the reference's outputs
(tests/golden/local_max_golden.npz) and the test-local tie-rule oracle (tests/local_max_oracle.py)."""
import numpy as np
import pytest

import local_max_oracle as lmo
from mtflearn_amd import _native
from mtflearn_amd.features import ZPs, local_max
from mtflearn_amd.synthetic import honeycomb_frame
from test_local_max_cpu import CASES

pytestmark = pytest.mark.gpu


def assert_same_rows(got, want):
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(case):
    img, r, t = case["image"], float(case["r"]), case["t"]
    got = local_max(img, r, t)
    ref = case["expected"]
    if case["distinct"]:
        assert_same_rows(got, ref)
    else:
        assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, ref.tolist()))
    assert_same_rows(got, lmo.local_max_raster(img, r, t))


_plateaus = lmo.plateaus


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("r", [1.0, np.sqrt(2), 2.5, 4.0])
def test_integer_plateaus_follow_the_raster_rule(dtype, r):
    img = _plateaus(dtype, seed=int(r * 10))
    hi = int(img.max())
    for t in (None, 0, hi // 2, hi // 2 + 0.5, hi - 1):
        assert_same_rows(local_max(img, r, t), lmo.local_max_raster(img, r, t))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.uint8, np.uint16, np.int16])
def test_every_dtype_and_strided_views(dtype):
    base = honeycomb_frame(200, 180, seed=5).astype(np.float64)
    if np.dtype(dtype).kind == "f":
        img = base.astype(dtype)
    elif dtype == np.int16:
        img = np.rint(base * 20000 - 6000).astype(dtype)
    else:
        img = np.rint(base * np.iinfo(dtype).max).astype(dtype)
    for view in (img, img[::2, 1::3], img.T, img[5:150, 7:170]):
        assert not view.flags.c_contiguous or view is img
        for r, t in ((3.0, None), (5.0, view.flat[len(view.flat) // 2].item())):
            assert_same_rows(local_max(view, r, t), lmo.local_max_raster(view, r, t))


def test_ramp_is_exact_and_needs_few_launches():
    ramp = [c for c in CASES if c["image"].shape == (3, 1021)][0]
    got = local_max(ramp["image"], 3.0)
    assert_same_rows(got, ramp["expected"])
    launches = _native.load().zk_local_max_last_launches()
    assert 0 < launches <= 64, launches                 # 509 rounds of a one-decision-per-round scheme


def test_large_radius_takes_the_global_rounds():
    """A radius whose halo does not fit LDS (one global round per launch) gives the same greedy result."""
    img = honeycomb_frame(160, 150, seed=9).astype(np.float64) + 0.05 * np.random.default_rng(1).standard_normal((160, 150))
    for r in (33.0, 45.5):
        assert_same_rows(local_max(img, r), lmo.local_max_raster(img, r))


def test_4096_frame_is_the_greedy_result():
    rng = np.random.default_rng(4096)
    frame = honeycomb_frame(4096, seed=21) + np.float32(0.1) * rng.standard_normal((4096, 4096), dtype=np.float32)
    got = local_max(frame, 5)
    pts, _ = lmo.candidates_by_priority(frame)
    rows, cols = np.nonzero(lmo.candidate_mask(frame))
    assert len(pts) == len(rows) > 100000
    assert lmo.check_greedy(frame, 5, got)
    vals = frame[got[:, 1], got[:, 0]]
    assert (np.diff(vals) <= 0).all()


def test_two_calls_are_identical():
    frame = honeycomb_frame(1024, seed=4)
    a, b = local_max(frame, 5), local_max(frame, 5)
    assert a.tobytes() == b.tobytes() and len(a) > 1000


def test_empty_and_degenerate():
    assert local_max(np.ones((64, 64), dtype=np.float32), 3).shape == (0, 2)
    assert local_max(np.random.default_rng(0).random((2, 64)), 1).shape == (0, 2)
    assert local_max(np.random.default_rng(0).random((64, 1)), 1).shape == (0, 2)
    img = np.zeros((16, 16))
    img[5, 7] = 1.0
    np.testing.assert_array_equal(local_max(img, 3), [[7, 5]])
    assert local_max(img, 3, threshold=1.0).shape == (0, 2)


def test_capacity_retry_returns_every_point():
    """More points than the first capacity guess (H W / 8): the second call with the exact size."""
    img = np.zeros((96, 256))
    img[1:-1:2, 1:-1:2] = np.random.default_rng(3).random((47, 127)) + 1.0
    got = local_max(img, 1.0)
    assert len(got) == 47 * 127 > 96 * 256 // 8
    assert_same_rows(got, lmo.local_max_raster(img, 1.0))


@pytest.mark.parametrize("kind", ["native", "torch"])
def test_device_chain_matches_transform_at(kind):
    from mtflearn_amd.distributed import local_max_device, points_moments_device
    frame = honeycomb_frame(384, 320, seed=8)
    z = ZPs(8, 24)
    plan = z._device_plan()
    want_pts = local_max(frame, 5)
    want = z.transform_at(frame, want_pts).data
    if kind == "native":
        img = _native.DeviceArray.from_numpy(frame, device=plan.device)
        pts = local_max_device(img, 5)
        mom = points_moments_device(plan, img, pts).numpy()
        pts = pts.numpy()
    else:
        torch = pytest.importorskip("torch")
        img = torch.from_numpy(frame).to(f"cuda:{plan.device}")
        pts = local_max_device(img, 5)
        assert pts.dtype == torch.int32 and pts.is_cuda
        mom = points_moments_device(plan, img, pts)
        torch.cuda.synchronize()
        mom, pts = mom.cpu().numpy(), pts.cpu().numpy()
    np.testing.assert_array_equal(pts, want_pts)
    np.testing.assert_allclose(mom, want, rtol=1e-12, atol=1e-15 * np.abs(want).max())
