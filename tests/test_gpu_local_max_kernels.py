"""The suppression kernels of local_max (csrc/zk_peaks.hip) where tests/test_gpu_local_max.py does not reach: halos wider and
taller than a tile, the LDS crossover between suppress_tile_kernel and suppress_global_kernel, halos clipped to the frame,
priority chains across tile borders, the value edges of the ordering keys (signed zeros, one-ulp neighbours, infinities,
negative frames, NaN) and the capacity contract of the C ABI.  Every result is compared row for row with the sequential
oracle (tests/local_max_oracle.py, licensed by tests/test_local_max_cpu.py); the inputs are tests/local_max_cases.py."""
from ctypes import byref, c_int64, c_void_p

import numpy as np
import pytest

import local_max_cases as lmc
import local_max_oracle as lmo
from mtflearn_amd import _native, resident
from mtflearn_amd.features import local_max

pytestmark = pytest.mark.gpu

# Which kernel ran (asserted per case through lmo.tile_lds_bytes, the host's own formula) and the suppression launches
# observed on an MI355X (zk_local_max_last_launches: a multiple of ROUNDS_PER_CHECK = 4, at most candidates + 4).  "a / b":
# threshold None / the mid-range threshold.
#   wide halos    96 x 160, suppress_tile_kernel throughout    r 9     16      17      24.5   30      31 (61 140 B of 61 440)
#                 honey64 (825 / 117 candidates)               4 / 4   4 / 4   4 / 4   8 / 8  8 / 8   8 / 8
#                 plateaus_u8 (3 168 / 67 candidates)          20 / 4  12 / 4  12 / 4  8 / 8  12 / 8  12 / 8
#   crossover     r 31 suppress_tile_kernel; r 31.4, 31.9, 32 suppress_global_kernel (one round per launch)
#                 honey64 8, 8, 8, 8 launches; plateaus_u8 12, 12, 12, 12
#   clipped       20 x 150 r 40 tiled (50 824 B) 4 launches; 150 x 20 r 40 tiled (60 904 B) 4 (float32) and 8 (uint8);
#                 20 x 20 r 1000 tiled (33 620 B) 4; 40 x 40 r 1e6 global (91 700 B would be needed) 4; 3 x 200 r 17 tiled 4;
#                 96 x 160 r 0 tiled (5 120 B, no offsets) 4
#   chains        48 x 130, 1 472 candidates, tiled            r 2     2.9     17
#                 boustrophedon                                8       4       8
#                 permutation                                  4       4       4
#                 (a tile settles its own chains in LDS within one launch; only what crosses a border costs another)
#   value edges   40 x 100 at r 1.5 and 5, determinism 96 x 160 at r 24.5, capacity 96 x 160 at r 9: all tiled
ROUNDS_PER_CHECK = 4


def same_rows(got, want):
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)


def launches():
    return int(_native.load().zk_local_max_last_launches())


def device_rows(image, r, t=None):
    """local_max_device of a torch copy of ``image``, back on the host as int64 rows."""
    import torch
    pts = resident.local_max_device(torch.from_numpy(np.ascontiguousarray(image)).cuda(), r, t)
    assert pts.dtype == torch.int32 and pts.is_cuda
    return pts.cpu().numpy().astype(np.int64).reshape(-1, 2)


@pytest.fixture(scope="module")
def wide():
    """{name: (image, mid-range threshold)} of the two 96 x 160 frames, with the oracle's results memoised per (name, r, t)."""
    frames = {name: (img, mid) for name, img, mid in lmc.wide_frames()}
    memo = {}

    def oracle(name, r, t):
        if (name, r, t) not in memo:
            memo[name, r, t] = lmo.local_max_raster(frames[name][0], r, t)
            memo[name, r, t].setflags(write=False)
        return memo[name, r, t]
    return frames, oracle


@pytest.mark.parametrize("r", lmc.WIDE_RADII)
@pytest.mark.parametrize("name", ["honey64", "plateaus_u8"])
def test_wide_halos_stay_on_the_tiled_kernel(wide, name, r):
    frames, oracle = wide
    img, mid = frames[name]
    assert img.shape == lmc.FRAME and lmo.tile_lds_bytes(r, *img.shape) <= lmo.TILE_LDS_MAX
    for t in (None, mid):
        want = oracle(name, r, t)
        same_rows(local_max(img, r, t), want)
        print(f"{name} r {r} t {t}: {len(want)} points, {launches()} launches, {lmo.tile_lds_bytes(r, *img.shape)} B")
        assert len(want) >= 8


@pytest.mark.parametrize("name", ["honey64", "plateaus_u8"])
def test_crossover_between_the_tiled_and_the_global_kernel(wide, name):
    frames, oracle = wide
    img, _ = frames[name]
    tiled = [lmo.tile_lds_bytes(r, *img.shape) <= lmo.TILE_LDS_MAX for r in lmc.CROSSOVER_RADII]
    assert lmc.CROSSOVER_RADII == (31, 31.4, 31.9, 32) and tiled == [True, False, False, False]
    for r in lmc.CROSSOVER_RADII:
        same_rows(local_max(img, r), oracle(name, r, None))
        print(f"{name} r {r}: {launches()} launches")


@pytest.mark.parametrize("case", lmc.CLIPPED, ids=[c[0] for c in lmc.CLIPPED])
def test_halos_clipped_to_the_frame(case):
    name, shape, r, tiled = case
    assert (lmo.tile_lds_bytes(r, *shape) <= lmo.TILE_LDS_MAX) == tiled
    for kind, img in lmc.clipped_frames(shape):
        want = lmo.local_max_raster(img, r)
        got = local_max(img, r)
        same_rows(got, want)
        print(f"{name} {kind}: {len(want)} points, {launches()} launches, {lmo.tile_lds_bytes(r, *shape)} B")
        if name == "all_in_reach":
            assert len(got) == 1
        if name == "radius_zero":
            assert lmo.tile_lds_bytes(0, *shape) == lmo.TILE_W * lmo.TILE_H * 5        # no offsets
            assert len(got) == lmo.candidate_mask(img).sum() > 100
        if name == "three_rows":
            assert len(got) >= 3


@pytest.mark.parametrize("r", lmc.CHAIN_RADII)
@pytest.mark.parametrize("pattern", ["boustrophedon", "permutation"])
def test_chains_across_tile_borders(pattern, r):
    img = lmc.chain_frame(pattern)
    n_cand = int(lmo.candidate_mask(img).sum())
    assert img.shape == (48, 130) and n_cand == 23 * 64 and lmo.tile_lds_bytes(r, *img.shape) <= lmo.TILE_LDS_MAX
    same_rows(local_max(img, r), lmo.local_max_raster(img, r))
    n = launches()
    print(f"{pattern} r {r}: {n} launches for {n_cand} candidates")
    # every launch resolves the highest-priority undecided candidate at least, and the host looks every 4 launches
    assert n > 0 and n % ROUNDS_PER_CHECK == 0 and n <= n_cand + ROUNDS_PER_CHECK


def both_entries(img, r, t=None):
    """local_max and local_max_device against the oracle (the value-edge frames: the tiled kernel)."""
    assert lmo.tile_lds_bytes(r, *img.shape) <= lmo.TILE_LDS_MAX
    want = lmo.local_max_raster(img, r, t)
    same_rows(local_max(img, r, t), want)
    same_rows(device_rows(img, r, t), want)
    return want


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_signed_zeros_tie(dtype, r):
    img = lmc.signed_zeros(dtype)
    assert len(both_entries(img, r)) <= 7                      # threshold 0: the peaks alone
    want = both_entries(img, r, -1.0)                           # every zero off the peaks is a candidate, all tied
    zeros = want[img[want[:, 1], want[:, 0]] == 0]
    assert len(zeros) > 20 and np.signbit(img[zeros[:, 1], zeros[:, 0]]).any() and not np.signbit(img[zeros[:, 1], zeros[:, 0]]).all()


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
def test_one_ulp_apart_needs_the_64_bit_key(r):
    img, pairs = lmc.ulp_pairs()
    kept = set(map(tuple, both_entries(img, r).tolist()))
    for big, small, apart in pairs:
        assert big in kept and ((small in kept) == (apart > r)), (big, small)


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_infinite_pixels(dtype, r):
    img = lmc.infinities(dtype)
    want = both_entries(img, r)
    assert np.isposinf(img[want[:, 1], want[:, 0]]).sum() >= 4
    both_entries(img, r, 0.0)


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_frames_negative_everywhere(dtype, r):
    assert len(both_entries(lmc.all_negative(dtype), r)) > 10


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
def test_int16_with_thresholds_about_zero(r):
    img = lmc.int16_about_zero()
    counts = [len(both_entries(img, r, t)) for t in lmc.INT16_THRESHOLDS]
    assert lmc.INT16_THRESHOLDS == (-1, -0.5, 0) and counts[0] > 0 and counts[2] > 0


@pytest.mark.parametrize("r", lmc.EDGE_RADII)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_rule(dtype, r):
    frames = lmc.nan_frames(dtype)
    assert set(frames) == {"scattered", "beside_a_peak", "on_the_border", "all_nan", "nan_and_constant"}
    for name, img in frames.items():
        for t in (None, 0.3):
            want = both_entries(img, r, t)
            assert not np.isnan(img[want[:, 1], want[:, 0]]).any()
            assert (len(want) == 0) == (name in ("all_nan", "nan_and_constant")), name
    beside = {tuple(p) for p in lmo.local_max_raster(frames["beside_a_peak"], r).tolist()}
    assert {(20, 10), (70, 20), (42, 30)} <= beside and ((40, 30) in beside) == (r < 2)


def test_two_calls_and_a_side_stream_are_byte_identical():
    import torch
    img, r = lmc.plateaus_u8(), 24.5
    assert lmo.tile_lds_bytes(r, *img.shape) <= lmo.TILE_LDS_MAX
    want = lmo.local_max_raster(img, r)
    first, second = local_max(img, r), local_max(img, r)
    dev = torch.from_numpy(img).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pts = resident.local_max_device(dev, r)
    side.synchronize()
    third = pts.cpu().numpy().astype(np.int64)
    same_rows(first, want)
    assert first.tobytes() == second.tobytes() == third.tobytes()


def test_capacity_contract_of_the_c_abi():
    """capacity 0 with no output counts; capacity < n writes the first capacity rows in priority order and nothing more;
    refusals carry a message and leave the library usable."""
    import torch
    lib = _native.load()
    img = lmc.honey64()
    h, w = img.shape
    r = 9.0
    want = lmo.local_max_raster(img, r)
    n = len(want)
    assert n > 16 and lmo.tile_lds_bytes(r, h, w) <= lmo.TILE_LDS_MAX
    dev = torch.from_numpy(img).cuda()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    found = c_int64(-1)

    def host(capacity, out, radius=r):
        found.value = -1
        return lib.zk_local_max(0, img.ctypes.data_as(c_void_p), _native.ZK_F64, h, w, radius, 0, 0.0,
                                None if out is None else out.ctypes.data_as(c_void_p), capacity, byref(found))

    def device(capacity, out, radius=r):
        found.value = -1
        return lib.zk_local_max_dev(0, c_void_p(dev.data_ptr()), _native.ZK_F64, h, w, radius, 0, 0.0,
                                    None if out is None else c_void_p(out.data_ptr()), capacity, byref(found), stream)

    # a pure count
    assert host(0, None) == 0 and found.value == n
    assert device(0, None) == 0 and found.value == n
    # a short buffer: the prefix in priority order, the rest untouched
    out = np.full((n, 2), -7, dtype=np.int64)
    assert host(n - 3, out) == 0 and found.value == n
    np.testing.assert_array_equal(out[:n - 3], want[:n - 3])
    assert (out[n - 3:] == -7).all()
    out_dev = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    assert device(n - 3, out_dev) == 0 and found.value == n
    torch.cuda.synchronize()
    got = out_dev.cpu().numpy()
    np.testing.assert_array_equal(got[:n - 3], want[:n - 3])
    assert (got[n - 3:] == -7).all()
    # refusals
    for call in (host, device):
        assert call(4, None) == _native.ZK_E_BADARG and "output" in _native.last_error()
        assert call(-1, None) == _native.ZK_E_BADARG and _native.last_error()
        for bad in (-1.0, float("inf"), float("nan")):
            assert call(0, None, bad) == _native.ZK_E_BADARG and "min_distance" in _native.last_error()
    # ... and a valid call afterwards
    full = np.full((n + 2, 2), -7, dtype=np.int64)
    assert host(n + 2, full) == 0 and found.value == n
    np.testing.assert_array_equal(full[:n], want)
    assert (full[n:] == -7).all()
    full_dev = torch.full((n + 2, 2), -7, dtype=torch.int32, device="cuda")
    assert device(n + 2, full_dev) == 0 and found.value == n
    torch.cuda.synchronize()
    np.testing.assert_array_equal(full_dev.cpu().numpy()[:n], want)
    assert (full_dev.cpu().numpy()[n:] == -7).all()
