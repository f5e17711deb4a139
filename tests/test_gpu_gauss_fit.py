"""mtflearn_amd.features.gaussian_fit_points / resident.gaussian_fit_device on the GPU against tests/golden/gauss_fit.npz (SciPy's
converged minimisers and the NumPy oracle's own errors, made by tests/make_golden_gauss_fit.py) and against the NumPy oracle
of tests/gauss_fit_oracle.py.  Neither SciPy nor the generator is needed here.

Bounds:
  parity     every point of the 36 parity cases ends with status 0 and lies within max(100 * d0, 1e-12) of SciPy's minimiser,
             column by column (x, y, A, a, b, c, g, rss) scaled by |p| + 1: the project's rule of 100 x the reference's own
             error (denoise).  d0 = 3.9e-10 is stored in the golden file.  Iterations are not compared: exp differs by
             an ulp and an accept / reject tie may fall the other way.
  recovery   the known truth of isolated noise-free Gaussians within 100 x the error the NumPy oracle shows on the same windows
             (stored: 1.3e-16 circular, 1.4e-16 elliptical, both of |p| + 1).
  sizes      on isolated noise-free Gaussians at every size where the lane mapping changes, the device against the oracle on the
             same windows within the parity bound, status 0 on both.
The observed figures are printed by each test and copied into DESIGN.md."""
import os
from ctypes import c_void_p

import numpy as np
import pytest

import gauss_fit_cases as gc
import gauss_fit_oracle as go
from conftest import ROOT
from mtflearn_amd import _native, features, resident

pytestmark = pytest.mark.gpu

COLUMNS = ("x", "y", "amplitude", "sigma_major", "sigma_minor", "theta", "background", "rss")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "gauss_fit.npz")) as f:
        return {k: f[k] for k in f.files}


def to_host(a):
    return a.numpy() if isinstance(a, _native.DeviceArray) else a.cpu().numpy()


def on_device(a, kind):
    if kind == "native":
        return _native.DeviceArray.from_numpy(np.ascontiguousarray(a))
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def table(fit):
    """The (M, 8) table of a GaussianFit, columns as the library writes them."""
    return np.column_stack([fit.xy, fit.amplitude, fit.sigma, fit.theta, fit.background, fit.rss])


def compared(params):
    a, b, c = gc.precision(params[:, 3], params[:, 4], params[:, 5])
    return np.stack([params[:, 0], params[:, 1], params[:, 2], a, b, c, params[:, 6], params[:, 7]], axis=1)


def on_corners(frame, pts, size, model="elliptical", mode=None, sigma=None, tol=1e-10, max_iter=100):
    """``zk_gauss_fit`` on the windows of ``pts``: ``(params, iterations, status)``."""
    first = np.ascontiguousarray(go.corners(pts, size), dtype=np.int32)
    frame = np.ascontiguousarray(frame)
    params, its, status = np.empty((len(first), 8)), np.empty(len(first), np.int32), np.empty(len(first), np.int32)
    _native.check(_native.load().zk_gauss_fit(0, frame.ctypes.data_as(c_void_p), _native.dtype_code(frame.dtype), *frame.shape,
                                              first.ctypes.data_as(c_void_p), len(first), size, _native.GAUSS_MODELS[model],
                                              _native.GAUSS_DISK if mode == "disk" else _native.GAUSS_BOX, size / 4 if sigma is None else sigma,
                                              tol, max_iter, params.ctypes.data_as(c_void_p), its.ctypes.data_as(c_void_p),
                                              status.ctypes.data_as(c_void_p)), "zk_gauss_fit")
    return params, its, status


def on_resident(frame, pts, size, kind, **kw):
    return tuple(to_host(a) for a in resident.gaussian_fit_device(on_device(frame, kind), on_device(pts, kind), size, **kw))


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_parity_with_scipys_minimisers_on_every_case(golden):
    bound = max(100 * float(golden["d0"]), 1e-12)
    worst, worst_rss, most = 0.0, 0.0, 0
    for name, (frame, pts, size, model, mode) in gc.parity_cases().items():
        fit = features.gaussian_fit_points(pts, frame, size, model=model, mode=mode)
        assert np.array_equal(fit.kept, np.arange(len(pts))) and fit.xy.shape == (16, 2), name
        got, want = compared(table(fit)), golden[f"{name}/scipy"]
        d, d_rss = gc.scaled_distance(got[:, :7], want[:, :7]), gc.scaled_distance(got[:, 7], want[:, 7])
        print(f"{name}: parameters {d:.3g}, rss {d_rss:.3g} of |p| + 1; iterations {fit.iterations.min()} .. {fit.iterations.max()} "
              f"(oracle {golden[f'{name}/iterations'].min()} .. {golden[f'{name}/iterations'].max()})")
        worst, worst_rss, most = max(worst, d), max(worst_rss, d_rss), max(most, int(fit.iterations.max()))
        assert (fit.status == 0).all(), (name, fit.status)
        assert d <= bound and d_rss <= bound, name
        if model == "circular":
            assert np.array_equal(fit.sigma[:, 0], fit.sigma[:, 1]) and (fit.theta == 0).all()
        else:
            assert (fit.sigma[:, 0] >= fit.sigma[:, 1]).all() and (fit.theta > -np.pi / 2).all() and (fit.theta <= np.pi / 2).all()
    print(f"all parity cases: parameters {worst:.3g}, rss {worst_rss:.3g}, bound {bound:.3g}, most iterations {most}")


@pytest.mark.parametrize("model", gc.MODELS)
def test_exact_recovery_of_isolated_gaussians(golden, model):
    """The truth of one noise-free Gaussian per window within 100 x the oracle's own error on these windows (1.3e-16 circular,
    1.4e-16 elliptical of |p| + 1, measured by tests/make_golden_gauss_fit.py)."""
    frame, pts, truth = gc.recovery_case(model)
    fit = features.gaussian_fit_points(pts, frame, gc.RECOVERY_SIZE, model=model, clear=False)
    err, bound = gc.recovery_error(table(fit), truth), 100 * float(golden[f"recovery/{model}/oracle_error"])
    print(f"recovery {model}: error {err:.3g} of |p| + 1, bound {bound:.3g}, rss {fit.rss.max():.3g}, iterations {fit.iterations.max()}")
    assert (fit.status == 0).all()
    assert err <= bound


SIZES = tuple(("box", s) for s in (3, 4, 8, 9, 11, 12, 16, 17, 22, 23, 32)) + tuple(("disk", s) for s in (5, 9, 31))


@pytest.mark.parametrize("mode,size", SIZES)
def test_window_sizes_where_the_lane_mapping_changes(golden, mode, size):
    bound = max(100 * float(golden["d0"]), 1e-12)
    width = max(0.8, size / 6)
    frame, pts, _ = gc.isolated(size, ((1.2 * width, width, 0.6), (width, width, 0.0), (1.1 * width, 0.9 * width, -1.2)), frame_shape=(32, 96))
    mode = None if mode == "box" else mode
    for model in gc.MODELS:
        want, _, want_status, _ = go.fit_points(pts, frame, size, model, mode)
        got, its, status = on_corners(frame, pts, size, model, mode)
        d = gc.scaled_distance(compared(got), compared(want))
        print(f"size {size} {mode} {model}: {d:.3g} of |p| + 1 from the oracle, iterations {its}")
        assert (want_status == 0).all() and (status == 0).all()
        assert d <= bound
        assert same_bits(on_corners(frame, pts, size, model, mode), (got, its, status))                 # a second run
        for kind in ("native", "torch"):
            assert same_bits(on_resident(frame, pts, size, kind, model=model, mode=mode), (got, its, status)), kind


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 257))
def test_point_counts(n):
    frame, sites = gc.lattice_frame(0.02)
    frame = frame.astype(np.float32)
    pts = np.ascontiguousarray(sites[np.arange(n) % len(sites)])
    every = features.gaussian_fit_points(sites, frame, 7, model="circular")
    fit = features.gaussian_fit_points(pts, frame, 7, model="circular")
    assert len(fit.xy) == n and (fit.status == 0).all()
    assert table(fit).tobytes() == table(every)[np.arange(n) % len(sites)].tobytes()                     # a fit does not depend on its neighbours in the batch
    assert np.array_equal(fit.iterations, every.iterations[np.arange(n) % len(sites)])


def test_windows_on_the_frame_borders():
    """Corners 0 and W - size / H - size: the four corner windows of a frame, odd and even size, against the oracle."""
    rng = np.random.default_rng(5)
    for size, shape in ((7, (23, 31)), (8, (24, 30))):
        frame = gc.BACKGROUND + rng.normal(0, 0.01, shape)
        half = size // 2
        pts = np.array([(half, half), (shape[1] - size + half, half), (half, shape[0] - size + half),
                        (shape[1] - size + half, shape[0] - size + half)], dtype=np.int32)
        first = go.corners(pts, size)
        assert first.min() == 0 and (first[:, 0] + size).max() == shape[1] and (first[:, 1] + size).max() == shape[0]
        for (cx, cy), (px, py) in zip(first, pts):
            frame[cy:cy + size, cx:cx + size] += gc.gaussian((size, size), px + 0.3, py - 0.2, 1.0, *gc.precision(1.6, 1.3, 0.4), origin=(cx, cy))
        fit = features.gaussian_fit_points(pts, frame, size, clear=False)
        want = go.fit_points(pts, frame, size)[0]
        assert (fit.status == 0).all() and gc.scaled_distance(compared(table(fit)), compared(want)) <= 1e-6
        assert np.abs(fit.xy - (pts + [0.3, -0.2])).max() < 0.05
        for kind in ("native", "torch"):
            assert on_resident(frame, pts, size, kind)[0].tobytes() == table(fit).tobytes()
        assert len(features.gaussian_fit_points(pts, frame, size).xy) == 0                                # the border clearing drops them all


def test_rounding_of_points():
    """int32 points and float64 points that round to the same corner give the same bits; x.5 rounds to even."""
    frame, sites = gc.lattice_frame(0.02)
    shifted = sites + np.tile([[0.3, -0.4], [-0.49, 0.49]], (8, 1))
    want = table(features.gaussian_fit_points(sites, frame, 9))
    assert table(features.gaussian_fit_points(shifted, frame, 9)).tobytes() == want.tobytes()
    for kind in ("native", "torch"):
        assert on_resident(frame, shifted, 9, kind)[0].tobytes() == want.tobytes()
        assert on_resident(frame, sites.astype(np.float64), 9, kind)[0].tobytes() == want.tobytes()
        assert on_resident(frame, sites, 9, kind)[0].tobytes() == want.tobytes()
    halves = sites + np.tile([[0.5, 0.5], [-0.5, 0.5]], (8, 1))                                         # 14.5 -> 14 (half up: 15), 13.5 -> 14 (half down: 13)
    even = np.rint(halves).astype(np.int32)
    assert np.array_equal(even, sites) and (sites % 2 == 0).all()
    want = table(features.gaussian_fit_points(even, frame, 9))
    assert table(features.gaussian_fit_points(halves, frame, 9)).tobytes() == want.tobytes()
    for kind in ("native", "torch"):
        assert on_resident(frame, halves, 9, kind)[0].tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("size", (3, 4, 5))
def test_corner_int32_and_float64_routes_share_one_window(size, dtype):
    """The corner entry point, int32 points and float64 points on the windows of tests/com_refine_cases.py ``edge_points`` (the
    frame's four edges, rint's ties at even and odd k): parameters, iterations and status byte for byte.  Beside
    ``test_rounding_of_points`` and ``test_windows_on_the_frame_borders``, which hold the same at size 9 inside a 64^2 frame and at
    sizes 7 / 8 for int32 points in the frame's corners."""
    import com_refine_cases as cc
    frame = (np.random.default_rng(size).random(cc.EDGE_SHAPE) + 0.5).astype(dtype)
    ints, reals = cc.edge_points(size)
    for model in gc.MODELS:
        want = on_corners(frame, ints, size, model)
        assert same_bits(on_corners(frame, reals, size, model), want)
        for pts in (ints, reals):
            assert same_bits(on_resident(frame, pts, size, "native", model=model), want), (model, pts.dtype)


def test_a_window_one_pixel_outside_is_refused_for_int32_and_float64_points():
    import com_refine_cases as cc
    size = 4
    frame = np.random.default_rng(4).random(cc.EDGE_SHAPE) + 0.5
    ints, reals = cc.edge_points(size)
    want = on_corners(frame, ints, size)
    for k, step in cc.ONE_PIXEL_OUT:
        for pts in (ints, reals):
            bad = pts.copy()
            bad[k] += step
            with pytest.raises(ValueError, match="leaves the frame"):
                resident.gaussian_fit_device(on_device(frame, "native"), on_device(bad, "native"), size)
            with pytest.raises(RuntimeError, match="leaves the frame"):
                on_corners(frame, bad, size)
            assert same_bits(on_resident(frame, pts, size, "native"), want)                               # the next call succeeds


def test_status_paths():
    frame, sites = gc.lattice_frame(0.02)
    usual = features.gaussian_fit_points(sites, frame, 9)
    one = features.gaussian_fit_points(sites, frame, 9, max_iter=1)                                      # status 1, finite parameters
    assert (one.status == 1).all() and (one.iterations == 1).all() and np.isfinite(table(one)).all()
    want = go.fit_points(sites, frame, 9, max_iter=1)
    assert gc.scaled_distance(compared(table(one)), compared(want[0])) <= 1e-9 and (want[2] == 1).all()
    spoiled = frame.copy()
    spoiled[20:31, 20:31] = 0.25                                                                         # the window of site 5 (26, 26): constant
    spoiled[38, 50] = np.nan                                                                             # in the window of site 11 (50, 38)
    spoiled[50, 14] = np.inf                                                                             # site 12 (14, 50)
    fit = features.gaussian_fit_points(sites, spoiled, 9)
    want = np.zeros(16, np.int32)
    want[[5, 11, 12]] = 2, 3, 3
    touched = np.array([np.isin(k, (5, 11, 12)) or not np.array_equal(go.windows(spoiled, sites[k:k + 1], 9), go.windows(frame, sites[k:k + 1], 9))
                        for k in range(16)])
    assert np.array_equal(fit.status[[5, 11, 12]], [2, 3, 3]) and (fit.status[~touched] == 0).all()
    assert np.isnan(table(fit)[[11, 12]]).all() and (fit.iterations[[5, 11, 12]] == 0).all()
    assert np.array_equal(table(fit)[5, [0, 1, 2, 5, 6, 7]], [26.0, 26.0, 0.0, 0.0, 0.25, 0.0])           # the start, sigma0 = 9 / 4
    assert np.abs(table(fit)[5, 3:5] - 2.25).max() <= 1e-14
    assert table(fit)[~touched].tobytes() == table(usual)[~touched].tobytes() and (~touched).sum() >= 10  # the neighbours are unaffected
    assert np.array_equal(fit.status[~touched], go.fit_points(sites, spoiled, 9)[2][~touched])
    assert np.array_equal(go.fit_points(sites, spoiled, 9)[2][[5, 11, 12]], [2, 3, 3])


def test_a_window_outside_the_frame_is_refused_on_both_routes():
    frame, sites = gc.lattice_frame(0.0)
    bad = np.concatenate([sites[:3], [[61, 30]], sites[3:6]]).astype(np.int32)
    with pytest.raises(ValueError, match="inside the frame"):
        features.gaussian_fit_points(bad, frame, 9, clear=False)                                         # the host route: before any launch
    with pytest.raises(RuntimeError, match="leaves the frame"):
        on_corners(frame, bad, 9)
    assert np.array_equal(features.gaussian_fit_points(bad, frame, 9).kept, [0, 1, 2, 4, 5, 6])           # cleared, not refused
    for kind in ("native", "torch"):
        for pts in (bad, bad.astype(np.float64), np.concatenate([sites[:2], [[np.nan, 30.0]]]), np.concatenate([sites[:2], [[1e300, 30.0]]]),
                    np.concatenate([sites[:2], [[30.0, -50.0]]])):
            with pytest.raises(ValueError, match="leaves the frame"):
                resident.gaussian_fit_device(on_device(frame, kind), on_device(pts, kind), 9)
        good = on_resident(frame, sites, 9, kind)                                                          # the next call succeeds
        assert (good[2] == 0).all()
    # nothing is written for the refused point: its rows keep what the output arrays held
    import torch
    lib = _native.load()
    d_frame, d_pts = torch.from_numpy(frame).cuda(), torch.from_numpy(bad).cuda()
    params, its, status = torch.full((7, 8), -7.0, dtype=torch.float64).cuda(), torch.full((7,), -7, dtype=torch.int32).cuda(), \
        torch.full((7,), -7, dtype=torch.int32).cuda()
    rc = lib.zk_gauss_fit_points_dev(0, c_void_p(d_frame.data_ptr()), _native.ZK_F64, 64, 64, c_void_p(d_pts.data_ptr()), _native.ZK_I32, 7, 9,
                                     _native.GAUSS_ELLIPTICAL, _native.GAUSS_BOX, 2.25, 1e-10, 100, c_void_p(params.data_ptr()),
                                     c_void_p(its.data_ptr()), c_void_p(status.data_ptr()), c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _native.ZK_E_BADARG
    assert (params.cpu().numpy()[3] == -7.0).all() and its.cpu().numpy()[3] == -7 and status.cpu().numpy()[3] == -7
    assert (status.cpu().numpy()[[0, 1, 2, 4, 5, 6]] == 0).all()
    with pytest.raises(ValueError, match="size"):
        resident.gaussian_fit_device(d_frame, d_pts, 33)
    with pytest.raises(ValueError, match="fitted pixels"):
        resident.gaussian_fit_device(d_frame, d_pts, 3, mode="disk")
    empty = resident.gaussian_fit_device(d_frame, d_pts[:0], 9)
    assert tuple(empty[0].shape) == (0, 8) and tuple(empty[1].shape) == (0,)


def test_determinism_routes_and_border_clearing():
    frame, sites = gc.lattice_frame(0.1)
    extra = np.concatenate([[[2, 30]], sites[:5], [[30, 62]], sites[5:], [[60.0, 3.0]]])                 # three of them near the border
    for frame_t in (frame, frame.astype(np.float32)):
        for model, mode, size in (("elliptical", None, 11), ("circular", "disk", 7), ("elliptical", "disk", 9), ("circular", None, 8)):
            fit = features.gaussian_fit_points(extra, frame_t, size, model=model, mode=mode)
            kept = np.flatnonzero([len(features.keypoints.clear_border(extra[k:k + 1], frame.shape, size)) for k in range(len(extra))])
            assert np.array_equal(fit.kept, kept) and len(kept) == 16 and fit.kept.dtype == np.int64
            again = features.gaussian_fit_points(extra, frame_t, size, model=model, mode=mode)
            assert same_bits(again[:8], fit[:8])                                                           # two runs
            cleared = features.gaussian_fit_points(extra[fit.kept], frame_t, size, model=model, mode=mode, clear=False)
            assert same_bits(cleared[:8], fit[:8])
            corners = on_corners(frame_t, extra[fit.kept], size, model, mode)
            assert same_bits(corners, (table(fit), fit.iterations, fit.status))
            for kind in ("native", "torch"):
                got = resident.gaussian_fit_device(on_device(frame_t, kind), on_device(extra[fit.kept], kind), size, model=model, mode=mode)
                assert all(isinstance(a, _native.DeviceArray) if kind == "native" else a.is_cuda for a in got)
                assert tuple(got[0].shape) == (16, 8) and same_bits(tuple(to_host(a) for a in got), corners), (kind, model, mode)
    kp = features.KeyPoints(extra, frame, 9)
    before = kp.pts.copy()
    assert same_bits(kp.fit_gaussians()[:8], features.gaussian_fit_points(extra, frame, 9)[:8]) and np.array_equal(kp.pts, before)
    assert kp.fit_gaussians(size=7, model="circular").xy.shape == (16, 2)


def test_resident_chain_local_max_gaussian_fit_bonds():
    """local_max_device -> gaussian_fit_device -> vnn_graph_device on a 128^2 honeycomb frame: the points stay on the device, and
    the bonds are as many as the same chain gives through com_refine_device."""
    import torch
    from mtflearn_amd.datasets import HoneyCombLattice
    frame = HoneyCombLattice(size=128, l=12, seed=3).to_image()                                           # float32, sigma l / 4
    assert frame.shape == (128, 128) and frame.dtype == np.float32
    d_frame = torch.from_numpy(frame).cuda()
    d_all = resident.local_max_device(d_frame, min_distance=3, threshold=float(frame.mean()))
    xy = d_all.to(torch.float64)
    margin = 9 // 2 + 1
    inside = (xy[:, 0] > margin) & (xy[:, 0] < 128 - margin) & (xy[:, 1] > margin) & (xy[:, 1] < 128 - margin)
    d_pts = d_all[inside].contiguous()                                                                    # border clearing on the device
    assert d_pts.dtype == torch.int32 and len(d_pts) > 30
    params, its, status = resident.gaussian_fit_device(d_frame, d_pts, 9, model="circular")
    assert params.is_cuda and tuple(params.shape) == (len(d_pts), 8) and bool(torch.isfinite(params).all()) and int(status.max()) <= 2
    assert float((params[:, :2] - d_pts).abs().max()) <= 4.5                                              # a centre stays in its window
    bonds = resident.vnn_graph_device(params[:, :2], threshold_method="otsu")
    through_com = resident.vnn_graph_device(resident.com_refine_device(d_frame, d_pts, 9), threshold_method="otsu")
    print(f"chain: {len(d_pts)} points, {len(bonds)} bonds, {len(through_com)} through com_refine; iterations up to {int(its.max())}")
    assert len(bonds) == len(through_com) and len(bonds) > len(d_pts)
