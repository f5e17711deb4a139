"""mtflearn_amd.features.com_refine_points / distributed.com_refine_device on the GPU against tests/golden/com_refine.npz (the
reference's ``com_refine`` with the thresholds of tests/thresholds_reference.py, made by tests/make_golden_com_refine.py) on
every case of tests/com_refine_cases.py, for both thresholds; the cases hold float32 and float64 frames.

Bounds, for the parity cases (no window is left out; the generator asserts their conditioning):
  Otsu thresholds   bit-equal (a bin centre).
  Li iterations     equal.
  Li thresholds     within 1e-12 of the window's range (what tests/test_gpu_estimate_d.py holds Li to).
  refined points    within 1e-10 px: the kept values of these non-negative frames give sums of relative error at most
                    n * 2^-53 <= 4.6e-13 in any order, the coordinates are below 64, so two such sums stay under 6e-11.
The branch cases (degenerate windows, negative data, windows on the frame's edges) compare NaN positions exactly and finite
values at 1e-9.  The GPU tests read only the golden file: neither SciPy nor scikit-image is needed here."""
import os
from ctypes import c_void_p

import numpy as np
import pytest

import com_refine_cases as cc
from conftest import ROOT
from mtflearn_amd import _native, distributed, features, graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "com_refine.npz")) as f:
        return {k: f[k] for k in f.files}


def to_host(a):
    return a.numpy() if isinstance(a, _native.DeviceArray) else a.cpu().numpy()


def resident(a, kind):
    if kind == "native":
        return _native.DeviceArray.from_numpy(a)
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def any_window(frame, pts, size, threshold):
    """``zk_com_refine`` on the windows of ``pts`` without border clearing, finished as the host function finishes:
    ``(points, thresholds, iterations)``."""
    first = np.ascontiguousarray(cc.corners(pts, size))
    frame = np.ascontiguousarray(frame)
    moved, levels, steps = np.empty((len(pts), 2)), np.empty(len(pts)), np.empty(len(pts), np.int32)
    _native.check(_native.load().zk_com_refine(0, frame.ctypes.data_as(c_void_p), _native.dtype_code(frame.dtype), *frame.shape,
                                               first.ctypes.data_as(c_void_p), len(first), size,
                                               _native.THRESHOLD_OTSU if threshold == "otsu" else _native.THRESHOLD_LI,
                                               moved.ctypes.data_as(c_void_p), levels.ctypes.data_as(c_void_p), steps.ctypes.data_as(c_void_p)),
                  "zk_com_refine")
    return (moved - size / 2) + pts, levels, steps


def spans(frame, pts, size):
    w = cc.windows(frame, pts, size)
    return w.max(axis=(1, 2)) - w.min(axis=(1, 2))


@pytest.mark.parametrize("threshold", cc.THRESHOLDS)
@pytest.mark.parametrize("name", cc.PARITY)
def test_parity_cases_against_the_golden_file(golden, name, threshold):
    frame, pts, size = cc.cases()[name]
    rule = None if threshold == "li" else "otsu"
    xy, t, it = features.com_refine_points(pts, frame, size, rule, return_thresholds=True)
    want_xy, want_t, want_it = (golden[f"{name}/{threshold}/{k}"] for k in ("xy", "t", "it"))
    assert xy.shape == want_xy.shape and xy.dtype == np.float64 and it.dtype == np.int32
    t_err = np.abs(t - want_t) / spans(frame, pts, size)
    print(f"{name} {threshold}: iterations differ in {int((it != want_it).sum())}, threshold error {t_err.max():.3g} of the range, "
          f"points {np.abs(xy - want_xy).max():.3g} px")
    assert np.array_equal(it, want_it)
    if threshold == "otsu":
        assert np.array_equal(t.view(np.int64), want_t.view(np.int64))
    else:
        assert t_err.max() <= 1e-12
    assert np.abs(xy - want_xy).max() <= 1e-10
    assert np.array_equal(features.com_refine_points(pts, frame, size, rule), xy)               # without the thresholds: the same points
    # the entry point that takes any window agrees bit for bit, and so does a second run
    again = any_window(frame, pts, size, threshold)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (xy, t, it)))


@pytest.mark.parametrize("threshold", cc.THRESHOLDS)
@pytest.mark.parametrize("name", cc.BRANCHES)
def test_branch_cases_against_the_golden_file(golden, name, threshold):
    frame, pts, size = cc.cases()[name]
    xy, t, it = any_window(frame, pts, size, threshold)
    want_xy, want_t, want_it = (golden[f"{name}/{threshold}/{k}"] for k in ("xy", "t", "it"))
    for got, want in ((xy, want_xy), (t, want_t)):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), name
        assert np.abs(got[~nan] - want[~nan]).max(initial=0.0) <= 1e-9, name
    assert np.array_equal(it, want_it)
    second = any_window(frame, pts, size, threshold)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(second, (xy, t, it)))
    for kind in ("native", "torch"):                                                           # the resident route: the same bits
        out = distributed.com_refine_device(resident(frame, kind), resident(pts, kind), size, None if threshold == "li" else "otsu")
        assert to_host(out).tobytes() == xy.tobytes(), (name, kind)


@pytest.mark.parametrize("kind", ("native", "torch"))
@pytest.mark.parametrize("name", ("bumps_f32_peaks_size2", "bumps_f64_random_size3", "bumps_f32_peaks_size16", "bumps_f64_random_size17",
                                  "bumps_f64_size64", "n65", "honeycomb_512_size8", "honeycomb_512_size9", "honeycomb_512_f32_size24"))
def test_host_and_resident_routes_are_bit_equal(name, kind):
    frame, pts, size = cc.cases()[name]
    for rule in (None, "otsu"):
        host = features.com_refine_points(pts, frame, size, rule)
        out = distributed.com_refine_device(resident(frame, kind), resident(pts, kind), size, rule)
        assert isinstance(out, _native.DeviceArray) if kind == "native" else out.is_cuda
        assert tuple(out.shape) == (len(pts), 2) and to_host(out).dtype == np.float64
        assert to_host(out).tobytes() == host.tobytes(), (name, rule)


def test_a_window_outside_the_frame_raises_and_the_next_call_succeeds(golden):
    import torch
    name, extra = cc.OUTSIDE
    frame, pts, size = cc.cases()[name]
    both = np.concatenate([pts, extra])
    for bad in (both, np.concatenate([[[2.0, 40.0]], pts]), np.concatenate([pts, [[30.0, 94.0]]]), np.concatenate([pts, [[30.0, -50.0]]]),
                np.concatenate([pts, [[np.nan, 40.0]]]), np.concatenate([pts, [[1e300, 40.0]]])):
        for kind in ("native", "torch"):                                                       # checked on the device: nothing is read out of bounds
            for rule in (None, "otsu"):
                with pytest.raises(ValueError, match="leaves the frame"):
                    distributed.com_refine_device(resident(frame, kind), resident(bad, kind), size, rule)
    with pytest.raises(RuntimeError, match="leaves the frame"):
        any_window(frame, both, size, "li")
    assert len(features.com_refine_points(both, frame, size)) == len(pts)                       # the host function clears the border
    with pytest.raises(ValueError, match="float"):
        distributed.com_refine_device(torch.zeros(32, 32, dtype=torch.int16).cuda(), resident(pts[:1], "torch"), size)
    with pytest.raises(TypeError, match="int32 or float64"):
        distributed.com_refine_device(resident(frame, "torch"), resident(pts.astype(np.float32), "torch"), size)
    for bad_size in (1, 65):
        with pytest.raises(ValueError, match="size"):
            distributed.com_refine_device(resident(frame, "torch"), resident(pts, "torch"), bad_size)
    with pytest.raises(ValueError, match="2\\^24"):
        distributed.com_refine_device(resident(frame, "torch"), torch.zeros((2 ** 24, 2), dtype=torch.int32).cuda(), size)
    assert tuple(distributed.com_refine_device(resident(frame, "torch"), resident(pts[:0], "torch"), size).shape) == (0, 2)
    for kind in ("native", "torch"):
        out = distributed.com_refine_device(resident(frame, kind), resident(pts, kind), size)
        assert np.abs(to_host(out) - golden[f"{name}/li/xy"]).max() <= 1e-10


@pytest.mark.parametrize("dtype", (np.float32, np.float64))
@pytest.mark.parametrize("size", (2, 4, 5))
def test_corner_int32_and_float64_routes_share_one_window(size, dtype):
    """The corner entry point, int32 points and float64 points on the same windows, on the frame's edges and at rint's ties: the
    same bytes once the corner route is finished as the host finishes it, ``(c - size / 2) + p``."""
    frame = (np.random.default_rng(size).random(cc.EDGE_SHAPE) + 0.5).astype(dtype)
    ints, reals = cc.edge_points(size)
    for threshold in cc.THRESHOLDS:
        rule = None if threshold == "li" else "otsu"
        for pts in (ints, reals):
            want = any_window(frame, pts, size, threshold)[0]
            got = to_host(distributed.com_refine_device(resident(frame, "native"), resident(pts, "native"), size, rule))
            assert np.isfinite(want).all() and got.tobytes() == want.tobytes(), (threshold, pts.dtype)


def test_a_window_one_pixel_outside_raises_for_int32_and_float64_points():
    size = 4
    frame = np.random.default_rng(4).random(cc.EDGE_SHAPE) + 0.5
    ints, reals = cc.edge_points(size)
    for k, step in cc.ONE_PIXEL_OUT:
        for pts in (ints, reals):
            bad = pts.copy()
            bad[k] += step
            with pytest.raises(ValueError, match="leaves the frame"):
                distributed.com_refine_device(resident(frame, "native"), resident(bad, "native"), size)
            with pytest.raises(RuntimeError, match="leaves the frame"):
                any_window(frame, bad, size, "li")
            good = to_host(distributed.com_refine_device(resident(frame, "native"), resident(pts, "native"), size))   # the next call succeeds
            assert good.tobytes() == any_window(frame, pts, size, "li")[0].tobytes()


def test_resident_chain_local_max_com_refine_bonds():
    """local_max_device -> com_refine_device -> vnn_graph_device on the 512^2 frame: frame and points stay on the device; the
    refined points equal the host function's on the same key points and feed the bonds."""
    import torch
    from mtflearn_amd.features.keypoints import clear_border
    frame = cc.rc.frame_512()
    d_frame = torch.from_numpy(frame).cuda()
    d_all = distributed.local_max_device(d_frame, min_distance=4, threshold=float(frame.mean()))
    keep = np.ascontiguousarray(clear_border(d_all.cpu().numpy(), frame.shape, 9))
    d_pts = torch.from_numpy(keep).cuda()
    assert d_pts.dtype == torch.int32 and len(keep) > 1000
    for rule in (None, "otsu"):
        d_xy = distributed.com_refine_device(d_frame, d_pts, 9, rule)
        assert d_xy.is_cuda and d_xy.dtype == torch.float64 and tuple(d_xy.shape) == (len(keep), 2)
        host = features.com_refine_points(keep, frame, 9, rule)
        assert d_xy.cpu().numpy().tobytes() == host.tobytes() and np.abs(host - keep).max() < 4.5
        d_ijs = distributed.vnn_graph_device(d_xy, threshold_method="otsu")
        ijs = graph.vnn_graph(host, threshold_method="otsu")
        assert np.array_equal(d_ijs.cpu().numpy(), ijs) and len(ijs) > len(keep)
