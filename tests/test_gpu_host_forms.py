"""The host-array entry points with an optional output left out, where no other GPU test leaves it out.

A host form takes its operands up, runs the body of the ``*_dev`` form on the null stream and brings the results down; an
output passed as a null pointer is neither allocated for the caller nor copied.  Both forms run the same kernels on the same
bytes, and none of the bodies below accumulates floating point with atomics (``com_refine`` counts histogram bins with integer
atomics), so what is asked here is bitwise equality: with the ``*_dev`` form where one exists, and with the same host form
called with every output present.

    zk_rows_knn_correlation  without P_out, 65 rows (the 64-row tile is crossed); no ``*_dev`` form: the call with P_out
    zk_tmd_render            frames without masks, and masks without frames (no blur), against ``tmd_frames_device``
    zk_eels_pls              without iterations (and without signal), against the full host call and ``baseline_device``
    zk_com_refine            without thresholds and iterations, against ``com_refine_points`` and ``com_refine_device``

And the five per-device byte knobs of these entry points, at what they refuse: negative bytes, and a device outside the table.
"""
from ctypes import POINTER, c_double, c_int64, c_void_p

import numpy as np
import pytest

import eels_cases as ec
import tmd_cases as tc
from mtflearn_amd import _native, datasets, eels, features, manifold, resident
from mtflearn_amd.clustering import DeviceRows

pytestmark = pytest.mark.gpu


def ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def test_knn_without_affinities():
    x = np.random.default_rng(5).standard_normal((65, 9))
    rows = DeviceRows(x)
    try:
        dist, ind, P = manifold._knn_affinities(rows, 5, 1, 5.0)
        ind2, dist2 = np.full(ind.shape, -1, np.int64), np.full(dist.shape, np.nan)
        _native.check(rows._lib.zk_rows_knn_correlation(rows._h, 5, 1, 5.0, ind2.ctypes.data_as(POINTER(c_int64)),
                                                        dist2.ctypes.data_as(POINTER(c_double)), None), "zk_rows_knn_correlation")
    finally:
        rows.close()
    assert np.isfinite(P).all() and (ind[:, 0] == np.arange(65)).all()          # the full call did its work: self first
    np.testing.assert_array_equal(ind2, ind)
    np.testing.assert_array_equal(dist2, dist)


@pytest.mark.parametrize("mode", list(tc.MODES))
def test_tmd_render_without_masks_and_without_frames(mode):
    sim = tc.build(datasets.TMDImageSimulator, "D", tc.MODES[mode])
    frames, masks = resident.tmd_frames_device([sim], return_masks=True)
    frames, masks = frames.numpy(), masks.numpy()
    layers = [(0,) + layer[1:] for layer in sim._layers()]
    host = np.full(frames.shape, np.nan, np.float32)
    datasets._tmd_render_host(host, None, layers, True, tc.MODES[mode])
    np.testing.assert_array_equal(host, frames)
    host_masks = np.full((len(layers),) + frames.shape[1:], np.nan, np.float32)
    datasets._tmd_render_host(None, host_masks, layers, False, tc.MODES[mode])
    np.testing.assert_array_equal(host_masks.reshape(masks.shape), masks)


def test_eels_pls_without_iterations():
    cube = ec.cube(33, (8,))                                                    # 8 spectra of 33 channels, float64
    spec = eels._arpls_spec(1e4, 0.05, 100)
    full, signal, iters = eels._run(cube, 0, spec, want_signal=True)
    assert iters.min() >= 1
    base = np.full(cube.shape, np.nan)
    eels._call(_native.load(), _native.default_device(), spec, ptr(cube), _native.dtype_code(cube.dtype), eels._layout(cube.shape, 0),
               None, 0, ptr(base), None, None)
    np.testing.assert_array_equal(base, full)
    dev = resident.baseline_device(_native.DeviceArray.from_numpy(cube, _native.default_device()), "arpls")
    np.testing.assert_array_equal(dev.numpy(), base)
    only_signal = np.full(cube.shape, np.nan)
    eels._call(_native.load(), _native.default_device(), spec, ptr(cube), _native.dtype_code(cube.dtype), eels._layout(cube.shape, 0),
               None, 0, ptr(base), ptr(only_signal), None)
    np.testing.assert_array_equal(only_signal, signal)


def test_com_refine_without_thresholds_and_iterations():
    yy, xx = np.mgrid[0:40, 0:48]
    img = sum(np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 6.0) for cx, cy in [(12.3, 11.6), (30.7, 25.2), (20.1, 29.9)])
    pts = np.array([[12, 12], [31, 25], [20, 30]], dtype=np.int32)
    size = 9
    want, levels, steps = features.com_refine_points(pts, img, size, return_thresholds=True)
    assert len(want) == 3 and (steps >= 1).all() and np.isfinite(levels).all()
    corners = np.ascontiguousarray(pts - size // 2, dtype=np.int32)
    moved = np.full((3, 2), np.nan)
    _native.check(_native.load().zk_com_refine(_native.default_device(), ptr(img), _native.dtype_code(img.dtype), *img.shape, ptr(corners), 3,
                                               size, _native.THRESHOLD_LI, ptr(moved), None, None), "zk_com_refine")
    np.testing.assert_array_equal((moved - size / 2) + pts, want)
    dev = resident.com_refine_device(_native.DeviceArray.from_numpy(img, _native.default_device()),
                                     _native.DeviceArray.from_numpy(pts, _native.default_device()), size)
    np.testing.assert_array_equal(dev.numpy(), want)


# setter -> its text for negative bytes
BYTE_KNOBS = {
    "zk_eels_set_chunk": "bad arguments",
    "zk_scan_resample_set_chunk": "bad arguments",
    "zk_gpa_set_run_bytes": "gpa_set_run_bytes: bytes must be >= 0 (0: the default)",
    "zk_align_set_host_chunk": "bad arguments",
    "zk_align_set_band_bytes": "bad arguments",
}


@pytest.mark.parametrize("name", list(BYTE_KNOBS))
def test_byte_knobs_refuse_negative_bytes_and_devices_outside_the_table(name):
    setter = getattr(_native.load(), name)
    for device, nbytes, text in [(0, -1, BYTE_KNOBS[name]), (64, 0, "device index out of range"), (-1, 0, "device index out of range")]:
        with pytest.raises(RuntimeError) as info:
            _native.check(setter(device, nbytes), name)
        assert str(info.value) == f"{name} failed with code {_native.ZK_E_BADARG}: {text}", (device, nbytes)
    _native.check(setter(0, 0), name)                                           # the default, on a device that is there
