"""Key-point detection: ``local_max`` of the reference's ``mtflearn.features`` (``features/_local_max_v2.py``), on the GPU.

The reference runs ``skimage.feature.peak_local_max(image, min_distance=1, threshold_abs=threshold)`` and then a greedy
distance filter in a Python loop (``filter_peaks_by_distance``).  Here every step -- threshold, 3 x 3 maxima, ordering,
suppression -- runs on the device (``zk_local_max``, ``csrc/zk_peaks.hip``); scikit-image is not needed.
"""
from __future__ import annotations

import numbers
from ctypes import byref, c_int64, c_void_p

import numpy as np

from .. import _native
from .zernike_polys import ZPs

__all__ = ["local_max"]


def _comparison_threshold(dtype, threshold):
    """``t`` (a Python float) such that ``float64(v) > t`` equals NumPy 2's ``v > threshold`` for every value ``v`` of
    ``dtype``.  NumPy compares in the promoted type (NEP 50: a Python scalar takes the array's kind where it can), so
    the threshold is rounded to that type first: a Python float against float32 compares in float32, against an
    integer image in float64; a Python int against an integer image compares exactly."""
    dtype = np.dtype(dtype)
    if isinstance(threshold, numbers.Integral) and not isinstance(threshold, (bool, np.bool_)) and dtype.kind in "biu":
        return float(threshold)   # exact integer comparison; float64 keeps it for every 8- / 16-bit value
    common = np.result_type(dtype, threshold)
    if common.kind not in "fiub":
        raise TypeError(f"threshold {threshold!r} does not compare with a {dtype} image")
    with np.errstate(over="ignore"):
        return float(np.asarray(threshold).astype(common))


def _local_max_call(lib, device, ptr, code, h, w, r, has_t, t, capacity, out):
    n = c_int64()
    _native.check(lib.zk_local_max(device, ptr, code, h, w, r, has_t, t, out.ctypes.data_as(c_void_p), capacity, byref(n)),
                  "zk_local_max")
    return n.value


def _check_distance(min_distance):
    r = float(min_distance)
    if not (np.isfinite(r) and r >= 0.0):
        raise ValueError(f"min_distance must be a finite number >= 0, not {min_distance!r}")
    return r


def local_max(image, min_distance, threshold=None):
    """Key points of ``image``: local maxima at least ``min_distance`` apart, strongest first.

    Same contract as the reference's ``local_max`` (``features/_local_max_v2.py``):

    * candidates are the pixels equal to the maximum of their 3 x 3 neighbourhood and ``> threshold`` (NumPy's
      comparison for the image's dtype; ``None`` = ``image.min()``), off the 1-px border; a constant image has none;
    * in descending intensity, a kept candidate drops every other candidate at Euclidean distance ``<= min_distance``
      (``min_distance`` may be fractional);
    * returns an ``(N, 2)`` int64 array of ``(x, y) = (column, row)``, strongest first; ``(0, 2)`` when there is nothing.

    Deviation: candidates of EQUAL intensity are ordered by raster position (row, then column), every time.  The
    reference orders them with ``np.argsort(...)[::-1]``, which is not stable and whose tie order depends on the CPU's
    sort kernel, so where equal candidates lie within ``min_distance`` of each other the kept set can differ from the
    reference's (``honeycomb_frame(512, seed=0)`` as uint8 0..255 at ``min_distance=5``: 811 tied pairs within reach, 3 437
    points here, 3 434 from the reference on one x86 host).  Without such ties the result is the reference's array.

    NaN pixels (neither the reference nor scikit-image defines them): the default threshold ``image.min()`` and the
    constant-image test are taken over the non-NaN pixels, and an image with no non-NaN pixel has no candidates; a NaN
    pixel is never a candidate, and a NaN neighbour never exceeds a pixel -- in the 3 x 3 maximum, and only there, NaN
    counts as ``-inf``.  ``+inf`` and ``-inf`` are ordinary values: equal infinities tie like any equal intensities.

    Accepts what :class:`ZPs` accepts (uint8 / uint16 / int16 cross to the device as they are and are widened there,
    exactly).  Runs on the GPU only: without a HIP device it raises ``RuntimeError``."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError(f"local_max needs a 2D image, not {image.ndim}-D")
    if np.iscomplexobj(image):
        raise TypeError("complex images are not supported")
    r = _check_distance(min_distance)
    has_t, t = (0, 0.0) if threshold is None else (1, _comparison_threshold(image.dtype, threshold))
    lib = _native.load()
    _native.require_device()
    operand = ZPs._device_operand(image)
    code = _native.dtype_code(operand.dtype)
    h, w = operand.shape
    device = _native.default_device()
    ptr = operand.ctypes.data_as(c_void_p)
    capacity = max(1024, h * w // 8)                   # kept points of a real frame: a few % of its pixels
    out = np.empty((capacity, 2), dtype=np.int64)
    n = _local_max_call(lib, device, ptr, code, h, w, r, has_t, t, capacity, out)
    if n > capacity:                                    # first guess short: once more with the exact size
        out = np.empty((n, 2), dtype=np.int64)
        n = _local_max_call(lib, device, ptr, code, h, w, r, has_t, t, n, out)
    return out[:n].copy() if n < out.shape[0] // 2 else out[:n]
