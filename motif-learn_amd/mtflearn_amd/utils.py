"""Image normalisation and clipping: the reference's ``mtflearn.utils`` subpackage (``utils/__init__.py``), on the GPU.

The first lines of every workflow -- ``img = normalize_image(img)``, ``percentile_clip`` for the hot pixels every detector
frame carries -- with the reference's names, signatures, defaults, return types and error messages:

* ``normalize_image`` / ``normalize_image_robust``  (``_preprocessing_image.py``): ``"minmax"``, ``"l1"``, ``"l2"``;
* ``standardize_image``                              (``_preprocessing_image.py``): zero mean, unit standard deviation;
* ``percentile_clip`` / ``value_clip``               (``_clip_image.py``): conditional percentile clipping;
* ``ensure_finite`` / ``mask_nonfinite``: the two small helpers, plain NumPy.

The device does the passes over the pixels (``zk_image_stats``, ``zk_image_order_stats``, ``zk_image_map``,
``csrc/zk_utils.hip``); everything scalar stays on the host and is NumPy's own scalar arithmetic on the few values that come
back.  What that pins:

* ``"minmax"``, ``value_clip`` and ``percentile_clip`` (the output and every ``info`` entry) are NumPy's results bit for bit:
  the order statistics are exact, the percentile interpolation and the median restate NumPy 2.2's, and the float32
  elementwise passes round once per operation in NumPy's order.
* ``"l1"``, ``"l2"`` and ``standardize_image`` take their sums from the device in float64 (exact to rounding), where NumPy adds
  float32 pairwise: they are **not** bit-equal to NumPy's.  Every element is within one float32 ulp of the formula evaluated
  in float64 (``standardize_image`` of a non-float32 image: within ``4 * 2**-53`` relative).

Deviations from the reference:

* ``percentile_clip`` raises ``ValueError`` on NaN / inf input (the reference's result there is an accidental all-NaN frame).
* ``standardize_image`` returns float32 for a float32 (or float16) image and float64 otherwise.
* ``vmin``, ``vmax``, ``eps`` and the clip bounds are taken as Python floats.
* Left out: ``remove_bg`` (scikit-image's disk top-hat; scikit-image is not a dependency, so it cannot be pinned) and
  ``find_all_dm4_files`` (file discovery).

There is no CPU fallback: without a HIP device every function but the two helpers raises ``RuntimeError``.  Frames already on
the GPU go through ``normalize_image_device`` / ``standardize_image_device`` / ``percentile_clip_device`` of
:mod:`mtflearn_amd.resident`.
"""
from __future__ import annotations

from ctypes import byref, c_int64, c_void_p

import numpy as np

from . import _device, _native
from ._device import to_host as _download

__all__ = [
    "normalize_image",
    "normalize_image_robust",
    "standardize_image",
    "percentile_clip",
    "value_clip",
    "ensure_finite",
    "mask_nonfinite",
]

_MODES = ("l1", "l2", "minmax")
_METHODS = ("ratio", "mad", "iqr", "auto")
_DEVICE_DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)
MAX_RANKS = 16


# ----------------------------------------------------------------------------------------------- the device side
class _Operand:
    """A flat device image: ``array`` (a :class:`~mtflearn_amd._native.DeviceArray` or a torch tensor) of one of the five
    element types, and what the ``zk_image_*_dev`` calls need of it."""

    def __init__(self, array, stream=0):
        self.array = array
        self.code = _device.code(array)
        self.shape = tuple(int(v) for v in array.shape)
        self.n = int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1
        self.device = int(array.device.index)
        self.stream = stream
        if not 1 <= self.n < 2 ** 31:
            raise ValueError(f"the image must hold between 1 and 2**31 - 1 elements, not {self.n}")

    @property
    def head(self):
        return self.device, c_void_p(self.array.data_ptr()), self.code, self.n


def _host_operand(img):
    """The array that crosses PCIe: the five device element types as they are (converted to float32 on the device, exactly
    as ``astype(np.float32)``), anything else through NumPy's own ``astype(np.float32)``."""
    img = np.asarray(img)
    if np.iscomplexobj(img):
        raise TypeError("complex images are not supported by the HIP kernels")
    if img.dtype not in _DEVICE_DTYPES:
        img = img.astype(np.float32)
    return np.ascontiguousarray(img)


def _upload(array):
    """Host array -> :class:`_Operand` on the default device (its size checked before anything touches the device)."""
    if not 1 <= array.size < 2 ** 31:
        raise ValueError(f"the image must hold between 1 and 2**31 - 1 elements, not {array.size}")
    _native.load()
    _native.require_device()
    return _Operand(_native.DeviceArray.from_numpy(array, _native.default_device()))


def _stats(operand, center=None, wide=False):
    """``(min, max, n_nonfinite, sums)`` of ``zk_image_stats_dev``: float32 min / max over the finite elements, the count of
    the others, and float64 ``[sum x, sum |x|, sum x^2]`` -- or ``[sum (x - center)^2, 0, 0]`` with ``center``."""
    minmax = np.empty(2, np.float32)
    sums = np.empty(3, np.float64)
    nonfinite = c_int64()
    mode = (_native.STATS_CENTERED if center is not None else 0) | (_native.STATS_WIDE if wide else 0)
    _native.check(_native.load().zk_image_stats_dev(*operand.head, mode, 0.0 if center is None else float(center),
                                                    minmax.ctypes.data_as(c_void_p), byref(nonfinite), sums.ctypes.data_as(c_void_p),
                                                    c_void_p(operand.stream)), "zk_image_stats_dev")
    return minmax[0], minmax[1], int(nonfinite.value), sums


def _order_stats(operand, ranks, center=None):
    """float32 elements at the zero-based ``ranks`` (at most 16) of the ascending sort of the image converted to float32 -- of
    ``|x - center|`` in float32 with ``center``.  The one device call of ``percentile_clip``'s statistics."""
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    if not 1 <= len(ranks) <= MAX_RANKS:
        raise ValueError(f"between 1 and {MAX_RANKS} ranks per call, not {len(ranks)}")
    values = np.empty(len(ranks), np.float32)
    mode = _native.ORDER_VALUES if center is None else _native.ORDER_DEVIATIONS
    _native.check(_native.load().zk_image_order_stats_dev(*operand.head, mode, 0.0 if center is None else float(center),
                                                          ranks.ctypes.data_as(c_void_p), len(ranks), values.ctypes.data_as(c_void_p),
                                                          c_void_p(operand.stream)), "zk_image_order_stats_dev")
    return values


def _map(operand, op, params, keep_nonfinite=False):
    """``zk_image_map_dev``: the elementwise pass ``op`` with up to four scalar ``params``; a device array of the operand's kind
    and shape, float32 (float64 for ``MAP_STANDARDIZE`` of a non-float32 image)."""
    dtype = np.float64 if (op == _native.MAP_STANDARDIZE and operand.code != _native.ZK_F32) else np.float32
    out = _device.empty(operand.shape, dtype, operand.array)
    p = np.zeros(4, np.float64)
    p[:len(params)] = params
    _native.check(_native.load().zk_image_map_dev(*operand.head, op, p.ctypes.data_as(c_void_p), int(bool(keep_nonfinite)),
                                                  c_void_p(out.data_ptr()), c_void_p(operand.stream)), "zk_image_map_dev")
    return out


# ----------------------------------------------------------------------------------------------- NumPy's scalar rules, restated
def _quantile_neighbours(n, q):
    """``(i_lo, i_hi, gamma)`` of ``np.percentile(a, q)`` (method ``'linear'``) for a float32 ``a`` of ``n`` elements: the two
    ranks NumPy reads and its interpolation weight, computed the way NumPy 2.2 computes them (``q / float32(100)``, so a
    Python ``q`` gives a float32 virtual index)."""
    quantile = np.true_divide(q, np.float32(100))
    if not (0 <= quantile <= 1):
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = (n - 1) * quantile
    if virtual >= n - 1:
        return n - 1, n - 1, (virtual - np.floor(virtual)).astype(virtual.dtype)
    lo = np.floor(virtual)
    return int(lo), int(lo) + 1, (virtual - lo).astype(virtual.dtype)


def _check_percentile(q):
    """NumPy's range check of a percentile, ahead of any device call."""
    _quantile_neighbours(2, q)


def _lerp(a, b, t):
    """NumPy's interpolation between two neighbours: ``a + (b - a) t``, and ``b - (b - a)(1 - t)`` from ``t = 0.5`` on."""
    diff = np.subtract(b, a)
    out = np.add(a, diff * t)
    if t >= 0.5:
        out = np.subtract(b, diff * (1 - t)).astype(out.dtype)
    return out


def _median_ranks(n):
    return [(n - 1) // 2] if n % 2 else [n // 2 - 1, n // 2]


def _median_of(values):
    """``np.median``'s last step: the mean of the middle one or two elements, in their dtype."""
    return np.mean(np.asarray(values, dtype=np.float32))


# ----------------------------------------------------------------------------------------------- _preprocessing_image.py
def _check_mode(mode):
    if mode not in _MODES:
        raise ValueError("mode must be 'l1', 'l2', or 'minmax'.")


def _normalize_core(operand, mode, eps, vmin, vmax, robust):
    """Device array of the normalised image (float32, the operand's kind)."""
    x_min, x_max, nonfinite, sums = _stats(operand)
    if robust:
        if nonfinite == operand.n:
            raise ValueError("All values are non-finite (NaN or inf)")
    elif nonfinite:
        raise ValueError("Input contains NaN or inf values. "
                         "Use `ensure_finite(img)` or `mask_nonfinite(img)` to handle them first.")
    if mode == "l1":
        return _map(operand, _native.MAP_DIVIDE, [sums[1] + eps], robust)
    if mode == "l2":
        return _map(operand, _native.MAP_DIVIDE, [np.sqrt(sums[2] + eps)], robust)
    if np.isclose(x_min, x_max):
        mid = np.float32((vmin + vmax) / 2)
        return _map(operand, _native.MAP_CLIP, [mid, mid], robust)
    scale = (x_max - x_min) + eps                     # float32, as NumPy adds a Python float to a float32 scalar
    return _map(operand, _native.MAP_RESCALE, [np.float32(vmin), x_min, np.float32(vmax - vmin), scale], robust)


def normalize_image(img, mode="minmax", eps=1e-8, vmin=0.0, vmax=1.0):
    """Normalise a ``(H, W)`` or ``(H, W, C)`` image, as float32: ``"l1"`` (``img / (sum |img| + eps)``), ``"l2"``
    (``img / sqrt(sum img^2 + eps)``) or ``"minmax"`` (``vmin + (img - min) (vmax - vmin) / (max - min + eps)``; a constant
    image becomes ``(vmin + vmax) / 2``).  The input must be finite (``ValueError`` otherwise; see :func:`ensure_finite`).
    ``"minmax"`` is NumPy's result bit for bit; ``"l1"`` / ``"l2"`` use float64 sums (see the module docstring)."""
    _check_mode(mode)
    eps, vmin, vmax = float(eps), float(vmin), float(vmax)
    return _download(_normalize_core(_upload(_host_operand(img)), mode, eps, vmin, vmax, False))


def normalize_image_robust(img, mode="minmax", eps=1e-8, vmin=0.0, vmax=1.0):
    """:func:`normalize_image` with NaN / inf elements left out of the statistics and kept where they are in the output.
    ``ValueError`` when no element is finite."""
    _check_mode(mode)
    eps, vmin, vmax = float(eps), float(vmin), float(vmax)
    return _download(_normalize_core(_upload(_host_operand(img)), mode, eps, vmin, vmax, True))


def _standardize_core(operand):
    wide = operand.code == _native.ZK_F64
    _, _, nonfinite, sums = _stats(operand, wide=wide)
    if nonfinite:                                       # NumPy's mean and std are NaN then, and so is every element
        mean = std = np.float64(np.nan)
    else:
        mean = sums[0] / operand.n
        std = np.sqrt(_stats(operand, center=mean, wide=wide)[3][0] / operand.n)
    if std == 0:
        raise ValueError("Standard deviation is zero, can't standardize the image.")
    return _map(operand, _native.MAP_STANDARDIZE, [mean, std])


def standardize_image(image):
    """``(image - mean) / std`` (population standard deviation, two passes), float32 for a float32 image and float64
    otherwise.  Mean and variance are float64 sums on the device; each element is computed in float64 and rounded once."""
    image = np.asarray(image)
    if np.iscomplexobj(image):
        raise TypeError("complex images are not supported by the HIP kernels")
    from .features.zernike_polys import ZPs
    return _download(_standardize_core(_upload(ZPs._device_operand(image))))


def ensure_finite(img, nan_value=0.0, inf_value=None):
    """A copy with NaN replaced by ``nan_value`` and +-inf by ``inf_value`` (``None``: by the largest / smallest finite
    value).  Plain NumPy."""
    out = np.array(img, copy=True)
    if inf_value is not None:
        out[np.isinf(out)] = inf_value
    elif np.isinf(out).any():
        finite = np.isfinite(out)
        if finite.any():
            lowest, highest = out[finite].min(), out[finite].max()
            out[out == -np.inf] = lowest
            out[out == np.inf] = highest
    out[np.isnan(out)] = nan_value
    return out


def mask_nonfinite(img):
    """``(finite_data, mask)``: the finite values, flattened, and the boolean mask (True = finite) of ``img``'s shape.  Plain
    NumPy."""
    mask = np.isfinite(img)
    return img[mask], mask


# ----------------------------------------------------------------------------------------------- _clip_image.py
def _clip_decision(operand, low, high, method, high_ratio_thresh, mad_k, iqr_k, eps):
    """``(did_clip, info)`` of ``percentile_clip``: two order-statistics calls on the device (the percentiles and the median
    in one, the MAD's median in the other), the rest the reference's scalar arithmetic on Python floats."""
    n = operand.n
    x_min, x_max, nonfinite, _ = _stats(operand)
    if nonfinite:
        raise ValueError("Input contains NaN or inf values. "
                         "Use `ensure_finite(img)` or `mask_nonfinite(img)` to handle them first.")
    wanted = [_quantile_neighbours(n, q) for q in (high, low, 25, 75)]
    ranks = [r for lo, hi, _ in wanted for r in (lo, hi)] + _median_ranks(n)
    values = _order_stats(operand, ranks)
    p_high, p_low, q1, q3 = (float(_lerp(values[2 * k], values[2 * k + 1], g)) for k, (_, _, g) in enumerate(wanted))
    median = _median_of(values[8:])
    mad = float(_median_of(_order_stats(operand, _median_ranks(n), center=np.float32(median))))
    x_min, x_max, med = float(x_min), float(x_max), float(median)

    high_ratio = x_max / (p_high + eps) if abs(p_high) > eps else np.inf
    ratio_flag = high_ratio > high_ratio_thresh
    robust_sigma = 1.4826 * mad
    mad_upper = med + mad_k * robust_sigma
    mad_flag = (robust_sigma > eps) and (x_max > mad_upper)
    iqr = q3 - q1
    iqr_upper = q3 + iqr_k * iqr
    iqr_flag = (iqr > eps) and (x_max > iqr_upper)
    did_clip = {"ratio": ratio_flag, "mad": mad_flag, "iqr": iqr_flag, "auto": ratio_flag or mad_flag or iqr_flag}[method]

    info = {
        "did_clip": did_clip, "method": method, "low": low, "high": high,
        "min": x_min, "p_low": p_low, "median": med, "p_high": p_high, "max": x_max,
        "high_ratio": float(high_ratio), "high_ratio_thresh": high_ratio_thresh, "ratio_flag": bool(ratio_flag),
        "mad": float(mad), "robust_sigma(1.4826*MAD)": float(robust_sigma), "mad_k": mad_k, "mad_upper": float(mad_upper),
        "mad_flag": bool(mad_flag),
        "q1": q1, "q3": q3, "iqr": float(iqr), "iqr_k": iqr_k, "iqr_upper": float(iqr_upper), "iqr_flag": bool(iqr_flag),
    }
    if did_clip:
        info.update({"vmin": p_low, "vmax": p_high})
    return did_clip, info


def _check_method(method):
    method = method.lower()
    if method not in _METHODS:
        raise ValueError("method must be 'ratio', 'mad', 'iqr', or 'auto'.")
    return method


def _clip_core(operand, low, high, method, high_ratio_thresh, mad_k, iqr_k, eps):
    """``(out, did_clip, info)`` with ``out`` a float32 device array of the operand's kind."""
    did_clip, info = _clip_decision(operand, low, high, method, high_ratio_thresh, mad_k, iqr_k, eps)
    bounds = [info["vmin"], info["vmax"]] if did_clip else [-np.inf, np.inf]       # unclipped: the float32 copy
    return _map(operand, _native.MAP_CLIP, bounds), did_clip, info


def percentile_clip(img, low=1.0, high=99.0, method="auto", high_ratio_thresh=5.0, mad_k=8.0, iqr_k=3.0, eps=1e-8, copy=True):
    """Clip a ``(H, W)`` or ``(H, W, C)`` image to its ``[low, high]`` percentiles, but only when a robust test finds an
    outlying maximum.  ``method``: ``"ratio"`` (``max / p_high > high_ratio_thresh``), ``"mad"`` (``max > median + mad_k *
    1.4826 * MAD``), ``"iqr"`` (``max > q3 + iqr_k * IQR``) or ``"auto"`` (any of them).  Returns ``(out, did_clip, info)``:
    the float32 image (clipped or not), whether it was clipped, and the statistics and thresholds used -- all NumPy's numbers
    bit for bit (``np.percentile``, ``np.median``, ``np.clip``).  NaN / inf input is a ``ValueError``.  ``copy`` is accepted for
    the reference's signature; the result is always a new array."""
    method = _check_method(method)
    _check_percentile(high)
    _check_percentile(low)
    out, did_clip, info = _clip_core(_upload(_host_operand(img)), low, high, method, high_ratio_thresh, mad_k, iqr_k, eps)
    return _download(out), did_clip, info


def value_clip(img, vmin, vmax, copy=True):
    """``np.clip(img.astype(np.float32), vmin, vmax)``, bit for bit."""
    vmin, vmax = float(vmin), float(vmax)
    return _download(_map(_upload(_host_operand(img)), _native.MAP_CLIP, [np.float32(vmin), np.float32(vmax)]))
