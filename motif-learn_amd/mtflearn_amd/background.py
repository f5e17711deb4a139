"""Background removal: the reference's ``mtflearn.background`` subpackage (``background/__init__.py``), on the GPU.

The slowly varying background that thickness, tilt and contamination put under the atomic columns, removed before
:func:`mtflearn_amd.features.local_max` thresholds the frame.  Three estimators, each with a ``remove_*`` twin that
returns ``(residual, background)``, and a parameter picker built on
:func:`~mtflearn_amd.features.estimate_patch_size`:

* ``opening``       ``scipy.ndimage.grey_opening(image, size)`` (``_morphology.py``): exact;
* ``rolling_ball``  ``skimage.restoration.rolling_ball(image, radius)`` (``_rolling_ball.py``), restated from scikit-image's
  published algorithm -- scikit-image is not a dependency, so parity with it is unpinned;
* ``baseline``      ``num_iters`` rounds of ``gaussian_filter`` and ``np.minimum(., image)`` (``_baseline.py``): bit for bit
  SciPy's.

Every estimator runs on the device (``zk_background_*``, ``csrc/zk_background.hip``), the residual included; the parameter
picker is host arithmetic.  Frames of one row or one column are served up to the ``height * width < 2^31`` the entry checks.

NaN and inf pixels (float frames), as pinned by ``tests/test_gpu_background_kernels.py``:

* ``baseline``: SciPy's and NumPy's arithmetic, ``np.minimum`` included -- a NaN on either side stays a NaN, so a NaN pixel
  (or ``inf - inf`` under the filter) spreads over the filter's reach; bit for bit, NaN positions and the signs of infinities;
* ``rolling_ball``: scikit-image's ``if min_value > tmp`` rule -- a NaN sum is skipped, so a NaN or ``+inf`` pixel is passed over,
  a ``-inf`` pixel takes every output whose ball holds it and no other, and an output whose ball holds NaN only is ``+inf``;
* ``opening``: exact on ``+inf`` and ``-inf``; NaN pixels are **unspecified** (SciPy's own 1-D min / max queue depends on the
  order it meets them in);
* residuals: NumPy's ``image - background`` (``inf - inf`` is NaN) and ``np.clip(., 0, None)`` (a NaN stays a NaN).
"""
from __future__ import annotations

import numbers
from ctypes import c_void_p

import numpy as np

from . import _native
from .features.zernike_polys import ZPs

__all__ = [
    "estimate_background_opening",
    "remove_background_opening",
    "estimate_background_rolling_ball",
    "remove_background_rolling_ball",
    "estimate_background_baseline",
    "remove_background_baseline",
    "estimate_characteristic_spacing",
    "suggest_background_parameters",
    "select_background_parameter",
]

METHODS = ("opening", "rolling_ball", "baseline")


# ----------------------------------------------------------------------------------------------- validation (host)
def _validate_image(image):
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("image must be a 2D array.")
    return image


def _opening_size(size):
    """``(size_y, size_x)`` of the opening footprint, with the reference's messages."""
    if np.isscalar(size):
        size = int(size)
        if size <= 0:
            raise ValueError("size must be a positive integer.")
        return size, size
    size = tuple(int(v) for v in size)
    if len(size) != 2 or any(v <= 0 for v in size):
        raise ValueError("size must be a positive int or a length-2 tuple.")
    return size


def _check_radius(radius):
    if radius <= 0:
        raise ValueError("radius must be positive.")
    r = float(radius)
    if not np.isfinite(r) or r > 1536:
        raise ValueError(f"radius must be finite and at most 1536 pixels on the device, not {radius!r}")
    return r


def _check_iters(num_iters):
    if num_iters <= 0:
        raise ValueError("num_iters must be positive.")
    return int(num_iters)


def _gaussian_weights(sigma):
    """Half of ``scipy.ndimage``'s Gaussian kernel for one axis, centre first (``w[0..r]``, truncate 4.0): the weights
    ``gaussian_filter1d`` uses, computed the way ``scipy.ndimage._filters._gaussian_kernel1d`` computes them.  An axis SciPy
    skips (``sigma <= 1e-15``) is radius 0 with weight 1, which leaves every value as it is."""
    sd = float(sigma)
    if not sd > 1e-15:
        return np.ones(1)
    radius = int(4.0 * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:])


def _baseline_weights(sigma):
    sigmas = (sigma, sigma) if np.isscalar(sigma) else tuple(sigma)
    if len(sigmas) != 2:
        raise RuntimeError("sequence argument must have length equal to input rank")
    return _gaussian_weights(sigmas[0]), _gaussian_weights(sigmas[1])


# ----------------------------------------------------------------------------------------------- device calls
def _run(method, image, param, clip, want_residual):
    """One ``zk_background_*`` call on a host image: returns ``(residual or None, background)`` in the dtypes the reference
    returns.  The five device formats cross PCIe as they are; any other dtype is widened the way ``ZPs`` widens it, and
    the result (and the residual, in the image's own dtype) is taken back to it on the host."""
    lib = _native.load()
    _native.require_device()
    operand = ZPs._device_operand(image)
    code = _native.dtype_code(operand.dtype)
    h, w = operand.shape
    out_dtype = np.float64 if method == "baseline" else operand.dtype
    native = operand.dtype == image.dtype
    background = np.empty((h, w), dtype=out_dtype)
    residual = np.empty((h, w), dtype=out_dtype) if (want_residual and (native or method == "baseline")) else None
    res_ptr = residual.ctypes.data_as(c_void_p) if residual is not None else None
    args = (_native.default_device(), operand.ctypes.data_as(c_void_p), code, h, w)
    if method == "opening":
        _native.check(lib.zk_background_opening(*args, param[0], param[1], int(bool(clip)), background.ctypes.data_as(c_void_p),
                                                res_ptr), "zk_background_opening")
    elif method == "rolling_ball":
        _native.check(lib.zk_background_rolling_ball(*args, param, int(bool(clip)), background.ctypes.data_as(c_void_p), res_ptr),
                      "zk_background_rolling_ball")
    else:
        (wy, wx), iters = param
        _native.check(lib.zk_background_baseline(*args, wy.ctypes.data_as(c_void_p), len(wy) - 1, wx.ctypes.data_as(c_void_p),
                                                 len(wx) - 1, iters, int(bool(clip)), background.ctypes.data_as(c_void_p),
                                                 res_ptr), "zk_background_baseline")
    if method != "baseline" and not native:
        background = background.astype(image.dtype)    # exact for the opening; the rolling ball's own astype otherwise
        if want_residual:
            residual = image - background
            if clip:
                residual = np.clip(residual, 0, None)
    return residual, background


# ----------------------------------------------------------------------------------------------- _morphology.py
def estimate_background_opening(image, size=15):
    """Background by grey-scale morphological opening: ``scipy.ndimage.grey_opening(image, size=size)`` (mode
    ``'reflect'``), in the image's dtype.  ``size``: an int or a ``(rows, columns)`` pair; even and unequal sizes follow
    SciPy (its dilation is shifted by one on an even axis).  Exact: the result is SciPy's array."""
    image = _validate_image(image)
    size = _opening_size(size)
    return _run("opening", image, size, False, False)[1]


def remove_background_opening(image, size=15, clip=True):
    """``(residual, background)`` of :func:`estimate_background_opening`: ``residual = image - background`` in the image's
    dtype, clipped at 0 when ``clip``."""
    image = _validate_image(image)
    size = _opening_size(size)
    return _run("opening", image, size, clip, True)


# ----------------------------------------------------------------------------------------------- _rolling_ball.py
def estimate_background_rolling_ball(image, radius=50):
    """Background by the rolling-ball algorithm: ``skimage.restoration.rolling_ball(image, radius=radius)``.

    Restated from scikit-image's published algorithm (``restoration/_rolling_ball.py``, 0.19-0.25), which is not a
    dependency here, so parity with it is **unpinned**: offsets ``o`` in ``[-ceil(r), ceil(r)]^2`` with ``|o| <= r``,
    ``diff[o] = k(0) - k(o)`` for the ball ``k(o) = sqrt(max(r^2 - |o|^2, 0))``, and ``background(p) = min over o of
    image[p + o] + diff[o]`` with ``+inf`` outside the frame.  The arithmetic is float32 for float16 / float32 images and
    float64 otherwise; the result is cast back to the image's dtype (integers truncate, as ``astype`` does).  Radii above
    1536 pixels are not served by the device kernel."""
    image = _validate_image(image)
    r = _check_radius(radius)
    return _run("rolling_ball", image, r, False, False)[1]


def remove_background_rolling_ball(image, radius=50, clip=True):
    """``(residual, background)`` of :func:`estimate_background_rolling_ball`, the residual in the image's dtype, clipped
    at 0 when ``clip``."""
    image = _validate_image(image)
    r = _check_radius(radius)
    return _run("rolling_ball", image, r, clip, True)


# ----------------------------------------------------------------------------------------------- _baseline.py
def estimate_background_baseline(image, sigma=20, num_iters=10):
    """Smooth lower envelope: ``gaussian_filter(image, sigma)`` then ``np.minimum(., image)``, ``num_iters`` times, in
    float64.  ``sigma``: a scalar or a per-axis pair; an axis with ``sigma <= 1e-15`` is not filtered, as in SciPy
    (truncate 4.0, mode ``'reflect'``).  Every round runs on the device and matches SciPy bit for bit."""
    image = _validate_image(image)
    iters = _check_iters(num_iters)
    return _run("baseline", image, (_baseline_weights(sigma), iters), False, False)[1]


def remove_background_baseline(image, sigma=20, num_iters=10, clip=True):
    """``(residual, background)`` of :func:`estimate_background_baseline`, both float64; the residual clipped at 0 when
    ``clip``."""
    image = _validate_image(image)
    iters = _check_iters(num_iters)
    return _run("baseline", image, (_baseline_weights(sigma), iters), clip, True)


# ----------------------------------------------------------------------------------------------- _parameter_selection.py
def estimate_characteristic_spacing(image, window_size=None, n_samples=16, random_state=0, **kwargs):
    """Characteristic foreground spacing (pixels) from :func:`~mtflearn_amd.features.estimate_patch_size`, with NumPy's
    global random state seeded by ``random_state`` for the call and restored afterwards (``None``: left alone)."""
    image = _validate_image(image)
    from .features.pickers import estimate_patch_size

    if random_state is None:
        return estimate_patch_size(image, window_size=window_size, n_samples=n_samples, **kwargs)
    state = np.random.get_state()
    np.random.seed(random_state)
    try:
        return estimate_patch_size(image, window_size=window_size, n_samples=n_samples, **kwargs)
    finally:
        np.random.set_state(state)


def suggest_background_parameters(image, spacing=None, window_size=None, n_samples=16, random_state=0,
                                  opening_factor=2.0, rolling_ball_factor=3.0, baseline_factor=1.5):
    """Parameters of all three methods from a characteristic spacing (estimated from the image when ``spacing`` is
    None): ``{"spacing", "opening_size" (odd, >= 3), "rolling_ball_radius" (>= 3), "baseline_sigma" (>= 1.0)}``."""
    image = _validate_image(image)
    if spacing is None:
        spacing = estimate_characteristic_spacing(image, window_size=window_size, n_samples=n_samples,
                                                  random_state=random_state)
    if spacing is None or spacing <= 0:
        raise ValueError("spacing must be positive or estimable from the image.")
    spacing = float(spacing)
    opening_size = max(3, int(round(opening_factor * spacing)))
    if opening_size % 2 == 0:
        opening_size += 1
    return {
        "spacing": spacing,
        "opening_size": opening_size,
        "rolling_ball_radius": max(3, int(round(rolling_ball_factor * spacing))),
        "baseline_sigma": max(1.0, float(baseline_factor * spacing)),
    }


def select_background_parameter(method, image, spacing=None, **kwargs):
    """The suggested parameter of one method: ``"opening"`` -> size, ``"rolling_ball"`` -> radius, ``"baseline"`` ->
    sigma.  ``kwargs`` go to :func:`suggest_background_parameters`."""
    method = str(method).lower()
    params = suggest_background_parameters(image, spacing=spacing, **kwargs)
    key = {"opening": "opening_size", "rolling_ball": "rolling_ball_radius", "baseline": "baseline_sigma"}.get(method)
    if key is None:
        raise ValueError("method must be one of {'opening', 'rolling_ball', 'baseline'}.")
    return params[key]


def _method_parameter(method, parameter, method_kw):
    """Validated device parameter of ``method`` (what the ``zk_background_*`` call takes), for the device-resident entry."""
    if method not in METHODS:
        raise ValueError("method must be one of {'opening', 'rolling_ball', 'baseline'}.")
    if method == "baseline":
        unknown = set(method_kw) - {"num_iters"}
        if unknown:
            raise TypeError(f"unexpected keyword arguments for baseline: {sorted(unknown)}")
        return _baseline_weights(parameter), _check_iters(method_kw.get("num_iters", 10))
    if method_kw:
        raise TypeError(f"unexpected keyword arguments for {method}: {sorted(method_kw)}")
    if method == "opening":
        return _opening_size(parameter)
    if not isinstance(parameter, (numbers.Real, np.generic)):
        raise TypeError("radius must be a number")
    return _check_radius(parameter)
