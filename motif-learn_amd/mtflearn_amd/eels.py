"""Baselines of whole spectrum cubes: the reference's ``mtflearn.eels`` (``eels/_baseline_correction.py``), on the GPU.

The reference holds four one-spectrum baseline estimators on one Whittaker smoother and never runs them over a spectrum
image.  Here every function keeps the reference's name, argument order and defaults, gains ``axis`` (the energy axis,
default 0) and takes any rank of at least 1: every other index is one spectrum, and all of them are solved in one device call
(``zk_eels_*``, ``csrc/zk_eels.hip``: one spectrum per lane, the whole reweighting loop inside one launch).

* ``baseline_als``     ``(W + lam D D^T) z = W y`` with second differences, ``niter`` reweightings ``p (y > z) + (1 - p) (y < z)``;
* ``baseline_arpls``   the same operator, logistic reweighting on the mean / population standard deviation of the negative
  residuals, stopped by ``norm(w - wt) / norm(w) < ratio``;
* ``baseline_airpls``  differences of ``porder``, the reference's weight rule (its overwrite of ``w[0]`` and ``w[-1]``
  included) and stop rule (``i == itermax`` included);
* ``baseline_snip``    the double-log / square-root transform, ``niter`` Jacobi clipping passes, the inverse transform;
* ``WhittakerSmooth``  one solve with given weights;
* ``remove_baseline``  ``(signal, baseline)`` with ``signal = data - baseline`` formed on the device.

A 1-D call returns what the reference's function returns for that spectrum: ``(L,)`` float64.  Input may be float32, float64,
uint8, uint16 or int16 (widened exactly to float64 on the device; other types are converted on the host first); output is
always float64.  The native layout is energy-major ``(E, H, W)`` (``axis=0``); another axis goes through a device transpose on
the way in and out.  A spectrum's numbers do not depend on its neighbours, on the chunking (:func:`set_scratch_bytes`) or on
the entry point: a 1-D call, a batch and :func:`mtflearn_amd.resident.baseline_device` agree bit for bit.

Deviations from the reference, all deliberate:

* for float32 input the reference's SNIP computes in float32; here it is float64, i.e. the reference on ``y.astype(float64)``;
* the reference prints ``airpls: max iteration reached!`` once per spectrum; here one ``RuntimeWarning`` per call says how many
  spectra took ``itermax`` solves (``baseline_arpls`` and ``baseline_airpls``);
* ``return_info=True`` also returns the solves each spectrum took (int32, the shape of the non-energy axes), which the
  reference does not expose;
* ``baseline_als`` needs ``niter >= 1`` (the reference has nothing to return for 0).

Not pinned: non-finite samples, SNIP input below -1, a spectrum whose residual has no negative sample (NumPy yields NaN
there), and airPLS runs that end at ``itermax``.  Every loop is bounded by ``itermax``, so nothing can hang.  There is no CPU
fallback: without a device every call raises ``RuntimeError`` -- after its arguments have been checked.
"""
from __future__ import annotations

import numbers
import warnings
from ctypes import c_void_p

import numpy as np

from . import _native
from .features.zernike_polys import ZPs

__all__ = ["baseline_als", "baseline_snip", "baseline_arpls", "baseline_airpls", "WhittakerSmooth", "remove_baseline",
           "set_scratch_bytes"]

METHODS = ("snip", "als", "arpls", "airpls")


# ----------------------------------------------------------------------------------------------- validation (host)
def _layout(shape, axis):
    """``(outer, L, inner)`` of an operand of ``shape`` whose energy axis is ``axis``."""
    if len(shape) < 1:
        raise ValueError("spectra need at least one axis")
    if not isinstance(axis, (numbers.Integral, np.integer)) or not -len(shape) <= axis < len(shape):
        raise ValueError(f"axis {axis!r} is out of bounds for an array of rank {len(shape)}")
    axis = int(axis) % len(shape)
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    if outer * inner == 0 or shape[axis] == 0:
        raise ValueError(f"an empty operand has no spectra: shape {tuple(shape)}")
    return outer, int(shape[axis]), inner


def _check_length(length, order):
    if length < order + 1:
        raise ValueError(f"a spectrum needs at least {order + 1} channels for differences of order {order}, not {length}")


def _check_lam(lam):
    lam = float(lam)
    if not (np.isfinite(lam) and lam > 0):
        raise ValueError(f"lam must be positive and finite, not {lam!r}")
    return lam


def _check_order(order, name):
    if not isinstance(order, (numbers.Integral, np.integer)) or not 1 <= order <= 3:
        raise ValueError(f"{name} must be 1, 2 or 3, not {order!r}")
    return int(order)


def _check_count(value, name, least):
    if not isinstance(value, (numbers.Integral, np.integer)) or value < least:
        raise ValueError(f"{name} must be an integer >= {least}, not {value!r}")
    return int(min(value, 2 ** 30))


def _snip_spec(niter=10):
    return {"snip": True, "itermax": _check_count(niter, "niter", 0), "order": 0}


def _als_spec(lam=105, p=0.1, niter=10):
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"p must lie in (0, 1), not {p!r}")
    return {"mode": _native.EELS_ALS, "order": 2, "lam": _check_lam(lam), "param": p, "itermax": _check_count(niter, "niter", 1)}


def _arpls_spec(lam=1e4, ratio=0.05, itermax=100):
    ratio = float(ratio)
    if not ratio > 0:
        raise ValueError(f"ratio must be positive, not {ratio!r}")
    return {"mode": _native.EELS_ARPLS, "order": 2, "lam": _check_lam(lam), "param": ratio,
            "itermax": _check_count(itermax, "itermax", 1), "warn": "baseline_arpls"}


def _airpls_spec(lam=100, porder=1, itermax=100):
    return {"mode": _native.EELS_AIRPLS, "order": _check_order(porder, "porder"), "lam": _check_lam(lam), "param": 0.0,
            "itermax": _check_count(itermax, "itermax", 1), "warn": "baseline_airpls"}


_SPECS = {"snip": _snip_spec, "als": _als_spec, "arpls": _arpls_spec, "airpls": _airpls_spec}


def _method_spec(method, kw):
    """Validated parameters of ``method`` (what the ``zk_eels_*`` call takes) from the reference's keyword names."""
    if method not in METHODS:
        raise ValueError("method must be one of {'snip', 'als', 'arpls', 'airpls'}.")
    try:
        return _SPECS[method](**kw)
    except TypeError as e:
        raise TypeError(f"{method}: {e}") from None


def _whittaker_weights(w, shape, axis, length):
    """``(weights, per_spectrum)``: float64, of the operand's shape or 1-D of length L."""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim == 1 and w.shape[0] == length:
        return w, 0
    if w.shape == tuple(shape):
        return w, 1
    raise ValueError(f"w must have the shape of x, {tuple(shape)}, or be 1-D of length {length}; not {w.shape}")


def _warn_itermax(spec, iterations):
    if "warn" in spec:
        hit = int(np.count_nonzero(iterations == spec["itermax"]))
        if hit:
            warnings.warn(f"{spec['warn']}: {hit} of {iterations.size} spectra took all itermax = {spec['itermax']} solves",
                          RuntimeWarning, stacklevel=4)


# ----------------------------------------------------------------------------------------------- device calls
def _call(lib, device, spec, data_ptr, code, layout, weights_ptr, per_spectrum, base_ptr, sig_ptr, it_ptr, stream=None):
    """One ``zk_eels_*`` call; ``stream`` None: the host-buffer entry points."""
    dev = stream is not None
    tail = (c_void_p(stream),) if dev else ()
    if spec.get("snip"):
        fn, name = (lib.zk_eels_snip_dev, "zk_eels_snip_dev") if dev else (lib.zk_eels_snip, "zk_eels_snip")
        rc = fn(device, data_ptr, code, *layout, spec["itermax"], base_ptr, sig_ptr, *tail)
    else:
        fn, name = (lib.zk_eels_pls_dev, "zk_eels_pls_dev") if dev else (lib.zk_eels_pls, "zk_eels_pls")
        rc = fn(device, data_ptr, code, *layout, spec["mode"], spec["order"], spec["lam"], spec["param"], spec["itermax"], weights_ptr,
                per_spectrum, base_ptr, sig_ptr, it_ptr, *tail)
    _native.check(rc, name)


def _run(data, axis, spec, weights=None, want_signal=False):
    """``(baseline, signal or None, iterations or None)`` of a host operand: everything is checked, then the cube crosses to
    the device once and the results come back once."""
    data = np.asarray(data)
    layout = _layout(data.shape, axis)
    _check_length(layout[1], spec["order"])
    per_spectrum = 0
    if weights is not None:
        weights, per_spectrum = _whittaker_weights(weights, data.shape, axis, layout[1])
    operand = ZPs._device_operand(data)
    lib = _native.load()
    _native.require_device()
    baseline = np.empty(data.shape, dtype=np.float64)
    signal = np.empty(data.shape, dtype=np.float64) if want_signal else None
    ax = int(axis) % data.ndim
    iterations = None if spec.get("snip") else np.empty(data.shape[:ax] + data.shape[ax + 1:], dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(c_void_p) if a is not None else None
    _call(lib, _native.default_device(), spec, ptr(operand), _native.dtype_code(operand.dtype), layout, ptr(weights), per_spectrum,
          ptr(baseline), ptr(signal), ptr(iterations))
    if iterations is not None:
        _warn_itermax(spec, iterations)
    return baseline, signal, iterations


# ----------------------------------------------------------------------------------------------- the reference's names
def baseline_als(y, lam=105, p=0.1, niter=10, axis=0):
    """Asymmetric least squares: ``niter`` solves of ``(W + lam D D^T) z = W y`` (``D`` the second differences), ``w = 1`` first
    and ``w = p (y > z) + (1 - p) (y < z)`` after each.  Spectra need at least 3 channels."""
    return _run(y, axis, _als_spec(lam, p, niter))[0]


def baseline_snip(y, niter=10, axis=0):
    """SNIP: ``v = log(log(sqrt(y + 1) + 1) + 1)``, for ``pp = 1 .. niter`` a Jacobi pass ``v[e] = min(v[e], (v[e - pp] +
    v[e + pp]) / 2)`` on ``pp <= e < L - pp`` (a pass whose window does not fit changes nothing), then the inverse transform.
    float64 for every input type."""
    return _run(y, axis, _snip_spec(niter))[0]


def baseline_arpls(y, lam=1e4, ratio=0.05, itermax=100, axis=0, return_info=False):
    """Asymmetrically reweighted penalised least squares (Baek et al., Analyst 140, 250 (2015)): the ALS operator with
    ``wt = 1 / (1 + exp(2 (d - (2 s - m)) / s))`` on the mean ``m`` and population standard deviation ``s`` of the negative
    residuals ``d = y - z``, until ``norm(w - wt) / norm(w) < ratio`` or ``itermax`` solves.  ``return_info``: also the solves
    each spectrum took."""
    baseline, _, iterations = _run(y, axis, _arpls_spec(lam, ratio, itermax))
    return (baseline, iterations) if return_info else baseline


def baseline_airpls(x, lam=100, porder=1, itermax=100, axis=0, return_info=False):
    """Adaptive iteratively reweighted penalised least squares (Zhang et al., Analyst 135, 1138 (2010)) with differences of
    ``porder`` (1, 2 or 3): solve ``i`` stops when ``|sum d[d < 0]| < 0.001 sum |x|`` or ``i == itermax``; otherwise ``w = 0``
    where ``d >= 0``, ``exp(i |d| / dssn)`` where ``d < 0``, and ``w[0] = w[-1] = exp(i max(d[d < 0]) / dssn)``.
    ``return_info``: also the solves each spectrum took."""
    baseline, _, iterations = _run(x, axis, _airpls_spec(lam, porder, itermax))
    return (baseline, iterations) if return_info else baseline


def WhittakerSmooth(x, w, lam, differences=1, axis=0):
    """One penalised least squares solve ``(W + lam D^T D) z = W x`` with differences of order ``differences`` (1, 2 or 3).
    ``w`` has the shape of ``x``, or is 1-D of length L and used for every spectrum."""
    spec = {"mode": _native.EELS_WHITTAKER, "order": _check_order(differences, "differences"), "lam": _check_lam(lam), "param": 0.0,
            "itermax": 1}
    return _run(x, axis, spec, weights=w)[0]


def remove_baseline(data, method="snip", axis=0, **kw):
    """``(signal, baseline)`` with ``signal = data - baseline`` (float64, formed on the device): the spectral twin of
    ``remove_background_*``.  ``method``: ``"snip"``, ``"als"``, ``"arpls"`` or ``"airpls"``; ``kw``: that estimator's
    parameters under the reference's names."""
    baseline, signal, _ = _run(data, axis, _method_spec(method, kw), want_signal=True)
    return signal, baseline


def set_scratch_bytes(scratch_bytes, device=None):
    """Cap of the scratch planes of one call (``zk_eels_set_chunk``; 0: the default, 1 GiB): the spectra are cut into chunks
    that stay under it.  The results do not depend on it."""
    _native.check(_native.load().zk_eels_set_chunk(_native.default_device() if device is None else int(device), int(scratch_bytes)),
                  "zk_eels_set_chunk")
