"""Stack registration: the rigid sub-pixel drift of every frame of a ``(B, H, W)`` stack against a reference frame, the stack
shifted back, and its average -- what turns a fast multi-frame acquisition (or ``N`` frames of
:func:`mtflearn_amd.denoise.apply_scan_noise`) into one clean frame.  The reference package has no counterpart.

* :func:`estimate_shifts`: Guizar-Sicairos / Thurman / Fienup (Opt. Lett. 33, 156 (2008)) -- the cross-power spectrum of the
  whole stack, a masked peak search and an upsampled local DFT around the peak (``zk_register_shifts``,
  ``csrc/zk_register.hip``; the contract is written out in ``include/zernike_hip.h``);
* :func:`shift_stack`: ``zk_scan_resample`` with constant shift rows;
* :func:`register_stack`: both, and the ordered float64 mean (``zk_stack_mean``).

Every argument check precedes the first device call; there is no CPU fallback.  The resident forms are
``estimate_shifts_device``, ``shift_stack_device`` and ``register_stack_device`` of :mod:`mtflearn_amd.resident`, bit for bit
the same numbers.
"""
from __future__ import annotations

import math
import numbers
from collections import namedtuple
from ctypes import c_void_p

import numpy as np

from . import _native

__all__ = ["Shifts", "Registered", "estimate_shifts", "shift_stack", "register_stack"]

Shifts = namedtuple("Shifts", ["shift", "peak"])
Registered = namedtuple("Registered", ["mean", "shifts", "peak", "aligned"], defaults=(None,))

REF_INDEX, REF_FRAME, REF_PREVIOUS = 0, 1, 2               # ZK_REGISTER_REF_*
_NORMALIZATIONS = {None: 0, "phase": 1}                     # ZK_REGISTER_NORM_*
_WINDOWS = {None: 0, "hann": 1}                             # ZK_REGISTER_WINDOW_*
MAX_EXTENT = 16384


def upsampled_size(upsample):
    """``S = ceil(1.5 * upsample)``: the edge of the upsampled plane."""
    return (3 * upsample + 1) // 2


def _check_options(upsample, max_shift, normalization, window):
    """``(upsample, max_shift as the library takes it, normalization code, window code)``."""
    if isinstance(upsample, bool) or not isinstance(upsample, (numbers.Integral, np.integer)) or not 1 <= upsample <= 1000:
        raise ValueError(f"upsample must be an integer in [1, 1000], not {upsample!r}")
    if max_shift is None:
        lags = -1
    else:
        if isinstance(max_shift, bool) or not isinstance(max_shift, (numbers.Real, np.integer, np.floating)) \
                or not math.isfinite(max_shift) or max_shift < 0:
            raise ValueError(f"max_shift must be a finite number >= 0 or None, not {max_shift!r}")
        lags = min(int(math.floor(max_shift)), MAX_EXTENT)  # lags are integers: |l| <= max_shift is |l| <= floor(max_shift)
    for name, value, table in (("normalization", normalization, _NORMALIZATIONS), ("window", window, _WINDOWS)):
        if not isinstance(value, (str, type(None))) or value not in table:
            raise ValueError(f"{name} must be one of {', '.join(repr(k) for k in table)}, not {value!r}")
    return int(upsample), lags, _NORMALIZATIONS[normalization], _WINDOWS[window]


def _check_stack_shape(shape):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError(f"stack must be a (B, H, W) stack, not {len(shape)}-D")
    if shape[0] < 1:
        raise ValueError(f"an empty stack has no frames to register: shape {shape}")
    if shape[1] < 2 or shape[2] < 2:
        raise ValueError(f"frames must be at least 2 x 2, not {shape[1]} x {shape[2]}")
    if shape[1] > MAX_EXTENT or shape[2] > MAX_EXTENT:
        raise ValueError(f"frames must be at most {MAX_EXTENT} x {MAX_EXTENT} on the device, not {shape[1]} x {shape[2]}")
    return shape


def _check_reference(reference, shape):
    """``(ZK_REGISTER_REF_* mode, frame index, the reference as given or None)``; an array is only checked for its shape."""
    b, h, w = shape
    if isinstance(reference, str):
        if reference != "previous":
            raise ValueError(f"reference must be a frame index, an (H, W) array or 'previous', not {reference!r}")
        return REF_PREVIOUS, 0, None
    if isinstance(reference, (numbers.Integral, np.integer)) and not isinstance(reference, bool):
        index = int(reference) + b if reference < 0 else int(reference)
        if not 0 <= index < b:
            raise IndexError(f"reference index {int(reference)} is out of range for a stack of {b} frames")
        return REF_INDEX, index, None
    if not hasattr(reference, "shape"):
        reference = np.asarray(reference)
    if tuple(int(v) for v in reference.shape) != (h, w):
        raise ValueError(f"a reference frame must have the frames' shape {(h, w)}, not {tuple(reference.shape)}")
    return REF_FRAME, 0, reference


def _host_operand(array, what):
    from .features import ZPs
    if np.iscomplexobj(array):
        raise TypeError(f"{what} must be real, not {array.dtype}")
    if array.dtype.kind not in "biuf":
        raise TypeError(f"{what} must be a numeric array, not {array.dtype}")
    return ZPs._device_operand(array)


def _check_shifts(shifts, b):
    shifts = np.ascontiguousarray(shifts, dtype=np.float64)
    if shifts.shape != (b, 2) or not np.isfinite(shifts).all():
        raise ValueError(f"shifts must be a finite ({b}, 2) array of (dy, dx), not {shifts.shape}")
    return shifts


def _shift_rows(shifts, h, w):
    """The constant rows of ``zk_scan_resample``: ``(dx (B, H), dy (B, W))`` with ``dx[b, :] = -shifts[b, 1]``, ``dy[b, :] = -shifts[b, 0]``."""
    return np.ascontiguousarray(np.repeat(-shifts[:, 1:2], h, axis=1)), np.ascontiguousarray(np.repeat(-shifts[:, 0:1], w, axis=1))


def _accumulate(mode, shift):
    """``'previous'``: the pairwise shifts become the running sum, frame 0 at ``(0, 0)``."""
    if mode == REF_PREVIOUS:
        shift[0] = 0.0
        shift = np.cumsum(shift, axis=0)
    return shift


def _ptr(a):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def _estimate_host(stack, ref, options, planes=False):
    """``zk_register_shifts`` on checked operands; with ``planes`` also the correlation plane and the upsampled plane."""
    mode, index, frame = ref
    upsample, lags, norm, win = options
    lib = _native.load()
    _native.require_device()
    b, h, w = stack.shape
    shift, peak = np.empty((b, 2), np.float64), np.empty((b,), np.float64)
    s = upsampled_size(upsample)
    corr = _native.pinned.empty((b, h, w)) if planes else None
    up = _native.pinned.empty((b, s, s)) if planes and upsample > 1 else None
    _native.check(lib.zk_register_shifts(_native.default_device(), _ptr(stack), _native.dtype_code(stack.dtype), b, h, w, mode, index,
                                         _ptr(frame), _native.dtype_code(frame.dtype) if frame is not None else 0, upsample, lags, norm, win,
                                         _ptr(shift), _ptr(peak), _ptr(corr), _ptr(up)), "zk_register_shifts")
    shifts = Shifts(_accumulate(mode, shift), peak)
    return (shifts, corr, up) if planes else shifts


def _checked_host(stack, reference, upsample, max_shift, normalization, window):
    options = _check_options(upsample, max_shift, normalization, window)
    stack = np.asarray(stack)
    shape = _check_stack_shape(stack.shape)
    mode, index, frame = _check_reference(reference, shape)
    stack = _host_operand(stack, "stack")
    if frame is not None:
        frame = _host_operand(np.asarray(frame), "reference")
    return stack, (mode, index, frame), options


def estimate_shifts(stack, reference=0, upsample=100, max_shift=None, normalization=None, window=None):
    """The rigid drift of every frame of ``stack`` ``(B, H, W)`` against a reference, to ``1 / upsample`` of a pixel:
    ``Shifts(shift (B, 2) float64 as (dy, dx), peak (B,) float64)``.

    ``shift[b]`` is the translation that, applied to frame ``b``, registers it onto the reference (scikit-image's sign
    convention): for ``frame_b(y, x) = ref(y - s_y, x - s_x)`` it is ``(-s_y, -s_x)``, and
    ``shift_stack(stack, shift)`` undoes the drift.

    ``reference``: a frame index (negative as in Python; out of range: ``IndexError``), an ``(H, W)`` array, or ``"previous"``
    -- frame ``b`` against frame ``b - 1``, frame 0 at ``(0, 0)``, ``shift`` the running sum (``np.cumsum`` on the host) and
    ``peak`` the pairwise peaks.  ``upsample``: an int in ``[1, 1000]``; 1 returns the integer lag.  ``max_shift``: a finite
    number ``>= 0``; only lags with ``|ly| <= max_shift`` and ``|lx| <= max_shift`` compete for the coarse peak (a lattice
    image correlates at every lattice vector: this says how far drift can have gone); the refined position is not clamped
    again.  ``normalization``: ``None`` or ``"phase"`` (the cross-power spectrum divided by ``max(|P|, 100 eps max|P|)``).
    ``window``: ``None`` or ``"hann"`` (the separable periodic Hann window, applied as the frames are widened).

    The algorithm (Guizar-Sicairos, Thurman, Fienup 2008) in float64: ``P = fft2(ref w) conj(fft2(frame w))``, the first
    maximum of ``real(ifft2(P))`` in flat order over the permitted lags at ``(y0, x0)``, then with ``S = ceil(1.5 upsample)``
    and ``off = S // 2`` the first maximum of ``C = real(Ey P Ex) / (H W)`` on the grid ``ys = y0 + (arange(S) - off) /
    upsample`` (``xs`` likewise), ``Ey[j, k] = exp(2 pi i ys[j] fftfreq(H)[k])``, ``Ex[k, i] = exp(2 pi i fftfreq(W)[k] xs[i])``.
    ``peak`` is the winning value.  ``tests/registration_oracle.py`` is the NumPy statement.

    Any dtype ``ZPs`` accepts; the integer detector types are widened on the device; complex input is a ``TypeError``; a stack
    that is not 3-D, is empty or has ``H < 2`` or ``W < 2`` a ``ValueError``.  Non-finite pixels are not defined: nothing scans
    for them.  The resident form is :func:`mtflearn_amd.resident.estimate_shifts_device`."""
    stack, ref, options = _checked_host(stack, reference, upsample, max_shift, normalization, window)
    return _estimate_host(stack, ref, options)


def _checked_shift(stack, order, mode):
    from .denoise import _SCAN_DTYPES, _check_scan_order_mode, _check_scan_shape
    order, mode_code = _check_scan_order_mode(order, mode)
    stack = np.asarray(stack)
    _check_scan_shape(stack.shape)
    if stack.dtype not in _SCAN_DTYPES:
        raise TypeError(f"images must be float32, float64, uint8, uint16 or int16, not {stack.dtype}")
    return np.ascontiguousarray(stack), order, mode_code


def shift_stack(stack, shifts, order=3, mode="grid-wrap"):
    """Every frame translated by its own ``shifts[b] = (dy, dx)``: ``out[b, y, x] = S_b(y - shifts[b, 0], x - shifts[b, 1])``,
    ``S_b`` the B-spline interpolant of ``order`` of frame ``b`` extended by ``mode``.  It is ``zk_scan_resample`` with constant
    shift rows, so the orders, modes, dtype rules and exceptions are those of :func:`mtflearn_amd.denoise.apply_scan_noise`
    (float32 / float64 return their own dtype, uint8 / uint16 / int16 float64), and the numbers are bit for bit what
    :func:`mtflearn_amd.resident.scan_noise_device` gives for ``dx[b, :] = -shifts[b, 1]``, ``dy[b, :] = -shifts[b, 0]``.
    ``shifts`` must be finite and ``(B, 2)``."""
    from .denoise import _resample_host
    stack, order, mode_code = _checked_shift(stack, order, mode)
    shifts = _check_shifts(shifts, stack.shape[0])
    dx, dy = _shift_rows(shifts, *stack.shape[1:])
    return _resample_host(stack, dx, dy, order, mode_code)


def _mean_host(stack):
    """``zk_stack_mean``: the per-pixel float64 sum over the frames in ascending order, divided once by ``B``."""
    b, h, w = stack.shape
    out = _native.pinned.empty((h, w))
    _native.check(_native.load().zk_stack_mean(_native.default_device(), _ptr(stack), _native.dtype_code(stack.dtype), b, h, w, _ptr(out)),
                  "zk_stack_mean")
    return out


def register_stack(stack, reference=0, upsample=100, max_shift=None, normalization=None, window=None, order=3, mode="grid-wrap",
                   return_aligned=False):
    """Estimate, shift back and average: ``Registered(mean (H, W) float64, shifts (B, 2), peak (B,), aligned)`` with ``aligned``
    the shifted stack when ``return_aligned`` and ``None`` otherwise.  The arguments are those of :func:`estimate_shifts` and
    :func:`shift_stack`; the dtype rules are the narrower ones of :func:`shift_stack`.  ``mean[y, x]`` is the float64 sum of
    ``aligned[b, y, x]`` over ``b`` in ascending order, divided once by ``B``, without atomics: two runs and
    :func:`mtflearn_amd.resident.register_stack_device` agree bit for bit."""
    options = _check_options(upsample, max_shift, normalization, window)
    stack, order, mode_code = _checked_shift(stack, order, mode)
    shape = _check_stack_shape(stack.shape)
    mode_ref, index, frame = _check_reference(reference, shape)
    if frame is not None:
        frame = _host_operand(np.asarray(frame), "reference")
    from .denoise import _resample_host
    shifts = _estimate_host(stack, (mode_ref, index, frame), options)
    dx, dy = _shift_rows(shifts.shift, *shape[1:])
    aligned = _resample_host(stack, dx, dy, order, mode_code)
    return Registered(_mean_host(aligned), shifts.shift, shifts.peak, aligned if return_aligned else None)
