"""Geometric phase analysis (GPA; Hytch, Snoeck, Kilaas, Ultramicroscopy 74, 131 (1998)): how the lattice of an
atomic-resolution frame is deformed -- the strain and rotation maps of a frame or a ``(B, H, W)`` stack from the phases of two
Bragg spots.  The reference package has no counterpart.

* :func:`gpa`: ``zk_gpa`` (``csrc/zk_strain.hip``; the contract is written out in ``include/zernike_hip.h``);
* :func:`pick_g`: the usual starting point, the two strongest independent spots of the Hann-windowed power spectrum -- a
  composition of :func:`~mtflearn_amd.features.window_size.fft_power_spectrum` and :func:`~mtflearn_amd.features.local_max`.

Every argument check precedes the first device call; there is no CPU fallback.  The resident form is
:func:`mtflearn_amd.resident.gpa_device`, bit for bit the same numbers.
"""
from __future__ import annotations

import math
import numbers
from collections import namedtuple
from ctypes import c_void_p

import numpy as np

from . import _native

__all__ = ["GPAResult", "gpa", "pick_g"]

GPAResult = namedtuple("GPAResult", ["exx", "eyy", "exy", "rotation", "amplitude", "g", "phase"], defaults=(None,))

_WINDOWS = {None: 0, "hann": 1}                             # ZK_GPA_WINDOW_*
MAX_EXTENT = 16384
MIN_EXTENT = 4
COLLINEAR = 1e-6                                            # |det g| <= COLLINEAR |g1| |g2|: the rows do not span the plane
MIN_ANGLE_DEG = 15.0                                        # pick_g: the second spot is at least this far from collinear


def default_sigma(g):
    """``min(|g1|, |g2|, |g1 - g2|) / 6``: the masks of neighbouring spots meet at three widths."""
    return min(math.hypot(*g[0]), math.hypot(*g[1]), math.hypot(*(g[0] - g[1]))) / 6.0


def _check_g(g):
    g = np.array(g, dtype=np.float64, copy=True, order="C") if not np.iscomplexobj(g) else None
    if g is None or g.shape != (2, 2) or not np.isfinite(g).all():
        raise ValueError("g must be a finite real (2, 2) array whose rows are the Bragg vectors (gy, gx) in cycles per pixel")
    if (np.abs(g) > 0.5).any():
        raise ValueError(f"the components of g must be within 0.5 cycles per pixel, not {g.tolist()}")
    n0, n1 = math.hypot(*g[0]), math.hypot(*g[1])
    if n0 == 0.0 or n1 == 0.0:
        raise ValueError("g has a zero row")
    if abs(g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]) <= COLLINEAR * n0 * n1:
        raise ValueError(f"the rows of g are collinear: {g.tolist()}")
    return g


def _check_options(g, sigma, reference, window, shape):
    """``(g (2, 2) float64, sigma, the rectangle as int64 (4,) or None, window code)`` for frames of ``shape = (H, W)``."""
    h, w = shape
    if h < MIN_EXTENT or w < MIN_EXTENT:
        raise ValueError(f"frames must be at least {MIN_EXTENT} x {MIN_EXTENT}, not {h} x {w}")
    if h > MAX_EXTENT or w > MAX_EXTENT:
        raise ValueError(f"frames must be at most {MAX_EXTENT} x {MAX_EXTENT} on the device, not {h} x {w}")
    g = _check_g(g)
    if sigma is None:
        sigma = default_sigma(g)
    elif isinstance(sigma, bool) or not isinstance(sigma, (numbers.Real, np.integer, np.floating)) or not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"sigma must be a finite number > 0 or None, not {sigma!r}")
    if not isinstance(window, (str, type(None))) or window not in _WINDOWS:
        raise ValueError(f"window must be one of {', '.join(repr(k) for k in _WINDOWS)}, not {window!r}")
    if reference is not None:
        try:
            ok = len(reference) == 4 and all(isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, bool) for v in reference)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"reference must be (y0, y1, x0, x1), four integers, not {reference!r}")
        y0, y1, x0, x1 = (int(v) for v in reference)
        if not (0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w):
            raise ValueError(f"the reference rectangle {(y0, y1, x0, x1)} is empty or leaves the {h} x {w} frame")
        reference = np.array([y0, y1, x0, x1], dtype=np.int64)
    return g, float(sigma), reference, _WINDOWS[window]


def _check_image_shape(shape):
    """``((B, H, W), was a stack)``."""
    shape = tuple(int(v) for v in shape)
    if len(shape) not in (2, 3):
        raise ValueError(f"image must be an (H, W) frame or a (B, H, W) stack, not {len(shape)}-D")
    stack = len(shape) == 3
    if stack and shape[0] < 1:
        raise ValueError(f"an empty stack has no frames: shape {shape}")
    return ((shape if stack else (1,) + shape), stack)


def _ptr(a):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def _result(maps, amp, g_out, phase, stack):
    """``GPAResult`` of the arrays of a call (host or device arrays: only leading-axis items are taken); a single frame sheds ``B``."""
    pick = (lambda a: a) if stack else (lambda a: a[0])
    return GPAResult(*(pick(maps[q]) for q in range(4)), pick(amp), pick(g_out), None if phase is None else pick(phase))


def _gpa_host(frames, options, return_phase, planes=False):
    """``zk_gpa`` on checked operands: ``(maps (4, B, H, W), amp, G, phase or None)`` and with ``planes`` the complex ``H_k``."""
    g, sigma, reference, window = options
    lib = _native.load()
    _native.require_device()
    b, h, w = frames.shape
    maps, amp = _native.pinned.empty((4, b, h, w)), _native.pinned.empty((b, 2, h, w))
    g_out = np.empty((b, 2, 2), np.float64)
    phase = _native.pinned.empty((b, 2, h, w)) if return_phase else None
    hk = np.empty((b, 2, h, w), np.complex128) if planes else None
    _native.check(lib.zk_gpa(_native.default_device(), _ptr(frames), _native.dtype_code(frames.dtype), b, h, w, _ptr(g), sigma, window,
                             _ptr(reference), _ptr(maps), _ptr(amp), _ptr(g_out), _ptr(phase), _ptr(hk)), "zk_gpa")
    return (maps, amp, g_out, phase, hk) if planes else (maps, amp, g_out, phase)


def _checked_host(image, g, sigma, reference, window):
    image = np.asarray(image)
    shape, stack = _check_image_shape(image.shape)
    options = _check_options(g, sigma, reference, window, shape[1:])
    from .registration import _host_operand
    frames = _host_operand(image, "image").reshape(shape)
    return frames, options, stack


def gpa(image, g, sigma=None, reference=None, window=None, return_phase=False):
    """Strain and rotation maps of ``image`` (``(H, W)`` or ``(B, H, W)``) by geometric phase analysis:
    ``GPAResult(exx, eyy, exy, rotation, amplitude, g, phase)``, the maps ``(H, W)`` or ``(B, H, W)`` float64, ``amplitude``
    ``(..., 2, H, W)``, ``g`` ``(..., 2, 2)`` and ``phase`` ``(..., 2, H, W)`` with ``return_phase`` (``None`` otherwise).

    ``g``: ``(2, 2)``, its rows ``(gy, gx)`` the two Bragg vectors in cycles per pixel (:func:`pick_g` finds them); ``sigma``: the
    width of the Gaussian masks in cycles per pixel, ``None`` for ``min(|g1|, |g2|, |g1 - g2|) / 6``; ``reference``: ``(y0, y1,
    x0, x1)``, a half-open rectangle of the frame taken as unstrained -- the mean phase gradients over it are removed and the
    refined Bragg vectors ``g + m / (2 pi)`` returned as ``g``; ``window``: ``None`` or ``"hann"``, as in
    :func:`mtflearn_amd.registration.estimate_shifts`.

    In float64: ``H_k = ifft2(fft2(I w) M_k)`` with ``M_k`` the Gaussian around ``g_k`` on the wrapped frequency grid,
    ``amplitude_k = |H_k|``; the phase gradient is ``arg(H_k[r + 1] conj(H_k[r - 1]) exp(-4 pi i g)) / 2`` per axis (one-sided
    in the first and last row and column) -- nothing is unwrapped, nothing grows with the position; ``e[j][a] = du_j/dr_a =
    -(1 / 2 pi) sum_k inv(G)[j][k] dP_k/dr_a``, ``exx = e[x][x]``, ``eyy = e[y][y]``, ``exy = (e[x][y] + e[y][x]) / 2``,
    ``rotation = (e[y][x] - e[x][y]) / 2`` in radians.  A frame ``I0(r - u(r))`` gives ``e = grad u`` to first order.  ``phase_k =
    arg(H_k exp(-2 pi i g_k . r))`` is for display.  ``tests/strain_oracle.py`` is the NumPy statement.

    Any dtype :func:`~mtflearn_amd.registration.estimate_shifts` takes; complex input is a ``TypeError``; a ``g`` that is not
    finite ``(2, 2)``, has a component beyond 0.5, a zero row or collinear rows, a ``sigma`` that is not finite and positive, a
    rectangle that is empty or leaves the frame, ``H < 4`` or ``W < 4`` or an extent above 16384 a ``ValueError``.  Non-finite
    pixels are not defined.  A frame's numbers do not depend on the stack it is in."""
    frames, options, stack = _checked_host(image, g, sigma, reference, window)
    return _result(*_gpa_host(frames, options, bool(return_phase)), stack)


def pick_g(image, window="hann", dc_radius=None):
    """The two Bragg vectors of a lattice frame, ``(2, 2)`` float64 with rows ``(gy, gx)`` in cycles per pixel: of the local maxima
    of the (Hann-windowed) power spectrum outside a disk of ``dc_radius`` bins about DC (``None``: ``max(3, min(H, W) / 32)``)
    and in the upper half plane (``gy > 0``, or ``gy = 0`` and ``gx > 0``), the strongest, and the strongest at least 15 degrees
    from collinear with it; each refined by the power centroid of its 3 x 3 bins.  ``ValueError`` when there are no two."""
    from .features.peaks import local_max
    from .features.window_size import fft_power_spectrum
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError(f"pick_g needs a 2D image, not {image.ndim}-D")
    if np.iscomplexobj(image):
        raise TypeError("complex images are not supported")
    if not isinstance(window, (str, type(None))) or window not in _WINDOWS:
        raise ValueError(f"window must be one of {', '.join(repr(k) for k in _WINDOWS)}, not {window!r}")
    h, w = image.shape
    if h < MIN_EXTENT or w < MIN_EXTENT:
        raise ValueError(f"frames must be at least {MIN_EXTENT} x {MIN_EXTENT}, not {h} x {w}")
    if dc_radius is None:
        dc_radius = max(3.0, min(h, w) / 32)
    elif not isinstance(dc_radius, (numbers.Real, np.integer, np.floating)) or not math.isfinite(dc_radius) or dc_radius < 0:
        raise ValueError(f"dc_radius must be a finite number >= 0 or None, not {dc_radius!r}")
    frame = image.astype(np.float64)
    if window == "hann":
        hann = lambda n: 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
        frame = frame * np.outer(hann(h), hann(w))
    power = fft_power_spectrum(frame) ** 2
    cy, cx = h // 2, w // 2                                 # DC after fftshift
    ky, kx = np.arange(h)[:, None] - cy, np.arange(w)[None, :] - cx
    power[ky * ky + kx * kx <= dc_radius * dc_radius] = 0.0
    picked = []
    for x, y in local_max(power, 1.0):                      # strongest first
        fy, fx = int(y) - cy, int(x) - cx
        if fy < 0 or (fy == 0 and fx <= 0):
            continue
        box = power[y - 1:y + 2, x - 1:x + 2]               # local_max leaves the 1-px border out
        total = box.sum()
        v = np.array([(fy + (box.sum(axis=1) @ np.arange(-1.0, 2.0)) / total) / h, (fx + (box.sum(axis=0) @ np.arange(-1.0, 2.0)) / total) / w])
        if picked:
            sine = abs(picked[0][0] * v[1] - picked[0][1] * v[0]) / (np.hypot(*picked[0]) * np.hypot(*v))
            if sine < math.sin(math.radians(MIN_ANGLE_DEG)):
                continue
        picked.append(v)
        if len(picked) == 2:
            return np.array(picked)
    raise ValueError("the power spectrum has no two independent spots outside the DC disk")
