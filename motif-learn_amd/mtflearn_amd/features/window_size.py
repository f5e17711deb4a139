"""Fourier window-size estimators and the angular spectrum average, on the GPU.

Drop-ins for ``mtflearn.features.compute_autocorrelation`` / ``get_characteristic_length`` /
``get_characteristic_length_fft`` (reference ``mtflearn/features/_window_size.py``) and ``fft_power_spectrum`` /
``angular_average`` (``mtflearn/features/_fft_related.py``): same names, arguments, defaults, return values and error
texts; ``debug`` is accepted and ignored (the reference's plots are UI).  Beyond the reference, every function but
``angular_average`` also takes a 3-D stack ``(B, H, W)`` -- a movie or a focal series -- and answers per frame: maps of shape
``(B, H, W)``, estimates of shape ``(B,)``.  For a stack the whole chain stays on the device (``csrc/zk_window_size.hip``:
FFT, magnitude with its first maximum, polar profile about each frame's own centre, SNIP / running mean / peak search of
the profile) and only ``B`` results come back.

What runs where.  Everything numeric goes through ``libzernike_hip.so`` (``zk_circular_autocorr``,
``zk_shifted_magnitude``, ``zk_char_length``, ``zk_char_length_fft``, ``zk_angular_average``); there is no CPU fallback.
Host work: the argument checks, ``numpy.linspace`` for the bin edges and centres of ``angular_average``,
``scipy.signal.find_peaks`` on the one profile of a 2-D ``get_characteristic_length`` call, and the final division.

Parity status.  ``compute_autocorrelation``, ``fft_power_spectrum`` and ``angular_average`` are pinned to the
reference's own code (NumPy only; ``tests/golden/window_size_golden.npz``).  The two ``get_characteristic_length*``
functions call ``skimage.transform.warp_polar``, which is not installed in the build image: they are pinned to the
reference's code running over ``oracle.pickers_oracle.warp_polar_linear`` and so share ``radial_profile``'s status,
**parity-unpinned** against scikit-image itself (see ``pickers.py``).

The centre hazard.  Both estimators take ``argmax`` of a map as the centre of the polar profile.  Every Fourier
coefficient of a real image has a conjugate twin of equal magnitude, so when the DC term is not the strict maximum (a
zero-mean image) the reference's ``argmax`` is decided by the last bit of its FFT, and hipFFT's last bit differs: that
case is not pinned.  An image with a positive offset -- any detector frame -- has the DC term as its strict maximum.
"""
from __future__ import annotations

from ctypes import c_void_p

import numpy as np
from scipy.signal import find_peaks

from .. import _native
from .pickers import _call

__all__ = ["compute_autocorrelation", "fft_power_spectrum", "angular_average", "get_characteristic_length",
           "get_characteristic_length_fft"]

_ZERO_STD = "Standard deviation is zero, can't standardize the image."
_NO_PEAK = "No peak detected in the radial profile."
_EMPTY_ARGMAX = "attempt to get argmax of an empty sequence"


def _frames(image, who):
    """``(stack (B, H, W) float32 / float64 C-contiguous, was_3d)``."""
    image = np.asarray(image)
    if np.iscomplexobj(image):
        raise TypeError("complex images are not supported")
    if image.ndim not in (2, 3):
        raise ValueError(f"{who} needs a 2-D image or a 3-D stack (B, H, W), got {image.ndim} dimensions")
    if image.size == 0:
        raise ValueError(f"{who} needs a non-empty image")
    if image.dtype not in (np.float32, np.float64):
        image = image.astype(np.float64)
    stack = image.ndim == 3
    return np.ascontiguousarray(image if stack else image[None]), stack


def _refuse_constant(frames, stack):
    """The reference's ``standardize_image`` refuses an image without variance.  A single image is looked at on the host, so
    the refusal needs no device (one min / max pass); a stack is not touched here: its frames' statistics are taken on the
    device, where a frame whose minimum equals its maximum has the standard deviation 0 exactly and fails the call with the
    same message."""
    if not stack and frames.max() == frames.min():
        raise ValueError(_ZERO_STD)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(c_void_p)


def _maps(name, frames, flag):
    lib = _native.load()
    _native.require_device()
    out = np.empty(frames.shape, dtype=np.float64)
    B, H, W = frames.shape
    _call(getattr(lib, name)(_native.default_device(), _ptr(frames), _native.dtype_code(frames.dtype), B, H, W, int(flag), _ptr(out)), name)
    return out


# ------------------------------------------------------------------------------------------ _window_size.py
def compute_autocorrelation(image, standardize=True):
    """``|fftshift(ifft2(F conj F))|`` of the (standardised) image: the CIRCULAR autocorrelation; reference
    ``_window_size.py:16-27``.  Any ``H x W``; a stack ``(B, H, W)`` gives ``(B, H, W)``."""
    frames, stack = _frames(image, "compute_autocorrelation")
    if standardize is True:
        _refuse_constant(frames, stack)
    out = _maps("zk_circular_autocorr", frames, standardize is True)
    return out if stack else out[0]


def _char_length(image, standardize, profiles):
    """``(centres (B, 2), cut profiles (list of B arrays) or None, first peaks (B,), -1 = none, was_3d)``."""
    frames, stack = _frames(image, "get_characteristic_length")
    if standardize is True:
        _refuse_constant(frames, stack)
    lib = _native.load()
    _native.require_device()
    B, H, W = frames.shape
    centres = np.empty((B, 2), dtype=np.int32)
    peaks = np.empty(B, dtype=np.int32)
    prof = np.empty((B, int(lib.zk_polar_radii(H, W))), dtype=np.float64) if profiles else None
    _call(lib.zk_char_length(_native.default_device(), _ptr(frames), _native.dtype_code(frames.dtype), B, H, W, int(standardize is True),
                             _ptr(centres), _ptr(prof), _ptr(peaks)), "zk_char_length")
    cut = None if prof is None else [p[:min(int(c[0]), len(p))] for p, c in zip(prof, centres)]
    return centres, cut, peaks.astype(np.int64), stack


def _first_peak(line_profile):
    """The tail of the reference's ``get_characteristic_length`` on one profile (host SciPy)."""
    peaks, _ = find_peaks(line_profile)
    if len(peaks) > 0:
        return peaks[0]
    raise ValueError(_NO_PEAK)


def get_characteristic_length(image, standardize=True, debug=False):
    """Radius of the first peak of the autocorrelation's mean polar profile; reference ``_window_size.py:36-46``
    (``scipy.signal.correlate(image, image, 'same', 'fft')`` of the standardised image, first maximum as centre, profile
    ``[0:i]``, ``find_peaks``).  Any ``H x W``.  A stack ``(B, H, W)`` gives ``(B,)`` with -1 for a frame without a peak,
    the peak search on the device as well."""
    if np.ndim(image) == 3:
        return _char_length(image, standardize, False)[2]
    _, cut, _, _ = _char_length(image, standardize, True)
    return _first_peak(cut[0])


def _char_length_fft(image, niter, size, use_log, profiles):
    """``(centres (B, 2), cut profiles or None, cut filtered profiles y2 or None, ind (B,), was_3d)``."""
    frames, stack = _frames(image, "get_characteristic_length_fft")
    niter, size = int(niter), int(size)
    if size < 1:
        raise RuntimeError("incorrect filter size")                     # scipy.ndimage.uniform_filter1d's refusal
    lib = _native.load()
    _native.require_device()
    B, H, W = frames.shape
    centres = np.empty((B, 2), dtype=np.int32)
    ind = np.empty(B, dtype=np.int32)
    R = int(lib.zk_polar_radii(H, W))
    prof = np.empty((B, R), dtype=np.float64) if profiles else None
    y2 = np.empty((B, R), dtype=np.float64) if profiles else None
    _call(lib.zk_char_length_fft(_native.default_device(), _ptr(frames), _native.dtype_code(frames.dtype), B, H, W, max(niter, 0), size,
                                 int(bool(use_log)), _ptr(centres), _ptr(prof), _ptr(y2), _ptr(ind)), "zk_char_length_fft")
    cut = lambda a: None if a is None else [p[:min(int(c[0]), R)] for p, c in zip(a, centres)]
    return centres, cut(prof), cut(y2), ind.astype(np.int64), stack


def _length_from_ind(n_rows, ind):
    """``image.shape[0] / ind``: ``inf`` with NumPy's warning where ``ind == 0``, as in the reference.  An empty profile
    (``ind`` -1: the centre on row 0) is the reference's ``argmax`` error for a single image and ``nan`` for that frame of a
    stack, as a frame without a peak is -1 on the other route."""
    if np.ndim(ind) == 0:
        if ind < 0:
            raise ValueError(_EMPTY_ARGMAX)
        return n_rows / ind
    out = np.full(len(ind), np.nan)
    filled = ind >= 0
    out[filled] = n_rows / ind[filled]
    return out


def get_characteristic_length_fft(image, niter=10, size=9, use_log=True, debug=True):
    """Real-space period of the strongest ring of the spectrum; reference ``_window_size.py:65-80``: shifted magnitude
    (``log(. + 1)`` with ``use_log``), first maximum as centre, mean polar profile ``[0:i]``, minus its SNIP baseline
    (``niter``), ``uniform_filter1d(size)``, ``ind = argmax``; returns ``image.shape[0] / ind``.  A stack gives ``(B,)``, ``nan`` for a frame whose profile is empty."""
    _, _, _, ind, stack = _char_length_fft(image, niter, size, use_log, False)
    return _length_from_ind(np.shape(image)[-2], ind if stack else ind[0])


# ------------------------------------------------------------------------------------------ _fft_related.py
def fft_power_spectrum(img):
    """``|fftshift(fft2(img))|`` -- the magnitude, as in the reference (``_fft_related.py:4-7``).  A stack gives ``(B, H, W)``."""
    frames, stack = _frames(img, "fft_power_spectrum")
    out = _maps("zk_shifted_magnitude", frames, 0)
    return out if stack else out[0]


def _angular_sums(power_spectrum, num_bins, use_mask):
    """``(angles, per-bin sums, per-bin pixel counts)``; the counts are exact."""
    ps = np.asarray(power_spectrum)
    if np.iscomplexobj(ps):
        raise TypeError("complex images are not supported")
    if ps.ndim != 2:
        raise ValueError(f"angular_average needs a 2-D power spectrum, got {ps.ndim} dimensions")
    num_bins = int(num_bins)
    if num_bins < 0:
        raise ValueError(f"Number of samples, {num_bins + 1}, must be non-negative.")
    angular_bins = np.linspace(0, 360, num_bins + 1)
    angles = (angular_bins[:-1] + angular_bins[1:]) / 2
    sums, counts = np.zeros(num_bins), np.zeros(num_bins, dtype=np.int64)
    if num_bins == 0 or ps.size == 0:
        return angles, sums, counts
    ps = np.ascontiguousarray(ps, dtype=np.float64)
    lib = _native.load()
    _native.require_device()
    _call(lib.zk_angular_average(_native.default_device(), _ptr(ps), 1, ps.shape[0], ps.shape[1], _ptr(angular_bins), num_bins,
                                 int(bool(use_mask)), _ptr(sums), _ptr(counts)), "zk_angular_average")
    return angles, sums, counts


def angular_average(power_spectrum, num_bins=360, use_mask=True):
    """Mean of a 2-D spectrum over angular sectors about its centre; reference ``_fft_related.py:12-66``.  Returns
    ``(angles, angular_profile)``: the bin centres in degrees and the mean per bin (0 for an empty bin)."""
    angles, sums, counts = _angular_sums(power_spectrum, num_bins, use_mask)
    angular_profile = np.zeros(len(sums))
    filled = counts > 0
    angular_profile[filled] = sums[filled] / counts[filled]
    return angles, angular_profile
