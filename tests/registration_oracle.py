"""The NumPy statement of ``estimate_shifts`` (include/zernike_hip.h, "Stack registration"), written from the contract:
``np.fft`` for the spectra, the explicit ``Ey @ P @ Ex`` for the upsampled plane, ``np.argmax`` for both peaks.  It is the
checker of the registration tests, never the product."""
import math

import numpy as np


def hann(n):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)


def window_of(h, w, window):
    if window is None:
        return np.ones((h, w))
    assert window == "hann"
    return np.outer(hann(h), hann(w))


def cross_power(frame, ref, normalization=None, window=None):
    h, w = frame.shape
    win = window_of(h, w, window)
    F = np.fft.fft2(np.asarray(frame, np.float64) * win)
    R = np.fft.fft2(np.asarray(ref, np.float64) * win)
    P = R * np.conj(F)
    if normalization == "phase":
        mag = np.abs(P)
        P = P / np.maximum(mag, 100 * np.finfo(np.float64).eps * mag.max())
    else:
        assert normalization is None
    return P


def planes(frame, ref, upsample=100, max_shift=None, normalization=None, window=None):
    """``(shift (2,), peak, c (H, W), C (S, S) or None)`` of one frame against one reference."""
    h, w = frame.shape
    P = cross_power(frame, ref, normalization, window)
    c = np.real(np.fft.ifft2(P))
    ly, lx = np.fft.fftfreq(h, 1 / h), np.fft.fftfreq(w, 1 / w)
    masked = c
    if max_shift is not None:
        allowed = (np.abs(ly) <= max_shift)[:, None] & (np.abs(lx) <= max_shift)[None, :]
        masked = np.where(allowed, c, -np.inf)
    at = int(np.argmax(masked))
    y0, x0 = ly[at // w], lx[at % w]
    if upsample == 1:
        return np.array([y0, x0]), c.flat[at], c, None
    s = math.ceil(1.5 * upsample)
    off = s // 2
    ys = y0 + (np.arange(s) - off) / upsample
    xs = x0 + (np.arange(s) - off) / upsample
    Ey = np.exp(2j * np.pi * ys[:, None] * np.fft.fftfreq(h)[None, :])
    Ex = np.exp(2j * np.pi * np.fft.fftfreq(w)[:, None] * xs[None, :])
    C = np.real(Ey @ P @ Ex) / (h * w)
    at = int(np.argmax(C))
    return np.array([ys[at // s], xs[at % s]]), C.flat[at], c, C


def estimate_shifts(stack, reference=0, upsample=100, max_shift=None, normalization=None, window=None):
    """``(shift (B, 2), peak (B,))``, the three forms of ``reference`` as in the package."""
    stack = np.asarray(stack)
    b = len(stack)
    shift, peak = np.zeros((b, 2)), np.zeros(b)
    for k in range(b):
        if isinstance(reference, str):
            assert reference == "previous"
            ref = stack[max(k - 1, 0)]
        elif np.ndim(reference) == 0:
            ref = stack[reference]
        else:
            ref = reference
        shift[k], peak[k] = planes(stack[k], ref, upsample, max_shift, normalization, window)[:2]
    if isinstance(reference, str):
        shift[0] = 0.0
        shift = np.cumsum(shift, axis=0)
    return shift, peak


def top_two_margin(plane):
    """``(max - second) / |max|`` of a plane."""
    flat = np.partition(np.asarray(plane).ravel(), -2)       # the two largest in their sorted places: the numbers of a full sort
    return (flat[-1] - flat[-2]) / abs(flat[-1])


def fourier_shift(frame, sy, sx):
    """``frame`` translated by ``(sy, sx)`` through its spectrum: ``out(y, x) = frame(y - sy, x - sx)`` for the band-limited
    periodic interpolant.  The caller has zeroed the Nyquist row / column of an even extent, so the result is real and exact."""
    h, w = frame.shape
    ky, kx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    return np.real(np.fft.ifft2(np.fft.fft2(frame) * np.exp(-2j * np.pi * (ky * sy + kx * sx))))


def band_limited_noise(h, w, seed):
    """A seeded white-noise frame with the Nyquist row and column of even extents zeroed."""
    F = np.fft.fft2(np.random.default_rng(seed).standard_normal((h, w)))
    if h % 2 == 0:
        F[h // 2, :] = 0
    if w % 2 == 0:
        F[:, w // 2] = 0
    return np.real(np.fft.ifft2(F))
