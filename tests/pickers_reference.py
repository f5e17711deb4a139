"""Independent high-precision statements of what the picker kernels compute -- TEST INFRASTRUCTURE.

Nothing here imports the product or ``oracle/``: each function states one operation of ``csrc/zk_pickers.hip`` through
a different route than the kernel and than ``oracle/pickers_oracle.py`` take (extended-precision FFT, the plain lag sum
without any FFT, SciPy's own interpolation), so that an error common to the kernel and the oracle does not hide.
``tests/test_pickers_cpu.py`` checks these statements and the oracle against each other without a GPU.
"""
from collections import namedtuple

import numpy as np
import scipy.fft
from scipy.ndimage import map_coordinates
from scipy.signal import correlate


def window_ref(name, size):
    """The 1-D taper of ``_estimate_n_max.py:45-53`` from its closed form (numpy.hanning / hamming / blackman,
    scipy.signal.windows.tukey(alpha=0.5)); None for no window."""
    if name is None:
        return None
    if size == 1:
        return np.ones(1)
    x = np.arange(size) / (size - 1.0)
    if name in ("hann", "hanning"):
        return 0.5 - 0.5 * np.cos(2 * np.pi * x)
    if name == "hamming":
        return 0.54 - 0.46 * np.cos(2 * np.pi * x)
    if name == "blackman":
        return 0.42 - 0.5 * np.cos(2 * np.pi * x) + 0.08 * np.cos(4 * np.pi * x)
    if name == "tukey":
        alpha = 0.5
        edge = np.minimum(x, 1.0 - x)                                     # distance to the nearer end, in [0, 1/2]
        return np.where(edge < alpha / 2, 0.5 - 0.5 * np.cos(2 * np.pi * edge / alpha), 1.0)
    raise ValueError(name)


def power_spectra_ref(img, size, origins, window_1d=None):
    """``|fftshift(fft2(window * outer(w, w)))|^2`` of every ``size x size`` window at ``origins`` (row, column), computed
    in extended precision (``np.longdouble`` -> complex256 transform) and rounded to float64 at the end."""
    img = np.asarray(img)
    taper = None if window_1d is None else np.outer(np.asarray(window_1d, np.longdouble), np.asarray(window_1d, np.longdouble))
    out = np.empty((len(origins), size, size), dtype=np.float64)
    for b, (y, x) in enumerate(origins):
        win = img[y:y + size, x:x + size].astype(np.longdouble)
        assert win.shape == (size, size)
        if taper is not None:
            win = win * taper
        spec = scipy.fft.fftshift(scipy.fft.fft2(win))
        assert spec.dtype == np.result_type(np.longdouble, np.complex64)
        out[b] = (spec.real ** 2 + spec.imag ** 2).astype(np.float64)
    return out


def autocorr_mean_ref(img, ws, origins, standardize=True):
    """Mean over the windows of their 'same' autocorrelation as the plain lag sum
    (``scipy.signal.correlate(..., method='direct')``: no FFT anywhere), float64; the windows are standardised with the
    population standard deviation first (``_patch_size.py:9-19``, which raises on a constant window)."""
    img = np.asarray(img)
    acc = np.zeros((ws, ws), dtype=np.float64)
    for y, x in origins:
        win = img[y:y + ws, x:x + ws].astype(np.float64)
        assert win.shape == (ws, ws)
        if standardize:
            std = win.std()
            if std == 0:
                raise ValueError("Standard deviation is zero, can't standardize the image.")
            win = (win - win.mean()) / std
        acc += correlate(win, win, mode="same", method="direct")
    return acc / len(origins)


def polar_radii(h, w):
    return int(np.ceil(np.hypot(h / 2, w / 2)))


def warp_polar_ref(data, center=None):
    """``skimage.transform.warp_polar(data, center, scaling='linear')`` for 2-D float data through SciPy's own linear
    interpolation: 360 angles x R = ceil(radius) radii, radius = hypot(h/2, w/2), sample (a, x) at
    ``row = x (radius / R) sin(a) + center_row``, ``col = x (radius / R) cos(a) + center_col``, zero outside the array,
    then clipped to the input's [min, max] (exact zeros stay when 0 lies outside that range)."""
    data = np.asarray(data, dtype=np.float64)
    h, w = data.shape
    ci, cj = (h // 2, w // 2) if center is None else center
    radius = np.hypot(h / 2, w / 2)
    R = int(np.ceil(radius))
    ang = (2 * np.pi * np.arange(360) / 360)[:, None]
    rad = (np.arange(R) * (radius / R))[None, :]
    rr = rad * np.sin(ang) + ci
    cc = rad * np.cos(ang) + cj
    out = map_coordinates(data, [rr, cc], order=1, mode="grid-constant", cval=0.0)
    lo, hi = data.min(), data.max()
    zero = out == 0
    out = np.clip(out, lo, hi)
    if not (lo <= 0 <= hi):
        out[zero] = 0
    return out


def radial_profile_ref(data, center=None, method="max"):
    """The 360 angles of ``warp_polar_ref`` aggregated per radius; 'mean' and 'sum' add in extended precision, so the
    reference carries no summation error of its own (a float64 sum down axis 0 is a plain running sum)."""
    polar = warp_polar_ref(data, center)
    if method == "max":
        return polar.max(axis=0)
    total = polar.astype(np.longdouble).sum(axis=0)
    return ({"mean": total / polar.shape[0], "sum": total}[method]).astype(np.float64)


DenoiseRef = namedtuple("DenoiseRef", "out k power order")


def denoise_fft_ref(image, p):
    """``denoise/_denoise_fft.py:4-47``: ``np.fft.fft2``, keep the ``k = ceil(p n)`` largest powers, real part of
    ``ifft2``.  Also returns ``k``, the powers (flat, float64) and ``order``, their flat indices from the largest down,
    so that a test can see how far the cut is from the next power."""
    image = np.asarray(image, dtype=np.float64)
    spec = np.fft.fft2(image)
    power = (np.abs(spec) ** 2).ravel()
    k = int(np.ceil(p * power.size))
    order = np.argsort(-power, kind="stable")
    mask = np.zeros(power.size, dtype=bool)
    mask[order[:k]] = True
    out = np.real(np.fft.ifft2(spec * mask.reshape(spec.shape)))
    return DenoiseRef(out, k, power, order)


def denoise_cut(ref, shape, rel=1e-9):
    """How the cut after the k-th largest power sits among the reference's powers: ``(decided, splits_pair)``.
    ``decided``: no power other than the conjugate partner of the k-th lies within ``rel`` of the largest power from
    the k-th, so the kept set does not depend on rounding.  ``splits_pair``: that partner is the (k+1)-th, so the cut
    keeps one half of a conjugate pair (either half gives the same real image)."""
    power, order, k = ref.power, ref.order, ref.k
    n = power.size
    if k >= n:
        return True, False
    kth = order[k - 1]
    u, v = divmod(int(kth), shape[1])
    partner = ((-u) % shape[0]) * shape[1] + (-v) % shape[1]
    near = np.flatnonzero(np.abs(power - power[kth]) <= rel * power[order[0]])
    near = [j for j in near if j != kth]
    if not near:
        return True, False
    if near != [partner]:
        return False, False
    return True, bool(order[k] == partner)
