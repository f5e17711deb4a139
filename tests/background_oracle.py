"""Host restatements of the background estimators whose reference is not callable here: the checker of
tests/test_background_cpu.py and tests/test_gpu_background.py and the host side of tools/time_background.py.  Written from
the published algorithms (scikit-image's rolling ball, SciPy's symmetric correlation), never the product.

* ``rolling_ball``: scikit-image's ``restoration.rolling_ball`` (0.19-0.25) -- ``ball_kernel``, ``diff = kernel[centre] -
  kernel``, the image padded with +inf, ``min over offsets (img[p + o] + diff[o])``, float32 for float16 / float32 images and
  float64 otherwise, cast back with ``astype``.
* ``gaussian_filter`` / ``baseline``: SciPy's ``gaussian_filter`` in SciPy's own summation order for symmetric weights
  (``t = x[0] w[0]``, then ``t += (x[-j] + x[+j]) w[j]`` for j from the radius down to 1), mode 'reflect'.
"""
import numpy as np


def float_type(dtype):
    """scikit-image's ``_supported_float_type`` for one dtype."""
    dtype = np.dtype(dtype)
    return np.dtype(np.float32) if dtype in (np.float16, np.float32) else np.dtype(np.float64)


def ball_diff(radius, dtype=np.float64):
    """``(2R + 1, 2R + 1)`` intensity difference of scikit-image's ``ball_kernel(radius, 2)`` in ``dtype``: +inf off the
    ball (R = ceil(radius))."""
    R = int(np.ceil(radius))
    coords = np.stack(np.meshgrid(*[np.arange(-R, R + 1, dtype=np.float64)] * 2, indexing="ij"), axis=-1)
    ss = np.sum(coords ** 2, axis=-1)
    kernel = np.sqrt(np.clip(radius ** 2 - ss, 0, None))
    kernel[np.sqrt(ss) > radius] = np.inf
    kernel = kernel.astype(dtype)
    diff = kernel[R, R] - kernel
    diff[kernel == np.inf] = np.inf
    return diff.astype(dtype)


def rolling_ball(image, radius):
    """scikit-image's ``rolling_ball(image, radius=radius)``, one ball offset at a time over the whole frame."""
    image = np.asarray(image)
    ft = float_type(image.dtype)
    img = image.astype(ft)
    diff = ball_diff(radius, ft)
    R = diff.shape[0] // 2
    h, w = img.shape
    padded = np.pad(img, R, mode="constant", constant_values=np.inf)
    out = np.full((h, w), np.inf, dtype=ft)
    for dy, dx in zip(*np.nonzero(np.isfinite(diff))):
        np.minimum(out, padded[dy:dy + h, dx:dx + w] + diff[dy, dx], out=out)
    return out.astype(image.dtype)


def rolling_ball_at(image, radius, points):
    """The same at a few ``(row, col)`` pixels only, by brute force over the ball (large frames)."""
    image = np.asarray(image)
    ft = float_type(image.dtype)
    img = image.astype(ft)
    diff = ball_diff(radius, ft)
    R = diff.shape[0] // 2
    padded = np.pad(img, R, mode="constant", constant_values=np.inf)
    out = np.empty(len(points), dtype=ft)
    for i, (y, x) in enumerate(points):
        out[i] = np.min(padded[y:y + 2 * R + 1, x:x + 2 * R + 1] + diff)
    return out.astype(image.dtype)


def gaussian_weights(sigma):
    """Full symmetric Gaussian kernel of ``scipy.ndimage`` (truncate 4.0), or None for an axis SciPy skips."""
    sd = float(sigma)
    if not sd > 1e-15:
        return None
    r = int(4.0 * sd + 0.5)
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    return phi / phi.sum()


def correlate_symmetric(x, weights, axis):
    """SciPy's ``correlate1d`` of float64 ``x`` with symmetric ``weights`` along ``axis``, mode 'reflect', in its order."""
    r = len(weights) // 2
    x = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    n = x.shape[-1]
    pad = [(0, 0)] * (x.ndim - 1) + [(r, r)]
    xp = np.pad(x, pad, mode="symmetric")
    t = xp[..., r:r + n] * weights[r]
    for j in range(r, 0, -1):
        t = t + (xp[..., r - j:r - j + n] + xp[..., r + j:r + j + n]) * weights[r - j]
    return np.moveaxis(t, -1, axis)


def gaussian_filter(image, sigma):
    """``scipy.ndimage.gaussian_filter(float64 image, sigma)``: axis 0, then axis 1."""
    sigmas = (sigma, sigma) if np.isscalar(sigma) else tuple(sigma)
    out = np.asarray(image, dtype=np.float64).copy()
    for axis, s in enumerate(sigmas):
        w = gaussian_weights(s)
        if w is not None:
            out = correlate_symmetric(out, w, axis)
    return out


def baseline(image, sigma, num_iters, gauss=gaussian_filter):
    """The reference's ``estimate_background_baseline`` loop around ``gauss``."""
    image = np.asarray(image, dtype=np.float64)
    out = np.minimum(gauss(image, sigma), image)
    for _ in range(int(num_iters) - 1):
        out = np.minimum(gauss(out, sigma), image)
    return out
