"""Host restatements of the background estimators whose reference is not callable here: the checker of
tests/test_background_cpu.py and tests/test_gpu_background.py and the host side of tools/time_background.py.  Written from
the published algorithms (scikit-image's rolling ball, SciPy's symmetric correlation), never the product.

* ``rolling_ball``: scikit-image's ``restoration.rolling_ball`` (0.19-0.25) -- ``ball_kernel``, ``diff = kernel[centre] -
  kernel``, the image padded with +inf, ``min over offsets (img[p + o] + diff[o])``, float32 for float16 / float32 images and
  float64 otherwise, cast back with ``astype``.  ``skip_nan`` keeps scikit-image's ``if min_value > tmp`` rule on non-finite
  pixels (a NaN sum is skipped); ``rolling_ball_dense`` is the same minimum taken source pixel by source pixel, which costs
  ``H W`` passes whatever the radius.
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


def ball_diff_window(radius, dtype, ry, rx):
    """The values of :func:`ball_diff` at the offsets ``[-ry, ry] x [-rx, rx]`` only (``[dy + ry, dx + rx]``), by the same
    expressions element by element; +inf off the ball, also beyond ``ceil(radius)``."""
    dy = np.arange(-ry, ry + 1, dtype=np.float64)[:, None]
    dx = np.arange(-rx, rx + 1, dtype=np.float64)[None, :]
    ss = dy ** 2 + dx ** 2
    kernel = np.sqrt(np.clip(radius ** 2 - ss, 0, None))
    kernel[np.sqrt(ss) > radius] = np.inf
    kernel = kernel.astype(dtype)
    centre = np.sqrt(np.clip(np.float64(radius) ** 2, 0, None)).astype(dtype)
    diff = centre - kernel
    diff[kernel == np.inf] = np.inf
    return diff.astype(dtype)


def rolling_ball(image, radius, skip_nan=False):
    """scikit-image's ``rolling_ball(image, radius=radius)``, one ball offset at a time over the whole frame.  ``skip_nan``:
    accumulate with ``np.fmin`` from +inf, which is scikit-image's ``if min_value > tmp: min_value = tmp`` on non-finite
    pixels -- a NaN sum is skipped and a neighbourhood of NaN sums only gives +inf (``np.minimum`` propagates the NaN)."""
    image = np.asarray(image)
    ft = float_type(image.dtype)
    img = image.astype(ft)
    diff = ball_diff(radius, ft)
    R = diff.shape[0] // 2
    h, w = img.shape
    padded = np.pad(img, R, mode="constant", constant_values=np.inf)
    out = np.full((h, w), np.inf, dtype=ft)
    smaller = np.fmin if skip_nan else np.minimum
    with np.errstate(invalid="ignore"):                                  # -inf + inf
        for dy, dx in zip(*np.nonzero(np.isfinite(diff))):
            smaller(out, padded[dy:dy + h, dx:dx + w] + diff[dy, dx], out=out)
    return out.astype(image.dtype)


def rolling_ball_dense(image, radius, return_source=False):
    """:func:`rolling_ball` with the loops exchanged: every pixel of the frame in turn as the source ``s`` of
    ``img[s] + diff[s - p]`` for all outputs ``p``.  The same ``ball_diff`` values, type rule and ``astype``, and ``H W`` passes
    over the frame whatever the radius.  ``return_source``: also the flat index of the source pixel each output took its
    minimum from (the first in row-major order among equals)."""
    image = np.asarray(image)
    ft = float_type(image.dtype)
    img = image.astype(ft)
    h, w = img.shape
    diff = ball_diff_window(radius, ft, h - 1, w - 1)                    # diff[sy - y + h - 1, sx - x + w - 1]
    out = np.full((h, w), np.inf, dtype=ft)
    source = np.full((h, w), -1, dtype=np.int64)
    for sy in range(h):
        for sx in range(w):
            cand = img[sy, sx] + diff[sy:sy + h, sx:sx + w][::-1, ::-1]
            if return_source:
                source[cand < out] = sy * w + sx
            np.minimum(out, cand, out=out)
    out = out.astype(image.dtype)
    return (out, source) if return_source else out


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
