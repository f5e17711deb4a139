"""Denoising: the reference's ``mtflearn.denoise`` subpackage (``denoise/__init__.py``), on the GPU.

The first step of the notebooks' chain, ahead of :mod:`mtflearn_amd.background` and
:func:`mtflearn_amd.features.local_max`:

* ``DenoiseSVD`` (and ``mtflearn_amd.denoise_svd`` at the package top level): patch-SVD denoising, a randomized rank-``k``
  truncation of the matrix of overlapping windows (:mod:`mtflearn_amd._denoise_svd`);
* ``denoise_svd_memory_view``: patch-PCA denoising on **every** window of the frame -- mean and covariance of the dense
  windows, ``numpy.linalg.eigh`` on the host, projection on the leading eigenvectors, overlap-add;
* ``denoise_fft``: the Fourier-coefficient filter of :mod:`mtflearn_amd.features.pickers`;
* ``extract_patches``, ``low_rank_svd``, ``reconstruct_patches``: the reference's helpers; ``apply_poisson_noise``;
* ``apply_scan_noise``: the STEM scan-distortion model -- every row and every column of every frame of a stack shifted by its
  own random sub-pixel amount and the stack resampled on the device (``zk_scan_resample``, ``csrc/zk_resample.hip``).

The window matrix is never formed: the frame is resident on the device and ``csrc/zk_denoise.hip`` works on its windows in
place (``zk_windows_*``).  There is no CPU fallback for the arithmetic; every argument check comes before the first device
call.  Like the reference's subpackage, this module does not expose ``denoise_svd`` (that name is the patch-SVD function at
the package top level; here the memory-view variant carries its explicit name).
"""
from __future__ import annotations

import numbers
from ctypes import c_void_p

import numpy as np

from . import _denoise_svd as _svd
from . import _native
from ._device import from_host, to_host
from ._denoise_svd import DenoiseSVD, extract_patches, low_rank_svd, reconstruct_patches
from .features.pickers import denoise_fft

__all__ = ["DenoiseSVD", "denoise_svd_memory_view", "extract_patches", "low_rank_svd", "reconstruct_patches", "denoise_fft",
           "apply_poisson_noise", "apply_scan_noise"]

SCAN_MODES = ("reflect", "mirror", "nearest", "grid-wrap", "grid-constant", "constant")
SCAN_CUBIC_MODES = ("reflect", "mirror", "grid-wrap")       # the modes whose spline prefilter has exact boundary conditions
_SCIPY_ONLY_MODES = ("wrap", "grid-mirror")                  # known to map_coordinates, not offered here
_SCAN_DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)


def _memory_view_patch(image_shape, patch_size):
    """The square patch edge, with the reference's exceptions; the device limits come after them."""
    edges = _svd._patch_edges(patch_size)
    if edges[0] != edges[1]:
        raise ValueError(f"denoise_svd currently supports only square patches; got patch_size={edges}.")
    p = edges[0]
    if len(image_shape) != 2:
        raise ValueError("image must be a 2D array.")
    if not 1 <= p <= min(image_shape):
        raise ValueError("patch_size must be at least 1 and at most the image dimensions.")
    if p > _svd.MOMENTS_MAX_PATCH:
        raise ValueError(f"patch_size must be at most {_svd.MOMENTS_MAX_PATCH} pixels on the device, not {p}")
    return p


def _select_components(cov, n_components, threshold):
    """Leading eigenvectors of the window covariance and how many are kept: ``(top (D, k), explained_variance_ratio (D,), k)``.
    The ratio lists every eigenvalue over their sum, largest first; ``n_components=None`` keeps components until the
    cumulated ratio reaches ``threshold``; ``k`` is clamped to ``[1, D]``.  A covariance whose eigenvalues sum to (nearly)
    zero has a ratio of zeros and keeps one component, without a division."""
    values, vectors = np.linalg.eigh(cov)                       # ascending
    values = values[::-1]
    total = values.sum()
    ratio = np.zeros_like(values) if np.isclose(total, 0.0) else values / total
    if n_components is None:
        n_components = int(np.count_nonzero(np.cumsum(ratio) < threshold)) + 1 if ratio.any() else 1
    k = min(max(int(n_components), 1), len(values))
    return vectors[:, len(values) - k:], ratio, k


def _memory_view_device(image, p, n_components, threshold):
    """``(recon on the device, explained_variance_ratio, n_components)`` of a device-resident frame."""
    h, w = (int(v) for v in image.shape)
    dense = _svd._Windows(image, (p, p), np.arange(h - p + 1), np.arange(w - p + 1))
    mean, cov = dense.moments_dev()
    top, ratio, n_components = _select_components(to_host(cov), n_components, threshold)
    proj = dense.apply_dev(from_host(top, image), n_components, mean)
    recon = dense.reconstruct_dev(proj, n_components, from_host(top.T, image), mean)
    return recon, ratio, n_components


def denoise_svd_memory_view(image, patch_size, n_components=None, threshold=0.9, batch_size=None,
                            target_memory_bytes=100 * 2 ** 20, show_progress=True):
    """Patch-PCA denoising over every window of the frame (reference ``_denoise_svd_memory_view.denoise_svd``).

    The mean and covariance of all ``(H - p + 1) (W - p + 1)`` dense ``p x p`` windows are formed on the device, the
    covariance is diagonalised on the host (``numpy.linalg.eigh``), every window is projected on the ``n_components``
    leading eigenvectors (``None``: as many as it takes for the cumulated explained-variance ratio to reach ``threshold``)
    and rebuilt, and overlapping windows are averaged.  Returns ``(recon, explained_variance_ratio, n_components)``:
    ``recon`` float64, the ratio of all ``p * p`` eigenvalues in descending order (all zero for a frame without variance,
    where ``n_components`` is 1).

    ``patch_size``: an int or a pair of equal ints, at most 48 on the device.  ``batch_size``, ``target_memory_bytes`` and
    ``show_progress`` are accepted for compatibility and have no effect: nothing is batched on the host and there is no
    progress bar."""
    image = np.asarray(image)
    p = _memory_view_patch(image.shape, patch_size)
    recon, ratio, n_components = _memory_view_device(_svd._upload_frame(image), p, n_components, threshold)
    return recon.numpy(), ratio, n_components


def apply_poisson_noise(image, dose_per_pixel=100):
    """Shot noise at ``dose_per_pixel`` expected counts per unit of intensity: a draw of ``np.random.poisson`` (NumPy's
    global state) at ``image * dose_per_pixel``, rescaled to the image's maximum and cast to its dtype.  Host NumPy."""
    counts = np.random.poisson(image * dose_per_pixel)
    max_val = np.max(image)
    if max_val > 0:
        counts = (counts / np.max(counts)) * max_val
    return counts.astype(image.dtype)


# ----------------------------------------------------------------------------------------------- scan noise
def _check_scan_order_mode(order, mode):
    """``(order, ZK_RESAMPLE_* code)``, with SciPy's exceptions where SciPy refuses and ``NotImplementedError`` where only
    this package does."""
    if isinstance(order, bool) or not isinstance(order, (numbers.Integral, np.integer)):
        raise TypeError(f"order must be an integer, not {order!r}")
    if order < 0 or order > 5:
        raise RuntimeError("spline order not supported")
    if mode in _SCIPY_ONLY_MODES:
        raise NotImplementedError(f"mode {mode!r} is not offered on the device; supported: {', '.join(SCAN_MODES)}")
    if mode not in SCAN_MODES:
        raise ValueError(f"boundary mode not supported: {mode!r}")
    if order not in (0, 1, 3):
        raise NotImplementedError(f"spline order {int(order)} is not offered on the device; supported: 0, 1 and 3")
    if order == 3 and mode not in SCAN_CUBIC_MODES:
        raise NotImplementedError(f"order 3 is offered for the modes {', '.join(SCAN_CUBIC_MODES)} (the ones whose spline prefilter "
                                  f"has exact boundary conditions), not for {mode!r}; orders 0 and 1 take every mode")
    return int(order), _native.RESAMPLE_MODES[mode]


def _check_scan_shape(shape):
    if len(shape) != 3:
        raise ValueError(f"images must be a (Z, H, W) stack, not {len(shape)}-D")
    if 0 in shape:
        raise ValueError(f"an empty stack has no frames to resample: shape {tuple(shape)}")
    return tuple(int(v) for v in shape)


def _jitter(seed, shape, jx, jy):
    """The reference's draws: ``(dx (Z, H), dy (Z, W))`` float64, both always drawn, ``dx`` first, whatever the factors."""
    z, h, w = shape
    jx, jy = (0 if j is None else j for j in (jx, jy))
    for name, j in (("jx", jx), ("jy", jy)):
        if isinstance(j, bool) or not isinstance(j, (numbers.Real, np.integer, np.floating)) or not np.isfinite(j):
            raise ValueError(f"{name} must be a finite number or None, not {j!r}")
    rng = np.random.default_rng(seed=seed)
    dx = rng.normal(0, 1, (z, h, 1)) * jx
    dy = rng.normal(0, 1, (z, 1, w)) * jy
    return np.ascontiguousarray(dx.reshape(z, h), dtype=np.float64), np.ascontiguousarray(dy.reshape(z, w), dtype=np.float64)


def _resample_host(images, dx, dy, order, mode_code):
    """One ``zk_scan_resample`` call: the stack goes up frame by frame through the staging ring, the ``Z (H + W)`` shifts go up
    once, the result comes down."""
    lib = _native.load()
    _native.require_device()
    z, h, w = images.shape
    out = _native.pinned.empty(images.shape, np.float32 if images.dtype == np.float32 else np.float64)
    ptr = lambda a: a.ctypes.data_as(c_void_p)
    _native.check(lib.zk_scan_resample(_native.default_device(), ptr(images), _native.dtype_code(images.dtype), z, h, w, ptr(dx), ptr(dy),
                                       order, mode_code, ptr(out)), "zk_scan_resample")
    return out


def apply_scan_noise(images, jx=1, jy=0, seed=None, order=1, mode='reflect'):
    """STEM scan distortion of a ``(Z, H, W)`` stack (reference ``denoise/_noise_models.py:28-57``): row ``y`` of frame ``z`` is
    shifted along x by ``dx[z, y]`` (fly-back jitter) and column ``x`` along y by ``dy[z, x]``,

        ``out[z, y, x] = S_z(y + dy[z, x], x + dx[z, y])``,

    ``S_z`` the B-spline interpolant of ``order`` of frame ``z``, extended by ``mode`` as ``scipy.ndimage.map_coordinates``
    extends it.  The shifts are the reference's draws, ``rng = np.random.default_rng(seed)``, ``dx = rng.normal(0, 1, (Z, H, 1))
    * jx``, then ``dy = rng.normal(0, 1, (Z, 1, W)) * jy`` -- both always drawn, in that order, so a seed moves the same rows as
    in the reference; ``None`` for a factor means 0.  Only these ``Z (H + W)`` numbers and the stack cross to the device: no
    coordinate array exists on either side.  The coordinate sums and all arithmetic are float64.

    ``order``: 0 (nearest, ``floor(c + 0.5)``), 1 or 3.  ``mode``: ``'reflect'``, ``'mirror'``, ``'nearest'``, ``'grid-wrap'``,
    ``'grid-constant'`` or ``'constant'`` (``cval`` is 0, the reference's signature has none); order 3 takes ``'reflect'``,
    ``'mirror'`` and ``'grid-wrap'``.  Orders 2, 4 and 5, order 3 with another mode and the modes ``'wrap'`` / ``'grid-mirror'``
    raise ``NotImplementedError``; an unknown mode is a ``ValueError`` and an order outside 0..5 a ``RuntimeError``, as in SciPy.
    float32 and float64 stacks return their own dtype (float32 is rounded once, at the store).

    Deviations from the reference, both deliberate:

    * uint8, uint16 and int16 stacks are widened exactly and return **float64**; the reference rounds the result back to the
      integer type.  Other dtypes are a ``TypeError``.
    * frames are independent.  The reference hands the whole 3-D stack to ``map_coordinates``, which at ``order > 1`` also
      prefilters along ``z`` -- coupling neighbouring frames -- and, for ``mode='reflect'``, starts each prefilter recursion from
      a series truncated to the axis length.  On an axis shorter than about 28 samples its result is therefore not the
      interpolant it documents (at integer positions it misses the input by 1.2e-4 at n = 3, 4.6e-7 at n = 5, 2e-16 at n = 16;
      the 3-D call and frame-by-frame calls differ by 1.6e-4 of the data at ``Z = 3``).  Here every prefilter segment starts
      from 32 samples of the extended signal (``|sqrt(3) - 2|^32`` is below one float64 ulp), which is the exact interpolant
      of each frame: **order 3 under 'reflect' on short axes, z included, differs from the reference for this reason**;
      ``'mirror'`` and ``'grid-wrap'`` agree with it to rounding, orders 0 and 1 in every mode.

    Every check precedes the first device call; there is no CPU fallback.  The resident form is
    :func:`mtflearn_amd.resident.scan_noise_device`, bit for bit the same numbers."""
    order, mode_code = _check_scan_order_mode(order, mode)
    images = np.asarray(images)
    shape = _check_scan_shape(images.shape)
    if images.dtype not in _SCAN_DTYPES:
        raise TypeError(f"images must be float32, float64, uint8, uint16 or int16, not {images.dtype}")
    dx, dy = _jitter(seed, shape, jx, jy)
    return _resample_host(np.ascontiguousarray(images), dx, dy, order, mode_code)
