"""Denoising: the reference's ``mtflearn.denoise`` subpackage (``denoise/__init__.py``), on the GPU.

The first step of the notebooks' chain, ahead of :mod:`mtflearn_amd.background` and
:func:`mtflearn_amd.features.local_max`:

* ``DenoiseSVD`` (and ``mtflearn_amd.denoise_svd`` at the package top level): patch-SVD denoising, a randomized rank-``k``
  truncation of the matrix of overlapping windows (:mod:`mtflearn_amd._denoise_svd`);
* ``denoise_svd_memory_view``: patch-PCA denoising on **every** window of the frame -- mean and covariance of the dense
  windows, ``numpy.linalg.eigh`` on the host, projection on the leading eigenvectors, overlap-add;
* ``denoise_fft``: the Fourier-coefficient filter of :mod:`mtflearn_amd.features.pickers`;
* ``extract_patches``, ``low_rank_svd``, ``reconstruct_patches``: the reference's helpers; ``apply_poisson_noise``.

The window matrix is never formed: the frame is resident on the device and ``csrc/zk_denoise.hip`` works on its windows in
place (``zk_windows_*``).  There is no CPU fallback for the arithmetic; every argument check comes before the first device
call.  Like the reference's subpackage, this module does not expose ``denoise_svd`` (that name is the patch-SVD function at
the package top level; here the memory-view variant carries its explicit name).
"""
from __future__ import annotations

import numpy as np

from . import _denoise_svd as _svd
from ._device import from_host, to_host
from ._denoise_svd import DenoiseSVD, extract_patches, low_rank_svd, reconstruct_patches
from .features.pickers import denoise_fft

__all__ = ["DenoiseSVD", "denoise_svd_memory_view", "extract_patches", "low_rank_svd", "reconstruct_patches", "denoise_fft",
           "apply_poisson_noise"]


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
