"""Patch-SVD denoising: the reference's ``mtflearn/denoise/_denoise_svd.py`` on the GPU, and the window operators both
denoisers share.

``denoise_svd`` is a rank-``k`` truncation of the matrix ``A`` of overlapping windows of a frame, put back by overlap-add.
``A`` is never formed here: the frame lives on the device and the four operations of ``csrc/zk_denoise.hip`` work on its
windows in place (``Y = (A - 1 mu^T) Q``, ``Z = A^T Y``, the dense window mean / covariance, the overlap-add).  The
randomized SVD is scikit-learn's ``randomized_svd`` (``sklearn/utils/extmath.py``, 1.7) restated around those products:
the same draw from NumPy's global random state, the same LU-normalised power iterations, QR, small SVD and sign rule, with
the thin ``(N, k + 10)`` / ``(D, k + 10)`` factors crossing to the host for ``scipy.linalg`` and every product with ``A``
on the device.  All device arithmetic is float64 whatever the frame's dtype (for a float32 frame scikit-learn would round
the factors to float32; that rounding is not reproduced).

``mtflearn_amd.denoise`` is the public face (it does not expose ``denoise_svd``, as the reference's subpackage does not);
``mtflearn_amd.denoise_svd`` / ``mtflearn_amd.DenoiseSVD`` are the top-level names.
"""
from __future__ import annotations

import numbers
from ctypes import c_void_p
from time import time

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

from . import _device, _native
from ._device import from_host, to_host

MOMENTS_MAX_PATCH = 48          # zk_windows_moments: largest patch edge (csrc/zk_denoise.hip)


# ----------------------------------------------------------------------------------------------- the window grid (host)
def _patch_start_indices(image_extent, patch_extent, step):
    """Window origins along one axis: ``0, step, 2 step, ...`` as long as they lie below the last possible origin
    ``image_extent - patch_extent``, and then that last origin itself (so the grid's final step may be shorter)."""
    if step <= 0:
        raise ValueError("extraction_step must be a positive integer.")
    last = image_extent - patch_extent
    if last <= 0:
        raise ValueError("patch_size must be strictly smaller than the image size.")
    regular = -(-last // step)                    # how many multiples of step are below the last origin
    return np.concatenate([step * np.arange(regular), [last]])


def _patch_edges(patch_size):
    """``(height, width)`` of a patch given as one number or as a pair: the validator both denoisers share."""
    edges = (patch_size, patch_size) if isinstance(patch_size, numbers.Number) else tuple(patch_size)
    if len(edges) != 2:
        raise ValueError("patch_size must be an int or a length-2 tuple.")
    return int(edges[0]), int(edges[1])


def _pair(value, ndim=2):
    return (value,) * ndim if isinstance(value, numbers.Number) else tuple(value)


def extract_patches(data, patch_shape=64, extraction_step=1):
    """``(N, ph, pw)`` windows of a 2-D array at the grid of :func:`_patch_start_indices`, rows of the grid first.  Host
    NumPy (a strided window view indexed at the grid): this is data the caller asks for, not a step of the denoisers,
    which never form it."""
    ph, pw = _pair(patch_shape)
    rows = _patch_start_indices(data.shape[0], ph, extraction_step)
    cols = _patch_start_indices(data.shape[1], pw, extraction_step)
    return sliding_window_view(data, (ph, pw))[np.ix_(rows, cols)].reshape(-1, ph, pw)


# ----------------------------------------------------------------------------------------------- device plumbing
def _ptr(array):
    return c_void_p(array.data_ptr()) if array is not None else None


class _Windows:
    """The implicit window matrix ``A`` (``N = ni * nj`` rows, ``D = ph * pw`` columns) of a device-resident frame."""

    def __init__(self, image, patch, ii, jj):
        self.image, self.code = image, _device.code(image)
        self.h, self.w = (int(v) for v in image.shape)
        self.ph, self.pw = int(patch[0]), int(patch[1])
        self.ii = np.ascontiguousarray(ii, dtype=np.int32)
        self.jj = np.ascontiguousarray(jj, dtype=np.int32)
        self.n, self.d = len(self.ii) * len(self.jj), self.ph * self.pw
        self.lib = _native.load()

    def _head(self):
        return (self.image.device.index, _ptr(self.image), self.code, self.h, self.w, self.ph, self.pw) + self._grid()

    def _grid(self):
        return (self.ii.ctypes.data_as(c_void_p), len(self.ii), self.jj.ctypes.data_as(c_void_p), len(self.jj))

    def _empty(self, shape):
        return _device.empty(shape, np.float64, self.image)

    def _stream(self):
        return c_void_p(_device.stream_ptr(self.image))

    def apply_dev(self, q_dev, n_columns, mean_dev=None):
        """``(A - 1 mean^T) Q`` -> ``(N, n_columns)`` on the device."""
        out = self._empty((self.n, n_columns))
        _native.check(self.lib.zk_windows_apply_dev(*self._head(), _ptr(q_dev), n_columns, _ptr(mean_dev), _ptr(out), self._stream()),
                      "zk_windows_apply_dev")
        return out

    def apply_t_dev(self, y_dev, n_columns):
        """``A^T Y`` -> ``(D, n_columns)`` on the device."""
        out = self._empty((self.d, n_columns))
        _native.check(self.lib.zk_windows_apply_t_dev(*self._head(), _ptr(y_dev), n_columns, _ptr(out), self._stream()),
                      "zk_windows_apply_t_dev")
        return out

    def apply(self, q):
        return to_host(self.apply_dev(from_host(q, self.image), q.shape[1]))

    def apply_t(self, y):
        return to_host(self.apply_t_dev(from_host(y, self.image), y.shape[1]))

    def moments_dev(self):
        """Mean ``(D,)`` and covariance ``(D, D)`` of the dense windows, on the device (the grid of this object is not used)."""
        mean = self._empty((self.d,))
        cov = self._empty((self.d, self.d))
        _native.check(self.lib.zk_windows_moments_dev(*self._head()[:7], _ptr(mean), _ptr(cov), self._stream()), "zk_windows_moments_dev")
        return mean, cov

    def reconstruct_dev(self, y_dev, n_components, v_dev=None, mean_dev=None):
        """Overlap-add of ``Y V + mean`` (or of the explicit batch ``Y`` when ``v_dev`` is None) -> ``(H, W)`` on the device."""
        out = self._empty((self.h, self.w))
        _native.check(self.lib.zk_windows_reconstruct_dev(self.image.device.index, self.h, self.w, self.ph, self.pw, *self._grid(), _ptr(y_dev),
                                                          n_components, _ptr(v_dev), _ptr(mean_dev), _ptr(out), self._stream()),
                      "zk_windows_reconstruct_dev")
        return out


def _upload_frame(img):
    """Host frame -> :class:`~mtflearn_amd._native.DeviceArray` in one of the five device formats (others widened as ``ZPs`` does)."""
    from .features.zernike_polys import ZPs
    _native.load()
    _native.require_device()
    return _native.DeviceArray.from_numpy(ZPs._device_operand(np.asarray(img)), _native.default_device())


# ----------------------------------------------------------------------------------------------- randomized SVD
def _randomized_svd_windows(win, n_components, n_oversamples=10):
    """``sklearn.utils.extmath.randomized_svd(A, n_components, random_state=None)`` (1.7: ``n_iter='auto'``,
    ``power_iteration_normalizer='auto'`` -> LU, ``transpose='auto'``, ``flip_sign=True``, ``gesdd``) with every product
    against ``A`` on the device.  The test matrix is drawn from NumPy's global ``RandomState`` exactly as scikit-learn draws
    it, so ``np.random.seed`` pins the result."""
    from scipy import linalg
    from sklearn.utils.extmath import svd_flip

    n_random = n_components + n_oversamples
    n_samples, n_features = win.n, win.d
    n_iter = 7 if n_components < 0.1 * min(n_samples, n_features) else 4
    transpose = n_samples < n_features                      # scikit-learn then factors A^T
    mul, mul_t = (win.apply_t, win.apply) if transpose else (win.apply, win.apply_t)      # M @ Q and M.T @ Q
    q = np.random.normal(size=(n_samples if transpose else n_features, n_random))
    lu = lambda x: linalg.lu(x, permute_l=True, check_finite=False)[0]
    for _ in range(n_iter):
        q = lu(mul(q))
        q = lu(mul_t(q))
    q = linalg.qr(mul(q), mode="economic", check_finite=False)[0]
    b = np.ascontiguousarray(mul_t(q).T)                    # Q^T M
    uhat, s, vt = linalg.svd(b, full_matrices=False, lapack_driver="gesdd")
    u = q @ uhat
    u, vt = svd_flip(u, vt, u_based_decision=not transpose)
    if transpose:
        return vt[:n_components, :].T, s[:n_components], u[:, :n_components].T
    return u[:, :n_components], s[:n_components], vt[:n_components, :]


def low_rank_svd(data, rank, compute_uv=False):
    """Leading ``rank`` singular values (or ``(u, s, v)``) of a host matrix the caller has formed:
    ``sklearn.utils.extmath.randomized_svd(data, rank)`` itself, as in the reference."""
    from sklearn.utils.extmath import randomized_svd
    u, s, v = randomized_svd(data, rank)
    return (u, s, v) if compute_uv else s


# ----------------------------------------------------------------------------------------------- the public calls
def _svd_arguments(img_shape, patch_size, extraction_step):
    """Validated ``(patch, step, row origins, column origins)`` with the reference's exceptions, before any device call."""
    if len(img_shape) != 2:
        raise ValueError("image must be a 2D array.")
    patch = _patch_edges(patch_size)
    if any(p >= n for p, n in zip(patch, img_shape)):
        raise ValueError("patch_size must be strictly smaller than the image dimensions.")
    step = max(1, int(patch[0] / 4)) if extraction_step is None else extraction_step
    ii, jj = (_patch_start_indices(n, p, step) for n, p in zip(img_shape, patch))
    return patch, step, ii, jj


def _check_components(n_components):
    if not isinstance(n_components, numbers.Integral) or n_components < 1:
        raise ValueError(f"n_components must be an int in the range [1, inf), not {n_components!r}")
    return int(n_components)


def _denoise_svd_device(image, patch, ii, jj, n_components, say=lambda *a: None):
    """``(clean (H, W) on the device, s)`` of a device-resident frame; ``say(line)`` prints the reference's progress lines."""
    win = _Windows(image, patch, ii, jj)
    say("Singular value decomposition...")
    t0 = time()
    u, s, vt = _randomized_svd_windows(win, n_components)
    say("done in %.2fs." % (time() - t0))
    say("Reconstructing...")
    t0 = time()
    k = len(s)
    clean = win.reconstruct_dev(from_host(u * s, image), k, from_host(vt, image))
    if not _device.is_native(clean):
        import torch
        torch.cuda.current_stream(clean.device).synchronize()
    say("done in %.2fs." % (time() - t0))
    return clean, s


def denoise_svd(img, patch_size, n_components, extraction_step=None, verbose=True, return_s=False):
    """Patch-SVD denoising (reference ``denoise_svd``): the windows of ``img`` at every ``extraction_step``-th origin
    (default ``max(1, int(patch_height / 4))``; the last origin of each axis is always included) are replaced by their
    rank-``n_components`` approximation from a randomized SVD and averaged back where they overlap.  ``patch_size``: an int
    or ``(height, width)``.  Returns the float64 frame, and the singular values with ``return_s``.

    The randomized SVD draws from NumPy's global random state like scikit-learn's with ``random_state=None``:
    ``np.random.seed`` before the call pins the result.  Runs on the GPU in float64 (float32 / float64 / uint8 / uint16 /
    int16 frames travel as they are); the window matrix is never formed.  There is no CPU fallback."""
    img = np.asarray(img)
    patch, _, ii, jj = _svd_arguments(img.shape, patch_size, extraction_step)
    n_components = _check_components(n_components)
    say = print if verbose == True else (lambda *a: None)     # noqa: E712 (the reference's own comparison)
    say("Extracting reference patches...")
    t0 = time()
    image = _upload_frame(img)
    say("done in %.2fs." % (time() - t0))
    clean, s = _denoise_svd_device(image, patch, ii, jj, n_components, say)
    clean = clean.numpy()
    return (clean, s) if return_s else clean


class DenoiseSVD:
    """The reference's object form of :func:`denoise_svd`: ``DenoiseSVD(image, n_components, patch_size,
    extraction_step).run()`` returns the clean frame and keeps it in ``img_clean``, the singular values in ``s_values``
    (``patches`` belongs to the reference's attribute set and stays ``None``: no patch matrix exists here)."""

    def __init__(self, image, n_components, patch_size, extraction_step):
        self.image, self.patch_size = image, patch_size
        self.n_components, self.extraction_step = n_components, extraction_step
        self.patches = self.s_values = self.img_clean = None

    def run(self, verbose=False):
        # the module's ``denoise_svd`` is looked up at call time, so a replacement of that attribute is what runs
        result = denoise_svd(self.image, self.patch_size, self.n_components, self.extraction_step, verbose, True)
        self.img_clean, self.s_values = result
        return self.img_clean


def reconstruct_patches(patches, img_shape, reconstruction_step):
    """Overlap-add of an ``(N, ph, pw)`` batch of patches laid on the grid of :func:`extract_patches` and divided by the
    number of patches on each pixel (reference ``reconstruct_patches``), on the GPU (``zk_windows_reconstruct``)."""
    img_height, img_width = _pair(img_shape)
    patches = np.asarray(patches)
    ph, pw = patches.shape[1:3]
    ii = _patch_start_indices(img_height, ph, reconstruction_step).astype(np.int32)
    jj = _patch_start_indices(img_width, pw, reconstruction_step).astype(np.int32)
    if patches.shape[0] != len(ii) * len(jj):
        raise ValueError(f"expected {len(ii) * len(jj)} patches for this grid, got {patches.shape[0]}")
    lib = _native.load()
    _native.require_device()
    batch = np.ascontiguousarray(patches, dtype=np.float64)
    out = np.empty((int(img_height), int(img_width)))
    _native.check(lib.zk_windows_reconstruct(_native.default_device(), int(img_height), int(img_width), int(ph), int(pw),
                                             ii.ctypes.data_as(c_void_p), len(ii), jj.ctypes.data_as(c_void_p), len(jj),
                                             batch.ctypes.data_as(c_void_p), 0, None, None, out.ctypes.data_as(c_void_p)),
                  "zk_windows_reconstruct")
    return out
