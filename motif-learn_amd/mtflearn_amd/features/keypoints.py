"""Key points around the moment transform: the caller side of SURVEY 8(f)2 -- reference ``mtflearn/features/_keypoint.py``.

``KeyPoints(pts, img, size)`` keeps the reference's constructor, attributes (``pts`` after border clearing, ``img``, ``size``,
``shape``, ``patches``) and methods, restated on whole arrays instead of per-point Python loops.  ``extract_patches`` returns the
``(N, size, size)`` batch the reference cuts (``_keypoint.py:60-78``) for callers that want the windows themselves;
``moments(zps)`` is the device shortcut this package adds: the moments of those same windows straight from the frame resident on
the GPU (``ZPs.transform_at`` -> ``zk_transform_points``), no batch in memory.  The reference's quirks are reproduced as they
are: the method ``KeyPoints.clear_border`` bounds y by the image WIDTH (``_keypoint.py:80-84``), a window that would start left
of / above the frame comes back empty or short from NumPy's slicing and makes the batch ragged (border clearing prevents it).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

__all__ = ["disk_patch", "center_of_mass_refine", "refine_points", "com_refine", "com_refine_points", "gaussian_fit_points",
           "GaussianFit", "clear_border", "KeyPoints"]


def _interior_mask(pts, x_limit, y_limit, size):
    """Which rows of ``pts`` (x, y) lie strictly more than ``size // 2 + 1`` away from 0 and from the given limits: the one
    statement of the border rule (``_keypoint.py:46-50``)."""
    margin = size // 2 + 1
    xy = np.asarray(pts)
    return (xy[:, 0] > margin) & (xy[:, 0] < x_limit - margin) & (xy[:, 1] > margin) & (xy[:, 1] < y_limit - margin)


def _interior(pts, x_limit, y_limit, size):
    """Rows of ``pts`` (x, y) strictly more than ``size // 2 + 1`` away from 0 and from the given limits."""
    return pts[_interior_mask(pts, x_limit, y_limit, size)]


def clear_border(pts, shape, size):
    """Points farther than ``size // 2 + 1`` from every border of an image of ``shape`` (``_keypoint.py:46-50``)."""
    return _interior(pts, shape[1], shape[0], size)


def _frame_and_points(img, pts, who):
    """``img`` as a 2-D float32 / float64 frame and ``pts`` as real, finite ``(N, 2)`` points with ``N < 2^24``, or the
    ``ValueError`` of ``who``."""
    img, pts = np.asarray(img), np.asarray(pts)
    if img.ndim != 2 or img.dtype not in (np.float32, np.float64):
        raise ValueError(f"{who} needs a 2-D float32 or float64 frame, not {img.ndim}-D {img.dtype}")
    if pts.size == 0:
        pts = pts.reshape(0, 2).astype(np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "iuf":
        raise ValueError(f"{who} needs real points of shape (N, 2), not {pts.dtype} {pts.shape}")
    if pts.dtype.kind == "f" and not np.isfinite(pts).all():
        raise ValueError(f"{who} needs finite points")
    if len(pts) >= 2 ** 24:
        raise ValueError(f"{who} needs len(pts) < 2^24")
    return img, pts


def _window_corners(pts, size, shape, who):
    """The int32 ``(x0, y0)`` of every point's ``size x size`` window, ``np.rint(pt).astype(int) - size // 2``; ``ValueError``
    when one leaves a frame of ``shape``."""
    first = np.rint(pts).astype(int) - size // 2
    if len(first) and (first.min() < 0 or (first[:, 0] + size > shape[1]).any() or (first[:, 1] + size > shape[0]).any()):
        raise ValueError(f"{who} needs every window inside the frame")
    return np.ascontiguousarray(first, dtype=np.int32)


def disk_patch(radius, dtype=np.uint8):
    """``(2 radius + 1)^2`` mask of the pixels within ``radius`` of the centre (``_keypoint.py:6-9``)."""
    d2 = np.add.outer(np.arange(-radius, radius + 1) ** 2, np.arange(-radius, radius + 1) ** 2)
    return (d2 <= radius ** 2).astype(dtype)


def center_of_mass_refine(data, pts, size=3, mode=None):
    """Intensity centroid of the ``(2 size + 1)^2`` box (``mode='disk'``: disk) around every integer point, rows ``(x, y)``
    (``_keypoint.py:12-23``).  As in the reference the regions are painted into ONE label image in point order -- where boxes
    overlap the later point owns the pixels (a disk also paints its box's corners with 0) -- and
    ``scipy.ndimage.center_of_mass`` reduces each label."""
    from scipy import ndimage
    stamp = disk_patch(size) if mode == 'disk' else 1
    owner = np.zeros_like(data)
    for label, (px, py) in enumerate(pts, start=1):
        owner[py - size:py + size + 1, px - size:px + size + 1] = label * stamp
    yx = np.array(ndimage.center_of_mass(data, owner, list(range(1, len(pts) + 1))))
    return yx[:, ::-1]


def refine_points(data, pts, size=3, mode=None):
    """``center_of_mass_refine(data, pts, size, mode)`` on the GPU (``zk_refine_points``): NumPy in, NumPy out, the same float64
    ``(N, 2)`` rows ``(x, y)`` bit for bit -- the last point whose box covers a pixel owns it, a disk's box corners belong to
    nobody, a point left with no pixels gives ``nan, nan``.  What the kernel does not take raises ``ValueError`` naming the
    condition, and the host function remains for those cases: ``data`` must be a 2-D float32 / float64 frame, ``pts`` integer
    ``(N, 2)`` with ``N < 2^24``, and every box must lie inside the frame (``KeyPoints`` guarantees it by border clearing)."""
    from ctypes import c_void_p
    from .. import _native
    data, pts = np.asarray(data), np.asarray(pts)
    if data.ndim != 2 or data.dtype not in (np.float32, np.float64):
        raise ValueError(f"refine_points needs a 2-D float32 or float64 frame, not {data.ndim}-D {data.dtype}")
    if pts.size == 0:
        pts = pts.reshape(0, 2).astype(np.int32)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.dtype.kind not in "iu":
        raise ValueError(f"refine_points needs integer points of shape (N, 2), not {pts.dtype} {pts.shape}")
    if len(pts) >= 2 ** 24:
        raise ValueError("refine_points needs len(pts) < 2^24 (the reference's label image has the frame's type)")
    size = int(size)
    if not 0 <= size <= 64:
        raise ValueError(f"size must be in [0, 64], not {size}")
    height, width = data.shape
    if len(pts) and not ((pts[:, 0] >= size).all() and (pts[:, 0] < width - size).all() and (pts[:, 1] >= size).all()
                         and (pts[:, 1] < height - size).all()):
        raise ValueError("refine_points needs every box inside the frame: size <= x < W - size and size <= y < H - size")
    out = np.empty((len(pts), 2), np.float64)
    if len(pts) == 0:
        return out
    data, pts = np.ascontiguousarray(data), np.ascontiguousarray(pts, dtype=np.int32)
    lib = _native.load()
    _native.require_device()
    _native.check(lib.zk_refine_points(_native.default_device(), data.ctypes.data_as(c_void_p), _native.dtype_code(data.dtype), height, width,
                                       pts.ctypes.data_as(c_void_p), len(pts), size,
                                       _native.REFINE_DISK if mode == 'disk' else _native.REFINE_BOX, out.ctypes.data_as(c_void_p)),
                  "zk_refine_points")
    return out


def com_refine(pts, img, size, threshold=None):
    """Thresholded centroid refinement of key points (``_keypoint.py:26-43``): every window is thresholded (Li by default,
    ``'otsu'``: Otsu -- scikit-image, exactly as the reference needs it) and its centroid moves the point."""
    from scipy import ndimage
    from skimage import filters
    level_of = filters.threshold_otsu if threshold == 'otsu' else filters.threshold_li
    kp = KeyPoints(pts, img, size)
    windows = kp.extract_patches(size)
    moved = np.empty((len(windows), 2))
    for k, w in enumerate(windows):
        w[w < level_of(w)] = 0
        moved[k] = np.subtract(ndimage.center_of_mass(w), size / 2)[::-1]
    return moved + kp.pts


def com_refine_points(pts, img, size, threshold=None, return_thresholds=False):
    """``com_refine(pts, img, size, threshold)`` on the GPU (``zk_com_refine``): NumPy in, NumPy out, the reference's argument
    order and rule.  The points are border-cleared by ``clear_border(pts, img.shape, size)``; the window of a kept point starts
    at ``np.rint(pt).astype(int) - size // 2`` and is ``size x size``; it is thresholded (``threshold='otsu'``: Otsu, anything
    else: Li, as in the reference), what lies below the threshold counts as zero, and the float64 ``(M, 2)`` result is
    ``(centroid_xy - size / 2) + pts_kept``.  With ``return_thresholds`` the call returns ``(points, thresholds (M) float64,
    iterations (M) int32)``: the threshold of every window and the steps Li's iteration took (0 for Otsu).

    The thresholds are defined on the window WIDENED TO FLOAT64: Otsu is the 256-bin histogram of ``np.histogram`` and the bin
    centre of the largest between-class variance, Li the iteration of ``threshold_li`` from the window's mean with half the
    smallest gap between distinct values as its tolerance.  Parity with scikit-image is unpinned, as for ``graph.estimate_d``
    (scikit-image is not installed where this package is tested); in particular scikit-image bins a float32 window in float32.
    A window of zeros gives ``nan, nan`` (0 / 0), as SciPy does.

    ``img`` must be a 2-D float32 or float64 frame and ``2 <= size <= 64``; anything else raises ``ValueError`` naming it
    (scikit-image takes another histogram route for integer frames: the host :func:`com_refine` remains for those).  Empty
    ``pts`` returns a ``(0, 2)`` array without touching the device."""
    from ctypes import c_void_p
    from .. import _native
    img, pts = _frame_and_points(img, pts, "com_refine_points")
    if int(size) != size or not 2 <= int(size) <= 64:
        raise ValueError(f"size must be an integer in [2, 64], not {size}")
    size = int(size)
    kept = clear_border(pts, img.shape, size)
    moved, levels, steps = np.empty((len(kept), 2), np.float64), np.empty(len(kept), np.float64), np.empty(len(kept), np.int32)
    if len(kept):
        first = _window_corners(kept, size, img.shape, "com_refine_points")               # border clearing guarantees them
        height, width = img.shape
        img = np.ascontiguousarray(img)
        lib = _native.load()
        _native.require_device()
        _native.check(lib.zk_com_refine(_native.default_device(), img.ctypes.data_as(c_void_p), _native.dtype_code(img.dtype), height, width,
                                        first.ctypes.data_as(c_void_p), len(first), size,
                                        _native.THRESHOLD_OTSU if threshold == 'otsu' else _native.THRESHOLD_LI,
                                        moved.ctypes.data_as(c_void_p), levels.ctypes.data_as(c_void_p), steps.ctypes.data_as(c_void_p)),
                      "zk_com_refine")
    out = (moved - size / 2) + kept
    return (out, levels, steps) if return_thresholds else out


GaussianFit = namedtuple("GaussianFit", "xy amplitude sigma theta background rss iterations status kept")


def gaussian_fit_options(size, model, mode, sigma, tol, max_iter):
    """``(size, model code, mask code, sigma0, tol, max_iter)`` of a Gaussian fit, as ``zk_gauss_fit`` takes them; what it would
    refuse is a ``ValueError`` here, before any device call (shared with ``resident.gaussian_fit_device``)."""
    from .. import _native
    if isinstance(size, bool) or int(size) != size or not 3 <= int(size) <= 32:
        raise ValueError(f"size must be an integer in [3, 32], not {size}")
    size = int(size)
    if model not in _native.GAUSS_MODELS:
        raise ValueError(f"model must be 'circular' or 'elliptical', not {model!r}")
    if mode not in (None, 'disk'):
        raise ValueError(f"mode must be None or 'disk', not {mode!r}")
    if mode == 'disk' and size % 2 == 0:
        raise ValueError(f"mode='disk' needs an odd size, not {size}")
    n_params = 7 if model == "elliptical" else 5
    n_pixels = int(disk_patch(size // 2).sum()) if mode == 'disk' else size * size
    if n_pixels <= n_params:
        raise ValueError(f"the {model} model has {n_params} parameters and the window only {n_pixels} fitted pixels: "
                         "a larger size or the box is needed")
    sigma = size / 4 if sigma is None else float(sigma)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError(f"sigma must be positive and finite, not {sigma}")
    tol = float(tol)
    if not (tol >= 0 and np.isfinite(tol)):
        raise ValueError(f"tol must be finite and not negative, not {tol}")
    if isinstance(max_iter, bool) or int(max_iter) != max_iter or not 1 <= int(max_iter) <= 10000:
        raise ValueError(f"max_iter must be an integer in [1, 10000], not {max_iter}")
    return size, _native.GAUSS_MODELS[model], _native.GAUSS_DISK if mode == 'disk' else _native.GAUSS_BOX, sigma, tol, int(max_iter)


def gaussian_fit_points(pts, img, size, model="elliptical", mode=None, sigma=None, tol=1e-10, max_iter=100, clear=True):
    """Least-squares fit of a 2-D Gaussian to the ``size x size`` window of every key point, on the GPU (``zk_gauss_fit``:
    Levenberg-Marquardt, one wave a point; the algorithm is written out in ``include/zernike_hip.h``).  NumPy in, a
    :class:`GaussianFit` of NumPy arrays out: ``xy`` ``(M, 2)`` the fitted centres in frame coordinates, ``amplitude``,
    ``sigma`` ``(M, 2)`` the major and minor widths (equal for the circular model), ``theta`` the angle of the major axis in
    ``(-pi/2, pi/2]`` (0 for the circular model), ``background``, ``rss``, ``iterations`` and ``status`` (int32: 0 converged,
    1 ``max_iter`` reached, 2 the damping passed 1e12 or the window is constant, 3 a fitted pixel is NaN or inf -- then the
    parameters are NaN) and ``kept``, the indices into ``pts`` of the fitted points.

    The window convention is :func:`com_refine_points`'s: with ``clear`` the points are filtered by
    ``clear_border(pts, img.shape, size)``; the window of a kept point starts at ``np.rint(pt).astype(int) - size // 2``.
    With ``clear=False`` every window must lie inside the frame, or ``ValueError`` is raised.  The fit starts at the window's
    centre pixel (the pixel the point rounds to) with width ``sigma`` (default ``size / 4``), so it depends on the window
    alone.  ``model`` is ``'elliptical'`` (7 parameters) or ``'circular'`` (5); ``mode='disk'`` fits only the pixels of
    ``disk_patch(size // 2)`` and needs an odd ``size``.  ``img`` must be a 2-D float32 or float64 frame, ``3 <= size <= 32``,
    ``len(pts) < 2^24``; every refusal is a ``ValueError`` before the first device call, and there is no CPU fallback.  Empty
    ``pts`` returns empty arrays without touching the device."""
    from ctypes import c_void_p
    from .. import _native
    img, pts = _frame_and_points(img, pts, "gaussian_fit_points")
    size, model_code, mask_code, sigma, tol, max_iter = gaussian_fit_options(size, model, mode, sigma, tol, max_iter)
    height, width = img.shape
    kept = np.flatnonzero(_interior_mask(pts, width, height, size)) if clear else np.arange(len(pts))
    kept = kept.astype(np.int64)
    first = _window_corners(pts[kept], size, img.shape, "gaussian_fit_points")
    params, steps, status = np.empty((len(kept), 8), np.float64), np.empty(len(kept), np.int32), np.empty(len(kept), np.int32)
    if len(kept):
        img = np.ascontiguousarray(img)
        lib = _native.load()
        _native.require_device()
        _native.check(lib.zk_gauss_fit(_native.default_device(), img.ctypes.data_as(c_void_p), _native.dtype_code(img.dtype), height, width,
                                       first.ctypes.data_as(c_void_p), len(first), size, model_code, mask_code, sigma, tol, max_iter,
                                       params.ctypes.data_as(c_void_p), steps.ctypes.data_as(c_void_p), status.ctypes.data_as(c_void_p)),
                      "zk_gauss_fit")
    return GaussianFit(params[:, 0:2].copy(), params[:, 2].copy(), params[:, 3:5].copy(), params[:, 5].copy(), params[:, 6].copy(),
                       params[:, 7].copy(), steps, status, kept)


class KeyPoints:
    """Key points of an image together with a window size (``_keypoint.py:53-92``)."""

    def __init__(self, pts, img, size):
        self.img, self.size, self.shape = img, size, img.shape
        self.pts = clear_border(pts, self.shape, size)
        self.patches = None

    def extract_patches(self, size=None, flat=False):
        """The window ``img[y - s1 : y + s2, x - s1 : x + s2]`` of every rounded point, ``s1 = size // 2``, ``s2 = size - s1``
        (``_keypoint.py:62-78``); ``flat=True`` flattens each window.  Windows that lie inside the frame (what border clearing
        leaves) are gathered in one indexing step; anything else falls back to the per-point slices of the reference."""
        size = self.size if size is None else size
        first = np.rint(self.pts).astype(int) - size // 2                                  # (x, y) of every window's corner
        height, width = self.img.shape[:2]
        whole = len(first) > 0 and first.min() >= 0 and (first[:, 0] + size <= width).all() and (first[:, 1] + size <= height).all()
        if whole and self.img.ndim == 2:
            view = np.lib.stride_tricks.sliding_window_view(self.img, (size, size))
            cut = view[first[:, 1], first[:, 0]]                                             # a copy: (N, size, size)
        else:
            cut = np.array([self.img[y:y + size, x:x + size] for x, y in first])
        self.patches = cut.reshape(len(cut), -1) if flat and cut.ndim == 3 else cut
        return self.patches

    def moments(self, zps):
        """Zernike moments of the windows ``extract_patches(zps.size)`` would cut, computed on the GPU from the frame itself
        (extension; ``zps``: a :class:`mtflearn_amd.ZPs`).  Same numbers as ``zps.transform(self.extract_patches(zps.size))``."""
        return zps.transform_at(self.img, self.pts)

    def clear_border(self, size):
        """In-place border clearing for another window size; y is bounded by ``shape[1]``, as in the reference."""
        self.pts = _interior(self.pts, self.shape[1], self.shape[1], size)

    def refine(self, data=None, r=3, mode=None):
        """Replace the points by the intensity centroids around their integer parts (``center_of_mass_refine``)."""
        self.pts = center_of_mass_refine(self.img if data is None else data, self.pts.astype(int), size=r, mode=mode)

    def refine_gpu(self, data=None, r=3, mode=None):
        """:meth:`refine` on the GPU (extension, in the spirit of :meth:`moments`): the same truncation ``pts.astype(int)``, the
        same numbers (:func:`refine_points`)."""
        self.pts = refine_points(self.img if data is None else data, self.pts.astype(int), size=r, mode=mode)

    def fit_gaussians(self, size=None, **kw):
        """The :class:`GaussianFit` of the points on the image (:func:`gaussian_fit_points`, on the GPU; extension).  ``size``
        defaults to the object's; the keywords are that function's.  The object is left as it is."""
        return gaussian_fit_points(self.pts, self.img, self.size if size is None else size, **kw)
