"""Synthetic frames: the reference's ``mtflearn.datasets`` subpackage (``datasets/__init__.py``), rasterised on the GPU.

The only way to a frame without microscope data, under the reference's names, signatures, defaults, dtypes and error messages:

* ``add_tapered_gaussian``                        (``_tapered_gaussian.py``): Gaussian atoms tapered to zero at ``r_factor * sigma``;
* ``HoneyCombLattice``                            (``_honeycomb_lattice.py``): graphene-like lattice, ``get_points`` / ``to_image``;
* ``get_zps_test_image`` / ``get_zps_test_patches`` (``_zps_test_data.py``);
* ``generate_data_gn``                            (``_generate_data_gn.py``): n-fold blob patterns;
* ``apply_poisson_noise`` / ``add_gaussian_noise`` / ``apply_poisson_gaussian_noise`` / ``estimate_counts_per_pixel_mle``
  (``_noise_models.py``).

Every pixel is drawn by ``zk_render_gaussians`` (``csrc/zk_datasets.hip``): the reference's float64 expressions, one rounding
per operation, and -- because the reference adds point after point and a float32 frame rounds at every add -- every pixel's
contributions in ascending point index with that same rounding.  What differs from NumPy is the device's ``exp`` (and
``t * t * t`` for ``t ** 3``): a float64 frame agrees to ``1e-12`` of its maximum, a float32 frame to one float32 spacing per
contribution to the pixel.  Where the values make every contribution exact the result is the reference's bit for bit, and
two runs always agree bit for bit.

The lattice coordinates are made on the host as whole arrays, with the reference's operations in the reference's order and its
``default_rng(seed)`` draws in the same sequence: ``_coords_A`` / ``_coords_B`` and ``get_points()`` are the reference's numbers.

The noise models are host code: the draw is NumPy's (``Generator.poisson`` / ``Generator.normal``) and is the whole cost, so
there is nothing for the device to do that would still give the reference's noise for a seed.

Deviations from the reference:

* points must be finite (the reference fails on ``int(nan)``), ``r_factor`` must be positive, and ``img`` must be float32 or
  float64;
* the pixels of a point's box outside its disc, to which the reference adds ``0.0``, are left alone (a ``-0.0`` there stays).

Left out: ``TMDImageSimulator`` and ``PerovskitesImageSimulator`` (another renderer: a delta image and a convolution), the
lattice-constant tables, and ``generate_two_blobs``.  :mod:`mtflearn_amd.synthetic` is the project's own older host generator
and stays as it is.

There is no CPU fallback: without a HIP device the rendering functions raise ``RuntimeError``.  Frames that should stay on the
GPU come from ``render_gaussians_device`` / ``honeycomb_image_device`` of :mod:`mtflearn_amd.resident`.
"""
from __future__ import annotations

from ctypes import c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _device, _native

__all__ = [
    "add_tapered_gaussian",
    "HoneyCombLattice",
    "get_zps_test_image",
    "get_zps_test_patches",
    "generate_data_gn",
    "apply_poisson_noise",
    "add_gaussian_noise",
    "apply_poisson_gaussian_noise",
    "estimate_counts_per_pixel_mle",
]


# ----------------------------------------------------------------------------------------------- the device side
def _ptr(array):
    return array.ctypes.data_as(c_void_p) if array is not None and array.size else None


def _render_args(pts, amps, shape, sigma, r_factor, taper, offsets, list_budget):
    """The arguments of ``zk_render_gaussians`` after the frame: ``shape`` is ``(H, W)`` or ``(B, H, W)``."""
    batch = 1 if len(shape) == 2 else int(shape[0])
    h, w = (int(v) for v in shape[-2:])
    return (h, w, batch, _ptr(pts), _ptr(amps), _ptr(offsets), len(pts), float(sigma), float(r_factor), int(bool(taper)),
            int(list_budget))


def _render_host(frame, pts, amps, sigma, r_factor, taper, offsets=None, list_budget=0):
    """``zk_render_gaussians`` on a C-contiguous float32 / float64 host array ``(H, W)`` or ``(B, H, W)``, in place."""
    lib = _native.load()
    _native.require_device()
    code = _native.ZK_F32 if frame.dtype == np.float32 else _native.ZK_F64
    _native.check(lib.zk_render_gaussians(_native.default_device(), frame.ctypes.data_as(c_void_p), code,
                                          *_render_args(pts, amps, frame.shape, sigma, r_factor, taper, offsets, list_budget)),
                  "zk_render_gaussians")


def _render_device(frame, pts, amps, sigma, r_factor, taper, offsets=None, list_budget=0):
    """``zk_render_gaussians_dev`` on a resident float32 / float64 frame (a DeviceArray or a torch tensor), in place."""
    _native.check(_native.load().zk_render_gaussians_dev(
        frame.device.index, c_void_p(frame.data_ptr()), _device.code(frame, _device.FLOATS),
        *_render_args(pts, amps, tuple(frame.shape), sigma, r_factor, taper, offsets, list_budget),
        c_void_p(_device.stream_ptr(frame))), "zk_render_gaussians_dev")


def _points_and_amplitudes(ndim, pts, sigma, amplitude, r_factor):
    """The reference's argument checks, in its order and words; ``(N, 2)`` float64 points and ``(N,)`` float64 amplitudes."""
    if ndim != 2:
        raise ValueError("img must be a 2D array")
    pts = np.ascontiguousarray(np.asarray(pts, dtype=float))
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError("pts must have shape (N, 2)")
    amps = np.asarray(amplitude, dtype=float)
    if amps.ndim == 0:
        amps = np.full(len(pts), float(amps), dtype=float)
    elif amps.shape[0] != len(pts):
        raise ValueError("If amplitude is array-like, its length must match number of points")
    if sigma <= 0:
        raise ValueError("sigma must be positive")
    if amps.ndim != 1:
        raise ValueError("If amplitude is array-like, its length must match number of points")
    if not r_factor > 0:
        raise ValueError("r_factor must be positive")
    if not np.isfinite(pts).all():
        raise ValueError("cannot convert float NaN or infinity to integer: pts must be finite")
    return pts, np.ascontiguousarray(amps)


def add_tapered_gaussian(img, pts, sigma, amplitude=1, r_factor=3.0, *, list_budget=0):
    """
    Add tapered 2D Gaussians to an image at given point locations.

    Parameters
    ----------
    img : 2D np.ndarray (float32 or float64)
        Target image. This array is modified in-place and also returned.
    pts : np.ndarray, shape (N, 2)
        Floating-point centres, ``pts[i] = (x, y)`` in pixel coordinates (col, row).  Centres may lie outside the image; they
        contribute as far as their support overlaps it.
    sigma : float
        Standard deviation of the (isotropic) Gaussian in pixels.
    amplitude : float or array-like
        Peak amplitude, one for all points or one per point.
    r_factor : float, optional
        The Gaussian is tapered to zero at ``r = r_factor * sigma``.
    list_budget : int, keyword only, not in the reference
        Most point-list entries the device builds at once (0: the library's default); past it the points are rendered in
        consecutive index ranges.  No result depends on it.

    Returns
    -------
    img : the modified image (the same object).
    """
    img_ndim = getattr(img, "ndim", None)
    pts, amps = _points_and_amplitudes(img_ndim, pts, sigma, amplitude, r_factor)
    if img.dtype not in (np.float32, np.float64):
        raise TypeError(f"img must be float32 or float64, not {img.dtype}")
    if img.size == 0 or len(pts) == 0:
        return img
    if img.flags.c_contiguous and img.flags.writeable:
        _render_host(img, pts, amps, sigma, r_factor, True, list_budget=list_budget)
    else:
        work = np.ascontiguousarray(img)
        _render_host(work, pts, amps, sigma, r_factor, True, list_budget=list_budget)
        img[...] = work
    return img


def _render_uncut(shape, dtype, points, amplitudes, counts, sigma):
    """``len(counts)`` zero frames of ``shape``, frame ``b`` with its own ``counts[b]`` uncut Gaussians, in one launch."""
    frames = np.zeros((len(counts),) + tuple(shape), dtype=dtype)
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 2))
    amps = np.ascontiguousarray(amplitudes, dtype=np.float64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if frames.size and len(pts):
        _render_host(frames, pts, amps, sigma, 0.0, False, offsets=offsets)
    return frames


# ----------------------------------------------------------------------------------------------- the honeycomb lattice
class HoneyCombLattice:
    """
    Graphene-like 2D honeycomb lattice in a square simulation box.

    Parameters
    ----------
    size : int
        Width and height of the simulation box (pixels).
    l : float, optional
        Nearest-neighbour bond length (default 12.0 pixels).
    a : float, optional
        Lattice constant of the 2D hexagonal Bravais lattice, ``sqrt(3) * l`` for ideal graphene; checked against ``l`` when
        given.
    angle : float
        Rotation of the lattice in degrees (counter-clockwise).
    random_shift : bool
        Shift the lattice origin by a random vector within one primitive cell.
    seed : int or None
        Seed of the shift and the jitter.
    jitter : float
        Standard deviation (pixels) of independent Gaussian noise on every site position (0.0: none).
    """

    def __init__(
            self,
            size: int = 512,
            l: float = 12.0,
            a: Optional[float] = None,
            angle: float = 0.0,
            random_shift: bool = True,
            seed: Optional[int] = None,
            jitter: float = 0.0,
    ):
        self.size = int(size)
        self.l = float(l)

        inferred_a = self.l * np.sqrt(3.0)
        if a is not None:
            a = float(a)
            if not np.isclose(a, inferred_a, rtol=1e-5, atol=1e-6):
                raise ValueError(
                    f"Inconsistent 'a' and 'l': got a={a}, l={self.l}, "
                    f"but for ideal graphene expect a≈sqrt(3)*l≈{inferred_a:.6f}."
                )
            self.a = a
        else:
            self.a = inferred_a

        self.angle_deg = float(angle)
        self.angle = np.deg2rad(self.angle_deg)

        # primitive vectors and the two-site basis, unrotated
        self.a1 = np.array([1.5 * self.l, np.sqrt(3.0) * self.l / 2.0], dtype=np.float64)
        self.a2 = np.array([1.5 * self.l, -np.sqrt(3.0) * self.l / 2.0], dtype=np.float64)
        self.dA = np.array([0.0, 0.0], dtype=np.float64)
        self.dB = np.array([self.l, 0.0], dtype=np.float64)

        self.rng = np.random.default_rng(seed)
        self.random_shift = random_shift
        if random_shift:
            self.shift_u1, self.shift_u2 = self.rng.random(2)
        else:
            self.shift_u1 = 0.0
            self.shift_u2 = 0.0

        self.jitter = float(jitter)
        self.N = int(np.ceil(self.size / self.l)) + 3       # over-generate in lattice index space
        self._coords_A: Optional[np.ndarray] = None
        self._coords_B: Optional[np.ndarray] = None

    def _update_rotation(self) -> None:
        c, s = np.cos(self.angle), np.sin(self.angle)
        self.Rmat = np.array([[c, -s], [s, c]], dtype=np.float64)

    def set_angle(self, angle: float) -> None:
        """Set a new rotation angle in degrees and invalidate the cached coordinates."""
        self.angle_deg = float(angle)
        self.angle = np.deg2rad(self.angle_deg)
        self._coords_A = None
        self._coords_B = None

    def _generate_coordinates(self) -> None:
        """All site coordinates, rotated, centred and jittered: the reference's double loop over ``(n1, n2)`` as whole arrays,
        ``n1`` the slow index, every element through the same operations in the same order."""
        self._update_rotation()
        offset = self.shift_u1 * self.a1 + self.shift_u2 * self.a2
        idx = np.arange(-self.N, self.N + 1)
        n1 = np.repeat(idx, len(idx))[:, None]
        n2 = np.tile(idx, len(idx))[:, None]
        R = n1 * self.a1 + n2 * self.a2
        coords_A = np.ascontiguousarray(R + self.dA + offset, dtype=np.float64)
        coords_B = np.ascontiguousarray(R + self.dB + offset, dtype=np.float64)

        coords_A = coords_A @ self.Rmat.T
        coords_B = coords_B @ self.Rmat.T

        box_center = np.array([self.size / 2.0, self.size / 2.0], dtype=np.float64)
        coords_A += box_center
        coords_B += box_center

        if self.jitter > 0.0:
            coords_A += self.rng.normal(0.0, self.jitter, coords_A.shape)
            coords_B += self.rng.normal(0.0, self.jitter, coords_B.shape)

        self._coords_A = coords_A
        self._coords_B = coords_B

    def get_points(self) -> Tuple[np.ndarray, np.ndarray]:
        """The A and B sublattice coordinates inside ``[0, size)``: ``(N_A, 2)`` and ``(N_B, 2)``."""
        if self._coords_A is None or self._coords_B is None:
            self._generate_coordinates()
        L = self.size

        def inside(c):
            return c[(c[:, 0] >= 0.0) & (c[:, 0] < L) & (c[:, 1] >= 0.0) & (c[:, 1] < L)]

        return inside(self._coords_A), inside(self._coords_B)

    def _render_lists(self, sigma, intensity_A, intensity_B):
        """``(sigma, points, amplitudes)`` of ``to_image``: the A sites, then the B sites, whose centre is within
        ``ceil(3 sigma)`` of the box (the reference's ``in_range``)."""
        if self._coords_A is None or self._coords_B is None:
            self._generate_coordinates()
        if sigma is None:
            sigma = self.l / 4.0
        radius = int(np.ceil(3 * sigma))

        def in_range(coords):
            if coords.size == 0:
                return coords
            mask = (
                    (coords[:, 0] >= -radius) & (coords[:, 0] <= self.size - 1 + radius) &
                    (coords[:, 1] >= -radius) & (coords[:, 1] <= self.size - 1 + radius)
            )
            return coords[mask]

        pts_a, pts_b = in_range(self._coords_A), in_range(self._coords_B)
        # the reference's two calls check their arguments one after the other; one launch draws both, A before B
        pts_a, amp_a = _points_and_amplitudes(2, pts_a, sigma, intensity_A, 3.0)
        pts_b, amp_b = _points_and_amplitudes(2, pts_b, sigma, intensity_B, 3.0)
        return sigma, np.concatenate([pts_a, pts_b]), np.concatenate([amp_a, amp_b])

    def to_image(
            self,
            sigma: Optional[float] = None,
            intensity_A: float = 1.0,
            intensity_B: float = 0.5,
            normalize: bool = False,
    ) -> np.ndarray:
        """
        Rasterise the lattice into a float32 ``(size, size)`` image of tapered Gaussian atoms, sites outside the box whose
        Gaussians reach into it included.

        sigma : Gaussian standard deviation in pixels (``None``: ``l / 4``).
        intensity_A, intensity_B : amplitudes of the two sublattices.
        normalize : divide the image by its maximum.
        """
        from .resident import honeycomb_image_device
        return honeycomb_image_device(self, sigma=sigma, intensity_A=intensity_A, intensity_B=intensity_B,
                                      normalize=normalize).numpy()


# ----------------------------------------------------------------------------------------------- test data
def get_zps_test_image():
    lattice = HoneyCombLattice(size=512, l=12)
    img = lattice.to_image()
    return img


def get_zps_test_patches(size=64, n_fold=3, num_patches=10, include_center=True, relative_center_intensity=1):
    """
    Gaussian blob patches with ``n_fold`` rotational symmetry, each at another orientation.

    size : patch size in pixels; n_fold : blobs on the circle; num_patches : orientations over the full turn;
    include_center : add a blob at the centre, ``relative_center_intensity`` times the others.

    Returns the ``(num_patches, size, size)`` float32 patches, each divided by its maximum.  The whole stack is one launch.
    """
    center = size / 2
    sigma = size / 10
    angles = np.linspace(0, 2 * np.pi, num_patches, endpoint=False)
    if len(angles) == 0:
        return np.array([])
    points, amplitudes = [], []
    for rotation_angle in angles:
        if include_center:
            points.append((center, center))
            amplitudes.append(relative_center_intensity)
        sector_angle = 2 * np.pi / n_fold if n_fold else 0.0
        radius = size / 3
        for fold in range(n_fold):
            angle = fold * sector_angle + rotation_angle
            points.append((center + radius * np.cos(angle), center + radius * np.sin(angle)))
            amplitudes.append(1.0)
    per_patch = int(bool(include_center)) + max(int(n_fold), 0)
    patches = _render_uncut((size, size), np.float32, points, amplitudes, [per_patch] * len(angles), sigma)
    return np.array([patch / patch.max() for patch in patches])


def generate_data_gn(size, n=6, sigma=None, include_center=True, radius_frac=0.25, rotation_angle=0.0):
    """
    A ``size x size`` float64 image of ``n`` Gaussian blobs on a circle of radius ``size * radius_frac``, rotated by
    ``rotation_angle`` degrees, with an optional blob at the centre; ``sigma`` defaults to ``size / 24``.  Values in [0, 1].
    """
    if sigma is None:
        sigma = size / 24.0
    rot_rad = np.deg2rad(rotation_angle)
    center = size / 2.0
    radius = size * radius_frac
    base_angles = np.linspace(0, 2 * np.pi, n, endpoint=False)
    angles = base_angles + rot_rad
    points = [(center + radius * np.cos(theta), center + radius * np.sin(theta)) for theta in angles]
    if include_center:
        points.append((center, center))
    img = _render_uncut((size, size), np.float64, points, np.ones(len(points)), [len(points)], sigma)[0]
    img /= img.max()
    return img


# ----------------------------------------------------------------------------------------------- noise models (host)
def apply_poisson_noise(img, counts_per_pixel, return_counts=False, seed=None):
    """
    Poisson (shot) noise on a normalised image: intensity 1.0 stands for ``counts_per_pixel`` expected counts.

    Returns the noisy float32 image in [0, 1] (and the raw counts with ``return_counts``).  Host code: the cost is NumPy's
    ``Generator.poisson`` draw, which is what makes a seed give the reference's noise.
    """
    img = np.asarray(img, dtype=np.float32)
    if counts_per_pixel <= 0:
        raise ValueError("counts_per_pixel must be positive.")
    rng = np.random.default_rng(seed)
    noisy_counts = rng.poisson(img * counts_per_pixel).astype(np.float32)
    noisy_img = noisy_counts / counts_per_pixel
    if return_counts:
        return noisy_img, noisy_counts
    return noisy_img


def add_gaussian_noise(img, sigma=0.1, seed=None):
    """Zero-mean Gaussian noise of standard deviation ``sigma`` added to a float32 copy of ``img``.  Host code: the cost is
    NumPy's ``Generator.normal`` draw."""
    img = np.asarray(img, dtype=np.float32)
    if sigma < 0:
        raise ValueError("sigma must be non-negative.")
    rng = np.random.default_rng(seed)
    noise = rng.normal(0.0, sigma, size=img.shape).astype(np.float32)
    return img + noise


def apply_poisson_gaussian_noise(img, counts_per_pixel, sigma, seed=None):
    """
    Poisson (shot) plus Gaussian (readout) noise: ``k ~ Poisson(counts_per_pixel * img)``,
    ``y = k / counts_per_pixel + N(0, sigma)``.  Host code: the two NumPy draws, Poisson first, are the cost.
    """
    img = np.asarray(img, dtype=np.float32)
    if counts_per_pixel <= 0:
        raise ValueError("counts_per_pixel must be positive.")
    if sigma < 0:
        raise ValueError("sigma must be non-negative.")
    rng = np.random.default_rng(seed)
    noisy_counts = rng.poisson(img * counts_per_pixel).astype(np.float32)
    poisson_part = noisy_counts / counts_per_pixel
    gaussian_part = rng.normal(0.0, sigma, size=img.shape).astype(np.float32)
    return poisson_part + gaussian_part


def estimate_counts_per_pixel_mle(noisy_img, clean_img, mask=None, s_min=1e-3):
    """
    Estimate ``counts_per_pixel`` from a noisy image and its clean template, with a Gaussian approximation of the Poisson
    likelihood, over the pixels where ``clean_img >= s_min`` (and ``mask``, if given).
    """
    noisy = np.asarray(noisy_img, dtype=np.float64)
    clean = np.asarray(clean_img, dtype=np.float64)
    if noisy.shape != clean.shape:
        raise ValueError("noisy_img and clean_img must have same shape.")
    valid = clean >= s_min
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != noisy.shape:
            raise ValueError("mask must match image shape.")
        valid &= mask
    noisy = noisy[valid]
    clean = clean[valid]
    if noisy.size == 0:
        raise ValueError("No valid pixels to fit counts_per_pixel.")
    residual = noisy - clean
    A = (residual**2) / clean
    sum_A = A.sum()
    if sum_A <= 0:
        return np.inf
    return A.size / sum_A
