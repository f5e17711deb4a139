"""Synthetic frames: the reference's ``mtflearn.datasets`` subpackage (``datasets/__init__.py``), rasterised on the GPU.

The only way to a frame without microscope data, under the reference's names, signatures, defaults, dtypes and error messages:

* ``add_tapered_gaussian``                        (``_tapered_gaussian.py``): Gaussian atoms tapered to zero at ``r_factor * sigma``;
* ``HoneyCombLattice``                            (``_honeycomb_lattice.py``): graphene-like lattice, ``get_points`` / ``to_image``;
* ``get_zps_test_image`` / ``get_zps_test_patches`` (``_zps_test_data.py``);
* ``generate_data_gn``                            (``_generate_data_gn.py``): n-fold blob patterns;
* ``apply_poisson_noise`` / ``add_gaussian_noise`` / ``apply_poisson_gaussian_noise`` / ``estimate_counts_per_pixel_mle``
  (``_noise_models.py``);
* ``TMDImageSimulator``                           (``_tmd_simulator.py``): a rotated two-species lattice with labelled single and
  double vacancies and dopants; per species a delta image and a blur (see below).

Every pixel of the first four is drawn by ``zk_render_gaussians`` (``csrc/zk_datasets.hip``): the reference's float64
expressions, one rounding per operation, and -- because the reference adds point after point and a float32 frame rounds at every add -- every pixel's
contributions in ascending point index with that same rounding.  What differs from NumPy is the device's ``exp`` (and
``t * t * t`` for ``t ** 3``): a float64 frame agrees to ``1e-12`` of its maximum, a float32 frame to one float32 spacing per
contribution to the pixel.  Where the values make every contribution exact the result is the reference's bit for bit, and
two runs always agree bit for bit.

The lattice coordinates are made on the host as whole arrays, with the reference's operations in the reference's order and its
``default_rng(seed)`` draws in the same sequence: ``_coords_A`` / ``_coords_B`` and ``get_points()`` are the reference's numbers.

The noise models are host code: the draw is NumPy's (``Generator.poisson`` / ``Generator.normal``) and is the whole cost, so
there is nothing for the device to do that would still give the reference's noise for a seed.

``TMDImageSimulator.simulate`` is ``zk_tmd_render`` (``csrc/zk_tmd.hip``).  The delta image of a species is NumPy's
``np.add.at`` -- several atoms on one pixel are added in ascending index with a float32 rounding per add -- and is the
reference's bit for bit.  With ``use_fft=False`` the blur is ``scipy.ndimage.gaussian_filter`` restated operation by operation
(axis 0 then axis 1 in float64, each pass stored as float32, ``A *`` and the sum over species in float32): the reference's
frame bit for bit for up to two species.  With ``use_fft=True`` it is the exact separable convolution the reference's
``fftconvolve`` approximates in single precision, each species added as ``float32(float64(total) + blurred)``: half a float32
spacing per species from the exact sum, where the reference is about ``1.5e-7`` of the peak away from it.  Its lattice, labels
and defect draws are host code and the reference's numbers, bit for bit and in its order.

Deviations from the reference:

* points must be finite (the reference fails on ``int(nan)``), ``r_factor`` must be positive, and ``img`` must be float32 or
  float64;
* the pixels of a point's box outside its disc, to which the reference adds ``0.0``, are left alone (a ``-0.0`` there stays);
* ``TMDImageSimulator`` adds its species in order of first appearance in ``basis``; the reference walks a ``set``, whose order
  changes from process to process (the same frame for up to two species, not for three);
* ``TMDImageSimulator.simulate`` takes a keyword-only ``consistent_defects=False``: the reference uses a stored global site
  index as an index into the species' own array, so the image dims another atom than the labels mark; ``True`` dims the
  labelled one.  The default is the reference's behaviour;
* ``TMDImageSimulator`` needs finite positions, ``species_params`` convertible with ``float()``, and kernels of radius 960 at
  the most (``sigma`` up to 240 with ``use_fft=False``, 320 with ``use_fft=True``); ``matplotlib`` is imported by ``plot`` only.

Left out: ``PerovskitesImageSimulator`` (an empty constructor in the reference), the lattice-constant tables, and
``generate_two_blobs``.  :mod:`mtflearn_amd.synthetic` is the project's own older host generator
and stays as it is.

There is no CPU fallback: without a HIP device the rendering functions raise ``RuntimeError``.  Frames that should stay on the
GPU come from ``render_gaussians_device`` / ``honeycomb_image_device`` / ``tmd_frames_device`` of :mod:`mtflearn_amd.resident`.
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
    "TMDImageSimulator",
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


# ----------------------------------------------------------------------------------------------- labelled defect frames
def _tmd_render_args(layers, batch, shape, blur, use_fft):
    """The arguments of ``zk_tmd_render`` after the two buffers, and the arrays they point into (to be kept alive by the
    caller).  ``layers``: ``(frame, points (n, 3) float64 of (x, y, scale), amplitude, half kernel)`` in frame order."""
    h, w = (int(v) for v in shape)
    frame_of = np.ascontiguousarray([layer[0] for layer in layers], dtype=np.int32)
    points = np.ascontiguousarray(np.concatenate([layer[1] for layer in layers]) if layers else np.zeros((0, 3)), dtype=np.float64)
    point_offsets = np.concatenate([[0], np.cumsum([len(layer[1]) for layer in layers])]).astype(np.int64)
    keep = [frame_of, points, point_offsets]
    if blur:
        amps = np.ascontiguousarray([layer[2] for layer in layers], dtype=np.float64)
        weights = np.ascontiguousarray(np.concatenate([layer[3] for layer in layers]), dtype=np.float64)
        weight_offsets = np.concatenate([[0], np.cumsum([len(layer[3]) for layer in layers])]).astype(np.int64)
        keep += [amps, weights, weight_offsets]
        tail = (_ptr(amps), _ptr(weight_offsets), _ptr(weights))
    else:
        tail = (None, None, None)
    args = (_native.ZK_F32, int(batch), h, w, len(layers), _ptr(frame_of), _ptr(point_offsets), _ptr(points), *tail,
            _native.TMD_FFT if use_fft else _native.TMD_GAUSSIAN)
    return args, keep


def _tmd_render_host(frames, masks, layers, blur, use_fft):
    """``zk_tmd_render`` into C-contiguous float32 host arrays: ``frames`` ``(B, H, W)`` (None without blur) and ``masks``
    ``(len(layers), H, W)`` (or None)."""
    lib = _native.load()
    _native.require_device()
    shape = (frames if frames is not None else masks).shape
    batch = shape[0] if frames is not None else max(layer[0] for layer in layers) + 1
    args, keep = _tmd_render_args(layers, batch, shape[-2:], blur, use_fft)
    _native.check(lib.zk_tmd_render(_native.default_device(), _ptr(frames), _ptr(masks), *args), "zk_tmd_render")
    del keep


def _tmd_render_device(frames, masks, layers, blur, use_fft):
    """``zk_tmd_render_dev`` into resident float32 arrays (DeviceArrays or torch tensors) of the same shapes."""
    first = frames if frames is not None else masks
    batch = frames.shape[0] if frames is not None else max(layer[0] for layer in layers) + 1
    args, keep = _tmd_render_args(layers, batch, tuple(first.shape)[-2:], blur, use_fft)
    dev_ptr = lambda a: None if a is None else c_void_p(a.data_ptr())
    _native.check(_native.load().zk_tmd_render_dev(first.device.index, dev_ptr(frames), dev_ptr(masks), *args,
                                                   c_void_p(_device.stream_ptr(first))), "zk_tmd_render_dev")
    del keep


def _on_frame(points, shape):
    """The rows of ``(n, 3)`` points whose pixel ``(rint(y), rint(x))`` is on the ``(H, W)`` frame, in order: the device drops
    the others by the same predicate, so leaving them on the host changes no pixel."""
    h, w = shape
    x, y = np.rint(points[:, 0]), np.rint(points[:, 1])
    return points[(x >= 0) & (x < w) & (y >= 0) & (y < h)]


class TMDImageSimulator:
    """
    Atomic-resolution frames of a transition-metal dichalcogenide monolayer with labelled point defects: the reference's
    ``TMDImageSimulator`` (``_tmd_simulator.py``), its constructor, attributes and methods.

    Parameters
    ----------
    size : (height, width) of the frame in pixels.
    a : lattice constant in pixels.
    theta : rotation of the lattice in degrees.
    species_params : ``{label: {'sigma': ..., 'A': ...}}``, the Gaussian of each species (a species without an entry gets
        ``sigma = 2.0, A = 1.0``).
    basis : ``[(dx, dy, label), ...]`` in fractions of the primitive vectors.
    use_fft : ``True``: every species' delta image is convolved with a ``int(6 sigma) | 1`` square Gaussian window, zeros
        outside the frame (the reference's ``fftconvolve``); ``False``: ``A * scipy.ndimage.gaussian_filter(delta, sigma)``.

    The lattice, the labels and the defect draws are host code and the reference's numbers; ``simulate`` renders on the GPU
    (:func:`mtflearn_amd.resident.tmd_frames_device` renders many simulators in one call and leaves the stack there).
    """

    def __init__(self, size=(512, 512), a=30, theta=0.0, species_params=None, basis=None, use_fft=True):
        self.size = size
        self.a = a
        self.theta = theta
        self.use_fft = use_fft
        self.species_params = species_params or {'TM': {'sigma': 2.0, 'A': 1.0}, 'X': {'sigma': 1.5, 'A': 0.6}}
        self.basis = basis or [(0.0, 0.0, 'TM'), (1 / 3, 1 / 3, 'X')]
        self.vacancies = []
        self.dopants = []
        self._cached_coords = None
        self.pts_all = None
        self.pts = None
        self.labels = None
        self.lbs = None
        self.filtered_indices = {}

    def rotation_matrix(self):
        theta = np.deg2rad(self.theta)
        return np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])

    def _species(self):
        """The species in order of first appearance in ``basis`` (the reference walks an unordered set)."""
        return list(dict.fromkeys(b[2] for b in self.basis))

    def generate_lattice(self):
        """All sites, rotated: the reference's loops over ``(i, j)`` and the basis as whole arrays, ``i`` the slow index and
        the basis entry the fastest, every element through the same operations in the same order.  Sets ``pts_all``, ``pts``,
        ``labels``, ``lbs``, ``filtered_indices`` and returns ``{label: (n, 2) coordinates}``."""
        self.defect_label_map = {}
        a1 = self.a * np.array([1, 0])
        a2 = self.a * np.array([0.5, np.sqrt(3) / 2])
        R = self.rotation_matrix()
        height, width = self.size
        nx = int(width // self.a * 2) + 4
        ny = int(height // (self.a * np.sqrt(3) / 2) * 2) + 4

        i = np.repeat(np.arange(-nx, nx), 2 * ny)[:, None]
        j = np.tile(np.arange(-ny, ny), 2 * nx)[:, None]
        base = i * a1 + j * a2
        d1 = np.array([dx * a1 for dx, _, _ in self.basis], dtype=np.float64)
        d2 = np.array([dy * a2 for _, dy, _ in self.basis], dtype=np.float64)
        pos = ((base[:, None, :] + d1[None]) + d2[None]).reshape(-1, 2)
        # the one whole-array form found equal, bit for bit, to the reference's `R @ pos` per site
        self.pts_all = np.ascontiguousarray(np.matmul(R, pos[:, :, None])[:, :, 0])

        site_labels = np.tile(np.array([b[2] for b in self.basis]), len(base))
        species = self._species()
        index_of = {label: np.flatnonzero(site_labels == label) for label in species}
        coords = {label: self.pts_all[index_of[label]] for label in species}
        self._cached_coords = coords
        self._index_of = index_of

        mask = ((self.pts_all[:, 0] >= 0) & (self.pts_all[:, 0] < width) &
                (self.pts_all[:, 1] >= 0) & (self.pts_all[:, 1] < height))
        self.pts = self.pts_all[mask]

        defect_labels = site_labels.copy()              # its string width is the longest species label's, as the reference's
        for vac_label, vac_idx, scale in self.vacancies:
            if scale == 0.5:
                defect_labels[vac_idx] = 'v1'
            elif scale == 0.0:
                defect_labels[vac_idx] = 'v2'
        for dop_label, dop_idx, dop_scale in self.dopants:
            defect_labels[dop_idx] = 'D'
        self.labels = defect_labels[mask]
        _, inverse = np.unique(defect_labels, return_inverse=True)
        self.lbs = inverse.reshape(-1)[mask].astype(int)

        for label in species:
            idx = index_of[label]
            self.filtered_indices[label] = idx[mask[idx]].tolist()
        return coords

    def add_single_vacancy(self, label='X', index=None):
        if index is not None:
            self.vacancies.append((label, index, 0.5))

    def add_double_vacancy(self, label='X', indices=None):
        if indices is not None and len(indices) >= 1:
            self.vacancies.append((label, indices[0], 0.0))

    def add_random_vacancies(self, label='X', num_single=0, num_double=0, seed=None):
        if self._cached_coords is None:
            self.generate_lattice()
        indices = self.filtered_indices.get(label, [])
        if len(indices) == 0:
            return
        rng = np.random.default_rng(seed)
        rng.shuffle(indices)                            # the list held in filtered_indices, in place
        selected = 0
        for _ in range(num_single):
            if selected >= len(indices):
                break
            self.add_single_vacancy(label, indices[selected])
            selected += 1
        for _ in range(num_double):
            if selected >= len(indices):
                break
            self.add_double_vacancy(label, [indices[selected]])
            selected += 1

    def add_random_dopants(self, label='TM', num_dopants=0, dopant_intensity=0.8, seed=None):
        if self._cached_coords is None:
            self.generate_lattice()
        indices = self.filtered_indices.get(label, [])
        if len(indices) == 0:
            return
        rng = np.random.default_rng(seed)
        dopant_indices = rng.choice(indices, size=min(num_dopants, len(indices)), replace=False)
        for idx in dopant_indices:
            self.dopants.append((label, idx, dopant_intensity))

    def place_atoms_delta(self, positions, scales):
        """The float32 delta image of ``size``: ``scales[k]`` added at the rounded ``positions[k] = (x, y)``, in ascending
        ``k``; on the GPU, through the renderer's entry point without a blur."""
        positions = np.asarray(positions, dtype=np.float64).reshape(-1, 2)
        scales = np.asarray(scales).astype(np.float32).astype(np.float64).reshape(-1)
        points = np.column_stack([positions, scales[:len(positions)]])
        if not np.isfinite(points).all():
            raise ValueError("positions and scales must be finite")
        h, w = (int(v) for v in self.size)
        img = np.zeros((1, h, w), dtype=np.float32)
        if img.size:
            _tmd_render_host(None, img, [(0, _on_frame(points, (h, w)), 0.0, None)], False, True)
        return img[0]

    def gaussian_kernel(self, size, sigma, A):
        r = np.arange(-size // 2 + 1, size // 2 + 1)
        X, Y = np.meshgrid(r, r)
        return A * np.exp(-(X ** 2 + Y ** 2) / (2 * sigma ** 2))

    def _scales(self, label, n_atoms, consistent_defects):
        """The float32 scales of a species' atoms.  The reference uses a stored *global* site index as an index into the
        species' own array; ``consistent_defects`` maps it to the site's place in that array instead."""
        scales = np.ones(n_atoms, dtype=np.float32)
        own = self._index_of[label]

        def place(index):
            if not consistent_defects:
                return index
            at = int(np.searchsorted(own, index))
            return at if at < len(own) and own[at] == index else -1

        for vac_label, vac_idx, scale in self.vacancies:
            if vac_label == label:
                at = place(vac_idx)
                if 0 <= at < n_atoms:
                    scales[at] = scale
        for dop_label, dop_idx, dop_scale in self.dopants:
            if dop_label == label:
                at = place(dop_idx)
                if 0 <= at < n_atoms:
                    scales[at] = dop_scale
        return scales

    def _layers(self, consistent_defects=False):
        """``generate_lattice`` and then, per species in order of first appearance, ``(label, points (n, 3) of (x, y, scale)
        on the frame, A, half kernel w[0..r])``."""
        from .background import _gaussian_weights
        coords = self.generate_lattice()
        shape = tuple(int(v) for v in self.size)
        layers = []
        for label, atoms in coords.items():
            scales = self._scales(label, len(atoms), consistent_defects)
            p = self.species_params.get(label, {'sigma': 2.0, 'A': 1.0})
            sigma = float(p['sigma'])
            if self.use_fft:
                radius = (int(6 * p['sigma']) | 1) // 2
                weights = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2 * sigma ** 2))
            else:
                weights = _gaussian_weights(sigma)
            points = _on_frame(np.column_stack([atoms, scales.astype(np.float64)]), shape)
            layers.append((label, points, float(p['A']), weights))
        return layers

    def simulate(self, return_masks=False, *, consistent_defects=False):
        """The float32 ``size`` frame (and, with ``return_masks``, ``{label: delta image}``), rendered on the GPU.

        ``consistent_defects`` (keyword only, not in the reference): the reference dims the atom whose place in its species'
        array equals the stored global site index -- another atom than the one the labels mark, often one off the frame.
        ``True`` dims the labelled atom; the default is the reference's behaviour."""
        from .resident import tmd_frames_device
        out = tmd_frames_device([self], return_masks=return_masks, consistent_defects=consistent_defects)
        if return_masks:
            frames, masks = out
            masks = masks.numpy()[0]
            return frames.numpy()[0], {label: masks[k] for k, label in enumerate(self._species())}
        return out.numpy()[0]

    def plot(self, img):
        import matplotlib.pyplot as plt
        plt.figure(figsize=(6, 6))
        plt.imshow(img, cmap='gray')
        plt.title("Simulated Atomic-Resolution TMD Image")
        plt.axis('off')
        plt.show()

    def get_defect_counts(self):
        if self.labels is None:
            raise ValueError("Run simulate() first to generate labels.")
        unique, counts = np.unique(self.labels, return_counts=True)
        return dict(zip(unique, counts))

    def save(self, img, path):
        np.save(path, img)


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
