"""Shared inputs of the alignment-map tests (tests/test_align_maps_cpu.py, tests/test_gpu_align_maps.py): the planted frame of
the end-to-end tests, its NumPy moments and the margins both files assert.

The frame: 96 x 96 float64, zero but for five 24 x 24 patches of ``generate_data_gn`` (tests/golden/align_maps_golden.npz, drawn by
the reference's generator, tests/make_golden_align_maps.py): four three-fold motifs at known centres, each rotated by a known
angle, and one four-fold motif.  A patch stamped at rows ``cy - 12 .. cy + 11`` is exactly the window the dense transform takes at
``(cy, cx)`` (window rows ``i - ea .. i + eb`` with ``eb = (size - 1) // 2 = 11``, ``ea = size - 1 - eb = 12``).  Templates: the
moments of the UNROTATED three-fold patch (template 0) and of the four-fold patch (template 1).

The search: ``m_select=(0, 3, 6)`` with ``symmetry=3`` (the pairing tests/align_cases.py documents for a three-fold f).  The
generator rotates the blob centres about the pixel coordinate ``size / 2 = 12`` while the basis is centred on 11.5, and the blobs
(sigma = 1 px) are sampled on the pixel grid: a rotated patch's moments are the rotated template's only up to that sampling.  The
half-pixel offset lands in the moments next to the three-fold ones (|m| = 1, 2, 4, 5, 7, 8); with all moments selected the NumPy
statement itself misses the planted angles by up to a degree and one of them altogether, with the three-fold moments alone by
less than 0.01 degree.

ANGLE_MARGIN is one step of the default search grid, ``(360 / 3) / 360 = 1 / 3`` degree: the resolution the grid promises before
any refinement, which no sampling error of this frame may eat up.  tests/test_align_maps_cpu.py establishes that the NumPy
statement of tests/align_cases.py stays inside it on this frame; the GPU test holds the kernel to the same number, and to the
statement's own angles within 1e-6 degree (the margin of test_gpu_align.py for angles).  Next to it both files assert the criterion
of ``test_gpu_align.py::test_end_to_end_three_fold_patches`` for the same generator: rotating a centre's moments by the recovered
angle never moves them away from the template, up to ``ac.score_bound``.  CENTRE_MARGIN: the cosine of the selected moments is flat
around a centre (a one-pixel shift moves it in the fourth decimal), so a peak of the cosine map counts as the planted centre when
it lies within one pixel of it in each direction -- the tolerance of the ground-truth test of tests/test_gpu_datasets.py.
"""
import os

import numpy as np

import align_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_maps_golden.npz")

SIZE, N_MAX, FRAME = 24, 8, 96
PATCHES = {                                             # name -> generate_data_gn keywords (size = SIZE)
    "three_0": dict(n=3, rotation_angle=0.0),
    "three_17": dict(n=3, rotation_angle=17.0),
    "three_49": dict(n=3, rotation_angle=49.0),
    "three_95": dict(n=3, rotation_angle=95.5),
    "three_110": dict(n=3, rotation_angle=110.0),
    "four_0": dict(n=4, rotation_angle=0.0),
}
# (patch, centre row, centre column, planted template, planted rotation in degrees)
PLANTED = (("three_17", 22, 22, 0, 17.0), ("three_49", 22, 73, 0, 49.0), ("three_95", 73, 22, 0, 95.5),
           ("three_110", 73, 73, 0, 110.0), ("four_0", 47, 47, 1, 0.0))
SYMMETRY, M_SELECT = 3, (0, 3, 6)
CENTRE_MARGIN = 1                                       # pixels, per axis
ANGLE_MARGIN = (360.0 / SYMMETRY) / 360                 # degrees; see the module docstring
COSINE_THRESHOLD, MIN_DISTANCE = 0.9, 8                 # the cosine map's peaks: local_max(cosine, 8, threshold=0.9)

_cache = {}


def patches():
    if "patches" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["patches"] = {k: z[k] for k in z.files}
    return _cache["patches"]


def frame():
    if "frame" not in _cache:
        img = np.zeros((FRAME, FRAME))
        half = SIZE // 2
        for name, cy, cx, _, _ in PLANTED:
            img[cy - half:cy + half, cx - half:cx + half] = patches()[name]
        _cache["frame"] = img
    return _cache["frame"]


def centres():
    """(rows, columns, planted template, planted angle) of the five motifs."""
    return (np.array([p[1] for p in PLANTED]), np.array([p[2] for p in PLANTED]), np.array([p[3] for p in PLANTED]),
            np.array([p[4] for p in PLANTED]))


def basis():
    """(n, m, V / area) of ZPs(N_MAX, SIZE): the package's host-built basis, what every transform sums against."""
    if "basis" not in _cache:
        from mtflearn_amd import ZPs
        z = ZPs(N_MAX, SIZE)
        _cache["basis"] = (z.n, z.m, z.polynomials / (np.pi * SIZE * SIZE / 4.0))
    return _cache["basis"]


def patch_moments(stack):
    """(N, size, size) patches -> (N, P) moments, NumPy: the sum ``ZPs.transform`` states for a batch."""
    return np.tensordot(np.asarray(stack, float), basis()[2], axes=([1, 2], [1, 2]))


def templates():
    return patch_moments(np.stack([patches()["three_0"], patches()["four_0"]]))


def dense_moments():
    """(P, H, W) moments of the frame, NumPy: at (i, k) the window of the zero-padded frame, rows i - 12 .. i + 11."""
    if "dense" not in _cache:
        _, _, table = basis()
        ea = SIZE - 1 - (SIZE - 1) // 2
        padded = np.pad(frame(), ((ea, SIZE - ea), (ea, SIZE - ea)))
        win = np.lib.stride_tricks.sliding_window_view(padded, (SIZE, SIZE))[:FRAME, :FRAME]
        _cache["dense"] = np.einsum("ikrc,jrc->jik", win, table, optimize=True)
    return _cache["dense"]


def cosine_map(score, norm2, t2):
    """max_t score_t / sqrt(norm2 |t|^2), 0 where the window holds nothing (norm2 = 0)."""
    score, norm2 = np.asarray(score), np.asarray(norm2)
    den = np.sqrt(norm2[None] * np.asarray(t2)[:, None, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, score / den, 0.0).max(axis=0)


def never_moved_away(x, t, n, m, angle):
    """The criterion of test_gpu_align.py::test_end_to_end_three_fold_patches: |rotate(x, angle) - t|^2 <= |x - t|^2 + bound."""
    moved = ((ac.rotate_numpy(x, n, m, angle) - t) ** 2).sum(axis=1)
    stayed = ((x - t) ** 2).sum(axis=1)
    bound = ac.score_bound(x, t[None], n, m, np.ones(len(n), bool))[:, 0]
    return moved, stayed, bound


def peaks_match_centres(points):
    """Every planted centre has exactly one of the (x, y) ``points`` within CENTRE_MARGIN, and there are no other points."""
    rows, cols, _, _ = centres()
    points = np.asarray(points).reshape(-1, 2)
    near = (np.abs(points[None, :, 0] - cols[:, None]) <= CENTRE_MARGIN) & (np.abs(points[None, :, 1] - rows[:, None]) <= CENTRE_MARGIN)
    return len(points) == len(rows) and (near.sum(axis=1) == 1).all()
