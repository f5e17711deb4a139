"""Inputs of the vnn_graph tests, regenerated from seeds: ``cases()`` maps a name to ``(pts float64 (N, 2), dmax, threshold)``.
Each case is named for what it exercises in csrc/zk_voronoi.hip; tests/make_golden_vnn.py asserts the conditioning of every
one (ridges, ``dmax`` and ``threshold`` margins) before it stores what SciPy's qhull gives.

``one_way`` has no threshold of its own here: the generator searches ``ONE_WAY_THRESHOLDS`` for the first one at which a pair
is kept in one direction only, asserts that there is one, and stores it in the golden file (``one_way/threshold``).
tests/point_cases.py has the sets past these: a strip, a blob in a halo, a density step, and the wheels around the vertex cap."""
import functools

import numpy as np

PAD = 0.05
CAP = 32                                             # vertices of one cell in csrc/zk_voronoi.hip
ONE_WAY_THRESHOLDS = (0.12, 0.15, 0.18, 0.2, 0.22, 0.25)


def honeycomb(nx, ny, jitter, seed):
    """``2 nx ny`` sites of a honeycomb with bond length 1, each moved by up to ``jitter`` in x and in y."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    cell = np.stack([np.sqrt(3.0) * i + np.sqrt(3.0) / 2 * j, 1.5 * j], axis=-1).reshape(-1, 2)
    pts = np.concatenate([cell, cell + [0.0, 1.0]])
    pts = pts + rng.uniform(-jitter, jitter, pts.shape)
    return pts[rng.permutation(len(pts))]


def square_patch(nx, ny, spacing, jitter, seed, origin=(0.0, 0.0)):
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pts = np.stack([i, j], axis=-1).reshape(-1, 2) * float(spacing)
    return pts + rng.uniform(-jitter, jitter, pts.shape) * spacing + np.asarray(origin, dtype=np.float64)


def wheel(spokes, seed):
    """A hub and ``spokes`` points around it at radius about 1: the hub's cell has ``spokes`` vertices."""
    rng = np.random.default_rng(seed)
    phi = 2 * np.pi * (np.arange(spokes) + rng.uniform(-0.1, 0.1, spokes)) / spokes
    rad = 1 + rng.uniform(-0.5, 0.5, spokes) / spokes ** 2      # little enough that every spoke keeps a side of the hub's cell
    return np.concatenate([[[0.0, 0.0]], np.stack([rad * np.cos(phi), rad * np.sin(phi)], axis=-1)]) + [3.0, -2.0]


def scattered(n, seed):
    return np.random.default_rng(seed).uniform(0.0, np.sqrt(n), (n, 2))


@functools.lru_cache(maxsize=None)
def cases():
    grid = square_patch(3, 3, 1.0, 0.05, 21)
    hc392 = honeycomb(14, 14, 0.04, 12)
    out = {
        "n1": (np.array([[0.25, -1.5]]), 1.5, 0.1),
        "n2": (np.array([[0.0, 0.0], [1.0, 0.125]]), 1.5, 0.1),
        "n3": (np.array([[0.0, 0.0], [1.0, 0.0625], [0.4375, 0.875]]), 1.5, 0.1),
        "collinear_5": (np.array([[0.0, 0.0], [1.0, 0.0], [2.25, 0.0], [3.0, 0.0], [4.5, 0.0]]), 1.3, 0.1),
        "grid_3x3_jittered": (grid, 1.3, 0.1),
        "n65": (scattered(65, 13), 1.6, 0.1),
        "n257": (scattered(257, 14), 1.6, 0.1),
        "wheel_24": (wheel(24, 15), 1.3, 0.1),
        "cluster_and_outlier": (np.concatenate([square_patch(6, 6, 1.0, 0.05, 16), [[205.0, 3.0]]]), 1.3, 0.1),
        "two_densities": (np.concatenate([square_patch(6, 6, 1.0, 0.05, 17), square_patch(16, 16, 0.125, 0.05, 18, origin=(6.5, 1.5))]),
                          1.3, 0.1),
        "honeycomb_392": (hc392, 1.3, 0.1),
        "honeycomb_2k": (honeycomb(32, 32, 0.04, 19), 1.3, 0.1),
        "dmax_huge": (grid, 1e6, 0.1),
        "threshold_0p3": (hc392, 1.3, 0.3),
    }
    for pts, _, _ in out.values():
        pts.setflags(write=False)
    return out


NAMES = tuple(cases())
ONE_WAY_POINTS = "n65"                               # the points of the one_way case (its dmax too)
OVER_CAP = wheel(CAP + 8, 20)                        # a hub with more spokes than a cell has vertices: an error, no golden
OVER_CAP.setflags(write=False)
