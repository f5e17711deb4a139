"""Inputs of the refinement and bond-length tests, regenerated from seeds (NumPy only: the GPU tests import this file).

``refine_cases()`` maps a name to ``(data (H, W) float32 / float64, pts int32 (N, 2) of (x, y), size, mode)``; each case is named
for what it exercises in csrc/zk_refine.hip.  ``point_sets()`` maps a name to float64 ``(N, 2)`` points for the neighbour
distances and the thresholds; ``LI_SETS`` are the jittered ones Li's iteration is pinned on (on a perfect lattice the gaps
between distinct distances are rounding noise and the published loop need not end).  The key points of the 512^2 frame are
detected on the CPU by tests/make_golden_refine.py and stored in the golden file; ``frame_512()`` regenerates the frame.
The point sets here are near-uniform; tests/point_cases.py has the ones that reach the edges of the neighbour search."""
import functools

import numpy as np

import vnn_cases as vc

MODES = (None, "disk")


def frame(height, width, dtype, seed):
    """Positive, smooth-ish data: a few Gaussian bumps on a noisy floor."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width]
    img = 0.1 * rng.random((height, width))
    for cx, cy in rng.uniform(0, 1, (40, 2)) * [width, height]:
        img += np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / 18.0)
    return img.astype(dtype)


def random_points(n, height, width, size, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(size, width - size, n), rng.integers(size, height - size, n)], axis=1).astype(np.int32)


def frame_512():
    from mtflearn_amd.synthetic import honeycomb_frame
    return honeycomb_frame(512, seed=5)


@functools.lru_cache(maxsize=None)
def refine_cases():
    f32, f64 = frame(64, 80, np.float32, 1), frame(96, 64, np.float64, 2)
    big32, big64 = frame(160, 128, np.float32, 3), frame(128, 160, np.float64, 4)
    signed = (frame(72, 64, np.float64, 5) - 0.4)                       # negative values, sums of either sign
    zero = frame(64, 64, np.float32, 6)
    zero[17:24, 17:24] = 0.0                                            # a box of zeros: 0 / 0 in both coordinates
    zero[37:44, 17:24] = 0.0
    zero[37:44, 17] = 1.0                                               # sum 0, column sum not: -inf in x, 0 / 0 in y
    zero[37:44, 23] = -1.0
    grid = np.array([(x, y) for y in range(8, 90, 16) for x in range(8, 60, 16)], dtype=np.int32)
    out = {}
    for mode in MODES:
        m = "disk" if mode else "box"
        out[f"one_point_{m}"] = (f32, np.array([[30, 20]], np.int32), 3, mode)
        out[f"isolated_{m}"] = (f64, grid, 3, mode)
        out[f"isolated_size1_{m}"] = (f32, np.array([[5, 5], [20, 9], [70, 50]], np.int32), 1, mode)
        out[f"isolated_size6_{m}"] = (f64, grid[::2], 6, mode)
        out[f"overlap_one_column_ab_{m}"] = (f32, np.array([[20, 30], [26, 30]], np.int32), 3, mode)
        out[f"overlap_one_column_ba_{m}"] = (f32, np.array([[26, 30], [20, 30]], np.int32), 3, mode)
        out[f"swallowed_by_four_later_{m}"] = (f64, np.array([[40, 40], [39, 39], [41, 39], [39, 41], [41, 41]], np.int32), 1, mode)
        out[f"duplicate_{m}"] = (f32, np.array([[12, 14], [40, 40], [12, 14], [50, 20]], np.int32), 3, mode)
        out[f"every_edge_{m}"] = (f64, np.array([[3, 40], [60, 50], [30, 3], [20, 92], [3, 3], [60, 92]], np.int32), 3, mode)
        out[f"every_edge_size6_{m}"] = (f32, np.array([[6, 30], [73, 30], [40, 6], [40, 57]], np.int32), 6, mode)
        out[f"negative_data_{m}"] = (signed, random_points(40, 72, 64, 3, 7), 3, mode)
        out[f"zero_sums_{m}"] = (zero, np.array([[20, 20], [20, 40], [50, 50]], np.int32), 3, mode)
        for n in (1, 63, 64, 65):
            out[f"n{n}_{m}"] = (big32 if n % 2 else big64, random_points(n, 128, 128, 3, 10 + n), 3, mode)
        out[f"n3000_{m}"] = (big32, random_points(3000, 160, 128, 3, 20), 3, mode)
        out[f"n3000_size6_{m}"] = (big64, random_points(3000, 128, 160, 6, 21), 6, mode)
    # a later box corner removes a pixel of an earlier disk: (30, 30) is the centre of the first disk and a corner of the second box
    out["disk_corner_removes_earlier_pixel"] = (f32, np.array([[30, 30], [33, 33]], np.int32), 3, "disk")
    out["disk_corner_removes_earlier_pixel_size6"] = (f64, np.array([[30, 30], [36, 36], [25, 36]], np.int32), 6, "disk")
    for data, pts, _, _ in out.values():
        data.setflags(write=False)
        pts.setflags(write=False)
    return out


REFINE_NAMES = tuple(refine_cases())


@functools.lru_cache(maxsize=None)
def point_sets():
    rng = np.random.default_rng(40)
    scattered = vc.scattered(50, 41)
    cluster = np.concatenate([vc.square_patch(6, 6, 1.0, 0.05, 42), [[205.0, 3.0]]])
    out = {
        "n12": vc.scattered(12, 43),
        "n13": vc.scattered(13, 44),
        "collinear_40": np.stack([np.arange(40.0), np.zeros(40)], axis=1),
        "duplicates": np.concatenate([scattered, scattered[5:15], scattered[7:8]]),
        "cluster_and_outlier": cluster,
        "honeycomb_257": vc.honeycomb(12, 12, 0.04, 45)[:257],
        "honeycomb_5k": vc.honeycomb(50, 50, 0.04, 46),
        "scattered_300": rng.uniform(0.0, 17.0, (300, 2)),
    }
    for pts in out.values():
        pts.setflags(write=False)
    return out


POINT_SET_NAMES = tuple(point_sets())
LI_SETS = ("honeycomb_257", "honeycomb_5k", "scattered_300")
