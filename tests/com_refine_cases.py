"""Inputs of the thresholded-refinement tests (``features.com_refine_points`` / ``distributed.com_refine_device``), regenerated
from seeds (NumPy only: the GPU tests import this file).

``cases()`` maps a name to ``(frame (H, W) float32 / float64, pts (N, 2) int32 or float64 of (x, y), size)``.  The window of a
point starts at ``np.rint(pt).astype(int) - size // 2`` (``corners``).  ``PARITY`` are the cases held to the golden file at the
tight bounds: the bump frames of tests/refine_cases.py with mean-filter peaks or random interior points, and the 512^2 honeycomb
frame with the key points tests/make_golden_refine.py detected on the CPU (read from its golden file); every point of them
survives ``clear_border``, so the host function and the resident one see the same points.  ``BRANCHES`` are the windows made
for one branch of csrc/zk_com_refine.hip each; they are compared at NaN positions and, where finite, at 1e-9."""
import functools
import os

import numpy as np

import refine_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
THRESHOLDS = ("li", "otsu")


def corners(pts, size):
    return (np.rint(pts).astype(int) - size // 2).astype(np.int32)


EDGE_SHAPE = (9, 12)


def edge_points(size):
    """Six int32 points of an ``EDGE_SHAPE`` frame whose ``size`` windows (2 <= size <= 5) sit at x0 = 0, x0 = W - size, y0 = 0,
    y0 = H - size and twice in the interior, and float64 points that round to them: offsets below a half, and the ties k + 0.5 at
    even k (down) and odd k (up).  Shared with tests/test_gpu_gauss_fit.py."""
    (h, w), half = EDGE_SHAPE, size // 2
    ints = np.array([(half, 4), (w - size + half, 3), (5, half), (7, h - size + half), (4, 4), (6, 4)], dtype=np.int32)
    reals = ints + np.array([(0.3, -0.4), (-0.49, 0.49), (0.49, -0.3), (-0.2, 0.0), (0.5, -0.5), (-0.5, 0.5)])   # 4.5 -> 4, 3.5 -> 4, 5.5 -> 6
    first = ints - half
    assert np.array_equal(np.rint(reals), ints) and first.min() == 0 and (first[:, 0] + size).max() == w and (first[:, 1] + size).max() == h
    return ints, reals


ONE_PIXEL_OUT = ((0, (-1, 0)), (1, (1, 0)), (2, (0, -1)), (3, (0, 1)))        # (row of edge_points, step): left, right, top, bottom


def windows(frame, pts, size):
    """The float64 windows the kernel works on, ``(N, size, size)``."""
    return np.array([frame[y:y + size, x:x + size].astype(np.float64) for x, y in corners(pts, size)]).reshape(len(pts), size, size)


def cleared(pts, shape, size):
    from mtflearn_amd.features.keypoints import clear_border
    return np.ascontiguousarray(clear_border(pts, shape, size))


def mean_filter_peaks(frame, size):
    """Local maxima (7 x 7) of the 5 x 5 mean of the frame, as int32 (x, y), border-cleared for ``size``."""
    view = np.lib.stride_tricks.sliding_window_view
    smooth = view(frame.astype(np.float64), (5, 5)).mean(axis=(2, 3))                    # smooth[r, c] is centred on (r + 2, c + 2)
    top = view(smooth, (7, 7)).max(axis=(2, 3))
    rows, cols = np.nonzero(smooth[3:-3, 3:-3] == top)
    return cleared(np.stack([cols + 5, rows + 5], axis=1).astype(np.int32), frame.shape, size)


def interior_points(n, shape, size, seed, subpixel=False):
    margin = size // 2 + 2
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.integers(margin, shape[1] - margin, n), rng.integers(margin, shape[0] - margin, n)], axis=1)
    if not subpixel:
        return pts.astype(np.int32)
    return pts + rng.uniform(-0.45, 0.45, (n, 2))


def keypoints_512():
    with np.load(os.path.join(HERE, "golden", "refine_golden.npz")) as f:
        return f["keypoints_512/pts"]


@functools.lru_cache(maxsize=None)
def _build():
    f32, f64 = rc.frame(64, 80, np.float32, 1), rc.frame(96, 64, np.float64, 2)
    big32, big64 = rc.frame(160, 128, np.float32, 3), rc.frame(128, 160, np.float64, 4)
    out = {}
    # the bump frames: one wave per window up to size 16, four waves from 17 on; 64 is the largest window (the LDS tile past 64 KiB)
    for size in (2, 3, 7, 8, 16, 17):
        out[f"bumps_f32_peaks_size{size}"] = (big32, mean_filter_peaks(big32, size), size)
        out[f"bumps_f64_random_size{size}"] = (f64, interior_points(40, f64.shape, size, 30 + size, subpixel=size % 2 == 1), size)
    out["bumps_f32_size64"] = (big32, interior_points(5, big32.shape, 64, 31), 64)
    out["bumps_f64_size64"] = (big64, interior_points(5, big64.shape, 64, 32, subpixel=True), 64)
    for n in (1, 63, 64, 65):
        out[f"n{n}"] = (f32 if n % 2 else big64, interior_points(n, (64, 80) if n % 2 else (128, 160), 7, 40 + n), 7)
    frame, pts = rc.frame_512(), keypoints_512()
    jitter = np.random.default_rng(50).uniform(-0.45, 0.45, pts.shape)
    wide = frame.astype(np.float64)
    for size in (5, 8, 9, 13, 24):                                                        # some 1300 points at size 9, every fourth elsewhere
        some = slice(0, 1300) if size == 9 else slice(None, None, 4)
        out[f"honeycomb_512_size{size}"] = (wide, cleared((pts + jitter if size in (8, 13) else pts)[some], frame.shape, size), size)
    out["honeycomb_512_f32_size9"] = (frame.astype(np.float32), cleared(pts[::4], frame.shape, 9), 9)
    out["honeycomb_512_f32_size24"] = (frame.astype(np.float32), cleared((pts + jitter)[1::4], frame.shape, 24), 24)
    parity = tuple(out)

    # one branch each
    made = rc.frame(64, 64, np.float64, 6)
    made[4:12, 4:12] = 0.25                                                               # a constant window: its value is the threshold
    made[20:29, 4:13] = 0.0                                                               # a window of zeros: 0 / 0
    made[36:44, 4:12] = 0.0
    made[39, 9] = 3.0                                                                     # one bright pixel on a zero floor: mean_back == 0
    made[4:13, 30:39] = 0.5
    made[6:9, 33:37] = 2.0                                                                # two distinct values
    for name, size, point in (("constant_window", 8, (8, 8)), ("window_of_zeros", 9, (8, 24)), ("one_bright_pixel", 8, (8, 40)),
                              ("two_values", 9, (34, 8))):
        out[name] = (made, np.array([point], np.int32), size)
    made32 = made.astype(np.float32)
    out["branches_f32_size24"] = (made32, np.array([[14, 14], [30, 30], [40, 20]], np.int32), 24)      # the same windows' surroundings, four waves
    signed = rc.frame(72, 64, np.float64, 5) - 0.4
    out["negative_data"] = (signed, interior_points(40, signed.shape, 7, 7), 7)
    out["negative_data_size24"] = (signed.astype(np.float32), interior_points(12, signed.shape, 24, 8, subpixel=True), 24)
    # windows that touch each edge of the frame (clear_border would drop them: they go to the entry points that take any window)
    h, w = f64.shape
    out["every_edge_size7"] = (f64, np.array([[3, 40], [w - 4, 50], [30, 3], [20, h - 4], [3, 3], [w - 4, h - 4]], np.int32), 7)
    out["every_edge_size8"] = (f32, np.array([[4, 30], [76, 30], [40, 4], [40, 60], [4, 4], [76, 60]], np.float64) + 0.25, 8)
    out["every_edge_size24"] = (f64, np.array([[12, 40], [w - 12, 50], [30, 12], [20, h - 12]], np.int32), 24)
    out["duplicated_points"] = (f32, np.array([[12, 14], [40, 40], [12, 14], [50, 20], [40, 40]], np.int32), 9)
    for data, pts, _ in out.values():
        data.setflags(write=False)
        pts.setflags(write=False)
    return out, parity


def cases():
    return _build()[0]


PARITY = _build()[1]
BRANCHES = tuple(k for k in cases() if k not in PARITY)
OUTSIDE = ("bumps_f64_random_size7", np.array([[61, 40]], np.int32))   # x0 + 7 = 65 > 64: one window outside, appended to that case
