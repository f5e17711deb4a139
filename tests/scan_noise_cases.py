"""Shared inputs, the case table and the tolerances of the scan-noise tests (tests/test_scan_noise_cpu.py,
tests/test_gpu_scan_noise.py, tests/make_golden_scan_noise.py).

Frames are seeded and regenerated, never stored per test: integer counts in [256, 4096) as float64, so the float32 and uint16
casts of a case hold exactly the same numbers, and no sample is near zero -- the float32 criterion below is relative to the
result, which presumes a result that is not the remainder of a cancellation.

Shapes.  The golden shapes (2, 19, 23) and (1, 5, 7) are the reference's own outputs.  The oracle shapes are the smallest at
which a kernel can go wrong: (1, 1, 1), (1, 1, 9), (1, 9, 1) are one lane and lines of one sample (every fold collapses);
(2, 2, 3) the shortest line with a mirror period; (3, 5, 7) is below any tile; (2, 33, 65) puts one element past a wave and
past a 32-sample warm-up; (2, 64, 130) has more than two waves in a row, more than two 56-column prefilter tiles and a
partial one, and a full 64-row tile.

Tolerances, derived and not measured (``tolerance`` below):

* order 0: equality -- one sample is copied;
* order 1, float64: ``1e-14 max|frame|`` -- four products of weights formed from one subtraction each, about 45 ulp;
* order 3, float64: ``1e-12 max|frame|`` -- the prefilter's l-infinity gain is 3 per axis, 9 overall, followed by 16 taps;
* float32 output: one float32 ulp of the oracle's value elementwise, ``np.spacing(|ref|)`` -- both sides round a float64
  result once.
"""
import numpy as np

MODES = ("reflect", "mirror", "nearest", "grid-wrap", "grid-constant", "constant")
CUBIC_MODES = ("reflect", "mirror", "grid-wrap")
PAIRS = [(order, mode) for order in (0, 1) for mode in MODES] + [(3, mode) for mode in CUBIC_MODES]       # every supported pair
GOLDEN_PAIRS = [p for p in PAIRS if p != (3, "reflect")]      # the reference's 3-D call is not the interpolant there
GOLDEN_SHAPES = [(2, 19, 23), (1, 5, 7)]
GOLDEN_JITTERS = [(1, 0), (2.5, 1.5), (60, 60)]
ORACLE_SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 2, 3), (3, 5, 7), (2, 33, 65), (2, 64, 130)]
BIG = (2, 64, 130)
BIG_JITTERS = [(jx, jy) for jx in (0, 0.3, 2.5) for jy in (0, 0.3, 2.5)] + [(60, 60)]
SMALL_JITTERS = [(0.3, 2.5), (60, 60)]                         # 60 folds several times at widths 1 to 9
DTYPES = (np.float64, np.float32)


def shape_id(shape):
    return "x".join(str(v) for v in shape)


def pair_id(pair):
    return f"o{pair[0]}-{pair[1]}"


def images(shape):
    """The float64 stack of a table shape: integer counts in [256, 4096)."""
    z, h, w = shape
    rng = np.random.default_rng(7919 * z + 31 * h + w)
    return rng.integers(256, 4096, size=shape).astype(np.float64)


def seed_of(shape, k):
    """Seed of jitter ``k`` of a shape."""
    return 100 * (shape[0] + shape[1] + shape[2]) + k


def golden_cases():
    """``(shape, dtype, order, mode, k)`` of every recorded output."""
    return [(shape, dtype, order, mode, k) for shape in GOLDEN_SHAPES for dtype in DTYPES for order, mode in GOLDEN_PAIRS
            for k in range(len(GOLDEN_JITTERS))]


def golden_output(golden, shape, dtype, order, mode, k):
    """The reference's output of a case out of the loaded golden file (tests/make_golden_scan_noise.py lays it out)."""
    return golden[f"{shape_id(shape)}/{np.dtype(dtype).name}"][GOLDEN_PAIRS.index((order, mode)), k]


def distance(got, ref, order, scale):
    """``(measured, bound, unit)`` of a result against the oracle's, both of the result dtype; passes when measured <= bound."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if order == 0:
        return float(np.count_nonzero(got != ref)), 0.0, "unequal samples"
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if got.dtype == np.float32:
        return float((err / np.spacing(np.abs(ref)).astype(np.float64)).max()), 1.0, "float32 ulp of the oracle"
    return float(err.max() / scale), (1e-14 if order == 1 else 1e-12), "max|frame|"
