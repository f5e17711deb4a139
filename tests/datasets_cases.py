"""Inputs of the datasets tests, regenerated identically by tests/make_golden_datasets.py (which stores only the outputs),
tests/test_datasets_cpu.py and tests/test_gpu_datasets.py.  Shapes are the smallest at which the rasteriser can go wrong:
one pixel, one row, one column, an odd frame inside one tile row, and a frame of more than two 16-pixel tiles each way with a
remainder."""
import numpy as np

DTYPES = (np.float32, np.float64)


def _frame(shape, seed):
    """A non-zero frame to accumulate into (no zeros, so no signed-zero question)."""
    return np.random.default_rng([seed, *shape]).normal(0.0, 0.3, shape) + 2.0


def render_cases():
    """name -> dict(shape, base (float64 or None for zeros), pts, amps (scalar or array), sigma, r_factor)."""
    rng = np.random.default_rng(2024)
    cases = {}
    cases["1x1"] = dict(shape=(1, 1), base=None, pts=np.array([[0.0, 0.0], [0.3, -0.4], [2.5, 1.0], [-7.25, 0.1], [40.0, 40.0]]),
                        amps=np.array([1.0, -0.5, 2.0, 3.0, 1.0]), sigma=1.0, r_factor=3.0)
    cases["1x67"] = dict(shape=(1, 67), base=_frame((1, 67), 1), pts=np.column_stack([rng.uniform(-4, 71, 12), rng.uniform(-3, 3, 12)]),
                         amps=1, sigma=1.3, r_factor=3.0)
    cases["53x1"] = dict(shape=(53, 1), base=None, pts=np.column_stack([rng.uniform(-3, 3, 12), rng.uniform(-4, 57, 12)]),
                         amps=rng.uniform(-1, 2, 12), sigma=1.1, r_factor=2.5)
    cases["37x53"] = dict(shape=(37, 53), base=_frame((37, 53), 2), pts=np.column_stack([rng.uniform(-6, 59, 40), rng.uniform(-6, 43, 40)]),
                          amps=rng.uniform(-1, 2, 40), sigma=1.7, r_factor=3.0)
    # 45 x 70: 3 x 5 tiles, remainders 13 and 6.  R = 6: points on 0 and on W - 1 + R, far outside, negative fractions, duplicates
    h, w, sigma = 45, 70, 2.0
    R = 3.0 * sigma
    special = np.array([[0.0, 0.0], [w - 1 + R, 10.0], [10.0, h - 1 + R], [w - 1 + R, h - 1 + R], [-R, 20.0], [20.0, -R],
                        [-5.75, 12.5], [-0.5, -0.25], [33.3, -5.999], [500.0, 500.0], [-300.5, 7.0], [16.0, 16.0], [16.0, 16.0],
                        [31.5, 15.5], [31.5, 15.5], [w + R + 0.5, 3.0]])
    pts = np.concatenate([special, np.column_stack([rng.uniform(-8, w + 8, 64), rng.uniform(-8, h + 8, 64)])])
    cases["tiles"] = dict(shape=(h, w), base=_frame((h, w), 3), pts=pts, amps=rng.uniform(-1, 2, len(pts)), sigma=sigma, r_factor=3.0)
    cases["tiles_zero"] = dict(shape=(h, w), base=None, pts=pts, amps=0.75, sigma=sigma, r_factor=3.0)
    # R = 0.6: a point reaches its own pixel at the most
    cases["small_R"] = dict(shape=(37, 53), base=None, pts=np.concatenate([[[5.0, 7.0], [5.4, 7.3], [5.5, 7.5], [52.0, 36.0], [0.0, 36.4]],
                                                                            np.column_stack([rng.uniform(0, 53, 30), rng.uniform(0, 37, 30)])]),
                            amps=1.5, sigma=0.2, r_factor=3.0)
    # R = 40: two and a half tiles
    cases["big_R"] = dict(shape=(h, w), base=None, pts=np.column_stack([rng.uniform(-30, w + 30, 9), rng.uniform(-30, h + 30, 9)]),
                          amps=rng.uniform(0.5, 2, 9), sigma=8.0, r_factor=5.0)
    # 5000 points inside one 8 x 8 region: lists far longer than any staging in on-chip memory
    cases["dense"] = dict(shape=(40, 40), base=None, pts=np.column_stack([rng.uniform(14, 22, 5000), rng.uniform(14, 22, 5000)]),
                          amps=rng.uniform(-1, 1, 5000), sigma=1.0, r_factor=3.0)
    return cases


def case_frame(case, dtype):
    return np.zeros(case["shape"], dtype) if case["base"] is None else case["base"].astype(dtype)


ORDER_AMPLITUDES = {"big_one_minus": (1e8, 1.0, -1e8), "big_minus_one": (1e8, -1e8, 1.0)}


def order_case(amplitudes):
    """Three points on one pixel centre of a float32 frame: there r = 0, Gaussian and taper are exactly 1, and the value
    depends on the order of the adds alone."""
    return dict(shape=(11, 13), base=None, pts=np.array([[6.0, 5.0]] * 3), amps=np.array(amplitudes), sigma=1.0, r_factor=3.0)


LATTICES = {
    "plain": (dict(size=96, l=12, seed=0, angle=17), dict()),
    "normalized": (dict(size=96, l=12, seed=0, angle=17), dict(normalize=True)),
    "jitter": (dict(size=96, l=12, seed=0, angle=17, jitter=0.5), dict()),
}
PATCHES = {"32_3_4": dict(size=32, n_fold=3, num_patches=4),
           "21_5_3": dict(size=21, n_fold=5, num_patches=3, include_center=True, relative_center_intensity=0.5),
           "16_2_1": dict(size=16, n_fold=2, num_patches=1, include_center=False)}
DATA_GN = {"33_6_10": dict(size=33, n=6, rotation_angle=10), "20_3": dict(size=20, n=3, sigma=2.5, include_center=False, radius_frac=0.3)}

# ground truth: a lattice whose sites local_max must find (parameters confirmed on the CPU by make_golden_datasets.py)
TRUTH = dict(lattice=dict(size=192, l=12, seed=5, angle=7), min_distance=5)


def uncut_batch_case(batch):
    """``batch`` float64 frames of 19 x 23 with their own point ranges (one of them empty when batch > 1)."""
    rng = np.random.default_rng(batch)
    counts = [4] if batch == 1 else [3, 0, 5][:batch]
    n = sum(counts)
    return dict(shape=(batch, 19, 23), base=_frame((batch, 19, 23), 7 + batch), counts=counts, sigma=2.2,
                pts=np.column_stack([rng.uniform(-3, 26, n), rng.uniform(-3, 22, n)]), amps=rng.uniform(-1, 2, n))


def noise_image():
    return (np.random.default_rng(11).random((24, 31)) * 0.9 + 0.05).astype(np.float32)
