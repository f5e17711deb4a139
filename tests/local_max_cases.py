"""Inputs of tests/test_gpu_local_max_kernels.py, built once: frames for the wide halos and the LDS crossover of the tiled
suppression kernel, the frame-clipped halos, priority chains across tile borders and the value edges of the ordering keys.
tests/test_local_max_cpu.py runs the smallest member of every family through both checkers of tests/local_max_oracle.py."""
import numpy as np

from local_max_oracle import plateaus
from mtflearn_amd.synthetic import honeycomb_frame

FRAME = (96, 160)                     # 6 tile rows by 3 tile columns of 16 x 64, the last column ragged at 32 px
WIDE_RADII = (9, 16, 17, 24.5, 30, 31)
CROSSOVER_RADII = (31, 31.4, 31.9, 32)
CHAIN_SHAPE, CHAIN_RADII = (48, 130), (2, 2.9, 17)      # 3 x 3 tiles
EDGE_SHAPE, EDGE_RADII = (40, 100), (1.5, 5)            # 3 x 2 tiles


def honey64(shape=FRAME):
    """float64 honeycomb plus noise: no two pixels equal."""
    return honeycomb_frame(*shape, seed=9).astype(np.float64) + 0.05 * np.random.default_rng(1).standard_normal(shape)


def plateaus_u8(shape=FRAME, seed=3):
    """uint8 frame full of ties; frames too small for the blobs of ``plateaus`` keep its texture and row of equal peaks."""
    if shape[0] >= 12 and shape[1] >= 12:
        return plateaus(np.uint8, shape, seed)
    img = np.random.default_rng(seed).integers(0, 6, shape) * 25
    img[shape[0] // 2, 10:40:2] = 250
    return img.astype(np.uint8)


def wide_frames():
    """(name, image, mid-range threshold) of the two frames of the wide-halo and crossover families."""
    return (("honey64", honey64(), 0.5), ("plateaus_u8", plateaus_u8(), 125))


# (name, shape, r, tiled?): the kernel the case is expected to take, asserted by the tests through tile_lds_bytes
CLIPPED = (
    ("short_wide", (20, 150), 40, True),          # Ry clipped to 19
    ("tall_narrow", (150, 20), 40, True),         # Rx clipped to 19: 60 904 B, 536 B under the limit
    ("all_in_reach", (20, 20), 1000, True),       # every offset of the frame in the disk: one point survives
    ("huge_radius", (40, 40), 1e6, False),
    ("three_rows", (3, 200), 17, True),
    ("radius_zero", FRAME, 0, True),              # n_off = 0: every candidate is kept
)


def disk_offsets(r, Rx, Ry):
    """Lattice offsets of the closed disk of radius r inside |dx| <= Rx, |dy| <= Ry, the centre excluded; counted one by one."""
    return sum(1 for dy in range(-Ry, Ry + 1) for dx in range(-Rx, Rx + 1) if (dx or dy) and dx * dx + dy * dy <= r * r)


def clipped_frames(shape, seed=5):
    return (("random_f32", np.random.default_rng(seed).random(shape, dtype=np.float32)), ("plateaus_u8", plateaus_u8(shape, seed)))


def chain_frame(pattern, shape=CHAIN_SHAPE):
    """float64 zeros with peaks on the spacing-2 lattice, every peak a candidate.  'boustrophedon': values rising along
    the path that runs right along the first lattice row, left along the next, ...; 'permutation': 1..K shuffled."""
    ys, xs = np.arange(1, shape[0] - 1, 2), np.arange(1, shape[1] - 1, 2)
    K = len(ys) * len(xs)
    if pattern == "boustrophedon":
        vals = np.arange(1, K + 1, dtype=np.float64).reshape(len(ys), len(xs))
        vals[1::2] = vals[1::2, ::-1]
    else:
        vals = np.random.default_rng(48130).permutation(K).reshape(len(ys), len(xs)) + 1.0
    img = np.zeros(shape)
    img[np.ix_(ys, xs)] = vals
    return img


def signed_zeros(dtype, shape=EDGE_SHAPE):
    """+0.0 / -0.0 in a checkerboard with a few positive peaks: below a negative threshold every zero off the peaks ties."""
    yy, xx = np.indices(shape)
    img = np.where((yy + xx) % 2 == 1, -0.0, 0.0).astype(dtype)
    assert np.signbit(img).sum() == img.size // 2
    for k, (y, x) in enumerate(((5, 7), (5, 9), (17, 62), (18, 66), (30, 64), (33, 90), (8, 40))):
        img[y, x] = 1 + k % 3
    return img


def ulp_pairs(shape=EDGE_SHAPE):
    """float64 frame at -5 with pairs of peaks one ulp apart, 3 px apart along x (beyond the 3 x 3 window, within r = 5) or
    adjacent, the larger one now first and now second in raster order.  Returns (image, [(larger xy, smaller xy, apart)])."""
    img = np.full(shape, -5.0)
    lows = [1.0, 1.0 + 2.0 ** -24, -1.0, 1e-300, 0.1, 3.0, -0.25, 65504.0, 2.0 ** -1074, -2.0 ** -1074, 7.0, 0.3]
    pairs, same32 = [], 0
    sites = [(y, x) for y in range(4, shape[0] - 4, 12) for x in range(6, shape[1] - 8, 14)]
    for k, lo in enumerate(lows):
        hi = np.nextafter(lo, np.inf)
        same32 += np.float32(lo) == np.float32(hi)
        y, x = sites[k]
        apart = 1 if k % 3 == 2 else 3
        first, second = (hi, lo) if k % 2 else (lo, hi)
        img[y, x], img[y, x + apart] = first, second
        big, small = ((x, y), (x + apart, y)) if k % 2 else ((x + apart, y), (x, y))
        pairs.append((big, small, apart))
    assert 0 < same32 < len(lows)          # pairs a float32 key cannot tell apart, and pairs it can
    return img, pairs


def infinities(dtype, shape=EDGE_SHAPE):
    """Noise with +inf pixels that tie (adjacent, within reach of each other, and far apart) and -inf pixels."""
    img = np.random.default_rng(77).standard_normal(shape).astype(dtype)
    for y, x in ((6, 10), (6, 11), (7, 13), (6, 60), (9, 63), (20, 66), (30, 30), (35, 95), (1, 1), (38, 98)):
        img[y, x] = np.inf
    for y, x in ((3, 3), (6, 12), (20, 65), (0, 50), (25, 25), (25, 26)):
        img[y, x] = -np.inf
    return img


def all_negative(dtype, shape=EDGE_SHAPE):
    rng = np.random.default_rng(78)
    if np.dtype(dtype).kind == "f":
        return (-1.0 - rng.random(shape)).astype(dtype)
    return rng.integers(-30000, 0, shape).astype(dtype)


def int16_about_zero(shape=EDGE_SHAPE):
    """int16 in -3 .. 3, for the thresholds -1, -0.5 and 0."""
    return np.random.default_rng(79).integers(-3, 4, shape).astype(np.int16)


INT16_THRESHOLDS = (-1, -0.5, 0)


def nan_frames(dtype, shape=EDGE_SHAPE):
    """{name: image} of the NaN cases."""
    rng = np.random.default_rng(80)
    base = rng.random(shape).astype(dtype)
    scattered = base.copy()
    scattered[rng.random(shape) < 0.08] = np.nan
    beside = np.full(shape, 0.25, dtype=dtype)
    beside += (0.01 * rng.random(shape)).astype(dtype)
    beside[10, 20], beside[10, 21] = 2.0, np.nan           # a NaN next to a peak
    beside[20, 70], beside[20, 71], beside[19, 70] = 1.0, np.nan, np.nan
    beside[30, 40], beside[30, 41], beside[30, 42] = 1.5, np.nan, 1.75    # a NaN between two peaks 2 px apart
    border = base.copy()
    border[0, :] = np.nan
    border[:, -1] = np.nan
    border[5:9, 0] = np.nan
    border[-1, 30] = np.nan
    constant = np.full(shape, 0.5, dtype=dtype)
    constant[::7, ::5] = np.nan
    return {"scattered": scattered, "beside_a_peak": beside, "on_the_border": border, "all_nan": np.full(shape, np.nan, dtype=dtype),
            "nan_and_constant": constant}


def cpu_families():
    """(name, image, r, threshold): the smallest member of every family above, for the two host checkers."""
    for name, img, mid in wide_frames():
        for r, t in ((WIDE_RADII[0], None), (CROSSOVER_RADII[1], mid)):
            yield f"wide_{name}", img, r, t
    for name, shape, r, _ in CLIPPED:
        for kind, img in clipped_frames(shape):
            yield f"clipped_{name}_{kind}", img, r, None
    for pattern in ("boustrophedon", "permutation"):
        for r in CHAIN_RADII:
            yield f"chain_{pattern}", chain_frame(pattern), r, None
    for r in EDGE_RADII:
        for dtype in (np.float32, np.float64):
            for t in (None, -1.0):
                yield "signed_zeros", signed_zeros(dtype), r, t
            yield "infinities", infinities(dtype), r, None
            for name, img in nan_frames(dtype).items():
                yield f"nan_{name}", img, r, None
                yield f"nan_{name}", img, r, 0.3
        yield "ulp_pairs", ulp_pairs()[0], r, None
        for dtype in (np.float32, np.int16):
            yield "all_negative", all_negative(dtype), r, None
        for t in INT16_THRESHOLDS:
            yield "int16_about_zero", int16_about_zero(), r, t
