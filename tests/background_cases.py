"""Case tables of tests/test_gpu_background_kernels.py: the shapes, radii and planted pixels at which the kernels of
csrc/zk_background.hip take another path, and the frames that go with them.  Data only; nothing here touches the device."""
import numpy as np

# the rolling ball's tile (RB_TW, RB_TH of csrc/zk_background.hip): a workgroup owns 16 rows x 256 columns, a wave 4 rows, a lane
# 4 outputs 64 columns apart; the staged row is 256 + 2 R wide and filled 256 columns per trip
RB_TW, RB_TH, RB_LANES = 256, 16, 64
RB_MAX_R = 1536


def frame(shape, dtype, seed=0):
    """A random frame of ``dtype``: floats in [-1, 3), int16 over +-30000, unsigned types over their whole range."""
    rng = np.random.default_rng(seed)
    x = rng.random(shape)
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return (x * 4 - 1).astype(dtype)
    if dtype == np.int16:
        return (x * 60000 - 30000).astype(dtype)
    return (x * np.iinfo(dtype).max).astype(dtype)


# ------------------------------------------------------------------------------------------------ A: rolling-ball seams
SEAM_SHAPES = [(16, 256), (15, 255), (17, 257), (33, 513), (31, 300)]
# 1: both outer chords empty; 2.5: a fractional ball; 17 > RB_TH: rows of three row tiles; 70 > 64: a chord wider than the lane
# stride; 130 > 128: the staging loop takes three trips (256 + 260 columns)
SEAM_RADII = [1, 2.5, 17, 70]
SEAM_CASES = [(shape, dtype, radius) for shape in SEAM_SHAPES for dtype in ("float64", "float32") for radius in SEAM_RADII]
SEAM_CASES += [((17, 257), "float64", 130), ((33, 513), "float64", 130)]
# the cases that also go through remove_background_device
SEAM_DEVICE_CASES = [((17, 257), "float32", 70), ((33, 513), "float64", 17), ((33, 513), "float64", 130)]

PLANTED_SHAPE, PLANTED_RADIUS, PLANTED_LEVEL, PLANTED_DEPTH = (33, 513), 17, 5000.0, 1000.0
PLANTED_ROWS = (15, 16)                                 # either side of the row-tile seam
PLANTED_COLS = (0, 63, 64, 255, 256, 512)               # the frame's edges, the lane-stride seam, the tile seam
# the column on the other side of the seam a planted column sits at (the frame's edge columns: their inner neighbour)
PLANTED_ACROSS = {0: 1, 63: 64, 64: 63, 255: 256, 256: 255, 512: 511}


def planted_frame(pixels, dtype=np.float64):
    out = np.full(PLANTED_SHAPE, PLANTED_LEVEL, dtype=dtype)
    for y, x in pixels:
        out[y, x] = PLANTED_LEVEL - PLANTED_DEPTH
    return out


# ------------------------------------------------------------------------------------------------ B: radius limits
CAP_SHAPE = (8, 300)
CAP_RADII = [1536, 1535.5]
# the largest difference the table holds between two pixels of the frame, r - sqrt(r^2 - 299^2) = 29.4 at the cap; the frame
# spans about 100 times that, so a far low pixel beats every near one
CAP_SCALE = 100 * (RB_MAX_R - np.sqrt(RB_MAX_R ** 2 - (CAP_SHAPE[1] - 1) ** 2))
CAP_PLANTED_AT = (2, 3)
REFUSED_RADII = [1536.5, float("nan"), float("inf")]
TINY_RADII = [0.5, 1e-3]


# ------------------------------------------------------------------------------------------------ C: non-finite pixels
NONFINITE_SHAPE, NONFINITE_RADIUS = (40, 70), 6
# the -inf pixel and the output that has it at offset (6, 3): off the ball (45 > 36) but inside the chord (half-width 5) of
# output row 7, which the same wave (rows 4 .. 7) walks in the same sweep
MINUS_INF_AT, OFF_BALL_OUTPUT, ON_BALL_OUTPUT = (10, 13), (4, 10), (7, 10)
PLUS_INF_AT, NAN_AT = (5, 60), (30, 10)
NAN_PATCH = (slice(22, 35), slice(40, 53))              # 13 x 13: the whole ball of its centre
NAN_PATCH_CENTRE = (28, 46)


def rolling_ball_nonfinite_frame(dtype):
    img = frame(NONFINITE_SHAPE, dtype, seed=31)
    img[MINUS_INF_AT] = -np.inf
    img[PLUS_INF_AT] = np.inf
    img[NAN_AT] = np.nan
    img[NAN_PATCH] = np.nan
    return img


OPENING_INF_SHAPE = (23, 37)
OPENING_INF_SIZES = [(3, 3), (4, 7)]
OPENING_INF_BLOCK = (slice(3, 9), slice(24, 33))        # +inf wider than either window: some of it survives the erosion
# corners, edges, interior
OPENING_INF_PIXELS = [((0, 0), np.inf), ((0, 36), -np.inf), ((22, 0), -np.inf), ((22, 36), np.inf), ((0, 17), np.inf),
                      ((11, 0), -np.inf), ((22, 20), -np.inf), ((9, 36), np.inf), ((10, 15), np.inf), ((14, 22), -np.inf),
                      ((15, 22), np.inf)]


def opening_inf_frame(dtype):
    img = frame(OPENING_INF_SHAPE, dtype, seed=32)
    for at, value in OPENING_INF_PIXELS:
        img[at] = value
    img[OPENING_INF_BLOCK] = np.inf
    return img


BASELINE_NONFINITE_SHAPE = (24, 31)
BASELINE_NONFINITE_SIGMAS = [3, (0, 5), 0]
BASELINE_NONFINITE_ITERS = [1, 3]
BASELINE_NONFINITE_PIXELS = {
    "plus_inf": [((3, 4), np.inf)],
    "minus_inf": [((20, 27), -np.inf)],
    "nan": [((12, 15), np.nan)],
    "together": [((3, 4), np.inf), ((5, 9), -np.inf), ((12, 15), np.nan), ((0, 0), np.nan), ((23, 30), -np.inf), ((23, 2), np.inf)],
}


def baseline_nonfinite_frame(kind):
    img = frame(BASELINE_NONFINITE_SHAPE, np.float64, seed=33)
    for at, value in BASELINE_NONFINITE_PIXELS[kind]:
        img[at] = value
    return img


# ------------------------------------------------------------------------------------------------ D: long axes
# (name, method, parameter, shape, dtype, long axis, rows of it per block of the launch that puts it on grid.y): each needs
# 65,537 blocks there.  gauss_kernel: 4 rows per block; vh_column_kernel: 4 segments of k = 2 rows (on the transposed copy for
# the columns); transpose_kernel: 64 rows; rolling_ball_kernel: 16 rows.
GRID_Y_BLOCKS = 65537
LONG_AXIS_CASES = [
    ("baseline_rows", "baseline", 0.5, (262145, 1), "float64", 0, 4),
    ("opening_rows", "opening", 2, (524290, 1), "float64", 0, 8),
    ("opening_columns", "opening", 2, (1, 524290), "float32", 1, 8),
    ("opening_transpose", "opening", (1, 2), (4194305, 1), "uint8", 0, 64),
    ("rolling_ball_rows", "rolling_ball", 1, (1048577, 1), "uint8", 0, 16),
]

# ------------------------------------------------------------------------------------------------ E: residual second sweep
RESIDUAL_THREADS = 2048 * 256                           # residual_kernel's grid: larger frames take a second sweep
RESIDUAL_SHAPE = (725, 724)                             # 524,900 pixels
RESIDUAL_DTYPES = ["uint16", "int16", "float32"]


def residual_frame(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.int16:                               # both ends of the range: image - background wraps
        return (np.random.default_rng(34).random(RESIDUAL_SHAPE) * 65535 - 32768).astype(np.int16)
    return frame(RESIDUAL_SHAPE, dtype, seed=34)


# ------------------------------------------------------------------------------------------------ F: baseline blocks and folds
# 64 columns per block: one block exactly, one column more, three blocks; a radius (80) beyond the 70 columns / rows folds twice
BASELINE_BLOCK_CASES = [((5, 64), 3), ((5, 65), 3), ((9, 130), 3), ((3, 70), 20), ((70, 3), 20), ((70, 3), 3)]

# ------------------------------------------------------------------------------------------------ G: opening segments
OPENING_SEGMENT_SHAPES = [(130, 67), (40, 131)]
OPENING_SEGMENT_SIZES = [(8, 5), (5, 4), (40, 1)]       # 40 divides 40; 5 divides 130 and 40; 8 divides 40
# a window of n - 1 .. 2 n + 1 along an axis of n pixels (2 n and more cover a whole period of the reflected line), n odd and even
OPENING_FOLD_LENGTHS = [33, 40]


def fold_windows(n):
    return [n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1]
