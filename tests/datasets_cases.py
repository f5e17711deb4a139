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


# ------------------------------------------------------------------------------------------------ kernel-level cases
# (tests/test_gpu_datasets_kernels.py; nothing below has a golden: the reference is tests/datasets_oracle.py)
TILE = 16                                                  # the rasteriser's tile side
SEAM_LENGTHS = (1, 2, 3, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2049)
SEAM_SHAPE = (48, 48)                                      # 3 x 3 tiles; the lists are built in the middle one, pixels 16 .. 31
PROBE_TRIPLES = {"one_last": ((1e8, -1e8, 1.0), 1.0), "one_second": ((1e8, 1.0, -1e8), 0.0)}
UNCUT_WINDOW_COUNTS = [0, 1, 255, 256, 257, 600]


def many_tiles_case(shape):
    """More than 1024 tiles, so the offset scan gives every lane two counts: ``(16, 16400)`` is 1 x 1025 tiles (lanes 0 .. 511
    full, lane 512 one tile, the rest empty), ``(33, 8200)`` is 3 x 513 = 1539 tiles (lane 769 takes the ragged last share, one
    row and eight columns are remainders).  About 60 points, R = 4.5: in tile 0, in the last tile, on the remainder columns and
    rows, either side of every tile seam next to x = 16368 / 16384 (or the frame's last two seams) and of the row seams, the
    rest scattered over the whole frame."""
    h, w = shape
    rng = np.random.default_rng([31, h, w])
    sx = [(w - 1) // TILE * TILE - TILE, (w - 1) // TILE * TILE]            # the last two column seams: 16368 and 16384
    special = [[2.25, 3.5], [0.0, 0.0], [15.5, 7.0], [w - 2.5, h - 1.25], [w - 1.0, h - 1.0], [w + 3.0, h - 2.0], [w - 6.5, 1.0]]
    for s in sx:
        special += [[s - 0.75, 5.0], [s + 0.25, 6.5], [s - 5.0, 2.0], [s + 5.5, h - 1.5], [float(s), 0.5 * h]]
    for s in range(TILE, h, TILE):                                           # row seams (the second frame only)
        special += [[100.3, s - 0.5], [101.0, float(s)], [sx[0] + 1.5, s + 0.75], [w - 3.0, s - 1.25], [7.0, s + 0.5]]
    special = np.array(special)
    n = 60 - len(special)
    pts = np.concatenate([special, np.column_stack([rng.uniform(-4, w + 4, n), rng.uniform(-4, h + 4, n)])])
    return dict(shape=shape, base=_frame(shape, 21), pts=pts, amps=rng.uniform(-1, 2, len(pts)), sigma=1.5, r_factor=3.0)


MANY_TILES_SHAPES = ((16, 16400), (33, 8200))


def seam_random_case(L):
    """``L`` points at random places of the middle tile of a 48 x 48 frame, sigma 1, R = 3, far enough inside that no box leaves
    the tile (x, y in [19, 28]): that tile's list has exactly ``L`` entries and every other list is empty."""
    rng = np.random.default_rng([41, L])
    return dict(shape=SEAM_SHAPE, base=_frame(SEAM_SHAPE, 22), pts=rng.uniform(19.0, 28.0, (L, 2)), amps=rng.uniform(-1, 2, L),
                sigma=1.0, r_factor=3.0)


def _probe_rows(L):
    """The triples' first indices ``q`` for a list of ``L`` entries: every ``q`` below ``L // 3`` while the tile has pixels for
    them, else the ones whose consecutive triple touches a window seam (a multiple of 256) and an even spread of the others."""
    T, room = L // 3, (TILE - 2) ** 2
    if T <= room:
        return np.arange(T)
    must = sorted({q for w in range(256, L, 256) for q in ((w - 2) // 3, (w - 1) // 3, w // 3) if q < T})
    rest = [q for q in np.unique(np.linspace(0, T - 1, room - len(must)).round().astype(int)) if q not in must]
    return np.array(sorted(must + rest))


def _probe_indices(L, layout, q):
    """List indices of triple ``q``; the last triple ends on the list's last entry, whatever ``L % 3`` is."""
    T = L // 3
    if layout == "consecutive":
        return (L - 3, L - 2, L - 1) if q == T - 1 else (3 * q, 3 * q + 1, 3 * q + 2)
    return (q, q + T, L - 1 if q == T - 1 else q + 2 * T)


def order_probe_case(L, layout):
    """A float32 frame whose value depends on the ORDER of a list of ``L`` entries alone.  sigma 0.2 and r_factor 3 give R = 0.6: a
    point on a pixel centre reaches that pixel only, with weight exactly its amplitude (r = 0: Gaussian and taper are 1).  Probed
    pixel number ``u`` (pixels 17 .. 30 of the middle tile, whose boxes stay inside it) carries three points at list indices
    ``(3q, 3q + 1, 3q + 2)`` (``layout = "consecutive"``) or ``(q, q + L // 3, q + 2 (L // 3))`` (``"spread"``), the last triple moved
    up to end on index ``L - 1``; their amplitudes are
    (1e8, -1e8, 1) for even ``u``, which sum to 1.0 in float32 only with the 1 last, and (1e8, 1, -1e8) for odd ``u``, which sum to
    0.0 unless the 1 comes last.  All other points have amplitude zero and sit on pixels of the same tile.
    Returns the case and ``{(row, col): expected float32 value}``."""
    rng = np.random.default_rng([43, L])
    span = TILE - 2
    pts = 17.0 + rng.integers(0, span, (L, 2)).astype(np.float64)
    amps = np.zeros(L)
    expect = {}
    for u, q in enumerate(_probe_rows(L)):
        idx = _probe_indices(L, layout, q)
        col, row = 17 + u % span, 17 + u // span
        triple, value = PROBE_TRIPLES["one_last" if u % 2 == 0 else "one_second"]
        pts[list(idx)] = [col, row]
        amps[list(idx)] = triple
        expect[row, col] = np.float32(value)
    return dict(shape=SEAM_SHAPE, base=None, pts=pts, amps=amps, sigma=0.2, r_factor=3.0), expect


def swapped_last_two(case, L, layout):
    """The same probe with the last two points of every triple exchanged: every probed pixel flips between 0.0 and 1.0."""
    amps = case["amps"].copy()
    for q in _probe_rows(L):
        idx = _probe_indices(L, layout, q)
        amps[idx[1]], amps[idx[2]] = amps[idx[2]], amps[idx[1]]
    return dict(case, amps=amps)


def uncut_window_case():
    """Six 19 x 23 frames without a cutoff, with 0, 1, 255, 256, 257 and 600 points: none, one lane, a window less one, one
    window, a window and one, and two windows with a ragged third."""
    rng = np.random.default_rng(47)
    counts, n = UNCUT_WINDOW_COUNTS, sum(UNCUT_WINDOW_COUNTS)
    return dict(shape=(len(counts), 19, 23), base=_frame((len(counts), 19, 23), 23), counts=counts, sigma=2.2,
                pts=np.column_stack([rng.uniform(-3, 26, n), rng.uniform(-3, 22, n)]), amps=rng.uniform(-1, 2, n))


UNCUT_PROBE_PIXEL = (7, 11)                                # (row, col)
UNCUT_PROBE_INDICES = ((254, 255, 256), (255, 256, 600), (3, 130, 255))


def uncut_probe_case():
    """Six float32 frames of 19 x 23 zeros with 257, 257, 601, 601, 256 and 256 points (index 600 needs 601), all on the centre of
    pixel (7, 11) where ``a * exp(-0)`` is exactly ``a``: the triples sit at indices 254, 255, 256 (across the first window seam),
    255, 256, 600 (the last of a window, the first of the next, the last of the ragged third) and 3, 130, 255 (inside one window:
    the order of the walk through it) of their frame's range, once as (1e8, -1e8, 1) and once as (1e8, 1, -1e8); every other
    point has amplitude zero.  Returns the case and the expected value of that pixel per frame."""
    counts, amps, expect = [], [], []
    for idx in UNCUT_PROBE_INDICES:
        for name in ("one_last", "one_second"):
            triple, value = PROBE_TRIPLES[name]
            a = np.zeros(idx[-1] + 1)
            a[list(idx)] = triple
            counts.append(len(a))
            amps.append(a)
            expect.append(np.float32(value))
    amps = np.concatenate(amps)
    row, col = UNCUT_PROBE_PIXEL
    return dict(shape=(len(counts), 19, 23), base=None, counts=counts, sigma=2.2, pts=np.tile([[float(col), float(row)]], (len(amps), 1)),
                amps=amps), expect


def cut_edge_case():
    """One point on the centre of pixel (10, 12) of a 24 x 27 frame of zeros, sigma 1, r_factor 3: the four pixels at distance
    exactly R = 3 (sqrt(9) is exact) receive ``a * exp(-4.5)`` without the taper and ``a * exp(-4.5) * 0 = +0.0`` with it; the
    pixels next to them along the box edge (distance sqrt(10)) receive nothing."""
    return dict(shape=(24, 27), base=None, pts=np.array([[12.0, 10.0]]), amps=np.array([1.75]), sigma=1.0, r_factor=3.0)
