"""Host restatement of ``local_max`` with the package's tie rule (equal intensities in raster order): the checker of
tests/test_local_max_cpu.py, tests/test_gpu_local_max.py and tests/test_gpu_local_max_kernels.py and the host side of
tools/time_local_max.py.  It is the checker, never the product."""
import numpy as np
from scipy import ndimage
from scipy.spatial import cKDTree


def candidate_mask(image, threshold=None):
    """3 x 3 maxima (``maximum_filter``, mode 'nearest') ``> threshold`` (NumPy's comparison; None: the minimum), off the
    1-px border; none in a constant image (scikit-image's trivial-image rule).

    NaN (the package's own rule; neither the reference nor scikit-image defines one): the minimum and the constant-image
    test are taken over the non-NaN pixels, an image with no non-NaN pixel has no candidates, a NaN pixel is never a
    candidate and a NaN neighbour never exceeds a pixel (NaN counts as -inf in the 3 x 3 maximum, and only there)."""
    image = np.asarray(image)
    mask = np.zeros(image.shape, dtype=bool)
    if image.size == 0:
        return mask
    nan = np.isnan(image) if image.dtype.kind == "f" else np.zeros(image.shape, dtype=bool)
    if nan.any():
        valid = image[~nan]
        if valid.size == 0 or valid.min() == valid.max():
            return mask
        lowest = valid.min()
        mask = image == ndimage.maximum_filter(np.where(nan, image.dtype.type(-np.inf), image), size=3, mode="nearest")
    else:
        lowest = image.min()
        mask = image == ndimage.maximum_filter(image, size=3, mode="nearest")
        if mask.all():
            mask[:] = False
    with np.errstate(invalid="ignore"):
        mask &= image > (lowest if threshold is None else threshold)
    mask[:1] = mask[-1:] = False
    mask[:, :1] = mask[:, -1:] = False
    return mask


# ---- which suppression kernel the host takes (csrc/zk_peaks.hip: TILE_W, TILE_H, TILE_LDS_MAX and the disk of local_max_core)
TILE_W, TILE_H, TILE_LDS_MAX = 64, 16, 60 * 1024


def tile_lds_bytes(r, H, W):
    """Dynamic LDS the tiled suppression kernel would need for radius ``r`` on an ``H x W`` frame, as the host computes it:
    a ``TILE_W x TILE_H`` tile plus a halo of ``floor(r)`` clipped to the frame (``Rx = min(floor(r), W - 1)``, ``Ry``
    likewise), 5 bytes per cell (int32 rank, one state byte), plus 4 bytes per offset of the inclusive disk
    ``dx^2 + dy^2 <= r^2`` inside that halo, the centre excluded.  The host takes the tiled kernel while this is
    ``<= TILE_LDS_MAX`` and one global round per launch otherwise."""
    r = float(r)
    Rx, Ry = int(min(np.floor(r), W - 1)), int(min(np.floor(r), H - 1))
    LW, LH = TILE_W + 2 * Rx, TILE_H + 2 * Ry
    dy, dx = np.mgrid[-Ry:Ry + 1, -Rx:Rx + 1].astype(np.int64)
    n_off = int(((dx * dx + dy * dy).astype(np.float64) <= r * r).sum()) - 1
    return LW * LH * 5 + 4 * n_off


def plateaus(dtype, shape=(96, 112), seed=0):
    """Integer frames full of ties: flat-topped blobs, equal peaks side by side, and a coarse random texture."""
    rng = np.random.default_rng(seed)
    hi = 250 if dtype == np.uint8 else 60000
    img = rng.integers(0, 6, shape) * (hi // 10)
    for _ in range(40):
        y, x = rng.integers(2, shape[0] - 4), rng.integers(2, shape[1] - 4)
        img[y:y + rng.integers(1, 4), x:x + rng.integers(1, 4)] = rng.choice([hi // 2, hi])
    img[10, 10:40:2] = hi                   # a row of equal peaks 2 px apart
    return img.astype(dtype)


def candidates_by_priority(image, threshold=None):
    """(x, y) of the candidates in priority order (intensity descending, then row, then column) and their values."""
    image = np.asarray(image)
    rows, cols = np.nonzero(candidate_mask(image, threshold))
    vals = image[rows, cols].astype(np.float64)
    order = np.lexsort((np.arange(rows.size), -vals))
    return np.stack([cols, rows], axis=1)[order].astype(np.int64), vals[order]


def within(a, b, r):
    """Exact inclusive distance test of the contract: float64(dx^2 + dy^2) <= r * r."""
    d = np.asarray(a, dtype=np.int64) - np.asarray(b, dtype=np.int64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(np.float64) <= float(r) * float(r)


def pairs_within(pts, r):
    """(i, j), i < j, of the points within r of each other (exact test)."""
    if len(pts) < 2:
        return np.empty((0, 2), dtype=np.int64)
    p = cKDTree(pts).query_pairs(float(r) + 1e-6, output_type="ndarray")
    return p[within(pts[p[:, 0]], pts[p[:, 1]], r)] if len(p) else p


def local_max_raster(image, min_distance, threshold=None):
    """The greedy suppression, sequentially: (N, 2) int64 (x, y) in priority order."""
    pts, _ = candidates_by_priority(image, threshold)
    if len(pts) == 0:
        return np.empty((0, 2), dtype=np.int64)
    tree = cKDTree(pts)
    keep = np.ones(len(pts), dtype=bool)
    for i in range(len(pts)):
        if not keep[i]:
            continue
        nb = np.asarray(tree.query_ball_point(pts[i], float(min_distance) + 1e-6), dtype=np.int64)
        nb = nb[(nb != i) & within(pts[nb], pts[i], min_distance)]
        keep[nb] = False
    return pts[keep]


def check_greedy(image, min_distance, points, threshold=None):
    """Whether ``points`` is THE greedy result, without the sequential loop: the points are candidates in non-increasing
    priority, no two kept points lie within r, and every dropped candidate has a kept higher-priority one within r."""
    pts, _ = candidates_by_priority(image, threshold)
    prio = {tuple(p): k for k, p in enumerate(pts.tolist())}
    ranks = np.array([prio.get(tuple(p), -1) for p in np.asarray(points).tolist()], dtype=np.int64)
    assert (ranks >= 0).all(), "a returned point is not a candidate"
    assert (np.diff(ranks) > 0).all(), "points are not in priority order"
    assert len(pairs_within(np.asarray(points), min_distance)) == 0, "two kept points within min_distance"
    dropped = np.setdiff1d(np.arange(len(pts)), ranks)
    if len(dropped):
        assert len(ranks), "candidates but nothing kept"
        m = cKDTree(pts[dropped]).sparse_distance_matrix(cKDTree(pts[ranks]), float(min_distance) + 1e-6, output_type="ndarray")
        d, k = dropped[m["i"]], ranks[m["j"]]
        ok = within(pts[d], pts[k], min_distance) & (k < d)
        covered = np.zeros(len(pts), dtype=bool)
        covered[d[ok]] = True
        assert covered[dropped].all(), "a dropped candidate has no kept higher-priority point within min_distance"
    return True


# ---- the images of tests/golden/local_max_golden.npz: stored there as this recipe plus a SHA-256 of their bytes
GOLDEN_IMAGES = ("img_honey32", "img_honey64", "img_noise64", "img_ramp", "img_const", "img_2xN", "img_Nx2")


def golden_image(name):
    """The fixture image ``name``: honeycomb frames and white noise regenerated from their seeds, the rest built."""
    from mtflearn_amd.synthetic import honeycomb_frame
    if name == "img_honey32":
        return honeycomb_frame(256, 240, seed=11)
    if name == "img_honey64":
        noise = np.random.default_rng(1201).standard_normal((240, 256))
        return honeycomb_frame(240, 256, seed=12).astype(np.float64) + 0.1 * noise
    if name == "img_noise64":
        return np.random.default_rng(1202).random((96, 128))
    if name == "img_ramp":                       # 509 isolated peaks, 2 px apart, rising to the right
        ramp = np.zeros((3, 2 * 509 + 3))
        ramp[1, 1:2 * 509:2] = np.arange(1, 510, dtype=np.float64)
        return ramp
    if name == "img_const":
        return np.full((32, 40), 0.5, dtype=np.float32)
    if name == "img_2xN":
        return np.random.default_rng(1203).random((2, 50))
    if name == "img_Nx2":
        return np.random.default_rng(1204).random((50, 2))
    raise KeyError(name)


def image_digest(image):
    """SHA-256 of an image's dtype, shape and bytes."""
    import hashlib
    image = np.ascontiguousarray(image)
    return hashlib.sha256(repr((image.dtype.str, image.shape)).encode() + image.tobytes()).hexdigest()
