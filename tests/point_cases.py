"""Point sets that reach the edges of the point-set kernels (csrc/zk_point_grid.h, csrc/zk_knn.hip,
csrc/zk_voronoi.hip), regenerated from seeds: NumPy only, read-only arrays.  The sets of tests/refine_cases.py and
tests/vnn_cases.py are near-uniform; each set here is named for the line of a kernel it exercises.

``knn_sets()`` maps a name to the ``(N, 2)`` points of the neighbour search, ``voronoi_sets()`` to smaller sets of the same
shapes for the cells (tests/vnn_oracle.py runs at test time and is O(N^2) per set), ``stats_matrix`` / ``hist_matrix`` /
``gaps_matrix`` make the synthetic ``(N, 12)`` distance matrices of the ``zk_knn_stats`` reductions.  ``knn_frame`` / ``bin_of``
restate the binning rule of the neighbour search; tests/test_gpu_points_kernels.py asserts with them that every set has the
property it is named for.

All sets have distinct points except ``many_duplicates`` and ``on_bin_sides``: with ``g = 32`` bins per axis there are only
``33 x 33 = 1089`` positions whose coordinates are all multiples of the bin side, so the 2048 points of ``on_bin_sides`` take
every position at most twice (``n = 2048`` is what gives ``g = 32`` and ``h = 2`` exactly)."""
import functools

import numpy as np

import refine_cases as rc
import vnn_cases as vc

KNN = 12
TINY_NS = tuple(range(1, 21))
WHEEL_SPOKES = tuple(range(25, 37))
STATS_SIZES = (1, 255, 256, 257, 131072, 131073, 300001)     # one lane; one workgroup -+ 1; 512 workgroups, one trip; the first
#                                                              row of the second trip; a ragged third trip
Q = 2.0 ** -10                                               # every entry of a stats matrix is a multiple of Q below 1024


def _readonly(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------
# the binning rule of knn_frame_kernel / zk_grid_frame, restated
# ---------------------------------------------------------------------------------------------------------
def grid_side(n):
    return min(max(int(np.ceil(np.sqrt(n / 2))), 1), 4096)


def knn_frame(pts):
    """``(x0, y0, h, g)`` of the neighbour search: square bins over the bounding box."""
    pts = np.asarray(pts, dtype=np.float64)
    g = grid_side(len(pts))
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    span = max(hi[0] - lo[0], hi[1] - lo[1])
    return lo[0], lo[1], (span / g if span > 0 else 1.0), g


def bin_of(pts, frame=None):
    """int ``(N, 2)``: the bin ``(bx, by)`` of every point."""
    pts = np.asarray(pts, dtype=np.float64)
    x0, y0, h, g = frame or knn_frame(pts)
    return np.clip(np.floor((pts - [x0, y0]) / h), 0, g - 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------
# point sets
# ---------------------------------------------------------------------------------------------------------
def tiny(n):
    return np.random.default_rng(100 + n).uniform(0.0, 1.0, (n, 2))


def blob_and_halo(n_blob, n_halo, seed, radius=0.01):
    """``n_blob`` points in a disc of ``radius`` at (37, 61), then ``n_halo`` uniform over [0, 100]^2."""
    rng = np.random.default_rng(seed)
    r, phi = radius * np.sqrt(rng.uniform(0, 1, n_blob)), rng.uniform(0, 2 * np.pi, n_blob)
    blob = np.stack([37 + r * np.cos(phi), 61 + r * np.sin(phi)], axis=1)
    return np.concatenate([blob, rng.uniform(0.0, 100.0, (n_halo, 2))])


def strip(n, length, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.0, length, n), rng.uniform(0.0, 1.0, n)], axis=1)


def on_bin_sides(seed):
    """(0, 0), (64, 64) and 2046 even-integer pairs in [0, 64]^2, every position at most twice, shuffled."""
    rng = np.random.default_rng(seed)
    sites = np.array([(x, y) for x in range(0, 65, 2) for y in range(0, 65, 2) if (x, y) not in ((0, 0), (64, 64))], dtype=np.float64)
    twice = np.concatenate([sites, sites])
    pts = np.concatenate([[[0.0, 0.0], [64.0, 64.0]], twice[rng.permutation(len(twice))[:2046]]])
    return pts[rng.permutation(len(pts))]


def two_scales(coarse, fine, seed, step=64):
    """A ``coarse`` x ``coarse`` lattice of spacing 1 beside a ``fine`` x ``fine`` lattice of spacing 1 / ``step``, jitter 5 %."""
    return np.concatenate([vc.square_patch(coarse, coarse, 1.0, 0.05, seed),
                           vc.square_patch(fine, fine, 1.0 / step, 0.05, seed + 1, origin=(coarse + 0.5, coarse / 2.0))])


def many_duplicates(seed):
    rng = np.random.default_rng(seed)
    pts = np.repeat(rng.uniform(0.0, 10.0, (100, 2)), 20, axis=0)
    return pts[rng.permutation(len(pts))]


def wheel(spokes):
    return vc.wheel(spokes, 300 + spokes)


def hub_vertex_counts(pts, pad=0.05):
    """The vertex count of the cell of point 0 after every clip, in the order csrc/zk_voronoi.hip clips: the four corner points,
    then the bins in rings around the point's own bin (the row above, the row below, then left and right bin of every row
    between), the points of a bin in index order.  No ring is skipped here, so the device visits a prefix of this order: where
    the largest count is at most 32, ``clip_cell`` has no reason to refuse the cell."""
    import vnn_oracle as oracle
    pts = np.asarray(pts, dtype=np.float64)
    n, g = len(pts), grid_side(len(pts))
    c = pts.mean(axis=0)
    v0, s = np.abs(pts - c).max(), 1 + pad
    v = v0 * s
    half = v * ((2 * s * s - 1) / (2 * pad * s)) * 17 / 16
    bins = bin_of(pts, (c[0] - v0, c[1] - v0, 2 * v0 / g, g))
    key = bins[:, 1] * g + bins[:, 0]
    m = c - pts[0]
    poly = np.array([(m[0] - half, m[1] - half), (m[0] + half, m[1] - half), (m[0] + half, m[1] + half), (m[0] - half, m[1] + half)])
    ids, counts = [-1] * 4, []
    order = [(c + [sx * v, sy * v], n + t) for t, (sx, sy) in enumerate(((-1, -1), (1, -1), (1, 1), (-1, 1)))]
    bx, by = bins[0]
    for r in range(g):
        cells = []
        xlo, xhi = max(bx - r, 0), min(bx + r, g - 1)
        if by - r >= 0:
            cells += [(x, by - r) for x in range(xlo, xhi + 1)]
        if r > 0 and by + r <= g - 1:
            cells += [(x, by + r) for x in range(xlo, xhi + 1)]
        for y in range(max(by - r + 1, 0), min(by + r - 1, g - 1) + 1):
            if bx - r >= 0:
                cells.append((bx - r, y))
            if r > 0 and bx + r <= g - 1:
                cells.append((bx + r, y))
        order += [(pts[j], int(j)) for x, y in cells for j in np.nonzero(key == y * g + x)[0] if j != 0]
    for q, j in order:
        q = q - pts[0]
        if ((poly @ q - 0.5 * (q @ q)) > 0).any():
            poly, ids = oracle._clip(poly, ids, q, j)
        counts.append(len(ids))
    return counts


@functools.lru_cache(maxsize=None)
def knn_sets():
    out = {f"tiny_{n}": tiny(n) for n in TINY_NS}
    out["blob_and_halo"] = blob_and_halo(3000, 1000, 51)
    out["strip"] = strip(4096, 1000.0, 52)
    out["on_bin_sides"] = on_bin_sides(53)
    out["two_scales"] = two_scales(24, 40, 54)
    out["far_offset"] = np.concatenate([rc.point_sets()["scattered_300"], [[1e8, -3e7]]])
    out["many_duplicates"] = many_duplicates(56)
    for s in WHEEL_SPOKES:
        out[f"wheel_{s}"] = wheel(s)
    return {name: _readonly(np.ascontiguousarray(pts, dtype=np.float64)) for name, pts in out.items()}


KNN_NAMES = tuple(knn_sets())
HALO_START = 3000                                    # blob_and_halo: the halo points are the last 1000


@functools.lru_cache(maxsize=None)
def voronoi_sets():
    """The shapes of ``knn_sets()`` at the sizes the O(N^2) oracle allows.  The density steps are milder than there (a disc of
    radius 1, a lattice step of 16): at the steps of the kNN sets qhull and the oracle differ by more than a hundredth of the
    project's ridge tolerance, in units of the median edge, which the dense part sets (tests/test_vnn_reference_cpu.py)."""
    out = {"strip": strip(600, 1000.0, 62), "blob_and_halo": blob_and_halo(400, 200, 71, radius=1.0),
           "two_scales": two_scales(12, 20, 74, step=16)}
    return {name: _readonly(np.ascontiguousarray(pts)) for name, pts in out.items()}


VORONOI_NAMES = tuple(voronoi_sets())
DMAX_FACTOR, THRESHOLD = 1.3, 0.1                    # dmax = 1.3 a, a = the set's median edge length from the oracle


def knn_reference(pts, k):
    """Brute force in float64, in row chunks of 1000: the kernel's own expression (it is compiled without contraction), and the
    sorted distances of a row do not depend on the order the points are visited in."""
    pts = np.asarray(pts, dtype=np.float64)
    out = np.empty((len(pts), k))
    for lo in range(0, len(pts), 1000):
        dx = pts[None, :, 0] - pts[lo:lo + 1000, None, 0]
        dy = pts[None, :, 1] - pts[lo:lo + 1000, None, 1]
        out[lo:lo + 1000] = np.sort(np.sqrt(dx * dx + dy * dy), axis=1)[:, :k]
    return out


# ---------------------------------------------------------------------------------------------------------
# synthetic distance matrices of zk_knn_stats: ascending rows, column 0 zero, every entry a multiple of Q
# ---------------------------------------------------------------------------------------------------------
def planted_rows(n):
    """Rows where extremes are planted: the last row, row 131072 (the first of the second grid-stride trip), a lane of the last
    wave of the first workgroup and of the last workgroup of the first trip; those that exist, without repeats."""
    rows = []
    for r in (n - 1, 131072, 200, 131071 - 3, n // 2):
        if 0 <= r < n and r not in rows:
            rows.append(r)
    return rows


def _ascending(rng, n, top):
    """``(n, 12)``: column 0 zero, columns 1 .. 11 ascending multiples of Q in [1, top]."""
    dd = np.zeros((n, KNN))
    dd[:, 1:] = np.sort(rng.integers(1024, int(top * 1024) + 1, (n, KNN - 1)), axis=1) * Q
    return dd


@functools.lru_cache(maxsize=None)
def stats_matrix(n):
    """Values in [1, 1000]; the smallest of column 1 (Q) and the largest of column j (1001 + j) stand in ``planted_rows(n)``."""
    dd = _ascending(np.random.default_rng(700 + n % 1000), n, 1000.0)
    rows = planted_rows(n)
    if len(rows) > 1:
        dd[rows[0], 1] = Q
        for j in range(1, KNN):
            r = rows[1 + j % (len(rows) - 1)]
            dd[r, j:] = 1001.0 + j + Q * np.arange(KNN - j)
    return _readonly(dd)


def hist_lasts(kind):
    if kind == "dyadic":
        return np.full(KNN - 1, np.round(1023.999 * 1024) * Q)
    if kind == "round":
        return np.full(KNN - 1, 1000.0)
    return 300.1 + 60.7 * np.arange(KNN - 1)                             # "uneven": one range per k, none of them dyadic


HIST_KINDS = ("dyadic", "round", "uneven")


def hist_edges(kind):
    return [np.linspace(0.0, last, 257) for last in hist_lasts(kind)]


@functools.lru_cache(maxsize=None)
def hist_matrix(n, kind):
    """Values in ``[0, lasts.min()]`` with, where ``n`` allows, entries equal to the bin edges of every ``k``, to ``np.nextafter``
    of them on both sides, to ``first = 0`` and to ``last``: whatever fits below the smallest ``last`` (column j belongs to every
    k > j).  Rows are sorted again after planting; the last row and the middle one are the eleven ``last`` themselves."""
    rng = np.random.default_rng(800 + n % 1000 + len(kind))
    lasts = hist_lasts(kind)
    top = lasts.min()
    dd = _ascending(rng, n, np.floor(top))
    plant = np.concatenate([np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)]) for e in hist_edges(kind)] + [[0.0, top]])
    plant = np.unique(plant[(plant >= 0) & (plant <= top)])
    plant = np.concatenate([[top, top, 0.0], plant[rng.permutation(len(plant))]])[:n * (KNN - 1) * 3 // 4 + 1]
    where = rng.permutation(n * (KNN - 1))[:len(plant)]
    dd[where // (KNN - 1), 1 + where % (KNN - 1)] = plant
    dd[:, 1:] = np.sort(dd[:, 1:], axis=1)
    dd[n - 1, 1:] = dd[n // 2, 1:] = lasts                               # column k - 1 holds last_k, which no later k exceeds
    return _readonly(dd)


@functools.lru_cache(maxsize=None)
def gaps_matrix(n):
    """Few distinct values, all multiples of 2 Q (at least 2^-9 apart), and ONE value a single Q above another: it stands in
    the last row, its partner in row 0 (more than 131072 rows apart where ``n`` allows), both in column 1, which belongs to
    every k.  With one row there is no gap to plant."""
    rng = np.random.default_rng(900 + n % 1000)
    dd = np.zeros((n, KNN))
    dd[:, 1:] = np.sort(rng.integers(8, 72, (n, KNN - 1)), axis=1) * (2 * Q) + 3.0
    if n > 1:
        dd[0, 1] = 3.0 + 4 * Q
        dd[n - 1, 1] = 3.0 + 5 * Q
    return _readonly(dd)
