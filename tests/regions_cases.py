"""Seeded inputs of the mtflearn_amd.graph tests: ``cases()`` -> ``{name: (pts float64 (N, 2), ijs int64 (E, 2))}``.
Nothing is stored; tests/make_golden_regions.py and the tests regenerate the same arrays.

Every case asserts its own CONDITIONING (``conditioning``), on the graph with the grown edge added: at every node the
smallest gap between two neighbour angles is >= 1e-9 rad, and no angle lies within 1e-9 of 0 or 2 pi unless dy is exactly 0.
An ``atan2`` that is a few ulp off the host's therefore cannot reorder any neighbour list, and parity with the reference is
exact equality."""
import numpy as np

MIN_GAP = 1e-9
TWO_PI = 2 * np.pi


def both_ways(pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    return np.vstack([pairs, pairs[:, ::-1]])


def bonds(pts, radius):
    """Both directions of every pair of points closer than ``radius``."""
    from scipy.spatial import cKDTree
    return both_ways(cKDTree(pts).query_pairs(radius, output_type="ndarray"))


def honeycomb(size, l, seed, jitter=0.4):
    """Honeycomb sites with bond length ``l`` inside ``[0, size)^2``, rotated a little, each moved by Gaussian noise."""
    rng = np.random.default_rng(seed)
    a1, a2 = np.array([1.5 * l, np.sqrt(3.0) * l / 2]), np.array([1.5 * l, -np.sqrt(3.0) * l / 2])
    n = int(np.ceil(size / l)) + 3
    idx = np.arange(-n, n + 1)
    cells = (np.repeat(idx, len(idx))[:, None] * a1 + np.tile(idx, len(idx))[:, None] * a2)
    sites = np.vstack([cells, cells + np.array([l, 0.0])]) + rng.random(2) * l
    c, s = np.cos(0.1), np.sin(0.1)
    sites = sites @ np.array([[c, -s], [s, c]]).T + size / 2.0
    sites = sites + rng.normal(0.0, jitter, sites.shape)
    return np.ascontiguousarray(sites[(sites >= 0).all(axis=1) & (sites < size).all(axis=1)])


def polygon(n, radius, centre=(0.0, 0.0), phase=0.1):
    t = phase + TWO_PI * np.arange(n) / n
    return np.array(centre) + radius * np.array([np.cos(t), np.sin(t)]).T


def ring_edges(n, first=0):
    i = np.arange(n)
    return both_ways(np.array([first + i, first + (i + 1) % n]).T)


def conditioning(pts, ijs):
    """``(smallest gap between two neighbour angles of one node, smallest distance of an angle with dy != 0 from 0 and 2 pi)``
    over the graph with the grown edge added; ``inf`` where there is nothing to measure."""
    pts = np.asarray(pts, dtype=np.float64)
    n = len(pts)
    if n == 0:
        return np.inf, np.inf
    i0 = int(np.argmin(pts[:, 0]))
    ext = np.vstack([pts, [pts[i0, 0] - 1, pts[i0, 1]]])
    e = np.unique(np.vstack([np.asarray(ijs, dtype=np.int64).reshape(-1, 2), [[i0, n], [n, i0]]]), axis=0)
    d = ext[e[:, 1]] - ext[e[:, 0]]
    theta = (np.arctan2(d[:, 1], d[:, 0]) + TWO_PI) % TWO_PI
    order = np.lexsort((theta, e[:, 0]))
    i, th = e[order, 0], theta[order]
    same = i[1:] == i[:-1]
    gap = float((th[1:] - th[:-1])[same].min()) if same.any() else np.inf
    off_axis = d[:, 1] != 0
    edge = float(np.minimum(theta[off_axis], TWO_PI - theta[off_axis]).min()) if off_axis.any() else np.inf
    return gap, edge


def _checked(name, pts, ijs):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    ijs = np.ascontiguousarray(np.asarray(ijs, dtype=np.int64).reshape(-1, 2))
    gap, edge = conditioning(pts, ijs)
    assert gap >= MIN_GAP and edge >= MIN_GAP, (name, gap, edge)
    return pts, ijs


def _build():
    out = {}
    out["01_point"] = ([[3.0, 4.0]], np.empty((0, 2), np.int64))
    out["02_triangle"] = ([[0.0, 0.0], [4.0, 0.5], [1.5, 3.0]], ring_edges(3))
    # a square with a bond dangling inside it: the dead end kills the inner face, the grown edge the outer one
    out["03_square_dangling"] = ([[0.0, 0.0], [4.0, 0.2], [4.1, 4.0], [0.3, 4.2], [1.5, 1.0]],
                                 np.vstack([ring_edges(4), both_ways([[0, 4]])]))
    # the second component is not touched by the grown edge: it keeps both of its faces, one per orientation
    out["04_two_triangles"] = ([[0.0, 0.0], [4.0, 0.5], [1.5, 3.0], [10.0, 0.0], [14.0, 0.7], [11.0, 3.5]],
                               np.vstack([ring_edges(3), ring_edges(3, 3)]))
    hexagon = polygon(6, 5.0, (20.0, 20.0))
    chain = np.array([[30.0, 14.0], [33.0, 17.5], [31.0, 21.0], [34.0, 25.0]])
    out["05_isolated_chain_hexagon"] = (np.vstack([hexagon, [[2.0, 30.0]], chain]),
                                        np.vstack([ring_edges(6), both_ways([[7, 8], [8, 9], [9, 10]])]))
    out["06_one_way_triangle"] = ([[0.0, 0.0], [4.0, 0.5], [1.5, 3.0]], [[0, 1], [1, 2], [2, 0]])
    shared = np.vstack([ring_edges(3), both_ways([[1, 3], [3, 4], [4, 2]])])       # a triangle and a quadrilateral on one bond
    out["07_duplicated_edges"] = ([[0.0, 0.0], [4.0, -1.0], [3.5, 3.0], [8.0, -0.5], [7.5, 4.0]], np.vstack([shared, shared, shared[::-1]]))
    # integer grid: tied minimum x (argmin takes the first), angles exact multiples of pi / 2, all faces squares
    gy, gx = np.divmod(np.arange(64), 8)
    grid = np.array([gx, gy], dtype=np.float64).T
    right = np.array([(k, k + 1) for k in range(64) if k % 8 != 7])
    up = np.array([(k, k + 8) for k in range(56)])
    out["08_grid"] = (grid, both_ways(np.vstack([right, up])))
    # a wheel: the hub has more neighbours than any small sorting network takes
    rng = np.random.default_rng(9)
    spokes = 20
    rim = polygon(spokes, 10.0, (0.0, 0.0), 0.05) + rng.normal(0, 0.3, (spokes, 2))
    out["09_wheel"] = (np.vstack([rim, [[0.2, -0.1]]]), np.vstack([ring_edges(spokes), both_ways([(k, spokes) for k in range(spokes)])]))
    small = honeycomb(96, 12.0, 10)
    out["10_honeycomb_96"] = (small, bonds(small, 1.3 * 12.0))
    large = honeycomb(512, 12.0, 11)
    large_bonds = bonds(large, 1.3 * 12.0)
    out["11_honeycomb_512"] = (large, large_bonds)
    from scipy.spatial import Delaunay
    cloud = np.random.default_rng(12).random((200, 2)) * 100
    tri = Delaunay(cloud).simplices
    out["12_delaunay"] = (cloud, both_ways(np.vstack([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])))
    # a long ring (two faces of 3000 vertices, one per orientation) and, further left, the triangle that takes the grown edge
    ring = polygon(3000, 1000.0, (0.0, 0.0), 0.1)
    out["13_ring_3000"] = (np.vstack([ring, [[-2000.0, 0.0], [-1990.0, 3.0], [-1995.0, 9.0]]]),
                           np.vstack([ring_edges(3000), ring_edges(3, 3000)]))
    # the large honeycomb with 5 % of its bonds missing: mixed ring sizes and dangling bonds
    undirected = large_bonds[: len(large_bonds) // 2]
    keep = np.random.default_rng(14).random(len(undirected)) >= 0.05
    out["14_honeycomb_512_holes"] = (large, both_ways(undirected[keep]))
    return {name: _checked(name, pts, ijs) for name, (pts, ijs) in out.items()}


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


NAMES = ["01_point", "02_triangle", "03_square_dangling", "04_two_triangles", "05_isolated_chain_hexagon", "06_one_way_triangle",
         "07_duplicated_edges", "08_grid", "09_wheel", "10_honeycomb_96", "11_honeycomb_512", "12_delaunay", "13_ring_3000",
         "14_honeycomb_512_holes"]

# polygon counts worked out by hand from the rules (dead ends, the grown edge, one face per orientation of a free component)
EXPECTED_FACES = {"01_point": 0, "02_triangle": 1, "03_square_dangling": 0, "04_two_triangles": 3, "06_one_way_triangle": 0,
                  "08_grid": 49}


# ------------------------------------------------------------------------------------------------ kernel-level cases
# (tests/test_gpu_regions_kernels.py; the reference is tests/regions_oracle.py, itself held to the reference's goldens on
# GOLDEN_KERNEL_NAMES by tests/test_regions_cpu.py)
RING_SIZES = (1021, 1022, 1023, 1024, 4093)
TIED_NODES = (2500, 1030, 2047)                            # strides 2, 1, 1 and lanes 452, 6, 1023 of a 1024-lane sweep
TIED_TRIANGLE_NODES = (2500, 1030, 2047, 2054)             # 2054 = 1030 + 1024: the same lane one stride later
FAR_LEFT_TRIANGLE = [[-2000.0, 0.0], [-1990.0, 3.0], [-1995.0, 9.0]]


def _build_kernel_cases():
    out = {}
    # cycles on both sides of 2^10 and 2^12 wedges; the triangle further left takes the grown edge, the ring keeps both faces
    for n in RING_SIZES:
        out[f"ring_{n}"] = (np.vstack([polygon(n, 1000.0, (0.0, 0.0), 0.1), FAR_LEFT_TRIANGLE]), np.vstack([ring_edges(n), ring_edges(3, n)]))
    # a dead-end path far longer than any cycle: out along the chain and back, 10 000 wedges that must not be taken for a face
    square = np.array([[0.0, 0.0], [4.0, 0.2], [4.1, 4.0], [0.3, 4.2]]) - [50.0, 0.0]
    links = 5000
    chain = np.column_stack([100.0 + np.arange(links), np.random.default_rng(3).normal(0.0, 0.2, links)])
    hang = np.array([[1, 4]] + [(4 + k, 5 + k) for k in range(links - 1)])
    out["chain_5000"] = (np.vstack([square, chain]), np.vstack([ring_edges(4), both_ways(hang)]))
    # a hub with 700 neighbours: the angular sort counts a row of 700 for each of its entries
    spokes = 700
    out["wheel_700"] = (np.vstack([polygon(spokes, 100.0, (0.0, 0.0), 0.003), [[0.2, -0.1]]]),
                        np.vstack([ring_edges(spokes), both_ways([(k, spokes) for k in range(spokes)])]))
    # the same wheel with its nodes renumbered at random: the order by neighbour index has nothing to do with the order by angle
    perm = np.random.default_rng(7).permutation(spokes + 1)
    pts, ijs = out["wheel_700"]
    relabelled = np.empty_like(pts)
    relabelled[perm] = pts
    out["wheel_700_shuffled"] = (relabelled, perm[ijs])
    # the minimum x three times, in different lanes and strides of the argmin sweep; np.argmin takes node 1030
    from scipy.spatial import Delaunay
    cloud = np.random.default_rng(5).random((3000, 2)) * 100 + 1
    cloud[list(TIED_NODES), 0] = 0.5
    tri = Delaunay(cloud).simplices
    out["tied_min_3000"] = (cloud, both_ways(np.vstack([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])))
    # the same tie where the choice SHOWS: 1000 separate triangles (nodes 3c, 3c + 1, 3c + 2).  A free triangle keeps two faces,
    # one per orientation; the one that takes the grown edge loses its outer face.  That must be the triangle of node 1030.
    rng = np.random.default_rng(6)
    tris = np.vstack([polygon(3, 2.0, (5.0, 10.0 * c), rng.uniform(0, TWO_PI)) for c in range(1000)])
    tris[list(TIED_TRIANGLE_NODES), 0] = 0.5
    out["tied_min_triangles"] = (tris, np.vstack([ring_edges(3, 3 * c) for c in range(1000)]))
    return {name: _checked(name, pts, ijs) for name, (pts, ijs) in out.items()}


_KERNEL_CASES = None


def kernel_cases():
    global _KERNEL_CASES
    if _KERNEL_CASES is None:
        _KERNEL_CASES = _build_kernel_cases()
    return _KERNEL_CASES


KERNEL_NAMES = [f"ring_{n}" for n in RING_SIZES] + ["chain_5000", "wheel_700", "wheel_700_shuffled", "tied_min_3000", "tied_min_triangles"]
GOLDEN_KERNEL_NAMES = ["ring_1024", "wheel_700"]          # the sizes the reference's quadratic walk finishes in under a minute

# name -> {polygon size: count}, from the rules (and the oracle, on the CPU)
KERNEL_EXPECTED_KS = {**{f"ring_{n}": {3: 1, n: 2} for n in RING_SIZES}, "chain_5000": {4: 1}, "wheel_700": {3: 700}, "wheel_700_shuffled": {3: 700},
                      "tied_min_3000": {3: 5978}, "tied_min_triangles": {3: 1999}}
