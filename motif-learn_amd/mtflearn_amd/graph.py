"""mtflearn_amd.graph -- the reference's ``mtflearn.graph``: polygons ("regions": the 5-, 6-, 7-rings) of a planar lattice
graph, their centres and ring sizes, and the graph of neighbouring polygons.

``find_regions`` is the hot path.  The reference walks the faces wedge by wedge on the host, quadratic in the size of the graph;
here the whole computation is one launch sequence on the GPU (``csrc/zk_regions.hip``: radix sorts, a successor permutation over
the wedges, cycle labelling and ranking by pointer doubling, scans), with exact integer parity to the reference and centres
bit-equal to ``nodes[region].mean(axis=0)``.  There is no CPU fallback: without a device ``find_regions`` and everything of
:class:`LatticeGraph` that needs regions raises ``RuntimeError``.  The classes and the sparse-matrix helpers around it are the
host-side bookkeeping of the reference, with its names and argument order.

Deviations from the reference in ``find_regions``:

* ``pts`` is converted to float64.  (The reference would compute float32 angles for float32 points.)
* ``ijs`` must be of an integer type with values in ``[0, N)`` and no self-loops; anything else raises ``ValueError``.
* ``N == 0`` returns the empty object array.
* A node with out-neighbours but no in-neighbour (possible only with one-directional pairs) makes the reference index its wedge
  groups by position instead of by node; here the successor of ``(a, b, c)`` is always the wedge that starts ``(b, c)``.

Elsewhere: ``PlanarGraph.is_symmetric`` reduces the sparse difference with ``max`` (the reference's ``np.all`` of a sparse
comparison fails on current SciPy), and ``decompose`` / ``remove_nodes`` hand the node labels on as ``lbs`` (the reference passes
them in the ``img`` slot).

Bonds come from ``vnn_graph`` (reference ``graph/vnn.py``): the Voronoi neighbours of the points plus four far corner points
(``add_corner_points``), cut at ``dmax`` and at a share ``threshold`` of each row's summed ridge lengths, symmetrised by OR.
The diagram is not qhull's: every point clips its own cell on the GPU (``csrc/zk_voronoi.hip``), and ``voronoi_neighbours``
returns what the graph is made of.  Without ``dmax`` the bond length comes from ``estimate_d``, as in the reference (below).
Deviations, each a ``ValueError`` before any launch: ``threshold`` must be ``> 0`` (at ``<= 0`` the reference's
sparse comparison densifies), ``pts`` must be finite and free of coincident points (qhull drops duplicates silently and the
reference's indexing then shifts); a cell may have at most 32 vertices (``RuntimeError`` from the device for a point with more
Voronoi neighbours, or with nearly as many: cells are clipped in bin order and may pass their final size on the way).

``estimate_d`` (reference ``graph/vnn.py:18-40``) keeps the reference's signature and rule: for ``k = 2 .. 12`` the distances to
the nearest ``k - 1`` neighbours are thresholded (Otsu, or Li's minimum cross-entropy for anything but ``'otsu'``) and the
threshold that splits its sample most evenly wins.  The device does every pass over the data (``csrc/zk_knn.hip``: the
12-neighbour distance matrix on a grid of bins, one pass for the eleven ranges, one for the eleven 256-bin histograms under
NumPy's own binning rule, one fixed-tree reduction per Li iteration, a radix sort for Li's tolerance); the host applies the
scalar rules to a few hundred numbers with NumPy.  The two thresholds are this project's statements of the published
algorithms (Otsu 1979; Li and Tam 1998 as scikit-image iterates it): scikit-image is not installed where this is tested, so
parity with ``skimage.filters.threshold_otsu`` / ``threshold_li`` is UNPINNED; what is pinned is tests/thresholds_reference.py,
an independent NumPy / scikit-learn statement of the same definitions.  Li's loop ends when two iterates differ by no more
than half the smallest gap between distinct values; on a perfect lattice those gaps are rounding noise and the published loop
need not end (``estimate_d`` raises ``RuntimeError`` after 1000 iterations) -- measured points, or a few per cent of jitter, end
it in a handful.

Not provided: ``vnn_distance`` (Delaunay edges of the unpadded hull),
``get_polygon_masks`` (scikit-image ``polygon2mask``), the ``show*`` and ``save`` mixins (matplotlib, h5py).
"""
from __future__ import annotations

from ctypes import byref, c_int64, c_void_p

import numpy as np

from . import _native

__all__ = ["add_corner_points", "voronoi_neighbours", "vnn_graph", "knn_distances", "estimate_d", "find_regions", "PlanarGraph", "LatticeGraph", "LatticeGraph1", "Motif", "MotifsGraph", "sort_lbs", "symmetric_edges",
           "cantor_pairing", "construct_motif", "find_n_nodes", "matrix2edges", "matrix2ijs", "matrix2lil", "matrix2inds",
           "edges2matrix", "ijs2matrix", "is_symmetric", "make_symmetric", "make_symmetric_more", "make_symmetric_less",
           "get_num_faces"]


# ---------------------------------------------------------------------------------------------------------
# sparse-matrix helpers (reference graph/utils.py)
# ---------------------------------------------------------------------------------------------------------
def matrix2edges(matrix):
    from scipy.sparse import coo_matrix
    coo = coo_matrix(matrix)
    return np.array([coo.row, coo.col]).T


matrix2ijs = matrix2edges


def matrix2lil(matrix):
    from scipy.sparse import lil_matrix
    return lil_matrix(matrix).rows


matrix2inds = matrix2lil


def edges2matrix(ijs, shape=None, fmt="coo"):
    from scipy.sparse import coo_matrix
    rows, cols = np.asarray(ijs).T
    if shape is None:
        side = int(np.max(ijs) + 1)
        shape = (side, side)
    matrix = coo_matrix((np.ones_like(rows), (rows, cols)), shape=shape)
    if fmt in ("csr", "csc", "lil"):
        matrix = matrix.asformat(fmt)
    elif fmt == "dense":
        matrix = np.array(matrix.todense())
    return matrix


def ijs2matrix(ijs, shape=None):
    return edges2matrix(ijs, shape)


def is_symmetric(matrix):
    from scipy.sparse import issparse
    if issparse(matrix):
        from scipy.sparse.linalg import norm
        return norm(matrix - matrix.T) == 0
    return (matrix == matrix.T).all()


def make_symmetric(matrix):
    from scipy.sparse import csr_matrix, issparse, lil_matrix
    if not issparse(matrix):
        return np.maximum(matrix.T, matrix)
    matrix = lil_matrix(matrix)
    i, j = matrix.nonzero()
    matrix[j, i] = matrix[i, j]
    return csr_matrix(matrix)


def make_symmetric_more(matrix):
    """0 / 1 matrix with an entry wherever ``matrix`` or its transpose has a positive one."""
    matrix = (matrix > 0) * 1
    return ((matrix + matrix.T) / 2 > 0) * 1


def make_symmetric_less(matrix):
    """0 / 1 matrix with an entry wherever ``matrix`` and its transpose both have a positive one."""
    matrix = (matrix > 0) * 1
    return ((matrix + matrix.T) / 2 > 0.5) * 1


def _num_faces_connected(matrix):
    matrix = make_symmetric(matrix)
    return len(matrix2ijs(matrix)) // 2 - matrix.shape[0] + 1


def get_num_faces(matrix):
    """Euler's count ``e - v + 1`` of bounded faces, summed over the connected components."""
    from scipy.sparse.csgraph import connected_components
    n_components, lbs = connected_components(matrix, directed=False)
    if n_components == 1:
        return _num_faces_connected(matrix)
    faces = []
    for e in np.unique(lbs):
        inds = np.where(lbs == e)[0]
        faces.append(_num_faces_connected(matrix[:, inds][inds, :]))
    return np.sum(faces)


# ---------------------------------------------------------------------------------------------------------
# label / edge helpers (reference graph/planar_graph.py)
# ---------------------------------------------------------------------------------------------------------
def sort_lbs(lbs):
    """Relabel so that 0 is the most frequent label, 1 the next, ..."""
    unique_lbs, counts = np.unique(lbs, return_counts=True)
    unique_lbs = unique_lbs[np.argsort(counts)[::-1]]
    order = dict(zip(unique_lbs, range(len(unique_lbs))))
    return np.vectorize(order.get)(lbs)


def symmetric_edges(edges):
    return np.unique(np.vstack([edges, np.fliplr(edges)]), axis=0)


def cantor_pairing(ij, symmetric=True):
    ij = np.array(ij).reshape(-1, 2)
    i, j = (ij.min(axis=1), ij.max(axis=1)) if symmetric else (ij[:, 0], ij[:, 1])
    return (i + j) * (i + j + 1) // 2 + j


def construct_motif(pts):
    """The closed ring through ``pts`` in their order, as a :class:`Motif`."""
    n = len(pts)
    i, j = np.arange(n), np.roll(np.arange(n), 1)
    return Motif(pts, np.vstack([np.array([i, j]).T, np.array([j, i]).T]))


def _expand_nodes(nodes, lil):
    grown = [nodes.tolist() + [e] for e in lil[nodes[-1]] if e not in nodes]
    return np.array(grown if grown else [nodes.tolist() + [-1]])


def find_n_nodes(ijs, n=2):
    """All simple paths of ``n`` nodes along the edges ``ijs``, one per row."""
    matrix = edges2matrix(ijs)
    ijs = matrix2edges(matrix)
    lil = matrix2lil(matrix)
    for _ in range(n - 2):
        ijs = np.vstack([_expand_nodes(row, lil) for row in ijs])
        ijs = ijs[ijs[:, -1] != -1]
    _, idx = np.unique(ijs, axis=0, return_index=True)
    return ijs[idx]


def get_connected_components(matrix):
    from scipy.sparse.csgraph import connected_components
    n_components, lbs = connected_components(matrix, directed=False, return_labels=True)
    return n_components, sort_lbs(lbs)


# ---------------------------------------------------------------------------------------------------------
# find_regions: the device call
# ---------------------------------------------------------------------------------------------------------
def _check_graph(pts, ijs):
    """``(pts float64 (N, 2), ijs int64 (E, 2))`` C-contiguous, or ValueError; nothing is launched before this returns."""
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"pts must have shape (N, 2), not {pts.shape}")
    if pts.dtype.kind not in "fiu":
        raise ValueError(f"pts must be real numbers, not {pts.dtype}")
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    ijs = np.asarray(ijs)
    if ijs.size == 0 and ijs.ndim <= 2:
        ijs = np.empty((0, 2), np.int64)
    if ijs.ndim != 2 or ijs.shape[1] != 2:
        raise ValueError(f"ijs must have shape (E, 2), not {ijs.shape}")
    if ijs.dtype.kind not in "iu":
        raise ValueError(f"ijs must be of an integer type, not {ijs.dtype}")
    if ijs.dtype == np.uint64 and ijs.size and ijs.max() >= len(pts):
        raise ValueError(f"ijs must index the {len(pts)} points")
    ijs = np.ascontiguousarray(ijs, dtype=np.int64)
    if ijs.size:
        if ijs.min() < 0 or ijs.max() >= len(pts):
            raise ValueError(f"ijs must index the {len(pts)} points: values in [0, {len(pts)})")
        if (ijs[:, 0] == ijs[:, 1]).any():
            raise ValueError("ijs must not join a node to itself")
    if len(pts) + len(ijs) + 4 >= 2 ** 31:
        raise ValueError("find_regions needs len(pts) + len(ijs) + 4 < 2^31")
    return pts, ijs


def _regions_arrays(pts, ijs):
    """``(offsets, vertices, ks, centers, adjacency)`` of checked host arrays, from one device call."""
    if len(pts) == 0:
        return (np.zeros(1, np.int64), np.empty(0, np.int64), np.empty(0, np.int64), np.empty((0, 2)), np.empty((0, 2), np.int64))
    lib = _native.load()
    _native.require_device()
    device = _native.default_device()
    state, counts = c_void_p(), (c_int64 * 3)()
    ptr = lambda a: a.ctypes.data_as(c_void_p)
    _native.check(lib.zk_find_regions(device, ptr(pts), len(pts), ptr(ijs), len(ijs), byref(state), counts, None, None, None, None, None),
                  "zk_find_regions")
    f, v, a = (int(c) for c in counts)
    offsets, vertices, ks = np.empty(f + 1, np.int64), np.empty(v, np.int64), np.empty(f, np.int64)
    centers, adjacency = np.empty((f, 2), np.float64), np.empty((a, 2), np.int64)
    _native.check(lib.zk_find_regions(device, None, 0, None, 0, byref(state), counts, ptr(offsets), ptr(vertices), ptr(ks), ptr(centers),
                                      ptr(adjacency)), "zk_find_regions")
    return offsets, vertices, ks, centers, adjacency


def _polygons(offsets, vertices, return_dict=False):
    """The reference's return value from the CSR form: the same ``np.array(list, dtype=object)`` call, so polygons of one
    common length come as a 2-D object array, as they do there."""
    polys = np.array([vertices[offsets[f]:offsets[f + 1]] for f in range(len(offsets) - 1)], dtype=object)
    if not return_dict:
        return polys
    ks = np.array([len(e) for e in polys])
    return {str(e): np.vstack(polys[ks == e]) for e in np.unique(ks)}


def find_regions(pts, ijs, return_dict=False):
    """The polygons of the planar graph with nodes ``pts`` ``(N, 2)`` and directed index pairs ``ijs`` ``(E, 2)``: an object
    array of int64 vertex arrays in the reference's order, or with ``return_dict`` a dict ``{str(k): (n_k, k) array}``.
    Pairs are taken as given (duplicates collapse, nothing is symmetrised); a face is found when it can be walked all the way
    round, so dangling bonds and one-directional pairs kill the faces they touch, and the outer face of the component that
    holds the leftmost point is dropped.  Computed on the GPU (see the module docstring for the deviations)."""
    pts, ijs = _check_graph(pts, ijs)
    offsets, vertices = _regions_arrays(pts, ijs)[:2]
    return _polygons(offsets, vertices, return_dict)


# ---------------------------------------------------------------------------------------------------------
# vnn_graph: Voronoi-neighbour bonds (reference graph/vnn.py)
# ---------------------------------------------------------------------------------------------------------
def add_corner_points(pts, pad=0.05):
    """``pts`` with four points appended, ``centre + (-+v, -+v)`` in the order ``(-,-) (+,-) (+,+) (-,+)``, where
    ``centre = pts.mean(axis=0)`` and ``v = max|pts - centre| * (1 + pad)``: they close every Voronoi cell.  Host NumPy."""
    pts = np.asarray(pts)
    center = pts.mean(axis=0)
    v = np.abs(pts - center).max() * (1 + pad)
    return np.vstack([pts, np.array([(-v, -v), (+v, -v), (+v, +v), (-v, +v)]) + center])


def _check_points(pts, pad):
    """``pts`` float64 ``(N, 2)`` C-contiguous, finite and without coincident points, or ValueError; nothing is launched
    before this returns."""
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"pts must have shape (N, 2), not {pts.shape}")
    if pts.dtype.kind not in "fiu":
        raise ValueError(f"pts must be real numbers, not {pts.dtype}")
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if not np.isfinite(pts).all():
        raise ValueError("pts must be finite")
    if len(pts) + 4 >= 2 ** 26:
        raise ValueError("the Voronoi neighbours need len(pts) < 2^26 - 4")
    if len(pts) > 1 and len(np.unique(pts, axis=0)) != len(pts):
        raise ValueError("pts holds coincident points")
    if not (np.isfinite(pad) and pad > 0):
        raise ValueError(f"pad must be positive and finite, not {pad}")
    return pts


def _voronoi_rows(pts, pad, mode, dmax, threshold):
    """``(ijs, ridge, edge)`` of checked host points, from one device call (``ridge`` / ``edge`` only in neighbour mode)."""
    lengths = mode == _native.VORONOI_NEIGHBOURS
    if len(pts) == 0:
        return np.empty((0, 2), np.int64), np.empty(0), np.empty(0)
    lib = _native.load()
    _native.require_device()
    device = _native.default_device()
    state, counts = c_void_p(), (c_int64 * 1)()
    ptr = lambda a: a.ctypes.data_as(c_void_p)
    _native.check(lib.zk_voronoi_cells(device, ptr(pts), _native.ZK_F64, len(pts), pad, mode, dmax, threshold, byref(state), counts,
                                       None, None, None), "zk_voronoi_cells")
    m = int(counts[0])
    ijs, ridge, edge = np.empty((m, 2), np.int64), np.empty(m if lengths else 0), np.empty(m if lengths else 0)
    _native.check(lib.zk_voronoi_cells(device, None, _native.ZK_F64, 0, pad, mode, dmax, threshold, byref(state), counts, ptr(ijs),
                                       ptr(ridge) if lengths else None, ptr(edge) if lengths else None), "zk_voronoi_cells")
    return ijs, ridge, edge


def voronoi_neighbours(pts, pad=0.05):
    """``(ijs, ridge_lengths, edge_lengths)``: for every point ``i`` every point ``j`` whose Voronoi cells share a ridge of
    positive length in the diagram of ``add_corner_points(pts, pad)``.  ``ijs`` is int64 ``(M, 2)``, sorted lexicographically,
    every pair in both directions; ``ridge_lengths[m]`` is the float64 length of the ridge as computed in the cell of ``i``,
    ``edge_lengths[m]`` is ``hypot(dx, dy)``.  Not a reference function: it is what ``vnn_graph`` is made of, and a source of
    ``dmax`` (a multiple of ``np.median(edge_lengths)``).  Computed on the GPU; centre and ``v`` of the corner points are
    reduced there and may differ from NumPy's by rounding."""
    pts = _check_points(pts, pad)
    return _voronoi_rows(pts, float(pad), _native.VORONOI_NEIGHBOURS, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------
# estimate_d: the bond length (reference graph/vnn.py:18-40)
# ---------------------------------------------------------------------------------------------------------
KNN = 12                                             # columns of the distance matrix: self and eleven neighbours
KS = tuple(range(2, KNN + 1))                        # the reference's ks
LI_MAX_ITERATIONS = 1000


def _check_knn_points(pts, k):
    """``pts`` float64 ``(N, 2)`` C-contiguous and finite with ``N >= k``, or ValueError; nothing is launched before this."""
    pts = np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"pts must have shape (N, 2), not {pts.shape}")
    if pts.dtype.kind not in "fiu":
        raise ValueError(f"pts must be real numbers, not {pts.dtype}")
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if not np.isfinite(pts).all():
        raise ValueError("pts must be finite")
    if not 1 <= k <= KNN:
        raise ValueError(f"k must be in [1, {KNN}], not {k}")
    if len(pts) < k:                                 # scikit-learn's kneighbors raises the same way
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {k}, n_samples_fit = {len(pts)}")
    if len(pts) >= 2 ** 26:
        raise ValueError("the neighbour distances need len(pts) < 2^26")
    return pts


def knn_distances(pts, k=12):
    """float64 ``(N, k)``: the ``k <= 12`` smallest Euclidean distances of every point to the points of ``pts``, itself included
    (column 0 is 0), ascending -- ``NearestNeighbors(k).fit(pts).kneighbors(pts)[0]``.  Computed on the GPU on a uniform grid
    of bins (``zk_knn_distances``); ``N < k`` raises ``ValueError`` as scikit-learn does."""
    k = int(k)
    pts = _check_knn_points(pts, k)
    lib = _native.load()
    _native.require_device()
    out = np.empty((len(pts), k), np.float64)
    _native.check(lib.zk_knn_distances(_native.default_device(), pts.ctypes.data_as(c_void_p), _native.ZK_F64, len(pts), k,
                                       out.ctypes.data_as(c_void_p)), "zk_knn_distances")
    return out


def _knn_stats(device, dd_ptr, n, op, params, stream):
    """``(counts int64 (11 * 256), sums float64 (22))`` of one ``zk_knn_stats_dev`` call on a resident distance matrix."""
    counts, sums = np.zeros(len(KS) * 256, np.int64), np.zeros(2 * len(KS), np.float64)
    params = np.ascontiguousarray(params, dtype=np.float64)
    _native.check(_native.load().zk_knn_stats_dev(device, c_void_p(dd_ptr), n, op, params.ctypes.data_as(c_void_p),
                                                  counts.ctypes.data_as(c_void_p), sums.ctypes.data_as(c_void_p), c_void_p(stream)),
                  "zk_knn_stats_dev")
    return counts, sums


def _otsu_from_counts(counts, edges):
    """Otsu's threshold of a histogram: the centre of the bin that maximises the between-class variance."""
    centers = (edges[:-1] + edges[1:]) / 2
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / w1
    m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
    return centers[np.argmax(w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2)]


def _otsu_thresholds(stats, first, lasts, parts):
    edges = [np.linspace(first, last if last > first else first + 1.0, 257) for last in lasts]
    params = np.concatenate([[first], [e[-1] for e in edges]] + edges)
    counts = stats(_native.KNN_HIST, params)[0].reshape(len(KS), 256)
    parts["counts"] = counts
    return [first if last == first else _otsu_from_counts(counts[c], edges[c]) for c, last in enumerate(lasts)]


def _li_thresholds(stats, n, first, lasts, parts):
    lens = np.array([n * (k - 1) for k in KS], np.float64)
    tol = stats(_native.KNN_GAPS, [first])[1][:len(KS)] / 2
    flat = np.array([last == first for last in lasts])                 # all values equal: that value is the threshold
    total = stats(_native.KNN_SIDES, [first] + [np.inf] * len(KS))[1][1::2]
    t_next, t_curr = total / lens, -2 * tol
    active, iterations = ~flat, np.zeros(len(KS), np.int64)
    with np.errstate(all="ignore"):
        while True:
            active &= np.abs(t_next - t_curr) > tol
            if not active.any():
                break
            if iterations.max() >= LI_MAX_ITERATIONS:
                raise RuntimeError(f"estimate_d: Li's iteration has not ended after {LI_MAX_ITERATIONS} steps (on a perfect lattice the "
                                   "gaps between distinct distances are rounding noise: jitter the points or use threshold='otsu')")
            t_curr = np.where(active, t_next, t_curr)
            counts, sums = stats(_native.KNN_SIDES, np.concatenate([[first], t_curr]))
            above = counts[:len(KS)].astype(np.float64)
            mean_fore, mean_back = sums[0::2] / above, sums[1::2] / (lens - above)
            iterations += active
            active &= mean_back != 0
            step = (mean_back - mean_fore) / (np.log(mean_back) - np.log(mean_fore))
            t_next = np.where(active, step, t_next)
    parts["iterations"], parts["tolerance"] = iterations, tol
    return [first if flat[c] else t_next[c] + first for c in range(len(KS))]


def _estimate_from_distances(device, dd_ptr, n, stream, threshold):
    """The reference's rule on a resident ``(n, 12)`` distance matrix; returns the parts ``estimate_d`` is made of."""
    stats = lambda op, params: _knn_stats(device, dd_ptr, n, op, params, stream)
    ranges = stats(_native.KNN_RANGES, [0.0])[1]
    first, lasts = ranges[0], ranges[1:KNN]
    parts = {"first": first, "lasts": lasts}
    ts = _otsu_thresholds(stats, first, lasts, parts) if threshold == 'otsu' else _li_thresholds(stats, n, first, lasts, parts)
    ts = np.array(ts, np.float64)
    above = stats(_native.KNN_SIDES, np.concatenate([[0.0], ts]))[0][:len(KS)]
    lens = np.array([n * (k - 1) for k in KS])
    scores = (above / lens) * ((lens - above) / lens)
    best = int(np.argmax(scores))
    parts.update(ts=ts, above=above, scores=scores, t=float(ts[best]), k=KS[best])
    return parts


def _estimate_d_parts(pts, threshold='otsu'):
    """``estimate_d`` with everything it is made of (``ts``, ``scores``, ``counts`` or ``iterations``, ``dd``): what the tests
    and tools/time_refine.py read."""
    pts = _check_knn_points(pts, KNN)
    _native.require_device()
    device = _native.default_device()
    d_pts = _native.DeviceArray.from_numpy(pts, device)
    dd = _native.DeviceArray((len(pts), KNN), np.float64, device)
    _native.check(_native.load().zk_knn_distances_dev(device, c_void_p(d_pts.data_ptr()), _native.ZK_F64, len(pts), KNN,
                                                      c_void_p(dd.data_ptr()), c_void_p(0)), "zk_knn_distances_dev")
    parts = _estimate_from_distances(device, dd.data_ptr(), len(pts), 0, threshold)
    parts["dd"] = dd
    return parts


def estimate_d(pts, threshold='otsu', return_k=False):
    """The reference's ``estimate_d``: the bond length of a point set.  For every ``k = 2 .. 12`` the distances of all points
    to their ``k - 1`` nearest neighbours are thresholded -- ``threshold='otsu'``: Otsu on a 256-bin histogram; anything else:
    Li's minimum cross-entropy, as in the reference -- and the threshold whose two sides are most even
    (``count(d > t) count(d <= t) / len(d)^2``, first maximum) is returned, with ``return_k`` together with its ``k``.
    Computed on the GPU (see the module docstring: which passes, and that parity with scikit-image is unpinned).  ``N < 12``
    raises ``ValueError`` as scikit-learn's query does.  Li needs points that are not a perfect lattice."""
    parts = _estimate_d_parts(pts, threshold)
    return (parts["t"], parts["k"]) if return_k else parts["t"]


def vnn_graph(pts, threshold=0.1, dmax=None, threshold_method=None, return_ijs=True):
    """The reference's ``vnn_graph``: bonds between Voronoi neighbours.  With ``R_i`` the Voronoi neighbours of point ``i``
    (the four corner points included) closer than ``dmax``, the entry ``(i, j)`` is kept when ``j`` is a point of ``R_i`` and its
    ridge is at least ``threshold`` of the summed ridge lengths of ``R_i``; the result is every pair kept in either direction, in
    both directions: int64 ``(E, 2)`` sorted lexicographically, or with ``return_ijs=False`` the SciPy CSR matrix of ones of
    shape ``(N, N)``.  Computed on the GPU.  Without ``dmax`` it is ``estimate_d(pts, threshold=threshold_method)``, as in the
    reference (``None`` means Li there, and here).

    Deviations from the reference, each a ``ValueError`` before any launch: ``threshold`` must be ``> 0``; ``pts`` must
    be finite ``(N, 2)`` (converted to float64) without coincident points; ``N == 0`` returns the empty ``(0, 2)`` array."""
    if dmax is None:
        if np.ndim(pts) == 2 and len(pts) < KNN:     # scikit-learn's refusal, with the way out
            raise ValueError(f"vnn_graph without dmax estimates it from the {KNN} nearest neighbours (estimate_d): Expected n_neighbors <= "
                             f"n_samples_fit, but n_neighbors = {KNN}, n_samples_fit = {len(pts)}; pass dmax, e.g. "
                             "1.3 * np.median(voronoi_neighbours(pts)[2])")
        dmax = estimate_d(pts, threshold=threshold_method)
    dmax, threshold = float(dmax), float(threshold)
    if not dmax > 0:
        raise ValueError(f"dmax must be positive, not {dmax}")
    if not threshold > 0:
        raise ValueError(f"threshold must be > 0, not {threshold}")
    pts = _check_points(pts, 0.05)
    ijs = _voronoi_rows(pts, 0.05, _native.VORONOI_GRAPH, dmax, threshold)[0]
    if return_ijs:
        return ijs
    from scipy.sparse import csr_matrix
    return csr_matrix((np.ones(len(ijs), np.int64), (ijs[:, 0], ijs[:, 1])), shape=(len(pts), len(pts)))


# ---------------------------------------------------------------------------------------------------------
# graph classes (reference graph/planar_graph.py, graph/_lattice_graph.py)
# ---------------------------------------------------------------------------------------------------------
class PlanarGraphBase:
    """Attribute aliases shared by the graph classes: ``pts`` / ``vertices`` are ``nodes``, ``ijs`` is ``edges``,
    ``polys`` / ``faces`` / ``polygons`` are ``regions``.  A subclass sets ``nodes`` and ``edges``."""

    aliases = {"polys": "regions", "faces": "regions", "polygons": "regions", "pts": "nodes", "vertices": "nodes", "ijs": "edges"}

    def __post_init__(self):
        for attr in ("nodes", "edges"):
            if not hasattr(self, attr):
                raise AttributeError(f"Missing attribute: '{attr}'")

    def __setattr__(self, name, value):
        object.__setattr__(self, self.aliases.get(name, name), value)

    def __getattr__(self, name):
        if name == "aliases":
            raise AttributeError(name)
        return object.__getattribute__(self, self.aliases.get(name, name))


class PlanarGraph(PlanarGraphBase):
    """Nodes ``(N, 2)`` and edges, the edges made symmetric (``symmetric_edges``); ``matrix`` (sparse adjacency), ``lil``
    (neighbour lists) and ``degs`` are derived on first use."""

    def __init__(self, nodes, edges):
        self.nodes = nodes
        self.edges = symmetric_edges(edges)
        self._matrix = None
        self._lil = None
        self._degs = None
        super().__post_init__()

    @property
    def matrix(self):
        if self._matrix is None:
            self._matrix = edges2matrix(self.edges, shape=(len(self.nodes), len(self.nodes)))
        return self._matrix

    @property
    def lil(self):
        if self._lil is None:
            self._lil = matrix2lil(self.matrix)
        return self._lil

    @property
    def degs(self):
        if self._degs is None:
            self._degs = np.array(np.sum(self.matrix, axis=1)).ravel()
        return self._degs

    def is_symmetric(self, tol=1e-8):
        diff = abs((self.matrix - self.matrix.T).tocsr())
        return bool(diff.nnz == 0 or diff.max() < tol)


class LatticeGraph(PlanarGraph):
    """A lattice of atoms and bonds.  ``regions``, ``centers`` and ``ks`` (and the region adjacency ``to_motifs_graph`` uses)
    come from ONE device call, made on first use of any of them and cached."""

    def __init__(self, nodes, edges, img=None, lbs=None):
        super().__init__(nodes, edges)
        self.img = img
        self.lbs = self.degs if lbs is None else lbs
        self._regions = None
        self._centers = None
        self._ks = None
        self._adjacency = None
        super().__post_init__()

    def _compute(self):
        if self._regions is None:
            pts, ijs = _check_graph(self.nodes, self.edges)
            offsets, vertices, ks, centers, adjacency = _regions_arrays(pts, ijs)
            self._regions, self._centers, self._ks, self._adjacency = _polygons(offsets, vertices), centers, ks, adjacency

    @property
    def regions(self):
        self._compute()
        return self._regions

    @property
    def centers(self):
        self._compute()
        return self._centers

    @property
    def ks(self):
        self._compute()
        return self._ks

    @property
    def is_loop(self):
        return np.all(self.degs == 2)

    @property
    def is_chain(self):
        return sum(self.degs) == 2 * (len(self.degs) - 1)

    def get_node_motifs(self):
        """Per node, the sizes of the regions it is a vertex of (in region order)."""
        out = [[] for _ in range(len(self.nodes))]
        for region in self.regions:
            for i in np.unique(np.asarray(region).astype(int)):
                out[i].append(len(region))
        return out

    def to_motifs_graph(self):
        motifs = np.array([construct_motif(np.asarray(self.pts)[np.asarray(region).astype(int)]) for region in self.regions], dtype=object)
        self._compute()
        return MotifsGraph(motifs, self.centers, self._adjacency)

    def get_level1(self):
        return self.lbs

    def get_level2(self):
        return [self.lbs[row] for row in self.lil]

    def _subgraph(self, mask):
        from scipy.sparse import lil_matrix
        ijs = matrix2edges(lil_matrix(self.matrix)[mask, :][:, mask])
        return LatticeGraph(self.nodes[mask], ijs, lbs=None if self.lbs is None else self.lbs[mask])

    def decompose(self, min_nodes=4):
        """One :class:`LatticeGraph` per connected component of at least ``min_nodes`` nodes."""
        from scipy.sparse.csgraph import connected_components
        n_components, lbs = connected_components(self.matrix, directed=False)
        return [self._subgraph(lbs == e) for e in range(n_components) if (lbs == e).sum() >= min_nodes]

    def remove_nodes(self, mask):
        """The graph of the nodes ``mask`` keeps."""
        return self._subgraph(mask)


LatticeGraph1 = LatticeGraph


class Motif(PlanarGraphBase):
    """One ring: its points and its (symmetric) edges.  ``a + b`` merges two motifs on their shared points."""

    def __init__(self, nodes, edges):
        self.nodes = nodes
        self.edges = symmetric_edges(edges)
        super().__post_init__()

    def __add__(self, other):
        edge_pts = np.vstack([self.pts[self.edges].reshape(-1, 2), other.pts[other.edges].reshape(-1, 2)])
        pts = np.unique(np.vstack([self.pts, other.pts]), axis=0)
        ijs = np.empty(len(edge_pts))
        for i, p in enumerate(pts):
            ijs[(edge_pts == p).all(axis=1).nonzero()[0]] = i
        return Motif(pts, np.unique(ijs.reshape(-1, 2).astype(int), axis=0))


class MotifsGraph(PlanarGraphBase):
    """The graph whose nodes are regions (``nodes``: their centres, ``motifs``: their rings, ``ks``: their sizes) and whose
    edges join regions that share a bond."""

    def __init__(self, motifs, nodes, edges, lbs=None):
        from scipy.stats import mode
        self.nodes = nodes
        edges = np.asarray(edges).reshape(-1, 2).astype(np.int64)
        self.edges = symmetric_edges(edges)
        self.motifs = motifs
        self.matrix = edges2matrix(self.edges, shape=(len(self.nodes), len(self.nodes)))
        self.degs = np.array(np.sum(self.matrix, axis=1)).ravel()
        self.ks = np.array([len(motif.pts) for motif in self.motifs])
        self.major_k = mode(self.ks)[0]
        self.n_components, self.component_lbs = get_connected_components(self.matrix)
        self.lbs = lbs
        super().__post_init__()

    def _masked(self, mask, lbs=None):
        from scipy.sparse import lil_matrix
        ijs = matrix2edges(lil_matrix(self.matrix)[mask, :][:, mask])
        return MotifsGraph(self.motifs[mask], self.pts[mask], ijs, lbs)

    def _k_mask(self, k):
        if k is None:
            k = [self.major_k]
        elif not np.iterable(k):
            k = [k]
        return np.isin(self.ks, k)

    def select(self, k=None):
        return self._masked(self._k_mask(k))

    def select_nodes(self, mask=None, k=None):
        if mask is None:
            mask = self._k_mask(k)
        return self._masked(mask, None if self.lbs is None else self.lbs[mask])

    def find_n_nodes(self, n=3):
        return find_n_nodes(self.edges, n=n)

    def select_connections(self, k1k2):
        mask = np.isin(cantor_pairing(self.ks[self.ijs]), cantor_pairing(k1k2))
        return MotifsGraph(self.motifs, self.pts, self.ijs[mask])

    def remove_edges(self, mask):
        return MotifsGraph(self.motifs, self.pts, self.ijs[mask])
