"""Host statement of mtflearn_amd.graph.find_regions, linear in the size of the graph (after its sorts): the yardstick for the
device kernels at sizes the reference's quadratic walk cannot reach, itself held to the reference's goldens by
tests/test_regions_cpu.py.  Written from the contract in include/zernike_hip.h, not from the kernels: the faces are WALKED
here, one after the other, where the device labels and ranks them by pointer doubling.

``regions(pts, ijs) -> (offsets, vertices, ks, centers, adjacency)`` with the meanings of the header."""
import numpy as np

TWO_PI = 2 * np.pi


def wedges(pts, ijs):
    """Sorted wedge rows ``(W, 3)`` of the graph with the grown edge added."""
    n = len(pts)
    i0 = int(np.argmin(pts[:, 0]))
    ext = np.vstack([pts, [pts[i0, 0] - 1, pts[i0, 1]]])
    e = np.unique(np.vstack([ijs.reshape(-1, 2), [[i0, n], [n, i0]]]).astype(np.int64), axis=0)
    d = ext[e[:, 1]] - ext[e[:, 0]]
    theta = (np.arctan2(d[:, 1], d[:, 0]) + TWO_PI) % TWO_PI
    e = e[np.lexsort((e[:, 1], theta, e[:, 0]))]                 # by node, then angle, then neighbour
    start = np.searchsorted(e[:, 0], np.arange(n + 2))
    deg = np.diff(start)
    node, slot = e[:, 0], np.arange(len(e)) - start[e[:, 0]]
    d_of = deg[node]
    prev = e[start[node] + (slot - 1) % d_of, 1]
    rows = np.where((d_of >= 2)[:, None], np.array([prev, node, e[:, 1]]).T, np.array([e[:, 1], np.full(len(e), -1), e[:, 1]]).T)
    lonely = np.flatnonzero(deg == 0)
    rows = np.vstack([rows, np.array([lonely, np.full(len(lonely), -1), np.full(len(lonely), -1)]).T]).astype(np.int64)
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def regions(pts, ijs):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    ijs = np.asarray(ijs, dtype=np.int64).reshape(-1, 2)
    if len(pts) == 0:
        return np.zeros(1, np.int64), np.empty(0, np.int64), np.empty(0, np.int64), np.empty((0, 2)), np.empty((0, 2), np.int64)
    rows = wedges(pts, ijs)
    w_n = len(rows)
    key = rows[:, 0] * (w_n + len(pts) + 2) + rows[:, 1] + 1     # (col0, col1 + 1), unique for col1 != -1, ascending
    want = rows[:, 1] * (w_n + len(pts) + 2) + rows[:, 2] + 1
    at = np.minimum(np.searchsorted(key, want), w_n - 1)
    succ = np.where((rows[:, 1] >= 0) & (key[at] == want), at, -1).tolist()
    col0 = rows[:, 0].tolist()
    seen = [False] * w_n
    polys = []
    for w in range(w_n):                                         # ascending: a cycle is met first at its smallest wedge
        if seen[w]:
            continue
        walk, v = [], w
        while v != -1 and not seen[v]:
            seen[v] = True
            walk.append(col0[v])
            v = succ[v]
        if v == w:                                               # came back to the start: a polygon (anything else is a path)
            polys.append(walk)
    ks = np.array([len(p) for p in polys], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
    vertices = np.array([v for p in polys for v in p], dtype=np.int64)
    centers = np.empty((len(polys), 2))
    xs, ys = pts[:, 0].tolist(), pts[:, 1].tolist()
    for f, p in enumerate(polys):                                # one add after the other, in vertex order
        x = y = 0.0
        for v in p:
            x += xs[v]
            y += ys[v]
        centers[f] = x / len(p), y / len(p)
    half = {}
    for f, p in enumerate(polys):
        for a, b in zip(p, p[1:] + p[:1]):
            half[a, b] = f
    adjacency = np.array([(f, half[b, a]) for (a, b), f in sorted(half.items()) if a < b and (b, a) in half], dtype=np.int64).reshape(-1, 2)
    return offsets, vertices, ks, centers, adjacency


def symmetrised(adjacency):
    """The set of pairs in both directions: the form in which adjacencies are compared (row order is nobody's contract)."""
    a = np.asarray(adjacency, dtype=np.int64).reshape(-1, 2)
    return set(map(tuple, np.vstack([a, a[:, ::-1]]).tolist()))
