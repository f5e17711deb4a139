"""NumPy-only brute-force restatement of ``mtflearn_amd.graph.voronoi_neighbours`` / ``vnn_graph``: TEST INFRASTRUCTURE.

Every cell is clipped against ALL other points (the four corner points included): no bins, no search radius, no qhull.  The cell
of point ``i`` starts as a square far larger than the whole set; among the points whose bisector still cuts the current
polygon -- all of them are tested, every time -- the nearest one clips it, until none cuts.  Every vertex is then the
intersection of the two bisectors that meet in it, solved in coordinates relative to the point, so the starting square leaves
no trace in the ridge lengths."""
import numpy as np


def add_corner_points(pts, pad=0.05):
    """The reference's formula (graph/vnn.py, ``add_corner_points``), restated."""
    pts = np.asarray(pts, dtype=np.float64)
    center = pts.mean(axis=0)
    vmax = np.abs(pts - center).max() * (1 + pad)
    corners = np.array([(-vmax, -vmax), (+vmax, -vmax), (+vmax, +vmax), (-vmax, +vmax)])
    return np.vstack([pts, corners + center])


def _clip(poly, ids, q, qid):
    """``poly`` (n, 2) counter-clockwise with ``ids[t]`` behind the edge that leaves vertex ``t``, cut by ``x . q <= |q|^2 / 2``."""
    d = poly @ q - 0.5 * (q @ q)
    new_poly, new_ids = [], []
    n = len(poly)
    for t in range(n):
        u = (t + 1) % n
        if d[t] <= 0:
            new_poly.append(poly[t])
            new_ids.append(ids[t])
        if (d[t] <= 0) != (d[u] <= 0):
            new_poly.append(poly[t] + d[t] / (d[t] - d[u]) * (poly[u] - poly[t]))
            new_ids.append(qid if d[t] <= 0 else ids[t])      # leaving: the new edge starts here; entering: the old one goes on
    return np.array(new_poly), new_ids


def cell(all_pts, i):
    """``(ids, vertices)`` of the Voronoi cell of point ``i`` among ``all_pts``: vertex ``t`` in coordinates relative to the
    point, ``ids[t]`` the neighbour behind the edge from vertex ``t`` to vertex ``t + 1``."""
    rel = np.delete(all_pts - all_pts[i], i, axis=0)
    idx = np.delete(np.arange(len(all_pts)), i)
    order = np.argsort((rel * rel).sum(axis=1), kind="stable")
    rel, idx = rel[order], idx[order]
    half_norm = 0.5 * (rel * rel).sum(axis=1)
    big = 64 * np.abs(all_pts - all_pts[i]).max()
    poly, ids = np.array([(-big, -big), (big, -big), (big, big), (-big, big)]), [-1, -1, -1, -1]
    fresh = np.ones(len(rel), dtype=bool)            # a point clips once: the vertices it made lie on its bisector up to rounding
    while True:
        cuts = fresh & ((rel @ poly.T) - half_norm[:, None] > 0).any(axis=1)
        if not cuts.any():
            break
        k = int(np.argmax(cuts))                     # the nearest point that still cuts
        fresh[k] = False
        poly, ids = _clip(poly, ids, rel[k], int(idx[k]))
    assert min(ids) >= 0, "the cell is not bounded by the points"
    where = {int(j): r for j, r in zip(idx, rel)}
    verts = np.empty((len(ids), 2))
    for t in range(len(ids)):
        a, b = where[ids[t - 1]], where[ids[t]]
        verts[t] = np.linalg.solve(np.array([a, b]), np.array([0.5 * (a @ a), 0.5 * (b @ b)]))
    return ids, verts


def rows(pts, pad=0.05):
    """Per real point ``i`` the list of ``(j, ridge length, edge length)`` over ALL its neighbours ``j`` (``j >= N``: a corner
    point) with a ridge of positive length, in ascending ``j``."""
    pts = np.asarray(pts, dtype=np.float64)
    if len(pts) <= 1:
        return [[] for _ in pts]                     # one point: the four corner points coincide with it, there is no diagram
    all_pts = add_corner_points(pts, pad)
    out = []
    for i in range(len(pts)):
        ids, verts = cell(all_pts, i)
        edge = np.roll(verts, -1, axis=0) - verts
        ridge = np.hypot(edge[:, 0], edge[:, 1])
        d = all_pts[ids] - all_pts[i]
        out.append(sorted((j, float(l), float(l1)) for j, l, l1 in zip(ids, ridge, np.hypot(d[:, 0], d[:, 1])) if l > 0))
    return out


def neighbours_from_rows(all_rows, n):
    got = [(i, j, l, l1) for i, row in enumerate(all_rows) for j, l, l1 in row if j < n]
    ijs = np.array([(i, j) for i, j, _, _ in got], dtype=np.int64).reshape(-1, 2)
    return ijs, np.array([g[2] for g in got], dtype=np.float64), np.array([g[3] for g in got], dtype=np.float64)


def graph_from_rows(all_rows, n, threshold, dmax):
    """``(ijs, directed, fractions)``: the symmetrised sorted pairs, the set of directed entries kept before the OR, and
    ``{(i, j): L_ij / sum}`` of every real entry with ``L1 < dmax``."""
    directed, fractions = set(), {}
    for i, row in enumerate(all_rows):
        near = [(j, l) for j, l, l1 in row if l1 < dmax]
        total = sum(l for _, l in near)
        for j, l in near:
            if j < n:
                fractions[(i, j)] = l / total
                if l / total >= threshold:
                    directed.add((i, j))
    pairs = sorted(directed | {(j, i) for i, j in directed})
    return np.array(pairs, dtype=np.int64).reshape(-1, 2), directed, fractions


def voronoi_neighbours(pts, pad=0.05):
    return neighbours_from_rows(rows(pts, pad), len(pts))


def vnn_graph(pts, threshold=0.1, dmax=None, pad=0.05):
    return graph_from_rows(rows(pts, pad), len(pts), threshold, dmax)[0]
