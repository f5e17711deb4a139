#!/usr/bin/env python3
"""Generate tests/golden/vnn_golden.npz from SciPy's qhull: what the REFERENCE's ``graph/vnn.py::vnn_graph`` returns with
``dmax`` given, and the Voronoi neighbours it is made of.

TEST INFRASTRUCTURE.  The reference's module imports scikit-image at its top and cannot be imported here, so ``qhull_rows`` and
``reference_graph`` restate it step by step (no text of it is copied):

  vnn.py 81-87    the diagram of ``add_corner_points(pts)``: ``scipy.spatial.Voronoi`` and its ``ridge_points`` / ``ridge_vertices``
  vnn.py 89-95    ridge length ``L`` = hypot of the two ridge vertices' difference, edge length ``L1`` = hypot of the two points'
  vnn.py 97-107   the ridges with ``L1 < dmax`` as a sparse matrix of ``L``, copied to both triangles (every ridge is listed once)
  vnn.py 109-113  rows divided by their sum (``normalize(norm='l1')``), ``>= threshold``, then OR with the transpose
  vnn.py 117-120  the last four rows and columns (the corner points) dropped, the pairs in row-major order

A ridge with a vertex at infinity joins two corner points (every cell of a real point is bounded), so it only ever enters rows
that are dropped; it is left out here.  One point alone has no diagram (its four corner points coincide with it and qhull
refuses them): the golden is the empty list.

Per case (inputs are not stored, tests/vnn_cases.py regenerates them): ``ijs`` the graph, ``nb_ijs`` / ``nb_ridge`` / ``nb_edge``
the neighbour rows between real points, ``a`` the median edge length.  ``d0`` is the largest difference between qhull's ridge
lengths and those of tests/vnn_oracle.py over all rows of all cases (corner neighbours included), in units of ``a``; the ridge
tolerance of the tests is ``tol = max(100 d0, 1e-12) a``, the rule of the denoise goldens.  It is written to the file and to
DESIGN.md.  The conditioning of every case is asserted: ridges between real points ``>= 1e-6 a``, ``|L1 - dmax| >= 1e-6 dmax``
on every edge, ``|fraction - threshold| >= 1e-6`` on every directed entry.

Usage:  python tests/make_golden_vnn.py
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "vnn_golden.npz")
DESIGN = os.path.join(HERE, "..", "DESIGN.md")
sys.path.insert(0, HERE)

import vnn_cases as vc          # noqa: E402
import vnn_oracle as oracle     # noqa: E402

MARGIN = 1e-6


def qhull_rows(pts, pad=vc.PAD):
    """Per real point the sorted ``(j, L, L1)`` of every finite ridge of its cell, from qhull."""
    from scipy.spatial import Voronoi
    n = len(pts)
    if n <= 1:
        return [[] for _ in range(n)]
    all_pts = oracle.add_corner_points(pts, pad)
    vor = Voronoi(all_pts)
    rows = [[] for _ in range(n)]
    for (i, j), (u, v) in zip(vor.ridge_points, vor.ridge_vertices):
        if u < 0 or v < 0:
            assert i >= n and j >= n, "an unbounded ridge at a real point"
            continue
        d = vor.vertices[u] - vor.vertices[v]
        e = vor.points[i] - vor.points[j]
        length, l1 = float(np.hypot(d[0], d[1])), float(np.hypot(e[0], e[1]))
        if i < n:
            rows[i].append((int(j), length, l1))
        if j < n:
            rows[j].append((int(i), length, l1))
    return [sorted(r) for r in rows]


def reference_graph(rows, n, threshold, dmax):
    """vnn.py 97-120 on the rows of the real points (the corner points' own rows are dropped there)."""
    from scipy.sparse import coo_matrix
    trip = [(i, j, l) for i, row in enumerate(rows) for j, l, l1 in row if l1 < dmax]
    if not trip:
        return np.empty((0, 2), np.int64), set(), {}
    i, j, l = (np.array(c) for c in zip(*trip))
    matrix = coo_matrix((l.astype(np.float64), (i, j)), shape=(n, n + 4)).tocsr()
    sums = np.asarray(matrix.sum(axis=1)).ravel()
    matrix = matrix.tocoo()
    frac = matrix.data / sums[matrix.row]
    real = matrix.col < n
    fractions = {(int(a), int(b)): float(f) for a, b, f in zip(matrix.row[real], matrix.col[real], frac[real])}
    directed = {ab for ab, f in fractions.items() if f >= threshold}
    pairs = sorted(directed | {(b, a) for a, b in directed})
    return np.array(pairs, dtype=np.int64).reshape(-1, 2), directed, fractions


def conditioned(rows, n, threshold, dmax, a):
    """None when the case keeps the margins, else what it misses."""
    for i, row in enumerate(rows):
        for j, l, l1 in row:
            if j < n and l < MARGIN * a:
                return f"ridge ({i}, {j}) of {l / a:.3g} a"
            if abs(l1 - dmax) < MARGIN * dmax:
                return f"edge ({i}, {j}) within {abs(l1 - dmax) / dmax:.3g} of dmax"
    for ij, f in reference_graph(rows, n, threshold, dmax)[2].items():
        if abs(f - threshold) < MARGIN:
            return f"fraction {ij} within {abs(f - threshold):.3g} of the threshold"
    return None


def median_edge(rows, n):
    edges = [l1 for row in rows for j, _, l1 in row if j < n]
    return float(np.median(edges)) if edges else 1.0


def build(verbose=False):
    """Every array of the golden file, and ``{name: oracle rows}`` for the tests that compare the two."""
    out, oracle_rows, d0 = {}, {}, 0.0
    cache = {}
    for name, (pts, dmax, threshold) in vc.cases().items():
        n = len(pts)
        if id(pts) not in cache:
            cache[id(pts)] = (qhull_rows(pts), oracle.rows(pts))
        rows, orows = cache[id(pts)]
        oracle_rows[name] = orows
        a = median_edge(rows, n)
        why = conditioned(rows, n, threshold, dmax, a)
        assert why is None, (name, why)
        for row, orow in zip(rows, orows):
            assert [r[0] for r in row] == [r[0] for r in orow], (name, "the oracle and qhull disagree on a cell's neighbours")
            d0 = max([d0] + [abs(r[1] - o[1]) / a for r, o in zip(row, orow)])
        ijs = reference_graph(rows, n, threshold, dmax)[0]
        nb = [(i, j, l, l1) for i, row in enumerate(rows) for j, l, l1 in row if j < n]
        out[f"{name}/ijs"] = ijs.astype(np.int32)
        out[f"{name}/nb_ijs"] = np.array([(i, j) for i, j, _, _ in nb], dtype=np.int32).reshape(-1, 2)
        out[f"{name}/nb_ridge"] = np.array([g[2] for g in nb], dtype=np.float64)
        out[f"{name}/nb_edge"] = np.array([g[3] for g in nb], dtype=np.float64)
        out[f"{name}/a"] = np.float64(a)
        if verbose:
            print(f"{name}: {n} points, {len(nb)} neighbour rows, {len(ijs)} graph rows, a = {a:.4f}")
    # the two wheels are what their names say: the hub (point 0) has 24 sides, and more than the cap
    assert sum(j < 25 for j, _, _ in cache[id(vc.cases()["wheel_24"][0])][0][0]) == 24
    assert sum(j < len(vc.OVER_CAP) for j, _, _ in qhull_rows(vc.OVER_CAP)[0]) > vc.CAP
    # one_way: the first threshold at which a pair survives in one direction only
    pts, dmax, _ = vc.cases()[vc.ONE_WAY_POINTS]
    rows, n = cache[id(pts)][0], len(pts)
    for threshold in vc.ONE_WAY_THRESHOLDS:
        ijs, directed, _ = reference_graph(rows, n, threshold, dmax)
        lonely = [ij for ij in directed if ij[::-1] not in directed]
        if lonely and conditioned(rows, n, threshold, dmax, median_edge(rows, n)) is None:
            break
    else:
        raise AssertionError("one_way: no threshold keeps a pair in one direction only")
    out["one_way/threshold"], out["one_way/ijs"], out["one_way/lonely"] = np.float64(threshold), ijs.astype(np.int32), np.int32(len(lonely))
    oracle_rows["one_way"] = oracle_rows[vc.ONE_WAY_POINTS]
    if verbose:
        print(f"one_way: threshold {threshold}, {len(lonely)} one-directional entries, {len(ijs)} graph rows")
    out["d0"] = np.float64(d0)
    out["tol_rel"] = np.float64(max(100 * d0, 1e-12))
    return out, oracle_rows


def main():
    out, _ = build(verbose=True)
    np.savez_compressed(OUT, **out)
    print(f"d0 = {out['d0']:.3g}, tol = {out['tol_rel']:.3g} a; wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")
    with open(DESIGN) as f:
        text = f.read()
    new, count = re.subn(r"(<!-- vnn-d0 -->).*?(<!-- /vnn-d0 -->)", rf"\g<1>d0 = {out['d0']:.2e}, tol = {out['tol_rel']:.2e} a\g<2>", text)
    if count and new != text:
        with open(DESIGN, "w") as f:
            f.write(new)


if __name__ == "__main__":
    main()
