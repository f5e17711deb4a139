"""The vnn_graph goldens without a GPU: the brute-force oracle (tests/vnn_oracle.py) against the qhull restatement
(tests/make_golden_vnn.py) on every case of tests/vnn_cases.py, the generator against the committed file, ``add_corner_points``
against the restated formula, and the argument errors that are raised before any launch.

For tests/test_gpu_points_kernels.py, which holds the device to the oracle alone: on the Voronoi sets and the wheels of
tests/point_cases.py the oracle's cells are qhull's, the sets keep the generator's margins at ``dmax = 1.3 a``, and what the two
differ by in ridge length stays within a hundredth of the stored tolerance (``d0_new``, printed, recorded in DESIGN.md).

The generator is run once per module (``built``); its conditioning asserts (ridges, ``dmax`` and ``threshold`` margins of 1e-6)
run with it."""
import os

import numpy as np
import pytest

import make_golden_vnn as gen
import point_cases as pc
import vnn_cases as vc
import vnn_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph


@pytest.fixture(scope="module")
def committed():
    with np.load(os.path.join(ROOT, "tests", "golden", "vnn_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def built():
    return gen.build()


def case_of(name, committed):
    if name == "one_way":
        pts, dmax, _ = vc.cases()[vc.ONE_WAY_POINTS]
        return pts, dmax, float(committed["one_way/threshold"])
    return vc.cases()[name]


def test_generator_reproduces_the_committed_file(built, committed):
    out = built[0]
    assert sorted(out) == sorted(committed)
    for key, value in out.items():
        value = np.asarray(value)
        assert value.dtype == committed[key].dtype and value.shape == committed[key].shape, key
        if key in ("d0", "tol_rel"):                                     # a measurement of qhull's rounding, not an output
            continue
        assert np.array_equal(value, committed[key]), key
    assert out["d0"] <= committed["tol_rel"] / 100 or committed["tol_rel"] == 1e-12
    assert int(committed["one_way/lonely"]) >= 1


@pytest.mark.parametrize("name", vc.NAMES + ("one_way",))
def test_oracle_equals_qhull(built, committed, name):
    pts, dmax, threshold = case_of(name, committed)
    rows = built[1][name]
    n = len(pts)
    ijs, ridge, edge = oracle.neighbours_from_rows(rows, n)
    points_name = vc.ONE_WAY_POINTS if name == "one_way" else name
    assert {tuple(r) for r in ijs.tolist()} == {tuple(r) for r in committed[f"{points_name}/nb_ijs"].tolist()}
    assert np.array_equal(ijs, committed[f"{points_name}/nb_ijs"])         # both sorted lexicographically
    tol = float(committed["tol_rel"]) * float(committed[f"{points_name}/a"])
    worst = np.abs(ridge - committed[f"{points_name}/nb_ridge"]).max() if len(ridge) else 0.0
    print(f"{name}: ridge lengths differ by at most {worst:.3g}, tol {tol:.3g}")
    assert worst <= tol
    assert np.array_equal(edge, committed[f"{points_name}/nb_edge"])
    graph_ijs = oracle.graph_from_rows(rows, n, threshold, dmax)[0]
    assert np.array_equal(graph_ijs, committed[f"{name}/ijs"])
    both = {tuple(r) for r in graph_ijs.tolist()}
    assert all((j, i) in both for i, j in both)


def new_sets():
    out = dict(pc.voronoi_sets())
    out.update({f"wheel_{s}": pc.wheel(s) for s in pc.WHEEL_SPOKES})
    return out


@pytest.mark.parametrize("name", tuple(new_sets()))
def test_oracle_equals_qhull_on_the_edge_sets(committed, name):
    pts = new_sets()[name]
    n = len(pts)
    rows, orows = gen.qhull_rows(pts), oracle.rows(pts)
    assert [[r[0] for r in row] for row in rows] == [[r[0] for r in row] for row in orows]
    a = gen.median_edge(orows, n)
    assert a == np.median(oracle.neighbours_from_rows(orows, n)[2])
    dmax = pc.DMAX_FACTOR * a
    assert gen.conditioned(orows, n, pc.THRESHOLD, dmax, a) is None and gen.conditioned(rows, n, pc.THRESHOLD, dmax, a) is None
    d0_new = max(abs(r[1] - o[1]) / a for row, orow in zip(rows, orows) for r, o in zip(row, orow))
    print(f"{name}: {n} points, a = {a:.4g}, d0_new = {d0_new:.3g} (tol_rel {float(committed['tol_rel']):.3g})")
    assert 100 * d0_new <= float(committed["tol_rel"]), name
    assert max(abs(r[2] - o[2]) / np.spacing(r[2]) for row, orow in zip(rows, orows) for r, o in zip(row, orow)) <= 1
    assert np.array_equal(gen.reference_graph(rows, n, pc.THRESHOLD, dmax)[0], oracle.graph_from_rows(orows, n, pc.THRESHOLD, dmax)[0])
    if name.startswith("wheel_"):
        assert sum(j < n for j, _, _ in rows[0]) == n - 1 == int(name[6:])          # the hub's cell has one side per spoke


def test_add_corner_points_is_the_restated_formula():
    for name in ("n2", "collinear_5", "n65", "honeycomb_392"):
        pts = vc.cases()[name][0]
        for pad in (0.05, 0.25):
            got, want = graph.add_corner_points(pts, pad), oracle.add_corner_points(pts, pad)
            assert got.shape == (len(pts) + 4, 2) and got.tobytes() == want.tobytes(), (name, pad)
    pts = np.array([[0.0, 0.0], [2.0, 1.0]])
    want = np.array([[-0.05, -0.55], [2.05, -0.55], [2.05, 1.55], [-0.05, 1.55]])      # the order (-,-) (+,-) (+,+) (-,+), after the points
    assert np.allclose(graph.add_corner_points(pts)[2:], want, rtol=0, atol=1e-15) and np.array_equal(graph.add_corner_points(pts)[:2], pts)


def test_argument_errors_raise_before_any_launch(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_library)
    pts = vc.cases()["grid_3x3_jittered"][0]
    with pytest.raises(ValueError, match="dmax"):
        graph.vnn_graph(pts)
    with pytest.raises(ValueError, match="median"):
        graph.vnn_graph(pts, threshold_method="li")
    for threshold in (0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            graph.vnn_graph(pts, threshold=threshold, dmax=1.3)
    for bad in (np.zeros((3, 3)), np.zeros(4), np.array([[0.0, np.nan], [1.0, 1.0]]), np.array([[0.0, np.inf], [1.0, 1.0]]),
                np.array([[0.0, 1.0], [2.0, 3.0], [0.0, 1.0]]), np.array([["a", "b"]])):
        with pytest.raises(ValueError):
            graph.vnn_graph(bad, dmax=1.3)
        with pytest.raises(ValueError):
            graph.voronoi_neighbours(bad)
    with pytest.raises(ValueError, match="pad"):
        graph.voronoi_neighbours(pts, pad=0)
    empty = graph.vnn_graph(np.empty((0, 2)), dmax=1.0)
    assert empty.shape == (0, 2) and empty.dtype == np.int64
    ijs, ridge, edge = graph.voronoi_neighbours(np.empty((0, 2)))
    assert ijs.shape == (0, 2) and ijs.dtype == np.int64 and ridge.shape == (0,) and edge.shape == (0,)
    assert graph.vnn_graph(np.empty((0, 2)), dmax=1.0, return_ijs=False).shape == (0, 0)
    assert {"add_corner_points", "voronoi_neighbours", "vnn_graph"} <= set(graph.__all__)
    assert {"vnn_graph_device", "voronoi_neighbours_device"} <= set(distributed.__all__)
