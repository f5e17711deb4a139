"""mtflearn_amd.graph.knn_distances / estimate_d and the ``dmax=None`` path of vnn_graph on the GPU, against the goldens of
tests/make_golden_refine.py (scikit-learn's ball tree, ``np.histogram``, tests/thresholds_reference.py) on the point sets of
tests/refine_cases.py.

Criteria: neighbour distances within 1e-12 relative of the golden, zeros exact (whether they came out bit-equal is printed, and
recorded in profiles/refine.txt); the eleven histograms equal to NumPy's count for count; Otsu's eleven thresholds and the
returned ``(t, k)`` bit-equal; Li's eleven thresholds within 1e-12 relative, the same ``k`` and the same iteration counts, on
jittered points only (on a perfect lattice the gaps between distinct distances are rounding noise and the published loop need
not end; a case whose reference stops within 1e-9 of the tolerance boundary is replaced in the golden script)."""
import os

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "estimate_d_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def otsu_parts():
    """One device run per point set, shared by the tests that read it."""
    return {name: graph._estimate_d_parts(pts, "otsu") for name, pts in rc.point_sets().items()}


def resident(a, kind):
    if kind == "native":
        return _native.DeviceArray.from_numpy(a)
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= RTOL * np.abs(want)))      # zeros exact


@pytest.mark.parametrize("name", rc.POINT_SET_NAMES)
def test_knn_distances(golden, name):
    pts, want = rc.point_sets()[name], golden[f"{name}/dd"]
    got = graph.knn_distances(pts)
    assert got.dtype == np.float64 and got.shape == (len(pts), 12)
    worst = np.max(np.abs(got - want) / np.where(want > 0, want, 1.0))
    print(f"{name}: {len(pts)} points, largest relative difference {worst:.3g}, bit-equal: {got.tobytes() == want.tobytes()}")
    assert close(got, want), name
    assert np.all(got[:, 0] == 0) and np.all(np.diff(got, axis=1) >= 0)
    for k in (1, 5):
        assert graph.knn_distances(pts, k=k).tobytes() == np.ascontiguousarray(got[:, :k]).tobytes()
    assert graph.knn_distances(pts).tobytes() == got.tobytes()
    assert graph.knn_distances(pts.astype(np.float32)).shape == got.shape


def test_knn_distances_of_int32_key_points_and_the_refusals(golden):
    pts = np.unique(np.random.default_rng(3).integers(0, 200, (400, 2)), axis=0).astype(np.int32)
    lib, n = _native.load(), len(pts)
    out, want = np.empty((n, 12)), graph.knn_distances(pts.astype(np.float64))
    ptr = lambda a: a.ctypes.data_as(_native.c_void_p)
    _native.check(lib.zk_knn_distances(0, ptr(pts), _native.ZK_I32, n, 12, ptr(out)), "zk_knn_distances")
    assert out.tobytes() == want.tobytes()
    assert lib.zk_knn_distances(0, ptr(pts), _native.ZK_I32, 11, 12, ptr(out)) == _native.ZK_E_BADARG and "k <= n_points" in _native.last_error()
    assert lib.zk_knn_distances(0, ptr(pts), _native.ZK_I32, n, 13, ptr(out)) == _native.ZK_E_BADARG
    assert lib.zk_knn_distances(0, ptr(pts), _native.ZK_F32, n, 12, ptr(out)) == _native.ZK_E_BADARG
    with pytest.raises(ValueError, match="n_neighbors"):
        graph.knn_distances(np.zeros((3, 2)), k=4)
    nan = rc.point_sets()["n13"].copy()
    nan[4, 0] = np.inf
    with pytest.raises(RuntimeError, match="finite"):
        distributed.estimate_d_device(resident(nan, "native"))
    assert close(graph.knn_distances(rc.point_sets()["n13"]), golden["n13/dd"])                      # the library is unharmed


def test_knn_distances_on_a_frame_of_zero_span():
    """A bounding box without extent takes the frame's ``span == 0`` branch (bin side 1); one without extent in x only bins by y
    alone (rc.point_sets() has a set without extent in y, none without extent in x)."""
    got = graph.knn_distances(np.full((12, 2), 3.5))
    assert got.shape == (12, 12) and got.tobytes() == np.zeros((12, 12)).tobytes()
    y = np.cumsum(1 + np.arange(13) % 5 / 8)                                                        # dyadic: every |yi - yj| is exact
    want = np.sort(np.abs(y[:, None] - y[None, :]), axis=1)[:, :12]
    got = graph.knn_distances(np.stack([np.full(13, 7.25), y], axis=1))
    assert got.shape == (13, 12) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("kind", ("native", "torch"))
def test_estimate_d_device_of_int32_points_equals_that_of_the_same_values_in_float64(kind):
    """One loader for both types: int32 pairs are widened exactly, so nothing after the load can differ."""
    pts = np.unique(np.random.default_rng(3).integers(0, 200, (400, 2)), axis=0).astype(np.int32)
    want = distributed.estimate_d_device(resident(pts.astype(np.float64), kind), return_k=True)
    assert distributed.estimate_d_device(resident(pts, kind), return_k=True) == want and want[0] > 0


@pytest.mark.parametrize("name", rc.POINT_SET_NAMES)
def test_histograms_and_otsu(golden, otsu_parts, name):
    parts = otsu_parts[name]
    assert close(parts["dd"].numpy(), golden[f"{name}/dd"])
    flat = parts["lasts"] == parts["first"]
    assert np.array_equal(parts["counts"][~flat], golden[f"{name}/otsu_counts"][~flat]), name
    assert parts["counts"][~flat].sum(axis=1).tolist() == [len(rc.point_sets()[name]) * (k - 1) for k in np.array(graph.KS)[~flat]]
    assert parts["ts"].tobytes() == golden[f"{name}/otsu_ts"].tobytes(), name
    t, k = graph.estimate_d(rc.point_sets()[name], threshold="otsu", return_k=True)
    assert (np.float64(t).tobytes(), k) == (golden[f"{name}/otsu_t"].tobytes(), int(golden[f"{name}/otsu_k"]))
    assert graph.estimate_d(rc.point_sets()[name]) == t                                              # 'otsu' is the default, as in the reference


def test_stats_host_twin_equals_the_resident_call(golden):
    dd, lib = np.ascontiguousarray(golden["honeycomb_257/dd"]), _native.load()
    ptr = lambda a: a.ctypes.data_as(_native.c_void_p)
    d_dd = _native.DeviceArray.from_numpy(dd)
    first, lasts = dd[:, 1].min(), dd[:, 1:].max(axis=0)
    for op, params in ((_native.KNN_RANGES, [0.0]), (_native.KNN_SIDES, [first] + list(np.linspace(0.1, 0.9, 11))), (_native.KNN_GAPS, [first]),
                       (_native.KNN_HIST, np.concatenate([[first], lasts] + [np.linspace(first, last, 257) for last in lasts]))):
        params = np.ascontiguousarray(params, dtype=np.float64)
        counts, sums = np.zeros(11 * 256, np.int64), np.zeros(22)
        _native.check(lib.zk_knn_stats(0, ptr(dd), len(dd), op, ptr(params), ptr(counts), ptr(sums)), "zk_knn_stats")
        c2, s2 = graph._knn_stats(0, d_dd.data_ptr(), len(dd), op, params, 0)
        assert counts.tobytes() == c2.tobytes() and sums.tobytes() == s2.tobytes(), op
        if op == _native.KNN_RANGES:
            assert sums[0] == first and np.array_equal(sums[1:12], lasts)
        if op == _native.KNN_GAPS:
            want = [np.diff(np.unique(dd[:, 1:k] - first)).min() for k in graph.KS]
            assert np.array_equal(sums[:11], want)
        if op == _native.KNN_SIDES:
            w = dd - first
            assert counts[:11].tolist() == [int((w[:, 1:k] > t).sum()) for k, t in zip(graph.KS, params[1:])]
            assert np.allclose(sums[0:22:2] + sums[1:22:2], [w[:, 1:k].sum() for k in graph.KS], rtol=1e-13)
    assert lib.zk_knn_stats(0, ptr(dd), len(dd), 7, None, None, None) == _native.ZK_E_BADARG


@pytest.mark.parametrize("name", rc.LI_SETS)
def test_li(golden, name):
    pts = rc.point_sets()[name]
    parts = graph._estimate_d_parts(pts, "li")
    want = golden[f"{name}/li_ts"]
    print(f"{name}: largest relative difference of the eleven thresholds {np.max(np.abs(parts['ts'] - want) / want):.3g}, iterations "
          f"{parts['iterations'].tolist()}")
    assert close(parts["ts"], want), name
    assert parts["iterations"].tolist() == golden[f"{name}/li_iterations"].tolist()
    t, k = graph.estimate_d(pts, threshold="li", return_k=True)
    assert k == int(golden[f"{name}/li_k"]) and abs(t - float(golden[f"{name}/li_t"])) <= RTOL * float(golden[f"{name}/li_t"])
    assert graph.estimate_d(pts, threshold=None) == t == graph.estimate_d(pts, threshold="anything else")      # Li, as in the reference


@pytest.mark.parametrize("kind", ("native", "torch"))
def test_estimate_d_device_equals_the_host_call(kind):
    pts = rc.point_sets()["honeycomb_257"]
    for method in ("otsu", "li"):
        want = graph.estimate_d(pts, threshold=method, return_k=True)
        assert distributed.estimate_d_device(resident(pts, kind), threshold=method, return_k=True) == want
        assert distributed.estimate_d_device(resident(pts, kind), threshold=method) == want[0]
    with pytest.raises(ValueError, match="n_neighbors"):
        distributed.estimate_d_device(resident(pts[:11], kind))


def test_vnn_graph_without_dmax_is_vnn_graph_at_the_estimate():
    pts = rc.point_sets()["honeycomb_257"]
    li, otsu = graph.estimate_d(pts, threshold=None), graph.estimate_d(pts, threshold="otsu")
    assert li != otsu
    want_li, want_otsu = graph.vnn_graph(pts, dmax=li), graph.vnn_graph(pts, dmax=otsu)
    assert len(want_li) > len(pts) and np.array_equal(graph.vnn_graph(pts), want_li)
    assert np.array_equal(graph.vnn_graph(pts, threshold_method="otsu"), want_otsu)
    assert (graph.vnn_graph(pts, return_ijs=False) != graph.vnn_graph(pts, dmax=li, return_ijs=False)).nnz == 0
    for kind in ("native", "torch"):
        got = distributed.vnn_graph_device(resident(pts, kind))
        assert np.array_equal(got.numpy() if kind == "native" else got.cpu().numpy(), want_li)
        got = distributed.vnn_graph_device(resident(pts, kind), threshold_method="otsu", threshold=0.1)
        assert np.array_equal(got.numpy() if kind == "native" else got.cpu().numpy(), want_otsu)
    with pytest.raises(ValueError, match="n_neighbors"):
        graph.vnn_graph(pts[:11])
    with pytest.raises(ValueError, match="n_neighbors"):
        distributed.vnn_graph_device(resident(pts[:11], "torch"))
