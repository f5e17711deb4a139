"""mtflearn_amd.graph.vnn_graph / voronoi_neighbours on the GPU against the goldens made from SciPy's qhull
(tests/make_golden_vnn.py) on every case of tests/vnn_cases.py, through the host API, the native ``DeviceArray`` and the torch
tensor.

Criteria: the graph ``np.array_equal`` to the golden (sorted, int64, both directions), the neighbour pairs equal to the golden's,
ridge lengths within ``tol = max(100 d0, 1e-12) a`` (``d0``: what qhull and the brute-force oracle differ by, stored in the
golden file; ``a``: the case's median edge length), edge lengths within 4 ulp, two calls identical byte for byte."""
import os

import numpy as np
import pytest

import vnn_cases as vc
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph

pytestmark = pytest.mark.gpu

KINDS = ("host", "native", "torch")


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "vnn_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def case_of(name, golden):
    """``(points name, pts, dmax, threshold)``"""
    if name == "one_way":
        pts, dmax, _ = vc.cases()[vc.ONE_WAY_POINTS]
        return vc.ONE_WAY_POINTS, pts, dmax, float(golden["one_way/threshold"])
    return (name,) + tuple(vc.cases()[name])


def to_host(a):
    return a.numpy() if isinstance(a, _native.DeviceArray) else a.cpu().numpy()


def resident(pts, kind):
    if kind == "native":
        return _native.DeviceArray.from_numpy(pts)
    import torch
    return torch.from_numpy(np.array(pts, order="C")).cuda()                # a copy: the cases are read-only


def run_graph(pts, dmax, threshold, kind):
    if kind == "host":
        return graph.vnn_graph(pts, threshold=threshold, dmax=dmax)
    out = distributed.vnn_graph_device(resident(pts, kind), dmax, threshold=threshold)
    assert isinstance(out, _native.DeviceArray) if kind == "native" else out.is_cuda
    return to_host(out)


def run_neighbours(pts, kind):
    if kind == "host":
        return graph.voronoi_neighbours(pts)
    out = distributed.voronoi_neighbours_device(resident(pts, kind))
    assert all(isinstance(a, _native.DeviceArray) if kind == "native" else a.is_cuda for a in out)
    return tuple(to_host(a) for a in out)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", vc.NAMES + ("one_way",))
def test_vnn_graph_equals_reference(golden, name, kind):
    _, pts, dmax, threshold = case_of(name, golden)
    ijs = run_graph(pts, dmax, threshold, kind)
    ref = golden[f"{name}/ijs"]
    assert ijs.dtype == np.int64 and ijs.shape == ref.shape and np.array_equal(ijs, ref), name
    pairs = {tuple(r) for r in ijs.tolist()}
    assert all((j, i) in pairs for i, j in pairs)
    again = run_graph(pts, dmax, threshold, kind)
    assert again.tobytes() == ijs.tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", vc.NAMES)
def test_voronoi_neighbours_equal_reference(golden, name, kind):
    pts = vc.cases()[name][0]
    ijs, ridge, edge = run_neighbours(pts, kind)
    ref = golden[f"{name}/nb_ijs"]
    assert ijs.dtype == np.int64 and ridge.dtype == np.float64 and edge.dtype == np.float64
    assert ijs.shape == ref.shape and np.array_equal(ijs, ref), name
    tol = float(golden["tol_rel"]) * float(golden[f"{name}/a"])
    if len(ref):
        worst = np.abs(ridge - golden[f"{name}/nb_ridge"]).max()
        ulps = (np.abs(edge - golden[f"{name}/nb_edge"]) / np.spacing(golden[f"{name}/nb_edge"])).max()
        print(f"{name} ({kind}): ridge lengths differ by at most {worst:.3g} (tol {tol:.3g}), edge lengths by {ulps:.2f} ulp")
        assert worst <= tol and ulps <= 4
    second = run_neighbours(pts, kind)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ijs, ridge, edge), second))


def test_over_the_vertex_cap_is_an_error_not_a_fault(golden):
    with pytest.raises(RuntimeError, match="more than 32"):
        graph.voronoi_neighbours(vc.OVER_CAP)
    with pytest.raises(RuntimeError, match="more than 32"):
        distributed.vnn_graph_device(_native.DeviceArray.from_numpy(vc.OVER_CAP), 1.3)
    pts, dmax, threshold = vc.cases()["wheel_24"]                         # the library is unharmed
    assert np.array_equal(graph.vnn_graph(pts, threshold=threshold, dmax=dmax), golden["wheel_24/ijs"])


def test_resident_nan_and_duplicate_fail_and_the_next_call_succeeds(golden):
    import torch
    pts, dmax, threshold = vc.cases()["n65"]
    nan = pts.copy()
    nan[7, 1] = np.nan
    dup = np.concatenate([pts, pts[5:6]])
    for bad, what in ((nan, "finite"), (dup, "coincide")):
        for kind in ("native", "torch"):
            with pytest.raises(RuntimeError, match=what) as err:
                distributed.vnn_graph_device(resident(bad, kind), dmax)
            assert "-10001" in str(err.value)                            # ZK_E_BADARG
            with pytest.raises(RuntimeError, match=what):
                distributed.voronoi_neighbours_device(resident(bad, kind))
    huge = pts * 1e307                                                   # finite, but their sum is not: refused like a NaN
    with pytest.raises(RuntimeError, match="finite"):
        distributed.vnn_graph_device(resident(huge, "torch"), dmax * 1e307)
    with pytest.raises(RuntimeError, match="finite"):
        graph.voronoi_neighbours(huge)
    for bad in (torch.zeros(3, 3).cuda(), torch.zeros(4).cuda(), torch.zeros(3, 2)):
        with pytest.raises(ValueError):
            distributed.vnn_graph_device(bad, 1.0)
    with pytest.raises(ValueError):
        distributed.vnn_graph_device(resident(pts, "torch"), 1.0, threshold=0)
    assert np.array_equal(to_host(distributed.vnn_graph_device(resident(pts, "torch"), dmax, threshold=threshold)), golden["n65/ijs"])


@pytest.mark.parametrize("kind", ("native", "torch"))
def test_int32_points_give_the_rows_of_the_same_values_in_float64(kind):
    """One loader for both types: int32 pairs are widened exactly, so pairs, ridge and edge lengths agree byte for byte."""
    pts = np.rint(12 * vc.honeycomb(7, 7, 0.04, 22)).astype(np.int32)       # 98 key points as local_max gives them: whole pixels
    want = [to_host(a) for a in distributed.voronoi_neighbours_device(resident(pts.astype(np.float64), kind))]
    got = [to_host(a) for a in distributed.voronoi_neighbours_device(resident(pts, kind))]
    assert len(want[0]) > len(pts) and all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_csr_matrix_of_the_graph(golden):
    pts, dmax, threshold = vc.cases()["grid_3x3_jittered"]
    matrix = graph.vnn_graph(pts, threshold=threshold, dmax=dmax, return_ijs=False)
    assert matrix.format == "csr" and matrix.shape == (9, 9) and (matrix != matrix.T).nnz == 0
    assert np.array_equal(graph.matrix2ijs(matrix), golden["grid_3x3_jittered/ijs"])


def test_lattice_graph_of_vnn_bonds_equals_lattice_graph_of_golden_bonds(golden):
    pts, dmax, threshold = vc.cases()["honeycomb_392"]
    got = graph.LatticeGraph(pts, graph.vnn_graph(pts, dmax=dmax))
    ref = graph.LatticeGraph(pts, golden["honeycomb_392/ijs"].astype(np.int64))
    assert len(ref.regions) > 100 and (ref.ks == 6).sum() > 100          # hexagons, not the triangles of a radius query
    assert len(got.regions) == len(ref.regions) and all(np.array_equal(a, b) for a, b in zip(got.regions, ref.regions))
    assert np.array_equal(got.ks, ref.ks) and got.centers.tobytes() == ref.centers.tobytes()


def test_resident_chain_local_max_to_regions():
    """local_max_device -> vnn_graph_device -> find_regions_device on a rendered honeycomb frame: no host copy of the points
    (only dmax, a scalar, is taken from the edge lengths on the host).  Equal to the host chain on the same points."""
    import torch
    from mtflearn_amd.synthetic import honeycomb_frame
    frame = honeycomb_frame(96, 128, seed=3).astype(np.float32)
    d_pts = distributed.local_max_device(torch.from_numpy(frame).cuda(), min_distance=3, threshold=float(frame.mean()))
    assert d_pts.is_cuda and d_pts.dtype == torch.int32 and d_pts.shape[1] == 2
    n = int(d_pts.shape[0])
    assert n > 20
    dmax = 1.3 * float(distributed.voronoi_neighbours_device(d_pts)[2].median())
    d_ijs = distributed.vnn_graph_device(d_pts, dmax)
    got = [to_host(a) for a in distributed.find_regions_device(d_pts, d_ijs)]
    pts = to_host(d_pts).astype(np.float64)                               # the host chain on the same points
    ijs = graph.vnn_graph(pts, dmax=dmax)
    assert np.array_equal(to_host(d_ijs), ijs) and len(ijs) > n
    want = graph._regions_arrays(*graph._check_graph(pts, ijs))
    assert len(want[2]) > 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
    # the int32 DeviceArray local_max_device returns for a native frame is taken as it is, too
    d_native = distributed.local_max_device(_native.DeviceArray.from_numpy(frame), min_distance=3, threshold=float(frame.mean()))
    assert isinstance(d_native, _native.DeviceArray) and d_native.dtype == np.int32
    assert np.array_equal(distributed.vnn_graph_device(d_native, dmax).numpy(), ijs)
