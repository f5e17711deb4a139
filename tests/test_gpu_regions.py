"""mtflearn_amd.graph on the GPU: the device result against goldens captured from the reference (tests/make_golden_regions.py) on
every case of tests/regions_cases.py, through ``find_regions``, ``LatticeGraph`` and ``distributed.find_regions_device``.

Criteria: ``np.array_equal`` on ``offsets`` / ``vertices`` / ``ks``, BIT equality on ``centers``, set equality on the
symmetrised adjacency.  No tolerance anywhere: the cases assert their own conditioning (neighbour angles at least 1e-9 rad
apart), so the device's ``atan2`` cannot reorder a neighbour list, and everything after the angular sort is integer work or a
sequential float64 sum."""
import os

import numpy as np
import pytest

import regions_cases as rc
import regions_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "regions_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def same_as_golden(golden, name, offsets, vertices, ks, centers, adjacency=None):
    for key, got in (("offsets", offsets), ("vertices", vertices), ("ks", ks)):
        ref = golden[f"{name}/{key}"]
        assert got.dtype == np.int64 and np.array_equal(got, ref), (name, key)
    ref = golden[f"{name}/centers"]
    assert centers.dtype == np.float64 and centers.shape == ref.shape and centers.tobytes() == ref.tobytes(), (name, "centers")
    if adjacency is not None:
        assert adjacency.dtype == np.int64 and adjacency.ndim == 2 and adjacency.shape[1] == 2
        assert oracle.symmetrised(adjacency) == oracle.symmetrised(golden[f"{name}/adjacency"]), (name, "adjacency")


def flat(polys):
    """(offsets, vertices) of what find_regions returned."""
    ks = np.array([len(p) for p in polys], dtype=np.int64)
    vertices = np.concatenate([np.asarray(p).astype(np.int64) for p in polys]) if len(polys) else np.empty(0, np.int64)
    return np.concatenate([[0], np.cumsum(ks)]).astype(np.int64), vertices, ks


@pytest.mark.parametrize("name", rc.NAMES)
def test_find_regions_equals_reference(golden, name):
    pts, ijs = rc.cases()[name]
    polys = graph.find_regions(pts, ijs)
    assert polys.dtype == object and all(np.asarray(p).dtype in (np.int64, object) for p in polys)
    offsets, vertices, ks = flat(polys)
    assert np.array_equal(offsets, golden[f"{name}/offsets"]) and np.array_equal(vertices, golden[f"{name}/vertices"]), name
    same = len(set(ks.tolist())) == 1
    assert polys.ndim == (2 if same else 1)                              # the reference's 2-D object array for equal lengths
    arrays = graph._regions_arrays(pts, ijs)                             # the five arrays of the same device call
    same_as_golden(golden, name, *arrays)


@pytest.mark.parametrize("name", rc.NAMES)
def test_lattice_graph_equals_reference(golden, name):
    pts, ijs = rc.cases()[name]
    if name == "06_one_way_triangle":                                    # LatticeGraph symmetrises its edges: the one-way triangle
        name = "02_triangle"                                             # (same points) becomes the two-way one
    g = graph.LatticeGraph(pts, ijs)
    offsets, vertices, ks = flat(g.regions)
    same_as_golden(golden, name, offsets, vertices, g.ks, g.centers, g._adjacency)
    assert np.array_equal(ks, g.ks) and g.polys is g.regions and g.faces is g.regions
    assert g.regions is g.regions and g.centers is g.centers            # cached: one device call


@pytest.mark.parametrize("kind", ["native", "torch"])
@pytest.mark.parametrize("name", rc.NAMES)
def test_find_regions_device_equals_reference(golden, name, kind):
    pts, ijs = rc.cases()[name]
    if kind == "native":
        d_pts, d_ijs = _native.DeviceArray.from_numpy(pts), _native.DeviceArray.from_numpy(ijs)
        out = distributed.find_regions_device(d_pts, d_ijs)
        assert all(isinstance(a, _native.DeviceArray) for a in out)
        host = [a.numpy() for a in out]
    else:
        import torch
        out = distributed.find_regions_device(torch.from_numpy(pts).cuda(), torch.from_numpy(ijs).cuda())
        assert all(a.is_cuda for a in out)
        host = [a.cpu().numpy() for a in out]
    same_as_golden(golden, name, *host)


def test_device_points_from_other_types_are_converted():
    import torch
    pts, ijs = rc.cases()["08_grid"]                                     # integer coordinates: exact in int32 and float32
    want = [a for a in graph._regions_arrays(pts, ijs)]
    for p_dtype, e_dtype in ((torch.int32, torch.int32), (torch.float32, torch.int64)):
        got = distributed.find_regions_device(torch.from_numpy(pts).to(p_dtype).cuda(), torch.from_numpy(ijs).to(e_dtype).cuda())
        assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def test_return_dict_matches(golden):
    for name in ("14_honeycomb_512_holes", "08_grid", "03_square_dangling"):
        pts, ijs = rc.cases()[name]
        got = graph.find_regions(pts, ijs, return_dict=True)
        offsets, vertices, ks = golden[f"{name}/offsets"], golden[f"{name}/vertices"], golden[f"{name}/ks"]
        assert sorted(got) == sorted(str(k) for k in np.unique(ks))
        for k in np.unique(ks):
            stack = np.vstack([vertices[offsets[f]:offsets[f + 1]] for f in np.flatnonzero(ks == k)])
            assert got[str(k)].shape == stack.shape and np.array_equal(got[str(k)].astype(np.int64), stack), (name, k)


def test_two_runs_give_identical_bytes():
    for name in ("12_delaunay", "13_ring_3000", "14_honeycomb_512_holes"):
        pts, ijs = rc.cases()[name]
        first, second = graph._regions_arrays(pts, ijs), graph._regions_arrays(pts, ijs)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second)), name


def test_motifs_graph_of_the_small_honeycomb(golden):
    name = "10_honeycomb_96"
    mg = graph.LatticeGraph(*rc.cases()[name]).to_motifs_graph()
    assert mg.major_k == 6
    adjacency = golden[f"{name}/adjacency"]
    pairs = np.unique(np.vstack([adjacency, adjacency[:, ::-1]]), axis=0)
    degs = np.bincount(pairs[:, 0], minlength=len(golden[f"{name}/ks"]))
    assert np.array_equal(mg.degs, degs) and np.array_equal(mg.ks, golden[f"{name}/ks"])
    assert mg.nodes.tobytes() == golden[f"{name}/centers"].tobytes()


def test_argument_errors_raise_before_any_launch(monkeypatch):
    import torch
    tri = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    good = np.array([[0, 1], [1, 0]])

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_library)
    for pts, ijs in [(tri, [[0, 3]]), (tri, [[1, 1]]), (tri, [[-1, 0]]), (tri, [[0.5, 1.0]]), (np.zeros((3, 3)), good), (tri, [[0, 1, 2]])]:
        with pytest.raises(ValueError):
            graph.find_regions(pts, ijs)
    d_tri, d_good = torch.from_numpy(tri).cuda(), torch.from_numpy(good).cuda()
    for pts, ijs in [(d_tri, d_good.double()), (d_tri[:, :1], d_good), (d_tri, d_good[:, :1]), (torch.from_numpy(tri), d_good),
                     (d_tri[:0], d_good)]:
        with pytest.raises(ValueError):
            distributed.find_regions_device(pts, ijs)
    monkeypatch.undo()
    # values of resident edges are checked on the device: an error, nothing computed, and the next call is unharmed
    with pytest.raises(RuntimeError, match="out of"):
        distributed.find_regions_device(d_tri, torch.tensor([[0, 1], [1, 7]]).cuda())
    with pytest.raises(RuntimeError, match="itself"):
        distributed.find_regions_device(d_tri, torch.tensor([[0, 1], [2, 2]]).cuda())
    assert len(graph.find_regions(tri, [[0, 1], [1, 0], [1, 2], [2, 1], [2, 0], [0, 2]])) == 1
