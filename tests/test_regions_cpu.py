"""mtflearn_amd.graph without a GPU: the host oracle (tests/regions_oracle.py) against the goldens captured from the reference
(tests/make_golden_regions.py) with exact equality on every case, the conditioning every case claims, the host-side classes and
helpers, the argument checks (all of which come before the first device call), and the C ABI's declarations."""
import os
import re

import numpy as np
import pytest

import regions_cases as rc
import regions_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "regions_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def oracles():
    return {name: oracle.regions(*case) for name, case in rc.cases().items()}


def test_cases_are_the_listed_ones_and_conditioned():
    cases = rc.cases()
    assert list(cases) == rc.NAMES
    for name, (pts, ijs) in cases.items():
        gap, edge = rc.conditioning(pts, ijs)
        assert gap >= rc.MIN_GAP and edge >= rc.MIN_GAP, (name, gap, edge)
        assert pts.dtype == np.float64 and ijs.dtype == np.int64 and ijs.shape[1] == 2
    pts, ijs = cases["08_grid"]
    assert (pts[:, 0] == pts[:, 0].min()).sum() == 8                     # the tied minimum the first argmin has to break
    assert len(np.unique(cases["07_duplicated_edges"][1], axis=0)) * 3 == len(cases["07_duplicated_edges"][1])
    assert len(cases["06_one_way_triangle"][1]) == 3
    degree = np.bincount(cases["09_wheel"][1][:, 0])
    assert degree.max() == 20
    assert len(cases["11_honeycomb_512"][0]) > 1024 and len(cases["13_ring_3000"][0]) == 3003


@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_equals_reference(golden, oracles, name):
    offsets, vertices, ks, centers, adjacency = oracles[name]
    for key, got in (("offsets", offsets), ("vertices", vertices), ("ks", ks)):
        ref = golden[f"{name}/{key}"]
        assert got.dtype == ref.dtype == np.int64 and np.array_equal(got, ref), (name, key)
    ref = golden[f"{name}/centers"]
    assert centers.shape == ref.shape and centers.tobytes() == ref.tobytes(), name       # bit equality
    assert oracle.symmetrised(adjacency) == oracle.symmetrised(golden[f"{name}/adjacency"]), name
    if name in rc.EXPECTED_FACES:
        assert len(ks) == rc.EXPECTED_FACES[name]


def test_golden_shapes_say_what_the_cases_are_for(golden):
    assert set(golden["10_honeycomb_96/ks"]) == {6} and set(golden["11_honeycomb_512/ks"]) == {6}
    assert sorted(golden["13_ring_3000/ks"]) == [3, 3000, 3000]
    assert len(set(golden["14_honeycomb_512_holes/ks"])) > 2
    assert set(golden["12_delaunay/ks"]) == {3} and len(golden["12_delaunay/ks"]) > 300
    assert set(golden["09_wheel/ks"]) == {3} and len(golden["09_wheel/ks"]) == 20


# ------------------------------------------------------------------------------------------------ the kernel-level cases
@pytest.fixture(scope="module")
def kernel_oracles():
    return {name: oracle.regions(*case) for name, case in rc.kernel_cases().items()}


def test_kernel_cases_are_conditioned_and_say_what_they_are_for(kernel_oracles):
    """What tests/test_gpu_regions_kernels.py hands to the device, proven here first."""
    cases = rc.kernel_cases()
    assert list(cases) == rc.KERNEL_NAMES and not set(cases) & set(rc.NAMES)
    for name, (pts, ijs) in cases.items():
        gap, edge = rc.conditioning(pts, ijs)
        assert gap >= rc.MIN_GAP and edge >= rc.MIN_GAP, (name, gap, edge)
        assert pts.dtype == np.float64 and ijs.dtype == np.int64 and ijs.shape[1] == 2
        sizes, counts = np.unique(kernel_oracles[name][2], return_counts=True)
        assert dict(zip(sizes.tolist(), counts.tolist())) == rc.KERNEL_EXPECTED_KS[name], name
    assert [len(cases[f"ring_{n}"][0]) - 3 for n in rc.RING_SIZES] == [1021, 1022, 1023, 1024, 4093]
    pts, ijs = cases["chain_5000"]
    degree = np.bincount(ijs[:, 0], minlength=len(pts))
    assert len(pts) == 5004 and degree[1] == 3 and degree[-1] == 1 and (degree[4:-1] == 2).all()      # 2 x 5000 wedges out and back
    assert np.bincount(cases["wheel_700"][1][:, 0]).max() == 700 == np.bincount(cases["wheel_700_shuffled"][1][:, 0]).max()
    pts, ijs = cases["wheel_700_shuffled"]
    hub = int(np.argmax(np.bincount(ijs[:, 0])))
    rim = np.sort(ijs[ijs[:, 0] == hub, 1])                              # by index: not by angle
    turn = np.diff(np.arctan2(*(pts[rim] - pts[hub]).T[::-1]))
    assert (turn < 0).sum() > 300 and (turn > 0).sum() > 300
    for name, tied in (("tied_min_3000", rc.TIED_NODES), ("tied_min_triangles", rc.TIED_TRIANGLE_NODES)):
        x = cases[name][0][:, 0]
        assert sorted(np.flatnonzero(x == x.min())) == sorted(tied) and int(np.argmin(x)) == 1030 == min(tied)
        assert len({t // 1024 for t in tied}) > 1                                # more than one stride of a 1024-lane sweep
    assert sorted(t % 1024 for t in rc.TIED_TRIANGLE_NODES) == [6, 6, 452, 1023]
    # the triangle that takes the grown edge keeps one face, every other one two
    offsets, vertices, ks, _, adjacency = kernel_oracles["tied_min_triangles"]
    faces_of = np.bincount(vertices[offsets[:-1]] // 3, minlength=1000)
    assert np.array_equal(np.flatnonzero(faces_of != 2), [1030 // 3]) and faces_of[1030 // 3] == 1 and len(adjacency) == 3 * 999


@pytest.mark.parametrize("name", rc.GOLDEN_KERNEL_NAMES)
def test_oracle_equals_reference_on_kernel_cases(golden, kernel_oracles, name):
    """The kernel-level cases the reference's quadratic walk can reach: the yardstick of the GPU tests is the reference there."""
    offsets, vertices, ks, centers, adjacency = kernel_oracles[name]
    for key, got in (("offsets", offsets), ("vertices", vertices), ("ks", ks)):
        ref = golden[f"{name}/{key}"]
        assert got.dtype == ref.dtype == np.int64 and np.array_equal(got, ref), (name, key)
    ref = golden[f"{name}/centers"]
    assert centers.shape == ref.shape and centers.tobytes() == ref.tobytes(), name
    assert oracle.symmetrised(adjacency) == oracle.symmetrised(golden[f"{name}/adjacency"]), name


# ------------------------------------------------------------------------------------------------ host-side classes
def test_polygons_reproduce_the_object_array_quirk(golden):
    same = graph._polygons(golden["08_grid/offsets"], golden["08_grid/vertices"])
    assert same.dtype == object and same.shape == (49, 4)                # equal lengths: NumPy makes it 2-D
    mixed = graph._polygons(golden["07_duplicated_edges/offsets"], golden["07_duplicated_edges/vertices"])
    assert mixed.dtype == object and mixed.shape == (2,) and mixed[0].dtype == np.int64
    none = graph._polygons(np.zeros(1, np.int64), np.empty(0, np.int64))
    assert none.dtype == object and none.shape == (0,)
    as_dict = graph._polygons(golden["14_honeycomb_512_holes/offsets"], golden["14_honeycomb_512_holes/vertices"], return_dict=True)
    ks = golden["14_honeycomb_512_holes/ks"]
    assert sorted(as_dict) == sorted(str(k) for k in np.unique(ks))
    assert all(as_dict[str(k)].shape == ((ks == k).sum(), k) for k in np.unique(ks))
    assert graph._polygons(np.zeros(1, np.int64), np.empty(0, np.int64), return_dict=True) == {}


def test_helpers():
    ijs = np.array([[0, 1], [1, 2], [0, 1]])
    sym = graph.symmetric_edges(ijs)
    assert sym.tolist() == [[0, 1], [1, 0], [1, 2], [2, 1]]
    m = graph.edges2matrix(sym)
    assert m.shape == (3, 3) and graph.is_symmetric(m) and graph.is_symmetric(m.toarray())
    assert sorted(map(tuple, graph.matrix2edges(m))) == sorted(map(tuple, sym)) == sorted(map(tuple, graph.matrix2ijs(m)))
    assert [list(r) for r in graph.matrix2lil(m)] == [[1], [0, 2], [1]] == [list(r) for r in graph.matrix2inds(m)]
    one_way = graph.ijs2matrix(np.array([[0, 1], [1, 2]]), shape=(3, 3))
    assert not graph.is_symmetric(one_way)
    assert graph.make_symmetric(one_way).toarray().tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    dense = np.array([[0, 2, 0], [0, 0, 1], [0, 1, 0]])
    assert graph.make_symmetric(dense).tolist() == [[0, 2, 0], [2, 0, 1], [0, 1, 0]]
    assert graph.make_symmetric_more(dense).tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    assert graph.make_symmetric_less(dense).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]]
    assert graph.edges2matrix(sym, fmt="dense").tolist() == [[0, 1, 0], [1, 0, 1], [0, 1, 0]]
    assert graph.edges2matrix(sym, fmt="csr").format == "csr"
    assert graph.cantor_pairing([[1, 2], [2, 1]]).tolist() == [8, 8] and graph.cantor_pairing([[1, 2], [2, 1]], symmetric=False).tolist() == [8, 7]
    assert graph.sort_lbs(np.array([5, 5, 2, 9, 9, 9])).tolist() == [1, 1, 2, 0, 0, 0]
    grid, bonds = rc.cases()["08_grid"]
    assert graph.get_num_faces(graph.edges2matrix(bonds, shape=(64, 64))) == 49
    two, bonds2 = rc.cases()["04_two_triangles"]
    assert graph.get_num_faces(graph.edges2matrix(bonds2, shape=(6, 6)).tocsr()) == 2
    assert graph.find_n_nodes(np.array([[0, 1], [1, 0], [1, 2], [2, 1]]), n=3).tolist() == [[0, 1, 2], [2, 1, 0]]


def test_planar_graph_and_motifs():
    pts, ijs = rc.cases()["07_duplicated_edges"]
    g = graph.PlanarGraph(pts, ijs[:6])
    assert g.pts is g.nodes and g.vertices is g.nodes and g.ijs is g.edges
    assert len(g.edges) == 2 * len(np.unique(np.sort(ijs[:6], axis=1), axis=0)) and g.is_symmetric()
    assert g.matrix.shape == (5, 5) and g.degs.sum() == len(g.edges) and len(g.lil) == 5
    g.polys = "x"
    assert g.regions == "x" and g.faces == "x" and g.polygons == "x"
    with pytest.raises(AttributeError):
        g.nothing_of_the_kind
    a = graph.construct_motif(np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]))
    b = graph.construct_motif(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]))
    assert len(a.edges) == 6 and len(a.pts) == 3
    both = a + b
    assert len(both.pts) == 4 and len(both.edges) == 10                  # 5 bonds, the shared one once
    lg = graph.LatticeGraph(pts, ijs)
    assert graph.LatticeGraph1 is graph.LatticeGraph and lg.get_level1() is lg.lbs and np.array_equal(lg.lbs, lg.degs)
    assert [list(v) for v in lg.get_level2()] == [list(lg.degs[row]) for row in lg.lil]
    assert not lg.is_loop and not lg.is_chain
    assert graph.LatticeGraph(pts[:3], ijs[:6]).is_loop
    chain = graph.LatticeGraph(pts[:3], [[0, 1], [1, 2]])
    assert chain.is_chain and not chain.is_loop
    parts = graph.LatticeGraph(*rc.cases()["04_two_triangles"]).decompose(min_nodes=3)
    assert [len(p.nodes) for p in parts] == [3, 3] and all(p.is_loop for p in parts)
    kept = lg.remove_nodes(np.array([True, True, True, False, False]))
    assert len(kept.nodes) == 3 and kept.is_loop and np.array_equal(kept.lbs, lg.lbs[:3])


def test_motifs_graph_from_golden(golden):
    """MotifsGraph on the reference's own polygons: the host-side bookkeeping needs no device."""
    name = "14_honeycomb_512_holes"
    pts = rc.cases()[name][0]
    polys = graph._polygons(golden[f"{name}/offsets"], golden[f"{name}/vertices"])
    motifs = np.array([graph.construct_motif(pts[p.astype(int)]) for p in polys], dtype=object)
    mg = graph.MotifsGraph(motifs, golden[f"{name}/centers"], golden[f"{name}/adjacency"])
    assert mg.major_k == 6 and np.array_equal(mg.ks, golden[f"{name}/ks"])
    assert mg.degs.sum() == len(mg.edges) and mg.n_components >= 1 and len(mg.component_lbs) == len(polys)
    six = mg.select()
    assert set(six.ks) == {6} and len(six.nodes) == (mg.ks == 6).sum()
    ten = mg.select_nodes(k=10)
    assert set(ten.ks) == {10}
    assert len(mg.select_nodes(mask=mg.ks > 6).nodes) == (mg.ks > 6).sum()
    cross = mg.select_connections([[6, 10]])
    assert len(cross.edges) and all({mg.ks[i], mg.ks[j]} == {6, 10} for i, j in cross.edges)
    assert len(mg.remove_edges(np.arange(len(mg.edges)) % 2 == 0).nodes) == len(mg.nodes)
    paths = six.find_n_nodes(3)
    assert paths.shape[1] == 3 and len(np.unique(paths, axis=0)) == len(paths)


# ------------------------------------------------------------------------------------------------ checks before any launch
def test_argument_errors_come_before_the_library_is_touched(monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_native, "load", no_library)
    tri = [[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]
    for pts, ijs in [(np.zeros((3, 3)), [[0, 1]]), (np.zeros(3), [[0, 1]]), (tri, [[0, 1, 2]]), (tri, [[0.0, 1.0]]), (tri, [[0, 3]]),
                     (tri, [[-1, 0]]), (tri, [[1, 1]]), (tri, np.array([[0, 2 ** 63]], dtype=np.uint64)),
                     (np.zeros((3, 2), complex), [[0, 1]]), (np.empty((0, 2)), [[0, 1]])]:
        with pytest.raises(ValueError):
            graph.find_regions(pts, ijs)
    with pytest.raises(ValueError):
        graph.LatticeGraph(np.zeros((3, 3)), np.array([[0, 1]])).regions
    with pytest.raises(ValueError):
        graph.LatticeGraph(np.array(tri), np.array([[0, 3]])).ks
    empty = graph.find_regions(np.empty((0, 2)), np.empty((0, 2), np.int64))
    assert empty.dtype == object and empty.shape == (0,)
    assert graph.find_regions(np.empty((0, 2)), [], return_dict=True) == {}


def test_no_device_is_an_error_not_a_fallback():
    if _native.device_count() > 0:
        pytest.skip("a device is visible")
    with pytest.raises(RuntimeError):
        graph.find_regions(*rc.cases()["02_triangle"])
    with pytest.raises(RuntimeError):
        graph.LatticeGraph(*rc.cases()["02_triangle"]).ks


def test_abi_is_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    lib = _native.load()
    for sym in ("zk_find_regions", "zk_find_regions_dev"):
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym)
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    assert "find_regions_device" in distributed.__all__
