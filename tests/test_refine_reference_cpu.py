"""The host statements behind the refinement and bond-length goldens, checked without a GPU: tests/thresholds_reference.py
reproduces tests/golden/estimate_d_golden.npz, the host ``center_of_mass_refine`` reproduces tests/golden/refine_golden.npz, the
sequential row-major float64 statement of the centroid sums is bit-equal to the SciPy route on every refine case (the
summation-order claim of csrc/zk_refine.hip, proven before any kernel runs), and the histogram rule stated for the kernel gives
``np.histogram``'s counts on every sample of every point set.  For tests/test_gpu_points_kernels.py: the brute-force neighbour
distances it holds the device to agree with scikit-learn on every set of tests/point_cases.py, and the histogram rule gives
``np.histogram``'s counts on the matrices with values planted on the bin edges, where both of its corrections are taken."""
import os
import re

import numpy as np
import pytest

import make_golden_refine as mg
import point_cases as pc
import refine_cases as rc
import thresholds_reference as ref
from conftest import ROOT


def load(name):
    with np.load(os.path.join(ROOT, "tests", "golden", name)) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def refine_golden():
    return load("refine_golden.npz")


@pytest.fixture(scope="module")
def estimate_golden():
    return load("estimate_d_golden.npz")


def same_bits(got, want):
    """Equal bit for bit where ``want`` is a number, NaN exactly where ``want`` is NaN (a NaN's sign and payload are not pinned)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def test_the_generator_reproduces_both_golden_files(refine_golden, estimate_golden):
    for stored, fresh in ((refine_golden, mg.build_refine()), (estimate_golden, mg.build_estimate())):
        assert sorted(stored) == sorted(fresh)
        for key, value in fresh.items():
            assert same_bits(stored[key], value) if np.asarray(value).dtype == np.float64 else np.array_equal(stored[key], value), key


@pytest.mark.parametrize("name", rc.REFINE_NAMES)
def test_sequential_row_major_sums_are_bit_equal_to_the_scipy_route(refine_golden, name):
    data, pts, size, mode = rc.refine_cases()[name]
    assert same_bits(ref.sequential_refine(data, pts, size, mode), refine_golden[f"{name}/xy"]), name


def test_sequential_sums_on_the_key_points_of_the_512_frame(refine_golden):
    frame, pts = rc.frame_512(), refine_golden["keypoints_512/pts"]
    assert len(pts) > 1000
    for mode in rc.MODES:
        assert same_bits(ref.sequential_refine(frame, pts, 3, mode), refine_golden[f"keypoints_512_{'disk' if mode else 'box'}/xy"])


def test_the_cases_hold_what_their_names_say(refine_golden):
    g = refine_golden
    assert np.isnan(g["swallowed_by_four_later_box/xy"][0]).all() and not np.isnan(g["swallowed_by_four_later_box/xy"][1:]).any()
    assert np.isnan(g["duplicate_box/xy"][0]).all() and not np.isnan(g["duplicate_box/xy"][2]).any()
    assert not same_bits(g["overlap_one_column_ab_box/xy"], g["overlap_one_column_ba_box/xy"][::-1])     # the order decides the column
    xy = g["zero_sums_box/xy"]
    assert np.isnan(xy[0]).all() and xy[1, 0] == -np.inf and np.isnan(xy[1, 1]) and np.isfinite(xy[2]).all()
    # the second box's corner is the first disk's centre pixel: it belongs to nobody, so the first centroid is not what it is alone
    data, pts, size, _ = rc.refine_cases()["disk_corner_removes_earlier_pixel"]
    alone = ref.sequential_refine(data, pts[:1], size, "disk")
    assert not same_bits(g["disk_corner_removes_earlier_pixel/xy"][:1], alone)
    assert int(np.isnan(g["n3000_box/xy"]).any(axis=1).sum()) > 1000 and len(rc.refine_cases()["n3000_box"][1]) > 64 * 40


@pytest.mark.parametrize("name", rc.POINT_SET_NAMES)
def test_the_kernels_histogram_rule_gives_numpys_counts(estimate_golden, name):
    dd = estimate_golden[f"{name}/dd"]
    for c, k in enumerate(ref.KS):
        d = dd[:, 1:k].ravel()
        if d.min() == d.max():
            continue
        want = np.histogram(d, bins=256)[0]
        assert np.array_equal(ref.kernel_bin_rule(d, d.min(), d.max()), want), (name, k)
        assert np.array_equal(estimate_golden[f"{name}/otsu_counts"][c], want), (name, k)
    first = dd[:, 1].min()                               # rows ascend: one pass gives the eleven ranges
    assert all(dd[:, 1:k].min() == first and dd[:, 1:k].max() == dd[:, k - 1].max() for k in ref.KS)


@pytest.mark.parametrize("name", pc.KNN_NAMES)
def test_brute_force_distances_of_the_edge_sets_agree_with_scikit_learn(name):
    from sklearn.neighbors import NearestNeighbors
    pts = pc.knn_sets()[name]
    k = min(12, len(pts))
    got, want = pc.knn_reference(pts, k), NearestNeighbors(n_neighbors=k, algorithm="ball_tree").fit(pts).kneighbors(pts)[0]
    assert got.shape == want.shape and np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), name       # zeros exact
    assert not got[:, 0].any() and np.all(np.diff(got, axis=1) >= 0)


@pytest.mark.parametrize("kind", pc.HIST_KINDS)
def test_the_histogram_rule_takes_both_corrections_on_the_planted_edges(kind):
    dd, lasts, edges = pc.hist_matrix(257, kind), pc.hist_lasts(kind), pc.hist_edges(kind)
    down = up = folded = 0
    for c, k in enumerate(ref.KS):
        d = dd[:, 1:k].ravel()
        want, want_edges = np.histogram(d, bins=256, range=(0.0, lasts[c]))
        assert np.array_equal(want_edges, edges[c]) and want.sum() == len(d)
        assert np.array_equal(ref.kernel_bin_rule(d, 0.0, lasts[c]), want), (kind, k)
        idx = ((d / lasts[c]) * 256.0).astype(np.int64)
        folded += int((idx == 256).sum())
        idx[idx == 256] = 255
        down += int((d < edges[c][idx]).sum())
        up += int(((d >= edges[c][idx + 1]) & (idx != 255)).sum())
    print(f"{kind}: {down} values one bin down, {up} one bin up, {folded} folded from 256 into 255")
    assert folded > 0 and (kind != "uneven" or (down > 0 and up > 0))      # with edges that are exact, the first index is right


def test_li_cases_are_jittered_and_stop_clear_of_the_tolerance_boundary(estimate_golden):
    for name in rc.LI_SETS:
        l = ref.estimate(rc.point_sets()[name], "li", estimate_golden[f"{name}/dd"])
        assert l["margins"].min() > mg.LI_MARGIN and (l["iterations"] >= 1).all() and l["iterations"].max() < 100
        assert np.array_equal(l["iterations"], estimate_golden[f"{name}/li_iterations"])


def test_the_new_entry_points_are_declared_bound_and_exported():
    import ctypes
    from mtflearn_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("zk_refine_points", "zk_refine_points_dev", "zk_knn_distances", "zk_knn_distances_dev", "zk_knn_stats", "zk_knn_stats_dev"):
        decl = re.search(rf"\bint {sym}\(([^;]*)\);", header)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym


def test_host_checks_raise_before_any_launch():
    """Every precondition of refine_points / estimate_d that the host can see is a ValueError naming it, with no device needed."""
    from mtflearn_amd import features, graph
    data = np.zeros((32, 40), np.float32)
    ok = np.array([[10, 10]])
    for bad_data, pts, what in ((data.astype(np.int32), ok, "float"), (data.astype(np.uint8), ok, "float"), (data[None], ok, "2-D"),
                                (data, np.array([[2, 10]]), "inside the frame"), (data, np.array([[10, 29]]), "inside the frame"),
                                (data, np.array([[37, 10]]), "inside the frame"), (data, np.array([[10, 2]]), "inside the frame"),
                                (data, np.array([[10.0, 10.0]]), "integer"), (data, np.array([10, 10, 10]), "integer")):
        with pytest.raises(ValueError, match=what):
            features.refine_points(bad_data, pts, size=3)
    with pytest.raises(ValueError, match="2\\^24"):
        features.refine_points(np.zeros((8, 8), np.float32), np.broadcast_to(np.array([[4, 4]], np.int32), (2 ** 24, 2)), size=1)
    assert features.refine_points(data, np.empty((0, 2), int)).shape == (0, 2)
    with pytest.raises(ValueError, match="n_neighbors"):
        graph.estimate_d(np.random.default_rng(0).random((11, 2)))
    with pytest.raises(ValueError, match="n_neighbors"):
        graph.vnn_graph(np.random.default_rng(0).random((11, 2)))
    with pytest.raises(ValueError, match="finite"):
        graph.knn_distances(np.full((20, 2), np.nan))
