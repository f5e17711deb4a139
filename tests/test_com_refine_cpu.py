"""What csrc/zk_com_refine.hip claims about NumPy, checked without a GPU on every window of tests/com_refine_cases.py: its edge
formula is ``np.linspace`` bit for bit, its bin rule gives ``np.histogram``'s counts, and Otsu with the two cumulative sums taken
sequentially in bin order is tests/thresholds_reference.py's bit for bit.  Also: the golden file is what its generator makes,
the cases hold what their names say, the three entry points are declared, bound and exported, and every precondition the host
can see raises ``ValueError`` before any launch."""
import os
import re

import numpy as np
import pytest

import com_refine_cases as cc
import make_golden_com_refine as mg
import thresholds_reference as ref
from conftest import ROOT

BINS = 256


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "com_refine.npz")) as f:
        return {k: f[k] for k in f.files}


def case_windows(name):
    """The windows of a case that have more than one value, flattened: ``(M, size * size)`` float64."""
    frame, pts, size = cc.cases()[name]
    w = cc.windows(frame, pts, size).reshape(len(pts), -1)
    return w[w.min(axis=1) != w.max(axis=1)]


def kernel_edges(lo, hi):
    """Edge k = k * step + lo with step = (hi - lo) / 256, product and sum rounded separately, the last edge set to hi; one row
    per window."""
    step = (hi - lo) / np.float64(BINS)
    edges = np.arange(BINS + 1, dtype=np.float64)[None, :] * step[:, None]
    edges = edges + lo[:, None]
    edges[:, BINS] = hi
    return edges


def kernel_otsu(w):
    """Otsu as the kernel states it, all windows of a case at once: the counts of the bin rule, then both cumulative sums of
    counts * centres one bin after the other (upwards, and downwards from the last bin), the variance of every split and its
    first maximum."""
    lo, hi = w.min(axis=1), w.max(axis=1)
    edges = kernel_edges(lo, hi)
    centers = (edges[:, :-1] + edges[:, 1:]) / 2
    counts = np.array([ref.kernel_bin_rule(row, a, b) for row, a, b in zip(w, lo, hi)])
    terms = counts * centers
    fwd, bwd, below = np.empty_like(terms), np.empty_like(terms), np.cumsum(counts, axis=1)
    acc_up, acc_down = terms[:, 0].copy(), terms[:, BINS - 1].copy()
    for q in range(BINS):
        if q:
            acc_up = acc_up + terms[:, q]
            acc_down = acc_down + terms[:, BINS - 1 - q]
        fwd[:, q], bwd[:, BINS - 1 - q] = acc_up, acc_down
    w1 = below[:, :-1]
    w2 = w.shape[1] - w1
    d = fwd[:, :-1] / w1 - bwd[:, 1:] / w2
    var = (w1 * w2).astype(np.float64) * (d * d)
    k = np.argmax(var, axis=1)
    rows = np.arange(len(w))
    return (edges[rows, k] + edges[rows, k + 1]) / 2


@pytest.mark.parametrize("name", tuple(cc.cases()))
def test_edges_bins_and_sequential_otsu_are_numpys(name):
    w = case_windows(name)
    if not len(w):
        assert name in ("constant_window", "window_of_zeros")
        return
    lo, hi = w.min(axis=1), w.max(axis=1)
    edges = kernel_edges(lo, hi)
    for row, a, b, e in zip(w, lo, hi, edges):
        assert np.array_equal(e.view(np.int64), np.linspace(a, b, BINS + 1).view(np.int64))
        assert np.array_equal(ref.kernel_bin_rule(row, a, b), np.histogram(row, bins=BINS)[0])
    want = np.array([ref.otsu(row)[0] for row in w])
    assert np.array_equal(kernel_otsu(w).view(np.int64), want.view(np.int64))


def test_the_generator_reproduces_the_golden_file(golden):
    fresh = mg.build()
    assert sorted(fresh) == sorted(golden)
    for key, value in fresh.items():
        assert golden[key].dtype == value.dtype and np.array_equal(golden[key], value, equal_nan=value.dtype == np.float64), key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "com_refine.npz")) < 2 ** 19


def test_the_cases_hold_what_their_names_say(golden):
    g = golden
    for threshold in cc.THRESHOLDS:
        assert g[f"constant_window/{threshold}/t"][0] == 0.25 and g[f"constant_window/{threshold}/it"][0] == 0
        assert np.allclose(g[f"constant_window/{threshold}/xy"][0], [7.5, 7.5])                  # the centre of an 8 x 8 window at (4, 4)
        assert np.isnan(g[f"window_of_zeros/{threshold}/xy"]).all() and g[f"window_of_zeros/{threshold}/t"][0] == 0
        assert np.array_equal(g[f"one_bright_pixel/{threshold}/xy"][0], [9.0, 39.0])
        assert np.array_equal(g[f"duplicated_points/{threshold}/xy"][0], g[f"duplicated_points/{threshold}/xy"][2])
    assert g["one_bright_pixel/li/it"][0] == 1 and g["one_bright_pixel/li/t"][0] == 3.0 / 64          # mean_back == 0: the mean stays
    assert g["two_values/li/it"][0] == 1
    frame, pts, size = cc.cases()["negative_data"]
    assert (cc.windows(frame, pts, size) < 0).any(axis=(1, 2)).sum() > 30 and len(pts) == 40
    sizes = {cc.cases()[name][2] for name in cc.PARITY}
    assert {2, 3, 7, 8, 16, 17, 64, 5, 9, 13, 24} <= sizes
    assert {len(cc.cases()[name][1]) for name in ("n1", "n63", "n64", "n65")} == {1, 63, 64, 65}
    assert 1250 < len(cc.cases()["honeycomb_512_size9"][1]) <= 1300
    its = np.concatenate([g[f"{name}/li/it"] for name in cc.PARITY])
    assert its.min() == 1 and its.max() > 20
    for name in ("every_edge_size7", "every_edge_size8", "every_edge_size24"):                 # each edge of the frame is touched
        frame, pts, size = cc.cases()[name]
        first = cc.corners(pts, size)
        assert first[:, 0].min() == 0 and first[:, 1].min() == 0
        assert (first[:, 0] + size).max() == frame.shape[1] and (first[:, 1] + size).max() == frame.shape[0]
    name, extra = cc.OUTSIDE
    frame, pts, size = cc.cases()[name]
    assert (cc.corners(extra, size)[:, 0] + size > frame.shape[1]).all()
    from mtflearn_amd.features.keypoints import clear_border
    for name in cc.PARITY:                                                                      # border clearing keeps every point
        frame, pts, size = cc.cases()[name]
        assert len(clear_border(pts, frame.shape, size)) == len(pts), name


def test_the_three_entry_points_are_declared_bound_and_exported():
    import ctypes
    from mtflearn_amd import _native, distributed, features
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("zk_com_refine", "zk_com_refine_dev", "zk_com_refine_points_dev"):
        decl = re.search(rf"\bint {sym}\(([^;]*)\);", header)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    assert re.search(r"#define ZK_THRESHOLD_LI\s+0\b", header) and re.search(r"#define ZK_THRESHOLD_OTSU\s+1\b", header)
    assert (_native.THRESHOLD_LI, _native.THRESHOLD_OTSU) == (0, 1)
    assert "com_refine_points" in features.__all__ and "com_refine_device" in distributed.__all__
    assert lib.zk_abi_version() == 2


def test_host_checks_raise_before_any_launch():
    """Every precondition of com_refine_points that the host can see is a ValueError naming it, with no device needed; empty
    points (or points the border clearing drops) come back as (0, 2)."""
    from mtflearn_amd import features
    data = np.zeros((32, 40), np.float32)
    ok = np.array([[10.0, 12.0]])
    for bad_data, pts, size, what in ((data.astype(np.int32), ok, 5, "float32 or float64"), (data.astype(np.uint8), ok, 5, "float32 or float64"),
                                      (data.astype(np.float16), ok, 5, "float32 or float64"), (data[None], ok, 5, "2-D"),
                                      (data, np.array([10.0, 12.0, 3.0]), 5, r"\(N, 2\)"), (data, np.array([[1 + 2j, 3]]), 5, "real points"),
                                      (data, ok, 1, "size"), (data, ok, 65, "size"), (data, ok, 4.5, "size"),
                                      (data, np.array([[np.nan, 12.0]]), 5, "finite"), (data, np.array([[np.inf, 12.0]]), 5, "finite")):
        with pytest.raises(ValueError, match=what):
            features.com_refine_points(pts, bad_data, size)
    with pytest.raises(ValueError, match="2\\^24"):
        features.com_refine_points(np.broadcast_to(np.array([[4, 4]], np.int32), (2 ** 24, 2)), data, 3)
    for threshold in (None, "otsu"):
        assert features.com_refine_points(np.empty((0, 2)), data, 5, threshold).shape == (0, 2)
        assert features.com_refine_points([], data, 5, threshold).dtype == np.float64
        assert features.com_refine_points(np.array([[1, 1], [39, 31]]), data, 5, threshold).shape == (0, 2)      # all cleared
    xy, t, it = features.com_refine_points(np.empty((0, 2)), data, 5, return_thresholds=True)
    assert xy.shape == (0, 2) and t.shape == (0,) and it.shape == (0,) and it.dtype == np.int32
