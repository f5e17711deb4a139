"""The point-set kernels past the near-uniform sets of tests/refine_cases.py and tests/vnn_cases.py: the ring search of
``knn_kernel`` and the cells of ``build_cell`` on the sets of tests/point_cases.py, the reductions of ``zk_knn_stats`` past one
grid-stride trip and at the corrections of the histogram rule, ``bin_start_kernel`` where bins outnumber points, and the vertex
cap of ``clip_cell`` at its boundary.  NumPy only: no golden, no SciPy, no scikit-learn (tests/test_refine_reference_cpu.py and
tests/test_vnn_reference_cpu.py check the references used here against both).

Criteria.
  neighbour distances   bit-equal to brute force in float64 with the kernel's own expression (``point_cases.knn_reference``); a
                        difference is diagnosed in the failure message: how many entries differ, whether each lies within one
                        ``np.spacing`` of the reference, and whether the squared distance under the root is identical.
  reductions            exact: every entry of the synthetic matrices is a multiple of 2^-10 below 1024, so every partial sum
                        is exact in float64 whatever the tree order; histograms count for count equal to ``np.histogram``.
  cells                 those of tests/test_gpu_vnn.py with the brute-force oracle of tests/vnn_oracle.py in place of the golden:
                        pair lists equal, edge lengths within 4 spacings, ridge lengths within ``tol_rel a`` (``tol_rel`` of
                        tests/golden/vnn_golden.npz, ``a`` the oracle's median edge length), two runs identical byte for byte.
  wheels                a hub of s spokes: s <= 28 equals the oracle (clipping with any subset S of the final neighbours after
                        the four corners gives at most |S| + 4 sides, so the polygon never passes 32 on the way); 29 <= s <= 32
                        equals the oracle or raises the ``more than 32`` error, which of the two is printed, and it may raise
                        only where the restated clipping order passes 32 vertices on the way; s >= 33 raises it."""
import functools
import os

import numpy as np
import pytest

import point_cases as pc
import vnn_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, distributed, graph

pytestmark = pytest.mark.gpu

KS = tuple(range(2, 13))


def ptr(a):
    return a.ctypes.data_as(_native.c_void_p)


# ---------------------------------------------------------------------------------------------------------
# the sets are what their names say (no GPU code runs here)
# ---------------------------------------------------------------------------------------------------------
def test_the_sets_have_the_properties_they_are_named_for():
    sets = pc.knn_sets()
    for n in pc.TINY_NS:
        g = pc.grid_side(n)
        assert len(sets[f"tiny_{n}"]) == n and (g * g + 1 > n) == (n in (1, 3, 4, 9))
    for name, pts in sets.items():
        if name not in ("many_duplicates", "on_bin_sides"):
            assert len(np.unique(pts, axis=0)) == len(pts), name

    pts = sets["blob_and_halo"]
    frame = pc.knn_frame(pts)
    g = frame[3]
    bins = pc.bin_of(pts, frame)
    share = np.bincount(bins[:, 1] * g + bins[:, 0], minlength=g * g).max() / len(pts)
    assert len(pts) == 4000 and share >= 0.7
    reach = 0                                            # the brute-force twelfth neighbour of a halo point, in bins
    for i in range(pc.HALO_START, len(pts)):
        j = np.argsort(np.hypot(*(pts - pts[i]).T), kind="stable")[11]
        reach = max(reach, int(np.abs(bins[j] - bins[i]).max()))
    assert reach >= 3

    pts = sets["strip"]
    frame = pc.knn_frame(pts)
    assert len(pts) == 4096 and frame[3] == 46 and np.unique(pc.bin_of(pts, frame)[:, 1]).tolist() == [0]

    pts = sets["on_bin_sides"]
    x0, y0, h, g = pc.knn_frame(pts)
    assert (len(pts), x0, y0, h, g) == (2048, 0.0, 0.0, 2.0, 32) and np.all(pts % h == 0)
    assert np.unique(pts, axis=0, return_counts=True)[1].max() == 2
    ref = pc.knn_reference(pts, 12)
    assert (ref[:, 1:] == np.roll(ref, 1, axis=1)[:, 1:]).mean() > 0.5      # exact distance ties

    pts = sets["two_scales"]
    assert len(pts) == 24 * 24 + 40 * 40
    d1 = pc.knn_reference(pts, 2)[:, 1]
    assert 40 < np.median(d1[:576]) / np.median(d1[576:]) < 90          # a density step of 64

    pts = sets["far_offset"]
    x0, y0, h, g = pc.knn_frame(pts)
    assert len(pts) == 301 and np.any((pts[:, 1] - y0) + y0 != pts[:, 1])       # y - y0 loses low bits
    assert len(np.unique(pc.bin_of(pts, (x0, y0, h, g))[:300], axis=0)) == 1

    pts = sets["many_duplicates"]
    assert len(pts) == 2000 and np.unique(pts, axis=0, return_counts=True)[1].tolist() == [20] * 100
    assert not pc.knn_reference(pts, 12).any()

    for n in pc.STATS_SIZES:                             # the planted extremes are where planted_rows says
        dd, rows = pc.stats_matrix(n), pc.planted_rows(n)
        assert dd.shape == (n, 12) and not dd[:, 0].any() and np.all(np.diff(dd, axis=1) >= 0) and np.all(dd * 1024 == np.rint(dd * 1024))
        if n > 1:
            assert int(np.argmin(dd[:, 1])) == rows[0] and {int(r) for r in np.argmax(dd[:, 1:], axis=0)} == set(rows[1:])
    assert {131072, 300000, 200} <= set(pc.planted_rows(300001)) and 131072 in pc.planted_rows(131073)
    for kind in pc.HIST_KINDS:                           # values on edges, beside them, at first and at last
        dd, edges, lasts = pc.hist_matrix(257, kind), pc.hist_edges(kind), pc.hist_lasts(kind)
        assert dd.min() == 0 and np.all(dd[:, 1:].max(axis=0) == lasts) and np.all(np.diff(dd, axis=1) >= 0)
        assert (dd[:-1, 1:] == lasts.min()).any()        # the smallest last also stands among the planted values
        inner = edges[0][1:-1]                           # the edges of k = 2, whose range is the smallest
        assert min(np.isin(v, dd).sum() for v in (inner, np.nextafter(inner, 0), np.nextafter(inner, np.inf))) > 100
    dd = pc.gaps_matrix(300001)
    u = np.unique(dd[:, 1])
    assert np.diff(u).min() == pc.Q and np.sort(np.diff(u))[1] >= 2 * pc.Q and len(np.unique(dd[:, 1:])) < 100
    assert dd[0, 1] + pc.Q == dd[300000, 1]


# ---------------------------------------------------------------------------------------------------------
# neighbour distances
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference12(name):
    pts = pc.knn_sets()[name]
    ref = pc.knn_reference(pts, min(12, len(pts)))
    ref.setflags(write=False)
    return ref


def assert_bit_equal(got, pts, k, what):
    want = np.ascontiguousarray(reference12(what)[:, :k])
    assert got.dtype == np.float64 and got.shape == want.shape, what
    if got.tobytes() == want.tobytes():
        return
    rows, cols = np.nonzero(got != want)
    one_ulp = np.abs(got[rows, cols] - want[rows, cols]) <= np.spacing(want[rows, cols])
    # is the reference's squared distance the same number as that of some point at the device's distance?
    same_square = []
    for r, c in zip(rows[:1000], cols[:1000]):
        dx, dy = pts[:, 0] - pts[r, 0], pts[:, 1] - pts[r, 1]
        sq = np.sort(dx * dx + dy * dy)
        same_square.append(bool(np.sqrt(sq[c]) == want[r, c] and abs(got[r, c] - np.sqrt(sq[c])) <= np.spacing(want[r, c])))
    worst = np.max(np.abs(got[rows, cols] - want[rows, cols]) / np.where(want[rows, cols] > 0, want[rows, cols], 1.0))
    pytest.fail(f"{what}, k = {k}: {len(rows)} of {got.size} entries differ from brute force (largest relative difference {worst:.3g}); "
                f"{int(one_ulp.sum())} of them within one spacing, {sum(same_square)} of the first {len(same_square)} with an identical squared "
                f"distance under the root; first at row {rows[0]} column {cols[0]}: {got[rows[0], cols[0]]!r} for {want[rows[0], cols[0]]!r}")


def ks_of(name):
    n = len(pc.knn_sets()[name])
    if name.startswith("tiny_"):
        return sorted({min(n, 12), 1})
    return (12, 1, 5) if name in ("blob_and_halo", "strip") else (12,)


@pytest.mark.parametrize("name", pc.KNN_NAMES)
def test_knn_distances_are_bit_equal_to_brute_force(name):
    pts = pc.knn_sets()[name]
    for k in ks_of(name):
        got = graph.knn_distances(pts, k=k)
        assert_bit_equal(got, pts, k, name)
        assert not got[:, 0].any() and np.all(np.diff(got, axis=1) >= 0)
    print(f"{name}: {len(pts)} points, k in {tuple(ks_of(name))}: bit-equal to brute force")


def test_knn_distances_of_int32_points_on_bin_sides():
    pts = pc.knn_sets()["on_bin_sides"]
    ipts, out = np.ascontiguousarray(pts.astype(np.int32)), np.empty((len(pts), 12))
    assert np.array_equal(ipts.astype(np.float64), pts)
    _native.check(_native.load().zk_knn_distances(0, ptr(ipts), _native.ZK_I32, len(ipts), 12, ptr(out)), "zk_knn_distances")
    assert_bit_equal(out, pts, 12, "on_bin_sides")


def test_knn_distances_of_resident_points_on_blob_and_halo():
    pts = pc.knn_sets()["blob_and_halo"]
    d_pts = _native.DeviceArray.from_numpy(pts)
    dd = _native.DeviceArray((len(pts), 12), np.float64, 0)
    _native.check(_native.load().zk_knn_distances_dev(0, _native.c_void_p(d_pts.data_ptr()), _native.ZK_F64, len(pts), 12,
                                                      _native.c_void_p(dd.data_ptr()), _native.c_void_p(0)), "zk_knn_distances_dev")
    assert_bit_equal(dd.numpy(), pts, 12, "blob_and_halo")
    t, k = distributed.estimate_d_device(d_pts, return_k=True)           # the whole resident entry runs on it, and agrees with the host's
    assert (t, k) == graph.estimate_d(pts, return_k=True) and t > 0


# ---------------------------------------------------------------------------------------------------------
# zk_knn_stats on synthetic matrices
# ---------------------------------------------------------------------------------------------------------
def host_stats(dd, op, params):
    dd = np.ascontiguousarray(dd)
    params = np.ascontiguousarray(params, dtype=np.float64)
    counts, sums = np.zeros(11 * 256, np.int64), np.zeros(22)
    _native.check(_native.load().zk_knn_stats(0, ptr(dd), len(dd), op, ptr(params), ptr(counts), ptr(sums)), "zk_knn_stats")
    return counts, sums


def resident_stats(dd, op, params):
    d_dd = _native.DeviceArray.from_numpy(np.ascontiguousarray(dd))
    return graph._knn_stats(0, d_dd.data_ptr(), len(dd), op, params, 0)


def both_stats(dd, op, params, resident):
    counts, sums = host_stats(dd, op, params)
    if resident:
        c2, s2 = resident_stats(dd, op, params)
        assert counts.tobytes() == c2.tobytes() and sums.tobytes() == s2.tobytes()
    return counts, sums


RESIDENT_TOO = 131073                                    # the size that also goes through graph._knn_stats on a resident copy


@pytest.mark.parametrize("n", pc.STATS_SIZES)
def test_ranges_past_one_grid_stride_trip(n):
    dd = pc.stats_matrix(n)
    _, sums = both_stats(dd, _native.KNN_RANGES, [0.0], n == RESIDENT_TOO)
    assert sums[0] == dd[:, 1].min() and np.array_equal(sums[1:12], dd[:, 1:].max(axis=0))
    assert not sums[12:].any()


@pytest.mark.parametrize("n", pc.STATS_SIZES)
def test_sides_with_tied_thresholds_are_exact(n):
    dd = pc.stats_matrix(n)
    shift = dd[:, 1].min()
    w = dd - shift
    # t_k = a value of column k - 1 of w itself: the comparison is strict, so the entries equal to it count as "the rest"
    ts = np.array([w[(7 * k) % n, k - 1] for k in KS])
    counts, sums = both_stats(dd, _native.KNN_SIDES, np.concatenate([[shift], ts]), n == RESIDENT_TOO)
    for c, k in enumerate(KS):
        d = w[:, 1:k]
        above = d > ts[c]
        assert (d == ts[c]).any() and np.all(d * 1024 == np.rint(d * 1024))
        assert counts[c] == int(above.sum()), (n, k)
        assert sums[2 * c] == d[above].sum() and sums[2 * c + 1] == d[~above].sum(), (n, k)
    assert not counts[11:].any()
    # thresholds of +inf, as Li's first pass sets them: everything is "the rest"
    counts, sums = host_stats(dd, _native.KNN_SIDES, [shift] + [np.inf] * 11)
    assert not counts.any() and not sums[0::2].any() and np.array_equal(sums[1::2], [w[:, 1:k].sum() for k in KS])


def hist_cases():
    for n in pc.STATS_SIZES:
        for kind in pc.HIST_KINDS if n in (257, 131073) else ("round",):
            yield n, kind


@pytest.mark.parametrize("n,kind", list(hist_cases()))
def test_histograms_at_the_edges_equal_numpys(n, kind):
    dd, lasts, edges = pc.hist_matrix(n, kind), pc.hist_lasts(kind), pc.hist_edges(kind)
    params = np.concatenate([[0.0], lasts] + edges)
    counts, _ = both_stats(dd, _native.KNN_HIST, params, n == RESIDENT_TOO and kind == "round")
    counts = counts.reshape(11, 256)
    for c, k in enumerate(KS):
        want, want_edges = np.histogram(dd[:, 1:k], bins=256, range=(0.0, lasts[c]))
        assert np.array_equal(want_edges, edges[c])
        assert want.sum() == n * (k - 1)                  # nothing fell outside the range
        assert np.array_equal(counts[c], want), (n, kind, k, np.nonzero(counts[c] != want)[0][:8])


def unique_gaps(w):
    """``np.diff(np.unique(w[:, 1:k])).min()`` for the eleven k, the unique values merged column by column."""
    out, seen = [], np.empty(0)
    for k in KS:
        seen = np.union1d(seen, w[:, k - 1])
        out.append(np.diff(seen).min() if len(seen) > 1 else np.inf)
    return np.array(out)


@pytest.mark.parametrize("n", pc.STATS_SIZES)
def test_gaps_find_one_planted_pair_far_apart(n):
    dd = pc.gaps_matrix(n)
    shift = dd[:, 1].min()
    want = unique_gaps(dd - shift)
    if n <= 257:
        assert np.array_equal(want, [np.diff(np.unique(dd[:, 1:k] - shift)).min() if n * (k - 1) > 1 else np.inf for k in KS])
    assert np.all(want == pc.Q) if n > 1 else want[0] == np.inf
    _, sums = both_stats(dd, _native.KNN_GAPS, [shift], n == RESIDENT_TOO)
    assert np.array_equal(sums[:11], want), n


def test_gaps_of_one_value_per_sample_and_of_negative_zero():
    dd = np.zeros((300, 12))
    dd[:, 1:] = 2.5                                     # a single distinct value in every sample: no gap
    assert np.array_equal(host_stats(dd, _native.KNN_GAPS, [2.5])[1][:11], [np.inf] * 11)
    assert np.array_equal(host_stats(dd, _native.KNN_GAPS, [0.0])[1][:11], [np.inf] * 11)
    dd = np.array(pc.gaps_matrix(257))
    dd[::3, 1] = 0.0                                    # zeros among the values: the smallest gap of d_2 .. is to 3 + 4 Q or Q
    plus = host_stats(dd, _native.KNN_GAPS, [0.0])[1]
    assert np.array_equal(plus[:11], unique_gaps(dd))
    minus = np.array(dd)
    minus[::6, 1] = -0.0
    assert np.signbit(minus[:, 1]).any() and np.array_equal(minus, dd)
    assert host_stats(minus, _native.KNN_GAPS, [0.0])[1].tobytes() == plus.tobytes()
    assert resident_stats(minus, _native.KNN_GAPS, [0.0])[1].tobytes() == plus.tobytes()


# ---------------------------------------------------------------------------------------------------------
# Voronoi cells
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tol_rel():
    with np.load(os.path.join(ROOT, "tests", "golden", "vnn_golden.npz")) as f:
        return float(f["tol_rel"])


@functools.lru_cache(maxsize=None)
def oracle_of(pts_bytes, n):
    """``(rows, (ijs, ridge, edge), a)`` of the brute-force oracle, once per set."""
    pts = np.frombuffer(pts_bytes, np.float64).reshape(n, 2)
    rows = oracle.rows(pts)
    nb = oracle.neighbours_from_rows(rows, n)
    return rows, nb, float(np.median(nb[2])) if len(nb[2]) else 1.0


def want_of(pts):
    return oracle_of(pts.tobytes(), len(pts))


def native_rows(pts):
    return tuple(a.numpy() for a in distributed.voronoi_neighbours_device(_native.DeviceArray.from_numpy(pts)))


def assert_cells_equal_oracle(pts, what, runs=(graph.voronoi_neighbours, native_rows)):
    _, (ijs, ridge, edge), a = want_of(pts)
    for run in runs:
        got = run(pts)
        assert got[0].dtype == np.int64 and got[0].shape == ijs.shape and np.array_equal(got[0], ijs), what
        worst = np.abs(got[1] - ridge).max()
        ulps = (np.abs(got[2] - edge) / np.spacing(edge)).max()
        print(f"{what} ({run.__name__}): {len(pts)} points, {len(ijs)} rows; ridge lengths differ by at most {worst / a:.3g} a "
              f"(tol {tol_rel():.3g} a), edge lengths by {ulps:.2f} spacings")
        assert worst <= tol_rel() * a and ulps <= 4, what
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, run(pts))), what


@pytest.mark.parametrize("name", pc.VORONOI_NAMES)
def test_voronoi_neighbours_equal_the_oracle(name):
    assert_cells_equal_oracle(pc.voronoi_sets()[name], name)


@pytest.mark.parametrize("name", pc.VORONOI_NAMES)
def test_vnn_graph_equals_the_oracle(name):
    pts = pc.voronoi_sets()[name]
    rows, _, a = want_of(pts)
    dmax = pc.DMAX_FACTOR * a
    want = oracle.graph_from_rows(rows, len(pts), pc.THRESHOLD, dmax)[0]
    assert len(want) > len(pts) / 2
    for run in (lambda: graph.vnn_graph(pts, threshold=pc.THRESHOLD, dmax=dmax),
                lambda: distributed.vnn_graph_device(_native.DeviceArray.from_numpy(pts), dmax, threshold=pc.THRESHOLD).numpy()):
        got = run()
        assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want), name
        assert run().tobytes() == got.tobytes()


def test_coincident_resident_points_are_refused():
    dup = pc.knn_sets()["many_duplicates"]
    with pytest.raises(RuntimeError, match="coincide"):
        distributed.voronoi_neighbours_device(_native.DeviceArray.from_numpy(dup))
    with pytest.raises(RuntimeError, match="coincide"):
        distributed.vnn_graph_device(_native.DeviceArray.from_numpy(dup), 1.0)
    assert_cells_equal_oracle(pc.wheel(25), "wheel_25 after the refusal", runs=(native_rows,))


@pytest.mark.parametrize("spokes", [s for s in pc.WHEEL_SPOKES if s <= 28])
def test_a_hub_of_up_to_28_spokes_never_reaches_the_cap(spokes):
    pts = pc.wheel(spokes)
    assert sum(j <= spokes for j, _, _ in want_of(pts)[0][0]) == spokes          # the hub's cell has that many sides
    assert_cells_equal_oracle(pts, f"wheel_{spokes}")


@pytest.mark.parametrize("spokes", [s for s in pc.WHEEL_SPOKES if 29 <= s <= 32])
def test_a_hub_of_29_to_32_spokes_is_exact_or_refused(spokes):
    """Equal to the oracle or refused, never anything else -- and refused only where the hub's polygon passes 32 vertices on the
    way: ``pc.hub_vertex_counts`` restates the clipping order, and on these wheels the polygon never holds more vertices than
    its final cell, so a refusal here would be a cap that is off by one."""
    pts = pc.wheel(spokes)
    assert sum(j <= spokes for j, _, _ in want_of(pts)[0][0]) == spokes
    on_the_way = max(pc.hub_vertex_counts(pts))
    try:
        graph.voronoi_neighbours(pts)
    except RuntimeError as err:
        assert "more than 32" in str(err)
        print(f"wheel_{spokes}: refused (at most {on_the_way} vertices on the way)")
        with pytest.raises(RuntimeError, match="more than 32"):                  # and the same on resident points
            native_rows(pts)
        assert on_the_way > 32, f"wheel_{spokes} was refused, but its polygon never holds more than {on_the_way} vertices"
        return
    print(f"wheel_{spokes}: computed (at most {on_the_way} vertices on the way)")
    assert_cells_equal_oracle(pts, f"wheel_{spokes}")


def test_a_hub_of_more_than_32_spokes_is_refused_and_the_next_call_succeeds():
    for spokes in (33, 34, 35, 36):
        pts = pc.wheel(spokes)
        assert sum(j <= spokes for j, _, _ in want_of(pts)[0][0]) == spokes
        with pytest.raises(RuntimeError, match="more than 32"):
            graph.voronoi_neighbours(pts)
        with pytest.raises(RuntimeError, match="more than 32"):
            distributed.vnn_graph_device(_native.DeviceArray.from_numpy(pts), 1.3)
    assert_cells_equal_oracle(pc.wheel(25), "wheel_25 after the last refusal")
