"""The kernels of csrc/zk_graph.hip one by one against the extended-precision statements of tests/graph_reference.py:
every instantiation of the matrix-core search, the candidate parts and their merge, the three scalar-operand kernels,
equal distances across every boundary where "the smaller index first" is implemented, rows without variation, the
bisection of the affinities at converging and at never-converging settings, and what the entry point refuses.

Bounds.  Indices: equal to the reference on EVERY row -- tests/test_graph_reference_cpu.py holds that on each input used
here the distances that decide a row's list are more than 1e-11 apart (or exactly equal, where the index decides).
Distances: |d - d_ref| <= 1e-13.  Affinities: the reference bisects on the distances the device returned; no step of it
comes within 1e-9 of the 1e-5 tolerance (asserted), so the device's beta is the reference's or the element bound
(4 + v beta) 2^-52 P_ref breaks; elements on the machine-epsilon floor and column 0 are equal exactly.
Every test prints its largest figures (pytest -s).

Largest figures observed, measured on one run on an MI355X (bound 1e-13 for the distances, 1 for the affinities):
  distance error, matrix-core kernels          1.3e-15 (1000 x 81, k = 16, <16, 24>; all 14 instantiations ran)
  distance error, parts + merge                1.1e-15 (2100 x 40, k = 16, two parts), bit-identical between settings
  distance error, knn_kernel<16, 4>            1.6e-15 (1000 x 96, k = 16); 4.5e-16 at D = 3
  distance error, knn_kernel<32, 1> / <64, 1>  1.8e-15 (777 x 91, every k)
  distance error, planted runs / constant rows 1.1e-15 / 8.9e-16
  affinity error as a fraction of its bound    0.44 (1000 x 20, k = 17, perplexity 8.5, local_connectivity 3)

A row without variation is one whose features are all equal, whatever its float64 mean rounds to: twelve features
of 0.1 (mean 0.09999999999999999) and 1e-3 are among the planted rows and must come out as zeros like 0.0 and 1.0.
"""
import numpy as np
import pytest

import graph_reference as gr

pytestmark = pytest.mark.gpu

ATOL = 1e-13


@pytest.fixture(scope="module")
def run():
    """run(X, k, lc, perplexity) -> (dist, ind, P) through DeviceRows and _knn_affinities."""
    from mtflearn_amd.clustering import DeviceRows
    from mtflearn_amd.manifold import _knn_affinities

    def call(X, k, lc=None, perplexity=None):
        with DeviceRows(X) as rows:
            return _knn_affinities(rows, k, min(1, k - 1) if lc is None else lc, k if perplexity is None else perplexity)
    return call


class Figures:
    """Mismatches of one test, collected so that one bad case does not hide the others, and its largest distance error."""

    def __init__(self):
        self.err, self.where, self.bad = 0.0, None, []

    def knn(self, where, dist, ind, ref):
        if not np.isfinite(dist).all():
            self.bad.append(f"{where}: {np.count_nonzero(~np.isfinite(dist))} distances are not finite")
            return
        wrong = np.flatnonzero((ind != ref.ind).any(axis=1))
        if wrong.size:
            r = int(wrong[0])
            self.bad.append(f"{where}: {wrong.size} rows with other neighbours, first row {r}: {ind[r].tolist()} for {ref.ind[r].tolist()}")
        err = float(np.abs(dist - ref.dist).max(initial=0.0))
        if err >= self.err:
            self.err, self.where = err, where
        if err > ATOL:
            self.bad.append(f"{where}: distance error {err:.3e} above {ATOL:.0e}")

    def close(self, name):
        print(f"\n[{name}] largest distance error {self.err:.3e} at {self.where}")
        assert not self.bad, "\n".join(self.bad)


@pytest.fixture
def fig():
    return Figures()


def test_every_matrix_core_instantiation(run, fig, request, monkeypatch):
    monkeypatch.delenv("ZK_KNN_SCALAR", raising=False)
    monkeypatch.delenv("ZK_KNN_PARTS", raising=False)
    ran = set()
    for n, d, k in gr.MFMA_CASES:
        X = gr.offset_rows(n, d, gr.MFMA_SEED)
        dist, ind, _ = run(X, k)
        fig.knn(f"{n} x {d}, k = {k}, <K, NS> = {gr.mfma_instance(d, k)}", dist, ind, gr.knn(X, k))
        ran.add(gr.mfma_instance(d, k))
    print(f"\ninstantiations run: {sorted(ran)}")
    assert ran == gr.MFMA_INSTANCES and len(ran) == 14
    fig.close(request.node.name)


@pytest.mark.parametrize("shape,settings", gr.PARTS_CASES, ids=["2100x40", "1600x50"])
def test_candidate_parts_and_the_merge(run, fig, request, monkeypatch, shape, settings):
    monkeypatch.delenv("ZK_KNN_SCALAR", raising=False)
    n, d, seed = shape
    X = gr.offset_rows(n, d, seed)
    for k in gr.PARTS_KS:
        ref, first = gr.knn(X, k), None
        for parts in settings:
            if parts is None:
                monkeypatch.delenv("ZK_KNN_PARTS", raising=False)
            else:
                monkeypatch.setenv("ZK_KNN_PARTS", str(parts))
            dist, ind, _ = run(X, k)
            fig.knn(f"{n} x {d}, k = {k}, ZK_KNN_PARTS = {parts}", dist, ind, ref)
            if first is None:
                first = dist, ind
            else:                                                       # the same bits however the candidates are cut
                np.testing.assert_array_equal(ind, first[1], err_msg=f"k = {k}, parts = {parts}")
                np.testing.assert_array_equal(dist, first[0], err_msg=f"k = {k}, parts = {parts}")
    fig.close(request.node.name)


@pytest.mark.parametrize("d", (3, 45, 96))
def test_the_four_wave_scalar_kernel(run, fig, request, monkeypatch, d):
    monkeypatch.setenv("ZK_KNN_SCALAR", "1")
    for n, dd in gr.SCALAR_SHAPES:
        if dd != d:
            continue
        X = gr.scalar_rows(n, d)
        for k in gr.SCALAR_KS:
            if k <= n:
                dist, ind, _ = run(X, k)
                fig.knn(f"{n} x {d}, k = {k}", dist, ind, gr.knn(X, k))
    fig.close(request.node.name)


@pytest.mark.parametrize("k", gr.WIDE_KS)
def test_the_one_wave_scalar_kernels(run, fig, request, monkeypatch, k):
    monkeypatch.delenv("ZK_KNN_SCALAR", raising=False)
    for n, d in gr.wide_shapes(k):
        X = gr.offset_rows(n, d, gr.WIDE_SEED)
        dist, ind, _ = run(X, k)
        fig.knn(f"{n} x {d}, k = {k}", dist, ind, gr.knn(X, k))
    fig.close(request.node.name)


KERNELS = {"matrix-core, one part": {"ZK_KNN_PARTS": "1"}, "matrix-core, two parts": {"ZK_KNN_PARTS": "2"},
           "scalar-operand": {"ZK_KNN_SCALAR": "1"}}


@pytest.mark.parametrize("d", gr.TIE_DS)
def test_equal_distances_go_by_index_across_every_boundary(run, fig, request, monkeypatch, d):
    X = gr.tie_rows(d)
    for k in gr.TIE_KS:
        ref = gr.knn(X, k)
        for name, env in KERNELS.items():
            monkeypatch.delenv("ZK_KNN_SCALAR", raising=False)
            monkeypatch.delenv("ZK_KNN_PARTS", raising=False)
            for var, value in env.items():
                monkeypatch.setenv(var, value)
            dist, ind, _ = run(X, k)
            for start, length in gr.TIE_RUNS:
                m, members = min(k, length), slice(start, start + length)
                first = np.broadcast_to(np.arange(start, start + m), (length, m))
                if (ind[members, :m] != first).any() or (dist[members, :m] != dist[members, :1]).any():
                    r = start + int(np.flatnonzero((ind[members, :m] != first).any(axis=1) | (dist[members, :m] != dist[members, :1]).any(axis=1))[0])
                    fig.bad.append(f"{name}, D = {d}, k = {k}: row {r} of the run at {start} returns {ind[r].tolist()} at {dist[r].tolist()}")
            fig.knn(f"{name}, D = {d}, k = {k}", dist, ind, ref)           # every row, the runs' members included
    fig.close(request.node.name)


@pytest.mark.parametrize("n,d", gr.CONSTANT_SHAPES)
def test_rows_without_variation_are_at_distance_one_from_everything(run, fig, request, monkeypatch, n, d):
    X, at = gr.constant_rows(n, d), gr.constant_index(n)
    for k in gr.CONSTANT_KS:
        ref = gr.knn(X, k)
        for scalar in ((False, True) if k <= 16 else (False,)):
            monkeypatch.delenv("ZK_KNN_PARTS", raising=False)
            monkeypatch.setenv("ZK_KNN_SCALAR", "1" if scalar else "0")
            dist, ind, P = run(X, k)
            where = f"{n} x {d}, k = {k}, {'scalar-operand' if scalar or k > 16 else 'matrix-core'} kernel"
            assert np.isfinite(dist).all() and np.isfinite(P).all(), where
            for r in at:
                if ind[r].tolist() != list(range(k)) or (dist[r] != 1.0).any():
                    fig.bad.append(f"{where}: constant row {r} (value {X[r, 0]}) returns {ind[r].tolist()} at {dist[r].tolist()}")
            fig.knn(where, dist, ind, ref)
    fig.close(request.node.name)


@pytest.mark.parametrize("n,d,k,settings", gr.affinity_cases(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_affinities(run, request, monkeypatch, n, d, k, settings):
    monkeypatch.delenv("ZK_KNN_SCALAR", raising=False)
    monkeypatch.delenv("ZK_KNN_PARTS", raising=False)
    X = gr.affinity_rows(n, d)
    knn_ref = gr.knn(X, k)
    worst, where, bad, exhausted, converged = 0.0, None, [], [], []
    for perplexity, lc in settings:
        dist, ind, P = run(X, k, lc, perplexity)
        what = f"{n} x {d}, k = {k}, perplexity {perplexity}, local_connectivity {lc}"
        np.testing.assert_array_equal(ind, knn_ref.ind, err_msg=what)
        np.testing.assert_allclose(dist, knn_ref.dist, rtol=0, atol=ATOL, err_msg=what)
        ref = gr.affinities(dist, perplexity, lc)                       # on the distances the device itself returned
        assert ref.margin.min() > gr.MARGIN_MIN, f"{what}: row {int(np.argmin(ref.margin))} is undecided ({ref.margin.min():.3e})"
        if gr.surely_exhausts(k, perplexity, lc):
            assert not ref.converged.any() and (ref.steps == gr.N_STEPS).all(), what
        exhausted += [what] * (not ref.converged.any())
        converged += [what] * bool(ref.converged.all())
        bound = gr.affinity_bound(dist, lc, ref)
        err = np.abs(P - ref.P)
        assert np.isfinite(P).all() and (P[:, 0] == 0.0).all(), what
        exact = bound == 0.0
        if (err[exact] != 0.0).any():
            bad.append(f"{what}: {np.count_nonzero(err[exact])} elements of column 0 / on the epsilon floor differ")
        ratio = float((err[~exact] / bound[~exact]).max(initial=0.0))
        if ratio >= worst:
            worst, where = ratio, what
        if ratio > 1.0:
            r, j = np.argwhere((err > bound) & ~exact)[0]
            bad.append(f"{what}: P[{r}, {j}] = {P[r, j]!r} for {ref.P[r, j]!r}, {ratio:.3e} of the bound (beta {ref.beta[r]!r}, "
                       f"{ref.steps[r]} steps)")
    print(f"\n[{request.node.name}] largest affinity error {worst:.3e} of its bound at {where}; "
          f"all rows exhaust 100 steps in {len(exhausted)} settings, all converge in {len(converged)}")
    assert not bad, "\n".join(bad)
    assert exhausted and converged, f"every row exhausts the steps in {exhausted}, every row converges in {converged}"


def test_one_neighbour_has_no_affinities(run):
    dist, ind, P = run(gr.affinity_rows(130, 45), 1, 0, 1.0)
    np.testing.assert_array_equal(ind[:, 0], np.arange(130))
    assert P.shape == (130, 1) and (P == 0.0).all()


def test_refusals(run):
    X = gr.offset_rows(16, 8, gr.MFMA_SEED)
    for k in (0, 65, 17):                                              # k = 0, k > 64, k = N + 1
        with pytest.raises(RuntimeError, match="need 1 <= n_neighbors <= min"):
            run(X if k != 65 else gr.offset_rows(129, 8, gr.MFMA_SEED), k, 0, 2.0)
    with pytest.raises(RuntimeError, match="bad affinity parameters"):
        run(X, 5, 5, 5.0)                                              # local_connectivity = k
    with pytest.raises(RuntimeError, match="bad affinity parameters"):
        run(X, 5, 1, 0.0)                                              # perplexity = 0
    rng = np.random.default_rng(9)
    wide = rng.standard_normal((40, 97))
    for k in (5, 17):                                                  # D > 96 is refused for every k
        with pytest.raises(RuntimeError, match="too many features for the query tile"):
            run(wide, k)
    for k in (5, 17):                                                  # ... and D = 96 is not
        dist, ind, _ = run(wide[:, :96], k)
        ref = gr.correlation_knn(wide[:, :96], k)
        assert ref.gap.min() > gr.GAP_MIN
        np.testing.assert_array_equal(ind, ref.ind)
        np.testing.assert_allclose(dist, ref.dist, rtol=0, atol=ATOL)
