"""tests/graph_reference.py against scikit-learn and oracle/manifold_oracle.py, and the conditions under which
tests/test_gpu_graph_kernels.py may ask the device for exact indices and betas: on every input that file uses, every
row's deciding distances are further apart than ``GAP_MIN`` and every bisection step is further from the tolerance
than ``MARGIN_MIN`` -- for the reference alone, no GPU.  A seed that fails a condition is changed, never the condition."""
import numpy as np
import pytest

import graph_reference as gr


def _assert_decided(what, X, ks):
    for k in ks:
        ref = gr.knn(X, k)
        assert ref.ind.shape == (len(X), k) and np.isfinite(ref.dist).all(), what
        worst = int(np.argmin(ref.gap))
        assert ref.gap[worst] > gr.GAP_MIN, f"{what}, k = {k}: row {worst} has a gap of {ref.gap[worst]:.3e}"


# ------------------------------------------------------------------------------------------------ the references
def test_correlation_knn_against_scikit_learn():
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.default_rng(5)
    for n, d, k in [(300, 7, 5), (257, 45, 17), (64, 3, 1), (130, 91, 64), (40, 12, 40)]:
        X = rng.standard_normal((n, d)) + rng.standard_normal(d)
        d_sk, i_sk = NearestNeighbors(n_neighbors=k, metric="correlation", algorithm="brute").fit(X).kneighbors(X, n_neighbors=k)
        ref = gr.correlation_knn(X, k)
        assert ref.gap.min() > gr.GAP_MIN                   # no ties: scikit-learn's order is defined
        np.testing.assert_array_equal(ref.ind, i_sk)
        np.testing.assert_allclose(ref.dist, d_sk, rtol=0, atol=1e-13)
        cached = gr.knn(X, k)
        np.testing.assert_array_equal(cached.ind, ref.ind)
        np.testing.assert_array_equal(cached.dist, ref.dist)
        np.testing.assert_array_equal(cached.gap, ref.gap)


def test_gap_is_the_closest_pair_of_distinct_distances_up_to_the_first_one_left_out():
    # unit rows at chosen angles on the circle that D = 3 leaves: distances 1 - cos(angle difference)
    basis = np.array([[1.0, -1.0, 0.0], [1.0, 1.0, -2.0]]) / np.sqrt([[2.0], [6.0]])
    angles = np.array([0.0, 0.3, 0.3 + 1e-4, 1.0, 2.0])
    X = np.cos(angles)[:, None] * basis[0] + np.sin(angles)[:, None] * basis[1] + 5.0
    expect = 1 - np.cos(angles[:, None] - angles[None, :])
    ref = gr.correlation_knn(X, 2)
    np.testing.assert_array_equal(ref.ind, [[0, 1], [1, 2], [2, 1], [3, 2], [4, 3]])
    # row 0: ranks 0, 1, 2 are rows 0, 1, 2 and its smallest gap is the one to the row LEFT OUT (rank 2)
    np.testing.assert_allclose(ref.gap[0], expect[0, 2] - expect[0, 1], rtol=1e-9)
    np.testing.assert_allclose(ref.gap[1], expect[1, 2], rtol=1e-6)
    # duplicated rows: equal distances are no gap, and the smaller index goes first
    ref = gr.correlation_knn(np.concatenate([X, X]), 3)
    np.testing.assert_array_equal(ref.ind[0], [0, 5, 1])
    np.testing.assert_array_equal(ref.ind[6], [1, 6, 2])
    np.testing.assert_allclose(ref.gap[0], expect[0, 1], rtol=1e-9)
    assert gr.correlation_knn(X, 5).gap.shape == (5,)       # k = N: no rank k


def test_affinities_against_the_oracle():
    from oracle import manifold_oracle as mo
    for (n, d), k in [((130, 45), 17), ((130, 45), 5), ((200, 20), 2)]:
        dist = gr.knn(gr.affinity_rows(n, d) if n == 130 else gr.offset_rows(n, d, 3), k).dist
        for perplexity, lc in gr.affinity_settings(k):
            ref = gr.affinities(dist, perplexity, lc)
            assert ref.margin.min() > gr.MARGIN_MIN
            np.testing.assert_allclose(ref.P, mo.calculate_asymmetric_Pij(dist.copy(), perplexity=perplexity, local_conectivity=lc),
                                       rtol=1e-12, atol=0, err_msg=str((n, d, k, perplexity, lc)))
            assert ((ref.steps == gr.N_STEPS) | ref.converged).all() and (ref.steps >= 1).all()
    # the two ways out of the loop: three neighbours at rho keep the sum at 3 or more, above log2(1.5), for any beta
    ref = gr.affinities(dist=gr.knn(gr.affinity_rows(130, 45), 5).dist, perplexity=1.5, local_connectivity=3)
    assert not ref.converged.any() and (ref.steps == 100).all() and (ref.beta == 2.0 ** 100).all()
    assert (ref.P[:, 1:4] == 1.0).all() and (ref.P[:, 4] == gr.EPS).all()
    # ... and a target above what k - 1 terms can reach halves beta every time
    ref = gr.affinities(dist=gr.knn(gr.affinity_rows(130, 45), 2).dist, perplexity=6.0, local_connectivity=0)
    assert not ref.converged.any() and (ref.beta == 2.0 ** -100).all()


def test_runs_of_identical_rows_take_the_smallest_indices_of_their_run():
    for d in gr.TIE_DS:
        X = gr.tie_rows(d)
        for k in gr.TIE_KS:
            ref = gr.knn(X, k)
            for start, length in gr.TIE_RUNS:
                m = min(k, length)
                members = slice(start, start + length)
                np.testing.assert_array_equal(ref.ind[members, :m], np.broadcast_to(np.arange(start, start + m), (length, m)))
                assert (ref.dist[members, :m] == ref.dist[members, :1]).all() and (ref.dist[members, 0] < 1e-15).all()


# ------------------------------------------------------------------------------- the inputs of the GPU tests are decided
def test_the_matrix_core_cases_reach_every_instantiation_at_three_sizes():
    seen = {}
    for n, d, k in gr.MFMA_CASES:
        assert k <= n and k <= 16 and d <= 96
        seen.setdefault(gr.mfma_instance(d, k), set()).add(n)
    assert set(seen) == gr.MFMA_INSTANCES and len(seen) == 14
    for inst, ns in seen.items():
        assert min(ns) < 64 and ns & {64, 65} and 1000 in ns, (inst, sorted(ns))
    assert {d for _, d, _ in gr.MFMA_CASES} == set(gr.MFMA_DS) == {8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96}
    assert {k for _, _, k in gr.MFMA_CASES} == {1, 10, 11, 16}
    assert {n for n, _, _ in gr.MFMA_CASES} == {16, 17, 63, 64, 65, 129, 1000}
    assert all(n <= 2200 and n * n * d <= 2.5e8 for n, d, _ in gr.MFMA_CASES)


def test_the_matrix_core_inputs_are_decided():
    for n, d, k in gr.MFMA_CASES:
        _assert_decided(f"matrix-core case {n} x {d}", gr.offset_rows(n, d, gr.MFMA_SEED), [k])


def test_the_part_inputs_are_decided_and_split_as_the_test_says():
    for (n, d, seed), settings in gr.PARTS_CASES:
        _assert_decided(f"parts case {n} x {d}", gr.offset_rows(n, d, seed), gr.PARTS_KS)
        n_stages = (n + 63) // 64 * 64 // gr.stage_rows(d)
        assert n_stages // 16 == max(s for s in settings if s is not None and s < 16)      # the clamp the kernel applies
    assert gr.part_bounds(2100, 40, 2) == [0, 1024] and gr.part_bounds(1600, 50, 3) == [0, 512, 1056]


@pytest.mark.parametrize("d", (3, 45, 96))
def test_the_scalar_kernel_inputs_are_decided(d):
    for n, dd in gr.SCALAR_SHAPES:
        if dd == d:
            _assert_decided(f"scalar case {n} x {d}", gr.scalar_rows(n, d), [k for k in gr.SCALAR_KS if k <= n])
    assert {n for n, dd in gr.SCALAR_SHAPES if dd == d} >= {8, 9, 63, 65, 200, 1000}


def test_the_wide_list_inputs_are_decided():
    for k in gr.WIDE_KS:
        for n, d in gr.wide_shapes(k):
            _assert_decided(f"wide case {n} x {d}", gr.offset_rows(n, d, gr.WIDE_SEED), [k])


def test_the_tie_inputs_are_decided_and_straddle_what_they_name():
    for d in gr.TIE_DS:
        _assert_decided(f"tie case D = {d}", gr.tie_rows(d), gr.TIE_KS)     # equal distances are no gap: the rest is decided
    ends = sorted((s, s + l - 1) for s, l in gr.TIE_RUNS)
    assert all(a[1] < b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] == gr.TIE_N - 1

    def straddled(boundary):
        return any(s < boundary <= s + l - 1 for s, l in gr.TIE_RUNS)
    assert gr.stage_rows(40) == 64 and gr.stage_rows(50) == 32 and straddled(64) and straddled(32)
    assert straddled(gr.part_bounds(gr.TIE_N, 40, 2)[1]) and straddled(gr.part_bounds(gr.TIE_N, 50, 2)[1])
    span = gr.scalar_wave_span(gr.TIE_N)
    assert span == 528 and all(straddled(w * span) for w in (1, 2, 3))
    assert any(s // 16 == (s + l - 1) // 16 for s, l in gr.TIE_RUNS) and any(s % 16 == 0 for s, l in gr.TIE_RUNS)


def test_the_constant_row_inputs_are_decided_and_sit_at_distance_one():
    for n, d in gr.CONSTANT_SHAPES:
        X = gr.constant_rows(n, d)
        at = gr.constant_index(n)
        assert at == [0, 15, 16, 63, n - 1] and (X[at] == X[at][:, :1]).all() and (X[0] == 0).all()
        _assert_decided(f"constant rows in {n} x {d}", X, gr.CONSTANT_KS)
        for k in gr.CONSTANT_KS:
            ref = gr.knn(X, k)
            np.testing.assert_array_equal(ref.ind[at], np.broadcast_to(np.arange(k), (5, k)))
            assert (ref.dist[at] == 1.0).all() and np.isfinite(ref.dist).all()
        full = gr.knn(X, min(n, gr.K_MAX))
        assert ((full.dist == 1.0) == np.isin(full.ind, at))[np.setdiff1d(np.arange(n), at)].all()


@pytest.mark.parametrize("n,d", gr.AFFINITY_SHAPES)
def test_the_affinity_inputs_are_decided(n, d):
    X = gr.affinity_rows(n, d)
    _assert_decided(f"affinity case {n} x {d}", X, gr.AFFINITY_KS)
    for nn, dd, k, settings in gr.affinity_cases():
        if (nn, dd) != (n, d):
            continue
        dist = gr.knn(X, k).dist
        exhausted = converged = 0
        for perplexity, lc in settings:
            ref = gr.affinities(dist, perplexity, lc)
            worst = int(np.argmin(ref.margin))
            assert ref.margin[worst] > gr.MARGIN_MIN, f"k = {k}, perplexity {perplexity}, lc {lc}: row {worst} margin {ref.margin[worst]:.3e}"
            if gr.surely_exhausts(k, perplexity, lc):
                assert not ref.converged.any() and (ref.steps == gr.N_STEPS).all(), (k, perplexity, lc)
            exhausted += not ref.converged.any()
            converged += bool(ref.converged.all())
        assert exhausted and converged, (k, exhausted, converged)     # both ways out of the loop, for every k


def test_the_affinity_settings():
    assert gr.affinity_settings(2) == [(1.0, 0), (1.0, 1), (1.5, 0), (1.5, 1), (2.0, 0), (2.0, 1), (6.0, 0), (6.0, 1)]
    assert len(gr.affinity_settings(40)) == 16 and (1.5, 3) in gr.affinity_settings(5)
    assert gr.surely_exhausts(5, 1.5, 3) and gr.surely_exhausts(2, 6.0, 0) and not gr.surely_exhausts(5, 2.5, 0)
    cases = gr.affinity_cases()
    assert {(n, d) for n, d, _, _ in cases} == set(gr.AFFINITY_SHAPES) and {k for _, _, k, _ in cases} == set(gr.AFFINITY_KS)
    assert all(settings == gr.affinity_settings(k) for _, _, k, settings in cases)                 # the full cross everywhere
