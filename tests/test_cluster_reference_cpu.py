"""tests/cluster_reference.py checked without a GPU: against scikit-learn's own routines and the NumPy stand-in (HostRows), and
-- on the very inputs of tests/test_gpu_cluster_kernels.py and tests/test_gpu_consumers.py -- that every label those tests
compare exactly is decided (margin above the bound), that no E-step row is undecided, and that the exact-arithmetic inputs
stay below 2^53.  The grids are taken for the 256 CUs of an MI355X."""

import numpy as np
import pytest

import cluster_reference as ref
import test_gpu_cluster_kernels as K
import test_gpu_consumers as G
from test_clustering_sharded_cpu import HostRows

N_CU = 256


def test_lloyd_matches_sklearn_kmeans():
    from sklearn.cluster import KMeans
    rng = np.random.default_rng(0)
    X = np.concatenate([rng.standard_normal((200, 5)) + c for c in (0.0, 4.0, -5.0)])
    model = KMeans(n_clusters=3, random_state=0, n_init=1).fit(X)
    mean = X.mean(axis=0)
    labels, margin, sums, mags, counts, changed = ref.lloyd(X, mean, model.cluster_centers_ - mean)
    np.testing.assert_array_equal(labels, model.labels_)
    assert margin.min() > 1e-6 and changed == len(X)
    inertia = float(ref.own_distance(X, mean, model.cluster_centers_ - mean, labels)[0].sum())
    assert abs(inertia - model.inertia_) <= 1e-10 * model.inertia_
    np.testing.assert_allclose((sums / counts[:, None]).astype(float) + mean, model.cluster_centers_, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(counts, np.bincount(model.labels_))


def test_estep_matches_sklearn_log_prob():
    from sklearn.mixture import GaussianMixture
    rng = np.random.default_rng(1)
    X = np.concatenate([rng.standard_normal((150, 4)) * s + c for s, c in ((1.0, 0.0), (0.5, 3.0))])
    for kind in ("full", "diag"):
        gm = GaussianMixture(2, covariance_type=kind, random_state=0).fit(X)
        chol = gm.precisions_cholesky_ if kind == "full" else np.stack([np.diag(p) for p in gm.precisions_cholesky_])
        log_det = np.log(np.einsum("kii->ki", chol)).sum(axis=1)
        total, mags, labels, margin, resp = ref.estep(X, chol, gm.means_, log_det, np.log(gm.weights_))
        np.testing.assert_array_equal(labels, gm.predict(X))
        assert abs(float(total) - gm.score_samples(X).sum()) <= 1e-10 * abs(gm.score_samples(X).sum())
        np.testing.assert_allclose(resp.astype(float), gm.predict_proba(X), rtol=0, atol=1e-12)
        lab2, mar2, _ = ref.estep_labels(X, chol, gm.means_, log_det, np.log(gm.weights_), screen=1.0)   # every row refined
        np.testing.assert_array_equal(lab2, labels)
        np.testing.assert_allclose(mar2.astype(float), margin.astype(float), rtol=1e-9, atol=1e-12)
        assert mags.sum() > abs(total)


def test_reference_matches_the_numpy_stand_in():
    X = K.float_matrix(449, 17, 0)
    host = HostRows(X)
    mean = X.mean(axis=0)
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a, dtype=float), b, rtol=1e-11, atol=1e-11)
    close(ref.colsum(X)[0], host.colsum())
    sq, xsq, bad = ref.center_at(X, mean)
    close(sq, host.center_at(mean)[0])
    close(xsq, host.xsq)
    cand = host.fetch([3, 77, 400])
    csq = np.einsum("ij,ij->i", cand, cand)
    dist, pot, mag = ref.seed_step(X, mean, cand, csq)
    close(pot, host.seed_step(cand, csq, False))
    vals = np.array([0.1, 0.5, 0.9]) * float(pot[1])
    idx, margin = ref.seed_pick(dist[1], vals)
    np.testing.assert_array_equal(idx, host.seed_pick(1, vals))
    assert margin.min() > 1e-9
    close(ref.seed_step(X, mean, cand, csq, np.asarray(dist[1], dtype=float))[1], host.seed_step(cand, csq, True))
    _, centres = K.lloyd_centres(X, 9, 0)
    labels, margin, sums, mags, counts, changed = ref.lloyd(X, mean, centres)
    s_h, c_h, ch_h = host.lloyd(centres, True)
    np.testing.assert_array_equal(labels, host.labels())
    close(sums, s_h)
    np.testing.assert_array_equal(counts, c_h)
    assert changed == ch_h
    close(ref.own_distance(X, mean, centres, labels)[0], host.own_distance(centres))
    mix = K.mixture(X, 5, "full", 0)
    total, mags, labels, margin, resp = ref.estep(X, *mix)
    assert abs(float(total) - host.estep(*mix)) <= 1e-11 * abs(float(total))
    np.testing.assert_array_equal(labels, host.labels())
    close(ref.moments(X, resp[:, 2], mean)[0], host.moments(2, mean))
    close(ref.moments(X, None, mean)[0], host.gram(mean))
    comp = np.random.default_rng(0).standard_normal((4, 17))
    close(ref.project(X, mean, comp)[0], host.project(mean, comp))


def test_exact_statements_agree_with_python_integers():
    """The integer-valued float64 statements against arbitrary-precision integers on a small dyadic matrix."""
    rng = np.random.default_rng(2)
    Q = rng.integers(-8, 9, (50, 4)).astype(np.int16)
    S = rng.integers(-4, 5, 4).astype(np.float64)
    C = rng.integers(-8, 9, (5, 4)).astype(np.float64)
    z = [[int(q) - int(s) for q, s in zip(row, S)] for row in Q]
    score = [[sum(int(c) * int(c) for c in cen) - 2 * sum(a * int(c) for a, c in zip(row, cen)) for cen in C] for row in z]
    labels = [min(range(5), key=lambda j: (sc[j], j)) for sc in score]
    got = ref.exact_lloyd(Q, S, C)
    np.testing.assert_array_equal(got[0], labels)
    for j in range(5):
        rows = [row for row, l in zip(z, labels) if l == j]
        np.testing.assert_array_equal(got[1][j] * 4, [sum(r[i] for r in rows) for i in range(4)])
        assert got[2][j] == len(rows)
        g = ref.exact_moments(Q, S, got[0], j) * 16
        assert g[0, 1] == sum(r[0] * r[1] for r in rows) and g[4, 4] == 16 * len(rows) and g[2, 4] == 4 * sum(r[2] for r in rows)
    np.testing.assert_array_equal(ref.exact_center(Q, S)[1] * 16, [sum(a * a for a in row) for row in z])
    d, pot = ref.exact_seed(Q, S, C[:2])
    assert d[1, 7] * 16 == sum((a - int(c)) ** 2 for a, c in zip(z[7], C[1]))
    np.testing.assert_array_equal(ref.exact_own_distance(Q, S, C, got[0]) * 16,
                                  [sum((a - int(c)) ** 2 for a, c in zip(row, C[l])) for row, l in zip(z, labels)])


@pytest.mark.parametrize("d,ragged", K.EXACT_SHAPES)
def test_exact_inputs_stay_below_2_53_and_fill_three_rounds(d, ragged):
    Q, S, centres, cand, comp = K.exact_case(d, ragged, N_CU)
    n = len(Q)
    assert ref.exact_headroom(Q, S, np.concatenate(list(centres.values()) + [cand])) < 2.0 ** 53
    assert np.abs(comp).sum(axis=1).max() * np.abs(Q - S).max() * 16 < 2.0 ** 53
    assert n % 64 == ragged % 64
    workers = [K.row_workers(d, N_CU)] + [K.lloyd_workers(d, k, N_CU) for k in K.EXACT_K] + \
              [K.wgram_workers(d, c, N_CU, v) for c in (1, 3) for v in (False, True)]
    for w in workers:
        assert min(K.rounds(n, w)) >= 3
    assert {K.tile_bufs(dd) for dd, _ in K.EXACT_SHAPES} == {1, 2}


def test_lloyd_and_moment_inputs_are_decided():
    for n, d in K.LLOYD_SHAPES:
        X = K.float_matrix(n, d, 2)
        for k in K.LLOYD_K:
            mean, centres = K.lloyd_centres(X, k, 3)
            assert ref.lloyd(X, mean, centres)[1].min() > K.LLOYD_MARGIN, (n, d, k)
    for d in (1, 2, 16, 17, 33, 47, 48, 91, 127):
        for n in K.SMALL_N:
            X, mean, centres = K.onehot_case(n, d)
            labels, margin = ref.lloyd(X, mean, centres)[:2]
            assert margin.min() > K.LLOYD_MARGIN and len(np.unique(labels)) == 8, (n, d)


def test_tie_inputs_tie_exactly():
    for n, d in K.TIE_SHAPES:
        for k in K.TIE_K:
            Q, Ck = K.tie_case(n, d, k)
            z = Q[::7][0]
            if k > 2:
                assert ((z - Ck[1]) ** 2).sum() == ((z - Ck[2]) ** 2).sum() == 1 and not np.array_equal(Ck[1], Ck[2])
                assert np.sort(((z - Ck) ** 2).sum(axis=1))[2] > 1          # the tie between 1 and 2 is the winning one
            labels = ref.exact_lloyd(Q, np.zeros(d), Ck)[0]
            np.testing.assert_array_equal(labels, ref.lloyd(Q, np.zeros(d), Ck)[0])       # both statements keep the lower index
            assert not np.any(labels == k - 1) and np.any(labels == 0)


@pytest.mark.parametrize("n,d,k,kind", K.ESTEP_CASES)
def test_estep_inputs_have_no_undecided_row(n, d, k, kind):
    X, mix = K.estep_case(n, d, k, kind)
    total, mags, labels, margin, resp = ref.estep(X, *mix, want_resp=False)
    assert int(np.sum(margin <= K.ESTEP_MARGIN * mags)) == 0


def test_large_estep_input_has_no_undecided_row():
    X, mix = K.estep_big_case(N_CU)
    labels, margin, mags = ref.estep_labels(X, *mix)
    assert int(np.sum(margin <= K.ESTEP_MARGIN * mags)) == 0 and len(np.unique(labels)) == 2
    for valu in (False, True):
        w, rows = K.estep_workers(17, 2, N_CU, valu)
        assert min(K.rounds(len(X), w, rows)) >= 3


def test_estep_inputs_of_the_consumer_tests_have_no_undecided_row():
    """The two E-step tests of tests/test_gpu_consumers.py compare labels exactly: every row of every input is decided."""
    cases = list(G.edge_estep_cases()) + list(G.matrix_core_estep_cases())
    assert len(cases) > 60
    for X, mix in cases:
        labels, margin, mags = ref.estep_labels(X, *mix)
        assert int(np.sum(margin <= K.ESTEP_MARGIN * mags)) == 0, (X.shape, len(mix[1]))


@pytest.mark.parametrize("d,k,valu", [c for c in K.DUPLICATE_CASES if not c[2]])
def test_duplicate_mixtures_are_decided_but_for_the_copy(d, k, valu):
    X, mix = K.duplicate_case(d, k)
    total, mags, labels, margin, _ = ref.estep(X, *[a[:k - 1] for a in mix], want_resp=False)
    assert int(np.sum(margin <= K.ESTEP_MARGIN * mags)) == 0 and np.any(labels == 0)
    full = ref.estep(X, *mix, want_resp=False)
    np.testing.assert_array_equal(full[2], labels)                            # the first maximum: the copy never wins
    assert np.all(full[3][labels == 0] == 0)                                   # and where component 0 wins, it ties exactly


def test_lloyd_inputs_of_the_consumer_tests_are_decided():
    """test_row_passes_on_edge_shapes compares Lloyd labels with HostRows exactly: every row of every pass is decided."""
    cases = list(G.edge_lloyd_cases())
    assert len(cases) > 100
    for X, mean, centres in cases:
        assert ref.lloyd(X, mean, centres)[1].min() > K.LLOYD_MARGIN, (X.shape, len(centres))
