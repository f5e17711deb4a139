"""CPU checks of the rotation alignment: the NumPy statement of tests/align_cases.py against ``zmoments.rotate``, the label
and argument checks (which run before any device call), and the NumPy twin of ``kmeans_aligned`` on planted data -- the
licence of the GPU tests in tests/test_gpu_align.py."""
import os
import re

import numpy as np
import pytest

import align_cases as ac
from mtflearn_amd import _native, zmoments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_SYMBOLS = ["zk_align_rows", "zk_align_rows_dev", "zk_align_set_host_chunk", "zk_rotate_rows", "zk_rotate_rows_dev"]


@pytest.mark.parametrize("n_max", [4, 8, 12])
def test_statement_recovers_exact_rotations(n_max):
    """z = rotate(t, alpha): the statement returns -alpha mod 360 within 1e-6 degree, and a score within the bound of |t|^2."""
    rows, t, alpha, n, m = ac.rotated_pairs(n_max, 200, seed=10 + n_max)
    mask = np.ones(len(n), bool)
    worst_angle = worst_score = 0.0
    for i in range(len(rows)):
        angle, score, best, _ = ac.align_statement(rows[i:i + 1], t[i:i + 1], n, m, mask)
        gap = ac.circular_gap(angle[0, 0], -alpha[i] % 360)
        short = abs(score[0, 0] - (t[i] ** 2).sum())
        worst_angle, worst_score = max(worst_angle, gap), max(worst_score, short / ac.score_bound(rows[i:i + 1], t[i:i + 1], n, m, mask)[0, 0])
        assert 0 <= angle[0, 0] < 360 and best[0] == 0
    print(f"n_max {n_max}: worst angle error {worst_angle:.3e} degree, worst score error {worst_score:.3f} of the bound")
    assert worst_angle <= 1e-6
    assert worst_score <= 1.0


def test_statement_symmetry_three():
    """Templates with only m in {0, 3, 6}: f has period 120; with symmetry=3 the angle lies in [0, 120) and is -alpha mod 120."""
    rows, t, alpha, n, m = ac.rotated_pairs(8, 100, seed=3, m_keep=(0, 3, 6))
    assert set(np.abs(m)) == {0, 3, 6}
    for i in range(len(rows)):
        angle, score, _, _ = ac.align_statement(rows[i:i + 1], t[i:i + 1], n, m, None, symmetry=3)
        assert 0 <= angle[0, 0] < 120
        assert ac.circular_gap(angle[0, 0], -alpha[i] % 120, 120.0) <= 1e-6
        assert abs(score[0, 0] - (t[i] ** 2).sum()) <= ac.score_bound(rows[i:i + 1], t[i:i + 1], n, m, np.ones(len(n), bool))[0, 0]


def test_statement_score_is_f_and_never_below_the_grid():
    x, t, n, m = ac.case_inputs(8)
    x, t = x[:65], t[:5]
    for sel, symmetry in ac.SELECTS.values():
        mask = ac.select_mask(m, sel)
        angle, score, best, grid = ac.align_statement(x, t, n, m, mask, 7, symmetry)
        bound = ac.score_bound(x, t, n, m, mask)
        assert (score >= grid.max(axis=2)).all()
        assert (np.abs(score - ac.f_longdouble(x, t, n, m, mask, angle)) <= bound).all()
        np.testing.assert_array_equal(best, ac.best_of(score, ac.key_values(t, mask, "distance"), "distance"))
    mask = ac.select_mask(m, (0,))
    angle, score, _, _ = ac.align_statement(x, t, n, m, mask, 360)
    assert (angle == 0).all()
    np.testing.assert_allclose(score, (x[:, mask]) @ t[:, mask].T, rtol=0, atol=ac.score_bound(x, t, n, m, mask).max())


def test_near_ties_of_the_grid_inputs_are_rare():
    """The refine=False index test of the GPU suite may skip pairs whose top two grid values lie within twice the bound, at most
    1 % of them: on the shared inputs the host statement leaves that cap far away."""
    for n_max in (1, 4, 8, 12, 13):
        x, t, n, m = ac.case_inputs(n_max)
        for name, (sel, symmetry) in ac.SELECTS.items():
            mask = ac.select_mask(m, sel)
            if not (np.abs(m[mask]) > 0).any():
                continue                                  # f is constant: the index is 0 on both sides, nothing is skipped
            bound = ac.score_bound(x, t, n, m, mask)
            cr, ci = ac.coefficients(x, t, n, m, mask)
            for n_theta in (2, 7, 360, 361):
                grid, _ = ac.grid_values(cr, ci, n_theta, symmetry)
                share = ac.near_tie(grid, bound).mean()
                print(f"n_max {n_max} {name} n_theta {n_theta}: near-tie share {share:.2e}")
                assert share <= 1e-3


def test_paired_labels_and_arguments_are_checked_on_the_host():
    n, m = ac.labels(4)
    _native.check_paired(n, m)
    n1, m1 = np.delete(n, 1), np.delete(m, 1)             # (1, -1) goes, (1, 1) stays
    sel = np.isin(np.abs(m), (0, 3))
    _native.check_paired(n[sel], m[sel])
    with pytest.raises(ValueError, match="not paired"):
        _native.check_paired(n1, m1)
    with pytest.raises(ValueError, match="not paired"):
        ac.pairs(n1, m1)
    with pytest.raises(ValueError, match="twice"):
        _native.check_paired(np.r_[n, 0], np.r_[m, 0])
    z = zmoments(np.ones((3, len(n))), n, m)
    with pytest.raises(ValueError, match="64 templates"):
        z.align(np.ones((65, len(n))))
    with pytest.raises(ValueError, match="n_theta"):
        z.align(np.ones((2, len(n))), n_theta=0)
    with pytest.raises(ValueError, match="n_theta"):
        z.align(np.ones((2, len(n))), n_theta=4097)
    with pytest.raises(ValueError, match="key"):
        z.align(np.ones((2, len(n))), key="euclid")
    with pytest.raises(ValueError, match="symmetry"):
        z.align(np.ones((2, len(n))), symmetry=0)
    with pytest.raises(ValueError, match="labels of the rows"):
        z.align(zmoments(np.ones((2, 6)), *ac.labels(2)))
    dense = zmoments(np.ones((len(n), 5, 5)), n, m)
    with pytest.raises(ValueError, match="rank-2"):
        dense.align(np.ones((2, len(n))))
    with pytest.raises(ValueError, match="rank-2"):
        dense.rotate_each(np.zeros(5))
    with pytest.raises(ValueError, match="one per row"):
        z.rotate_each(np.zeros(4))
    unpaired = zmoments(np.ones((3, len(n) - 1)), n1, m1)
    with pytest.raises(ValueError, match="not paired"):
        unpaired.align(np.ones((2, len(n) - 1)))
    with pytest.raises(ValueError, match="not paired"):
        unpaired.rotate_each(np.zeros(3))


def test_align_spec_tables_are_numpys():
    """The uploaded grid trigonometry and key values are the statement's own bits."""
    n, m = ac.labels(6)
    t = np.random.RandomState(0).standard_normal((4, len(n)))
    mask = ac.select_mask(m, (0, 3, 6))
    spec = _native.AlignSpec(n, m, t, mask.astype(np.int32), 7, 3, 3, "cosine")
    theta = ac.theta_grid(7, 3)
    np.testing.assert_array_equal(spec.theta, theta)
    arg = np.multiply.outer(np.deg2rad(theta), np.arange(1, 7))
    np.testing.assert_array_equal(spec.trig, np.hstack([np.cos(arg), np.sin(arg)]))
    np.testing.assert_array_equal(spec.key_values, ac.key_values(t, mask, "cosine"))
    assert spec.trig_m == 6 and spec.newton_iters == 3


def test_kmeans_aligned_twin_recovers_planted_classes():
    X, truth, init, n, m = ac.planted()
    labels, templates, angles, inertia, n_iter = ac.kmeans_aligned_numpy(X, n, m, 3, init)
    np.testing.assert_array_equal(labels, truth)          # init row c is of class c: no permutation
    assert 1 <= n_iter < 50 and templates.shape == init.shape and angles.shape == (len(X),)
    assert inertia <= 2 * 0.01 ** 2 * (np.linalg.norm(templates, axis=1)[truth] ** 2).sum()
    # plain distances cannot do this: the nearest initial row without rotation mislabels most rows
    plain = ((X[:, None, :] - init[None]) ** 2).sum(axis=2).argmin(axis=1)
    assert (plain != truth).mean() > 0.2


def test_align_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = _native.load()
    for sym in ALIGN_SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    from mtflearn_amd import clustering, resident
    assert callable(clustering.kmeans_aligned) and callable(resident.align_device) and callable(resident.rotate_rows_device)
