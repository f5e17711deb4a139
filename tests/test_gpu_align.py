"""GPU tests of the rotation alignment (csrc/zk_align.hip) against the NumPy statement and the derived bounds of
tests/align_cases.py (licensed by tests/test_align_cpu.py)."""
import numpy as np
import pytest

import align_cases as ac
from mtflearn_amd import ZPs, _native, zmoments
from mtflearn_amd.clustering import kmeans_aligned

pytestmark = pytest.mark.gpu


def _check(x, t, n, m, sel, symmetry, n_theta, refine, key, tally):
    """One call against the statement; ``tally`` collects (pairs compared by index, pairs skipped as near ties)."""
    mask = ac.select_mask(m, sel)
    res = zmoments(x, n, m).align(t, m_select=sel, n_theta=n_theta, symmetry=symmetry, refine=refine, key=key)
    assert res.angle.shape == res.score.shape == (len(x), len(t)) and res.best.shape == (len(x),)
    assert res.angle.dtype == res.score.dtype == np.float64 and res.best.dtype == np.int32
    bound = ac.score_bound(x, t, n, m, mask)
    _, _, _, grid = ac.align_statement(x, t, n, m, mask, n_theta, symmetry, False, key)
    err = np.abs(res.score - ac.f_longdouble(x, t, n, m, mask, res.angle))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    assert (res.score >= grid.max(axis=2) - bound).all()
    period = 360 / symmetry
    assert ((res.angle >= 0) & (res.angle < period)).all()
    np.testing.assert_array_equal(res.best, ac.best_of(res.score, ac.key_values(t, mask, key), key))
    constant = not (np.abs(m[mask]) > 0).any()
    if constant:                                          # f does not depend on the angle
        assert (res.angle == 0).all()
        assert (np.abs(res.score - x[:, mask] @ t[:, mask].T) <= bound).all()
    elif not refine:
        theta = ac.theta_grid(n_theta, symmetry)
        j = np.rint(res.angle / (period / n_theta)).astype(int)
        np.testing.assert_array_equal(theta[j], res.angle)
        skip = ac.near_tie(grid, bound) if n_theta > 1 else np.zeros(j.shape, bool)
        np.testing.assert_array_equal(j[~skip], grid.argmax(axis=2)[~skip])
        tally[0] += j.size
        tally[1] += int(skip.sum())
    return res


@pytest.mark.parametrize("refine", [True, False])
@pytest.mark.parametrize("select", list(ac.SELECTS))
@pytest.mark.parametrize("n_max", ac.NMAX_GRID)
def test_align_matches_statement_over_the_grid(n_max, select, refine):
    sel, symmetry = ac.SELECTS[select]
    X, Tm, n, m = ac.case_inputs(n_max)
    tally = [0, 0]
    for rows in ac.N_GRID:
        for t in ac.T_GRID:
            for n_theta in ac.NTHETA_GRID:
                _check(X[:rows], Tm[:t], n, m, sel, symmetry, n_theta, refine, "distance", tally)
    if tally[0]:
        print(f"n_max {n_max} {select}: {tally[1]} of {tally[0]} pairs skipped as near ties ({tally[1] / tally[0]:.2e})")
        assert tally[1] <= 0.01 * tally[0]


@pytest.mark.parametrize("key", ["distance", "cosine"])
def test_best_ties_go_to_the_lowest_index(key):
    X, Tm, n, m = ac.case_inputs(8)
    t = np.vstack([Tm[:3], Tm[1:2], Tm[3:5], Tm[0:1]])    # templates 3 and 6 repeat 1 and 0
    res = _check(X[:257], t, n, m, None, 1, 360, True, key, [0, 0])
    np.testing.assert_array_equal(res.score[:, 3], res.score[:, 1])
    np.testing.assert_array_equal(res.score[:, 6], res.score[:, 0])
    assert not np.isin(res.best, (3, 6)).any() and np.isin(res.best, (0, 1)).any()


@pytest.mark.parametrize("n_max", [4, 8, 12])
def test_exact_rotations_are_recovered(n_max):
    rows, t, alpha, n, m = ac.rotated_pairs(n_max, 200, seed=10 + n_max)
    for t0 in range(0, 200, 50):                          # 64 templates at most: four blocks of 50, the diagonal of each
        res = zmoments(rows[t0:t0 + 50], n, m).align(t[t0:t0 + 50])
        at = np.arange(50)
        gap = ac.circular_gap(res.angle[at, at], -alpha[t0:t0 + 50] % 360)
        print(f"n_max {n_max}: worst angle error {gap.max():.3e} degree")
        assert gap.max() <= 1e-6
        bound = ac.score_bound(rows[t0:t0 + 50], t[t0:t0 + 50], n, m, np.ones(len(n), bool))[at, at]
        assert (np.abs(res.score[at, at] - (t[t0:t0 + 50] ** 2).sum(axis=1)) <= bound).all()
        np.testing.assert_array_equal(res.best, at)


def test_rotating_by_the_angle_never_moves_a_row_away():
    """|rotate_each(angle) - t|^2 <= |x - t|^2 + bound: angle 0 is on the grid."""
    X, Tm, n, m = ac.case_inputs(12)
    x, t = X[:257], Tm[:5]
    z = zmoments(x, n, m)
    res = z.align(t)
    bound = ac.score_bound(x, t, n, m, np.ones(len(n), bool))
    for c in range(len(t)):
        moved = ((z.rotate_each(res.angle[:, c]).data - t[c]) ** 2).sum(axis=1)
        stayed = ((x - t[c]) ** 2).sum(axis=1)
        assert (moved <= stayed + bound[:, c]).all(), (moved - stayed - bound[:, c]).max()


@pytest.mark.parametrize("n_max", [0, 1, 8, 13])
def test_rotate_rows(n_max):
    X, _, n, m = ac.case_inputs(n_max)
    rng = np.random.RandomState(5)
    for rows in (1, 65, 1000):
        x = X[:rows]
        a = rng.uniform(-720, 720, rows)
        a[0] = 0.0
        got = _native.rotate_rows(x, n, m, a)
        bound = ac.rotate_bound(x, n, m, a)
        err = np.abs(got.astype(np.longdouble) - ac.rotate_longdouble(x, n, m, a))
        print(f"n_max {n_max} rows {rows}: worst rotate error {float((err / np.maximum(bound, 1e-300)).max()):.3f} of the bound")
        assert (err <= bound).all()
        np.testing.assert_array_equal(got[0], x[0])
        np.testing.assert_array_equal(got[:, m == 0], x[:, m == 0])
        back = _native.rotate_rows(got, n, m, -a)
        assert (np.abs(back - x) <= 2 * bound).all()
        inplace = x.copy()
        assert _native.rotate_rows(inplace, n, m, a, out=inplace) is inplace
        np.testing.assert_array_equal(inplace, got)
        np.testing.assert_array_equal(zmoments(x, n, m).rotate_each(a).data, got)
        one = zmoments(x[:1], n, m)
        np.testing.assert_allclose(one.rotate_each(a[:1]).data, one.rotate(a[0]).to_real().data, rtol=0, atol=bound[:1].max() + 1e-300)


def test_runs_chunks_streams_and_resident_calls_agree_bit_for_bit():
    import torch
    X, Tm, n, m = ac.case_inputs(8)
    x, t = X[:1000], Tm[:5]
    z = zmoments(x, n, m)
    first = z.align(t)
    again = z.align(t)
    a = first.angle[:, 2].copy()
    rot = _native.rotate_rows(x, n, m, a)
    try:
        _native.align_set_host_chunk(1)                   # 256 rows per chunk: four chunks
        small = z.align(t)
        rot_small = _native.rotate_rows(x, n, m, a)
    finally:
        _native.align_set_host_chunk(0)
    for other in (again, small):
        for u, v in zip(first, other):
            np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(rot, rot_small)

    from mtflearn_amd import resident
    xd = torch.from_numpy(x).cuda()
    res = resident.align_device(xd, n, m, t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res_side = resident.align_device(xd, n, m, t)
        rot_side = resident.rotate_rows_device(xd, n, m, res_side.angle[:, 2].contiguous())
    side.synchronize()
    rot_dev = resident.rotate_rows_device(xd, n, m, res.angle[:, 2].contiguous())
    torch.cuda.synchronize()
    for u, v, w in zip(first, res, res_side):
        np.testing.assert_array_equal(u, v.cpu().numpy())
        np.testing.assert_array_equal(u, w.cpu().numpy())
    np.testing.assert_array_equal(rot, rot_dev.cpu().numpy())
    np.testing.assert_array_equal(rot, rot_side.cpu().numpy())
    nd = _native.DeviceArray.from_numpy(x)
    res_nd = resident.align_device(nd, n, m, zmoments(t, n, m))
    for u, v in zip(first, res_nd):
        np.testing.assert_array_equal(u, v.numpy())


def test_refusals_come_with_a_message_before_any_launch():
    n, m = ac.labels(4)
    x = np.ones((3, len(n)))
    lib = _native.load()
    n32, m32 = n.astype(np.int32), m.astype(np.int32)
    bad_n, bad_m = np.delete(n32, 1), np.delete(m32, 1)
    from ctypes import POINTER, c_double, c_int32, c_void_p
    pi, pd = POINTER(c_int32), POINTER(c_double)
    out = np.empty((3, 65))

    def call(nn, mm, cols, T, n_theta):
        rows, t = np.ones((3, cols)), np.ones((T, cols))
        return lib.zk_align_rows(0, rows.ctypes.data_as(c_void_p), 3, cols, nn.ctypes.data_as(pi), mm.ctypes.data_as(pi), t.ctypes.data_as(pd),
                                 T, None, n_theta, 1, 3, 0, None, 0, None, out.ctypes.data_as(c_void_p), None, None)

    for args, word in (((bad_n, bad_m, len(n) - 1, 2, 360), "not paired"), ((n32, m32, len(n), 65, 360), "64 templates"),
                       ((n32, m32, len(n), 2, 0), "n_theta")):
        assert call(*args) == _native.ZK_E_BADARG
        assert word in _native.last_error()
    assert call(n32, m32, len(n), 2, 7) == 0
    z = zmoments(x, n, m)
    for kwargs, word in ((dict(templates=np.ones((65, len(n)))), "64 templates"), (dict(templates=x, n_theta=0), "n_theta")):
        with pytest.raises(ValueError, match=word):
            z.align(**kwargs)
    with pytest.raises(ValueError, match="not paired"):
        zmoments(x[:, 1:], np.delete(n, 1), np.delete(m, 1)).align(x[:, 1:])
    with pytest.raises(ValueError, match="rank-2"):
        zmoments(np.ones((len(n), 4, 4)), n, m).align(x)


def test_kmeans_aligned_follows_its_numpy_twin():
    X, truth, init, n, m = ac.planted()
    want = ac.kmeans_aligned_numpy(X, n, m, 3, init)
    got = kmeans_aligned(X, n, m, 3, init=init)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[0], truth)
    assert got[4] == want[4] and got[0].dtype == np.int32
    np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-12)
    assert ac.circular_gap(got[2], want[2]).max() <= 1e-6
    np.testing.assert_allclose(got[3], want[3], rtol=1e-9)
    drawn = kmeans_aligned(X, n, m, 3, random_state=0, max_iter=5)
    assert drawn[0].shape == (len(X),) and drawn[1].shape == init.shape


def test_end_to_end_three_fold_patches():
    from mtflearn_amd.datasets import get_zps_test_patches
    patches = get_zps_test_patches(size=32, n_fold=3, num_patches=16)
    mom = ZPs(8, 32).transform(np.asarray(patches))
    res = mom.align(mom.data[:1], symmetry=3)
    count = mom.data.shape[0]
    assert res.angle.shape == res.score.shape == (count, 1) and res.best.shape == (count,)
    assert res.angle.dtype == res.score.dtype == np.float64 and res.best.dtype == np.int32
    t = mom.data[0]
    moved = ((mom.rotate_each(res.angle[:, 0]).data - t) ** 2).sum(axis=1)
    stayed = ((mom.data - t) ** 2).sum(axis=1)
    bound = ac.score_bound(mom.data, mom.data[:1], mom.n, mom.m, np.ones(len(mom.n), bool))[:, 0]
    assert (moved <= stayed + bound).all(), (moved - stayed - bound).max()
