"""The kernels of csrc/zk_rows.hip, zk_kmeans.hip and zk_mixture.hip against tests/cluster_reference.py: past one tile per wave, at every template
instantiation, at ties, with non-finite rows, and at the limits the C ABI refuses.

C1 (``test_exact_*``) uses matrices of integers / 4 with one column holding ``r mod 1024`` and one ``r // 1024``: every sum a
kernel forms is exact in float64 in any order, so results are compared with ``assert_array_equal``.  The row counts come from
the grid formulae of the host code (restated in ``row_workers`` / ``wgram_workers`` / ``estep_workers`` below) and the CU count
of the device: every workgroup walks at least three tiles and the ragged last tile (1, 63 or a full 64 rows) lands on a wave
that has already done full ones.  tests/test_cluster_reference_cpu.py proves on the CPU that these inputs stay below 2^53, and
that every label the other tests compare exactly is decided (margin above ``LLOYD_MARGIN`` / ``ESTEP_MARGIN``).

Inexact quantities are bounded as ``c * 2^-53 * sum|terms|`` with sum|terms| from the longdouble reference.  The record of the
observed ratios is the dict ``C`` below: it holds, per operation, the worst ratio |got - ref| / (2^-53 sum|terms|) observed on an MI355X (256 CUs) over every case of this module
and the bound, about four times that, because the kernels' summation order follows the grid, i.e. the CU count.  The old
tolerances against HostRows (rtol 1e-10 .. 1e-12 of the VALUES, plus absolute floors) were guesses between two float64
computations; every bound here is tighter than they were except where cancellation makes the values much smaller than their
terms.  ``moments_after_estep`` is the one large figure, and not a summation error: the weights are responsibilities
exp(lp - lse), which carry the rounding of lp -- 2^-53 times the terms of the quadratic form, hundreds to thousands here -- as
a RELATIVE error, before the moment sums add their own.

Departures from the shapes named in the issue, for memory and time: the exact tests run all three ragged sizes at D = 3 and
one ragged size each at D = 45, 64, 66 and 127 (a 100-MB matrix each), not the full cross product; k = 256 with column sums
needs k (D + 1) doubles of LDS beside a tile and is refused at D = 66 and 127 (checked as a refusal there).
"""
import ctypes

import numpy as np
import pytest

import cluster_reference as ref

pytestmark = pytest.mark.gpu

LLOYD_MARGIN = 1e-12        # relative to |x|^2 + |c|^2: D * 2^-53 * a few, for D <= 127
ESTEP_MARGIN = 1e-12        # relative to the magnitude of the row's terms (cluster_reference.estep): 2 D * 2^-53 and a few

# bounds c of |got - ref| <= c * 2^-53 * sum|terms| per operation: (observed worst ratio on the MI355X, bound)
C = {
    "colsum": (2.33, 10.0),
    "center_at": (3.16, 13.0),
    "seed_pot": (1.48, 6.0),
    "lloyd_sums": (2.43, 10.0),
    "own_distance": (1.89, 8.0),
    "estep_lse": (0.842, 4.0),
    "moments": (4.01, 16.0),
    "moments_after_estep": (432.0, 1700.0),      # worst at (130 x 127, k = 48): the largest quadratic forms
    "gram": (3.72, 16.0),
    "project": (3.73, 15.0),
}

def bounded(op, got, want, mag, what=""):
    r = ref.ratio(got, want, mag)
    print(f"ratio {op} {what}: {r:.3g}")
    assert r <= C[op][1], (op, what, r)


# ---- the host code's grids, restated ----------------------------------------------------------------------------------
LDS = 160 * 1024


def tile_bufs(d, extra=0):
    return 2 if 8 * (2 * 64 * d * 8 + extra + 512) <= LDS else 1


def row_workers(d, n_cu, extra=0):
    lds = tile_bufs(d, extra) * 64 * d * 8 + extra
    return max(1, min(8, LDS // ((lds + 511) & ~511))) * n_cu


def lloyd_workers(d, k, n_cu, update=True):
    return row_workers(d, n_cu, k * (d + 1) * 8 if update and k > 16 else 0)


def lloyd_fits(d, k):
    """The LDS table of the column sums (k > 16) beside one tile."""
    extra = k * (d + 1) * 8 if k > 16 else 0
    return tile_bufs(d, extra) * 64 * d * 8 + extra <= LDS


def wgram_workers(d, count, n_cu, valu):
    if d + 1 <= 48 and d >= 2 and not valu:
        return n_cu * 8 // 6                                                  # sets of six waves
    t = (d + 4) // 4
    n_ut = t * (t + 1) // 2
    threads = max(256, (n_ut + 63) & ~63)
    lds = (64 * (4 * t + 4) + 64 * count) * 8
    per_cu = min(LDS // (lds + 512), 2048 // threads)
    return max(1, min(per_cu, 4 if count > 1 else 6)) * n_cu


def estep_workers(d, k, n_cu, valu):
    """(workers, rows per worker and round)"""
    nb = (d + 15) // 16
    if nb <= 3 and k <= 8 and d >= 2 and not valu:
        tab = (k * 2 * nb * (nb + 1) * 64 + k * nb * 16) * 8
        return n_cu * (12 if tab + 12 * (16 * d + 132) * 8 <= LDS else 8), 16
    lds = 64 * d * 8 + 4 * k * 64 * 8
    return max(1, min(LDS // (lds + 512), 8)) * n_cu, 64


def rounds(n, workers, rows=64):
    """(tiles the least loaded worker walks, tiles the worker of the last tile walked before it)"""
    tiles = -(-n // rows)
    return tiles // workers, (tiles - 1) // workers


def exact_rows(d, n_cu, ragged):
    w = max(row_workers(d, n_cu), wgram_workers(d, 1, n_cu, True), wgram_workers(d, 1, n_cu, False))
    return 64 * 3 * w + ragged


# ---- input builders (also imported by tests/test_cluster_reference_cpu.py) ---------------------------------------------
EXACT_SHAPES = [(3, 1), (3, 63), (3, 64), (45, 63), (64, 1), (66, 64), (127, 1)]      # (D, rows of the last tile)
EXACT_K = (3, 8, 16, 17)


def exact_case(d, ragged, n_cu):
    """Q (N, D) int16 in quarter units, shift S (D) and per k the centres (k, D), all integers."""
    n = exact_rows(d, n_cu, ragged)
    rng = np.random.default_rng([d, ragged])
    Q = rng.integers(-8, 9, (n, d), dtype=np.int16)
    r = np.arange(n)
    Q[:, 0], Q[:, 1] = r % 1024, r // 1024
    S = rng.integers(-4, 5, d).astype(np.float64)
    S[0], S[1] = 512, (n // 1024) // 2
    centres = {}
    for k in EXACT_K:
        Ck = rng.integers(-8, 9, (k, d)).astype(np.float64)
        Ck[:, 0] = np.where(np.arange(k) % 2, 192, -192)
        Ck[:, 1] = rng.integers(-2, 3, k)
        centres[k] = Ck
    cand = rng.integers(-8, 9, (8, d)).astype(np.float64)
    cand[:, 0], cand[:, 1] = rng.integers(-500, 500, 8), rng.integers(-20, 20, 8)
    comp = rng.integers(-4, 5, (min(d, 20), d)).astype(np.float64)
    return Q, S, centres, cand, comp


def float_matrix(n, d, seed):
    rng = np.random.default_rng([n, d, seed])
    return rng.standard_normal((n, d)) * (1 + rng.random(d)) + rng.standard_normal(d) * 2


SMALL_N = (64 * 7 - 1, 64 * 7, 64 * 7 + 1)
LLOYD_K = (1, 4, 5, 8, 9, 16, 17, 64, 256)
LLOYD_SHAPES = [(447, 3), (448, 45), (449, 66), (448, 127)]


def lloyd_centres(X, k, seed):
    """k distinct rows of the centred matrix, nudged: margins are checked on the CPU."""
    rng = np.random.default_rng([len(X), X.shape[1], k, seed])
    mean = X.mean(axis=0)
    return mean, (X[rng.choice(len(X), k, replace=False)] - mean) + 0.01 * rng.standard_normal((k, X.shape[1]))


def mixture(X, k, kind, seed, spread=0.1):
    """Factors of k components around rows of X: (prec_chol, means, log_det, log_w)."""
    from scipy import linalg
    n, d = X.shape
    rng = np.random.default_rng([n, d, k, seed, kind == "full"])
    means = X[rng.choice(n, k, replace=k > n)] + spread * rng.standard_normal((k, d))
    prec = np.zeros((k, d, d))
    for c in range(k):
        if kind == "full":
            a = rng.standard_normal((d, d)) * 0.3 + np.eye(d) * 2
            prec[c] = linalg.solve_triangular(linalg.cholesky(a @ a.T, lower=True), np.eye(d), lower=True).T
        else:
            prec[c] = np.diag(0.5 + rng.random(d))
    log_det = np.log(np.einsum("kii->ki", prec)).sum(axis=1)
    log_w = np.log(rng.dirichlet(np.ones(k) * 5))
    return prec, means, log_det, log_w


# (N, D, k, kind): the last two are the largest k whose tables fit the LDS beside a tile of 127 / 80 features; NB = 1, 2, 3; twelve waves (small tables) and eight (k = 8 at NB = 3); k = 9 and 64 take the vector kernel
ESTEP_CASES = [(n, d, k, kind) for n, d in ((447, 2), (448, 16), (449, 17), (448, 33), (447, 45), (449, 48))
               for k in (1, 8, 9) for kind in ("full", "diag")] + [(449, 17, 64, "full"), (447, 45, 64, "diag"), (130, 127, 48, "full"),
                                                              (130, 80, 60, "diag")]


def estep_case(n, d, k, kind):
    X = float_matrix(n, d, 7)
    return X, mixture(X, k, kind, 1)


def estep_big_rows(n_cu):
    return 64 * 3 * 8 * n_cu + 64 + 5          # three rounds of the vector kernel's 8 n_cu workgroups, then a ragged tile


def estep_big_case(n_cu):
    X = float_matrix(estep_big_rows(n_cu), 17, 3)
    return X, mixture(X, 2, "full", 2, spread=1.0)


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(X):
    from mtflearn_amd.clustering import DeviceRows
    return DeviceRows(X)


# ---- C1: several tiles per wave, exact arithmetic ------------------------------------------------------------------------
@pytest.mark.parametrize("d,ragged", EXACT_SHAPES)
def test_exact_row_passes_over_several_tiles_per_wave(d, ragged, n_cu, monkeypatch):
    monkeypatch.delenv("ZK_WGRAM_VALU", raising=False)
    Q, S, centres, cand, comp = exact_case(d, ragged, n_cu)
    n = len(Q)
    assert n % 64 == ragged % 64
    for w in [row_workers(d, n_cu)] + [lloyd_workers(d, k, n_cu) for k in EXACT_K] + \
             [wgram_workers(d, c, n_cu, v) for c in (1, 3) for v in (False, True)]:
        least, before_last = rounds(n, w)
        assert least >= 3 and before_last >= 3, (d, ragged, w, least, before_last)
    assert ref.exact_headroom(Q, S, np.concatenate(list(centres.values()) + [cand])) < 2.0 ** 53
    X, shift = Q / 4.0, S / 4.0
    with _rows(X) as dev:
        np.testing.assert_array_equal(dev.colsum(), ref.exact_colsum(Q))
        sq, xsq = ref.exact_center(Q, S)
        sq_d, bad = dev.center_at(shift)
        np.testing.assert_array_equal(sq_d, sq)
        assert bad == 0
        # seeding: three candidates from nothing, pick one, eight folded with it, pick again
        d3, pot3 = ref.exact_seed(Q, S, cand[:3])
        np.testing.assert_array_equal(dev.seed_step(cand[:3] / 4, (cand[:3] ** 2).sum(axis=1) / 16, False), pot3)
        closest = d3[1]
        cum = np.cumsum(closest)
        at = np.array([0, 1023, 1024, 1025, n // 2, n - 65, n - 1])
        vals = np.concatenate([cum[at], cum[at] - 0.5 * closest[at], [0.0, cum[-1], cum[-1] + 1.0]])
        want = np.minimum(np.searchsorted(cum, vals, side="left"), n - 1)
        np.testing.assert_array_equal(dev.seed_pick(1, vals), want)
        d8, pot8 = ref.exact_seed(Q, S, cand, closest)
        np.testing.assert_array_equal(dev.seed_step(cand / 4, (cand ** 2).sum(axis=1) / 16, True), pot8)
        cum = np.cumsum(d8[7])
        vals = cum[at] - 0.25 * d8[7][at]
        np.testing.assert_array_equal(dev.seed_pick(7, vals), np.minimum(np.searchsorted(cum, vals, side="left"), n - 1))
        # Lloyd
        dev.reset_labels()
        prev = None
        for k in EXACT_K:
            Ck = centres[k]
            labels, sums, counts, changed = ref.exact_lloyd(Q, S, Ck, prev)
            s_d, c_d, ch_d = dev.lloyd(Ck / 4, True)
            np.testing.assert_array_equal(dev.labels(), labels)
            np.testing.assert_array_equal(s_d, sums)
            np.testing.assert_array_equal(c_d, counts)
            assert ch_d == changed, (k, ch_d, changed)
            s_d, c_d, ch_d = dev.lloyd(Ck / 4, True)
            np.testing.assert_array_equal(s_d, sums)
            assert ch_d == 0
            assert dev.lloyd(Ck / 4, False)[2] == 0
            np.testing.assert_array_equal(dev.labels(), labels)
            np.testing.assert_array_equal(dev.own_distance(Ck / 4), ref.exact_own_distance(Q, S, Ck, labels))
            prev = labels
            if k == 8:
                lab8 = labels
                dev.resp_from_labels(8)
                g8 = np.stack([ref.exact_moments(Q, S, lab8, c) for c in range(8)])
                for valu in (False, True):
                    if valu:
                        monkeypatch.setenv("ZK_WGRAM_VALU", "1")
                    np.testing.assert_array_equal(dev.moments(2, shift), g8[2])
                    np.testing.assert_array_equal(dev.moments(1, shift, 3), g8[1:4])
                    np.testing.assert_array_equal(dev.moments(0, shift, 8), g8)
                    np.testing.assert_array_equal(dev.gram(shift), ref.exact_moments(Q, S))
                monkeypatch.delenv("ZK_WGRAM_VALU")
        # a labels-only pass from scratch (for k > 16 it has its own LDS size, tile buffers and grid)
        for k in (3, 17):
            want = ref.exact_lloyd(Q, S, centres[k])[0]
            dev.reset_labels()
            assert dev.lloyd(centres[k] / 4, False)[2] == n
            np.testing.assert_array_equal(dev.labels(), want)
        np.testing.assert_array_equal(dev.project(shift, comp / 4), ref.exact_project(Q, S, comp))


def test_mixture_passes_over_several_rounds(n_cu, monkeypatch):
    """estep_mfma (16-row blocks over n_cu workgroups of 12 waves) and the vector-pipe estep_kernel (tiles over 8 n_cu
    workgroups) with every workgroup going round at least three times and a ragged end; the responsibilities then feed
    wgram_mfma / wgram_kernel over the same rows."""
    monkeypatch.delenv("ZK_ESTEP_VALU", raising=False)
    monkeypatch.delenv("ZK_WGRAM_VALU", raising=False)
    X, mix = estep_big_case(n_cu)
    n, d = X.shape
    for valu in (False, True):
        w, rows = estep_workers(d, 2, n_cu, valu)
        assert min(rounds(n, w, rows)) >= 3, (valu, w, rounds(n, w, rows))
    total, mags, labels, margin, resp = ref.estep(X, *mix)
    assert np.all(margin > ESTEP_MARGIN * mags)
    shift = X.mean(axis=0)
    g_ref = [ref.moments(X, resp[:, c], shift) for c in range(2)]
    with _rows(X) as dev:
        for valu in (False, True):
            if valu:
                monkeypatch.setenv("ZK_ESTEP_VALU", "1")
                monkeypatch.setenv("ZK_WGRAM_VALU", "1")
            bounded("estep_lse", dev.estep(*mix), total, mags.sum(), f"big valu={valu}")
            np.testing.assert_array_equal(dev.labels(), labels)
            got = dev.moments(0, shift, 2)
            for c in range(2):
                bounded("moments_after_estep", got[c], g_ref[c][0], g_ref[c][1], f"big valu={valu} c={c}")


# ---- C2: every instantiation at small N -------------------------------------------------------------------------------------
def onehot_case(n, d):
    """Matrix, shift, eight well separated centres and the labels they give (the one-hot weights of the moment passes)."""
    X = float_matrix(n, d, 1)
    mean, centres = lloyd_centres(X, 8, 2)
    return X, mean, centres


@pytest.mark.parametrize("d", (1, 2, 16, 17, 33, 47, 48, 91, 127))
def test_moments_every_count(d, monkeypatch):
    """wgram_mfma_kernel<1..8> (2 <= D <= 47) and wgram_kernel<1..3>: every plane of a multi-component pass against the
    reference and against the one-component pass."""
    monkeypatch.delenv("ZK_WGRAM_VALU", raising=False)
    for n in SMALL_N:
        X, mean, centres = onehot_case(n, d)
        labels, margin = ref.lloyd(X, mean, centres)[:2]
        assert margin.min() > LLOYD_MARGIN
        shift = mean + 0.25
        g_ref = [ref.moments(X, labels == c, shift) for c in range(8)]
        with _rows(X) as dev:
            dev.center_at(mean)
            dev.lloyd(centres, False)
            np.testing.assert_array_equal(dev.labels(), labels)
            dev.resp_from_labels(8)
            for valu in (False, True):
                if valu:
                    monkeypatch.setenv("ZK_WGRAM_VALU", "1")
                mfma = 2 <= d <= 47 and not valu
                single = [dev.moments(c, shift) for c in range(8)]
                for count in range(1, 9):
                    if count > 3 and not mfma:           # the wrapper would split the call: the ABI's limit is in C5
                        break
                    got = dev.moments(0, shift, count)
                    for c in range(count):
                        bounded("moments", got[c], g_ref[c][0], g_ref[c][1], f"n={n} d={d} count={count} c={c} valu={valu}")
                        np.testing.assert_array_equal(got[c], single[c])
                bounded("gram", dev.gram(shift), *ref.moments(X, None, shift), f"n={n} d={d} valu={valu}")
            monkeypatch.delenv("ZK_WGRAM_VALU")


@pytest.mark.parametrize("n,d", LLOYD_SHAPES)
def test_seeding_and_lloyd_every_instantiation(n, d):
    X = float_matrix(n, d, 2)
    mean = X.mean(axis=0)
    with _rows(X) as dev:
        s, a = ref.colsum(X)
        bounded("colsum", dev.colsum(), s, a, f"n={n} d={d}")
        sq, xsq, bad = ref.center_at(X, mean)
        sq_d, bad_d = dev.center_at(mean)
        bounded("center_at", sq_d, sq, sq, f"n={n} d={d}")
        assert bad_d == bad == 0
        rng = np.random.default_rng([n, d, 9])
        closest = None
        for t in (1, 4, 5, 8):
            cand = dev.fetch(rng.integers(0, n, t))
            csq = np.einsum("ij,ij->i", cand, cand)
            dist, pot, mag = ref.seed_step(X, mean, cand, csq, closest)
            bounded("seed_pot", dev.seed_step(cand, csq, closest is not None), pot, mag, f"n={n} d={d} t={t}")
            which = t - 1
            vals = np.sort(rng.random(4)) * float(pot[which])
            idx, margin = ref.seed_pick(dist[which], vals)
            got = dev.seed_pick(which, vals)
            decided = margin > 1e-12                       # the stored distances carry D roundings of size 2^-53 |x|^2
            assert decided.all() and np.array_equal(got, idx), (t, got, idx, margin)
            closest = np.asarray(dist[which], dtype=np.float64)
        dev.reset_labels()
        prev = None
        for k in LLOYD_K:
            if k > n:
                continue
            _, centres = lloyd_centres(X, k, 3)
            labels, margin, sums, mags, counts, changed = ref.lloyd(X, mean, centres, prev)
            assert margin.min() > LLOYD_MARGIN
            for update in (True, False):
                if update and not lloyd_fits(d, k):
                    with pytest.raises(RuntimeError, match="LDS"):
                        dev.lloyd(centres, True)
                    continue
                s_d, c_d, ch_d = dev.lloyd(centres, update)
                np.testing.assert_array_equal(dev.labels(), labels)
                assert ch_d == (changed if update or not lloyd_fits(d, k) else 0), (k, update, ch_d, changed)
                if update:
                    np.testing.assert_array_equal(c_d, counts)
                    bounded("lloyd_sums", s_d, sums, mags, f"n={n} d={d} k={k}")
            bounded("own_distance", dev.own_distance(centres), *ref.own_distance(X, mean, centres, labels), f"n={n} d={d} k={k}")
            prev = labels
        comp = rng.standard_normal((min(d, 20), d))
        bounded("project", dev.project(mean, comp), *ref.project(X, mean, comp), f"n={n} d={d}")


@pytest.mark.parametrize("n,d,k,kind", ESTEP_CASES)
def test_estep_every_instantiation(n, d, k, kind, monkeypatch):
    """estep_mfma_kernel<NB, FULL, NW> for NB = 1, 2, 3, full and diagonal factors, twelve and eight waves, and the vector-pipe
    kernel (forced, and by k > 8): sum of log-sum-exp, exact labels, responsibilities through the weighted moments."""
    monkeypatch.delenv("ZK_ESTEP_VALU", raising=False)
    X, mix = estep_case(n, d, k, kind)
    total, mags, labels, margin, resp = ref.estep(X, *mix)
    assert np.all(margin > ESTEP_MARGIN * mags)
    shift = X.mean(axis=0)
    probe = sorted({0, k // 2, k - 1})
    g_ref = {c: ref.moments(X, resp[:, c], shift) for c in probe}
    with _rows(X) as dev:
        for valu in (False, True):
            if valu:
                monkeypatch.setenv("ZK_ESTEP_VALU", "1")
            what = f"n={n} d={d} k={k} {kind} valu={valu}"
            lse = dev.estep(*mix)
            bounded("estep_lse", lse, total, mags.sum(), what)
            np.testing.assert_array_equal(dev.labels(), labels)
            for c in probe:
                bounded("moments_after_estep", dev.moments(c, shift), g_ref[c][0], g_ref[c][1], what + f" c={c}")
            assert dev.estep(*mix, want_resp=False) == lse                     # the same sum and labels without the stores
            np.testing.assert_array_equal(dev.labels(), labels)


# ---- C3: ties ------------------------------------------------------------------------------------------------------------
TIE_SHAPES = [(449, 3), (447, 45), (448, 66)]
TIE_K = (2, 6, 8, 16, 17, 40)


def tie_case(n, d, k):
    """Dyadic matrix (quarter units), centres with duplicates at (0, k - 1) and (3, 4), and every 7th row put exactly half
    way between centres 1 and 2, which differ by two quarter units in one column: the row is at squared distance 1 from both
    and at 5 or more from every other centre (all coordinates are even), so the tie between 1 and 2 is the winning one."""
    rng = np.random.default_rng([n, d, k, 5])
    Q = rng.integers(-8, 9, (n, d)).astype(np.float64)
    Ck = rng.integers(-4, 5, (k, d)).astype(np.float64) * 2
    if k > 2:
        Ck[2] = Ck[1]
        Ck[2, 0] += 2
        Q[::7] = (Ck[1] + Ck[2]) / 2
    Ck[k - 1] = Ck[0]
    if k > 4:
        Ck[4] = Ck[3]
    return Q, Ck


@pytest.mark.parametrize("n,d", TIE_SHAPES)
def test_lloyd_ties_go_to_the_lower_index(n, d):
    S = np.zeros(d)
    for k in TIE_K:
        Q, Ck = tie_case(n, d, k)
        labels, sums, counts, _ = ref.exact_lloyd(Q, S, Ck)
        assert not np.any(labels == k - 1) and (k <= 4 or not np.any(labels == 4))
        if k > 2:
            assert np.all(labels[::7] == 1)                                    # centre 2 ties with 1 there
        with _rows(Q / 4) as dev:
            dev.center_at(S)
            s_d, c_d, _ = dev.lloyd(Ck / 4, True)
            np.testing.assert_array_equal(dev.labels(), labels)
            np.testing.assert_array_equal(c_d, counts)
            np.testing.assert_array_equal(s_d, sums)
            assert c_d[k - 1] == 0 and not s_d[k - 1].any()


DUPLICATE_CASES = [(17, 4, False), (45, 8, False), (45, 8, True), (66, 9, False), (127, 12, False)]


def duplicate_case(d, k):
    """A mixture whose last component is a copy of the first, weights included."""
    X, (prec, means, log_det, log_w) = estep_case(449, d, k, "full")
    prec[k - 1], means[k - 1], log_det[k - 1], log_w[k - 1] = prec[0], means[0], log_det[0], log_w[0]
    return X, (prec, means, log_det, log_w)


@pytest.mark.parametrize("d,k,valu", DUPLICATE_CASES)
def test_duplicate_mixture_components(d, k, valu, monkeypatch):
    """The matrix-core kernel, the vector-pipe kernel with one column block per slot (D <= 64) and with two (D = 66, 127)."""
    monkeypatch.delenv("ZK_ESTEP_VALU", raising=False)
    if valu:
        monkeypatch.setenv("ZK_ESTEP_VALU", "1")
    X, mix = duplicate_case(d, k)
    want = ref.estep(X, *[a[:k - 1] for a in mix], want_resp=False)[2]           # the copy never wins: decided on the CPU
    shift = X.mean(axis=0)
    with _rows(X) as dev:
        dev.estep(*mix)
        np.testing.assert_array_equal(dev.labels(), want)
        assert np.any(want == 0)
        np.testing.assert_array_equal(dev.moments(0, shift), dev.moments(k - 1, shift))       # equal responsibilities


def test_seed_pick_on_cumulative_sums():
    """Closest distances that are small integers: the cumulative sums are exact, and draws that equal one (at elements 1023,
    1024, 1025: the edges of the 1024-element blocks), 0 and the total have exact answers (side 'left', clipped)."""
    n, d = 3000, 3
    rng = np.random.default_rng(8)
    Q = rng.integers(-8, 9, (n, d)).astype(np.float64)
    Q[5] = Q[1024] = Q[2047] = 0                                 # zero distances: plateaux of the cumulative sum
    cand = np.zeros((1, d))
    closest = (Q * Q).sum(axis=1)
    cum = np.cumsum(closest)
    with _rows(Q) as dev:
        dev.center_at(np.zeros(d))
        np.testing.assert_array_equal(dev.seed_step(cand, np.zeros(1), False), [cum[-1]])
        at = np.array([0, 4, 5, 1022, 1023, 1024, 1025, 2046, 2047, 2048, n - 2, n - 1])
        vals = np.concatenate([cum[at], cum[at] + 0.5, [0.0, cum[-1], cum[-1] + 3]])
        want = np.minimum(np.searchsorted(cum, vals, side="left"), n - 1)
        assert want[-1] == want[-2] == n - 1 and want[-3] == 0
        np.testing.assert_array_equal(dev.seed_pick(0, vals), want)


# ---- C4: non-finite rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (3, 66))
def test_non_finite_rows_are_counted_on_tile_edges(d, n_cu):
    w = row_workers(d, n_cu)
    n = 64 * 3 * w + 1
    X = float_matrix(n, d, 4)
    bad_rows = [64, 127, 64 * (2 * w + 1) + 5, 64 * 2 * w, n - 1]        # first / last row of a full tile, third tiles, ragged
    for i, r in enumerate(bad_rows):
        X[r, (i * 2) % d] = (np.nan, np.inf, -np.inf)[i % 3]
    X[64, d - 1] = np.inf                                                 # two bad elements in one row count once
    assert rounds(n, w) == (3, 3)
    with _rows(X) as dev:
        assert dev.center_at(np.zeros(d))[1] == len(bad_rows)
        X[bad_rows] = 0.0
    with _rows(X) as dev:
        assert dev.center_at(np.zeros(d))[1] == 0


# ---- C5: refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from mtflearn_amd.clustering import DeviceRows, _p
    X = float_matrix(300, 48, 6)
    shift, out = np.zeros(48), np.empty((9, 49, 49))
    with pytest.raises(RuntimeError, match="1 <= D <= 127"):
        DeviceRows(np.zeros((4, 128)))
    with DeviceRows(X) as dev:
        lib, h = dev._lib, dev._h
        handle = ctypes.c_void_p()
        assert lib.zk_rows_create(dev.device, _p(X), 0, 48, ctypes.byref(handle)) != 0 and not handle.value
        with pytest.raises(RuntimeError, match="zk_rows_center first"):
            dev.seed_step(X[:2], np.ones(2), False)
        with pytest.raises(RuntimeError, match="no such component"):
            dev.moments(0, shift)
        want = dev.colsum()
        dev.center_at(shift)
        for t in (0, 9):
            with pytest.raises(RuntimeError, match="1 to 8 candidates|null pointer"):
                dev.seed_step(np.zeros((t, 48)), np.zeros(t), False)
        with pytest.raises(RuntimeError, match="1 to 256 clusters"):
            dev.lloyd(np.zeros((257, 48)))
        mix = mixture(X, 65, "diag", 0)
        with pytest.raises(RuntimeError, match="1 to 64 mixture"):
            dev.estep(*mix)
        dev.lloyd(np.zeros((3, 48)), False)
        dev.resp_from_labels(9)
        assert lib.zk_gmm_moments(h, 0, 4, _p(shift), _p(out)) != 0            # four planes per pass need D <= 47
        assert lib.zk_gmm_moments(h, 0, 9, _p(shift), _p(out)) != 0
        assert lib.zk_gmm_moments(h, 0, 3, _p(shift), _p(out)) == 0
        np.testing.assert_array_equal(dev.colsum(), want)
        assert dev.lloyd(np.zeros((3, 48)), True)[1][0] == 300
