"""NumPy statement of the rotation alignment (``zmoments.align`` / ``zk_align_rows``), its bounds and shared inputs.

Written from the formulas in DESIGN.md ("Rotation alignment"), not from the kernel:

    z_k = x_{n,+m} + i x_{n,-m} over the pairs k = (n, m >= 0);  s_k the 0 / 1 selection
    c_m = sum_{k: m_k = m} s_k z_k conj(t_k);   f(theta) = sum_m Re(c_m exp(-i m theta))

grid: ``linspace(0, 360 / symmetry, n_theta, endpoint=False)`` degrees, first maximum; refinement: 3 Newton steps on f' from the
grid maximum theta_0, a step only where f'' < 0, every iterate clamped to theta_0 +- one grid step, the result wrapped into
[0, 360 / symmetry) and kept only if f there is >= the grid maximum.

Bounds (u = 2^-53, P moments per row, A = sum_k s_k (|Re z_k| + |Im z_k|) (|Re t_k| + |Im t_k|)):
  score   |score - f_longdouble(angle)| <= 4 (P + 8) u A: a sum of at most 2P three-factor terms in any order with trigonometry
          good to a few ulp (the form of the bound in tests/test_gpu_inverse.py)
  rotate  elementwise (|a| + |b|) (8 + 2 m |theta_rad|) u: one rounding each for the degree-to-radian and m theta products (each
          moves the argument by at most m |theta_rad| u), the device sincos (no OCML accuracy table ships with the ROCm
          install this was written against, so SINCOS_ULP = 2 ulp is ASSUMED: 2 ulp of a value below 1 is at most 2u per
          factor, 4u over the two), two products and a sum (at most 3u) -- 7u + 2 m |theta_rad| u, stated as 8.
"""
import numpy as np

U = 2.0 ** -53
SINCOS_ULP = 2   # assumed, see above
PI_LD = np.longdouble(4) * np.arctan(np.longdouble(1))


def labels(n_max):
    nm = [(n, m) for n in range(n_max + 1) for m in range(-n, n + 1, 2)]
    return np.array([a for a, _ in nm]), np.array([b for _, b in nm])


def pairs(n, m):
    """Columns (ia of m >= 0, ib of -m; ib = ia for m = 0) and |m| of every pair; ValueError for an unpaired set."""
    n, m = np.asarray(n), np.asarray(m)
    at = {(int(a), int(b)): j for j, (a, b) in enumerate(zip(n, m))}
    if len(at) != len(n):
        raise ValueError("a label (n, m) occurs twice")
    for (a, b) in at:
        if (a, -b) not in at:
            raise ValueError(f"the label set is not paired: ({a}, {b})")
    keep = [j for j in range(len(n)) if m[j] >= 0]
    ia = np.array(keep, dtype=int)
    ib = np.array([at[(int(n[j]), -int(m[j]))] for j in keep], dtype=int)
    return ia, ib, np.asarray(m)[ia]


def select_mask(m, m_select):
    m = np.asarray(m)
    return np.ones(len(m), bool) if m_select is None else np.isin(np.abs(m), np.abs(np.atleast_1d(m_select)))


def _pair_parts(x, t, n, m, mask, dtype=np.float64):
    """Re and Im of s_k z_k conj(t_k), shape (N, T, K), and m_k."""
    ia, ib, mk = pairs(n, m)
    s = np.asarray(mask, bool)[ia]
    x, t = np.asarray(x, dtype=dtype), np.asarray(t, dtype=dtype)
    a, b = x[:, ia] * s, np.where(mk > 0, x[:, ib], 0) * s
    tr, ti = t[:, ia], np.where(mk > 0, t[:, ib], 0)
    re = a[:, None, :] * tr[None] + b[:, None, :] * ti[None]
    im = b[:, None, :] * tr[None] - a[:, None, :] * ti[None]
    return re, im, mk


def magnitude(x, t, n, m, mask):
    """A (N, T)."""
    ia, ib, mk = pairs(n, m)
    s = np.asarray(mask, bool)[ia]
    x, t = np.abs(np.asarray(x, float)), np.abs(np.asarray(t, float))
    za = (x[:, ia] + np.where(mk > 0, x[:, ib], 0)) * s
    ta = t[:, ia] + np.where(mk > 0, t[:, ib], 0)
    return za @ ta.T


def score_bound(x, t, n, m, mask):
    return 4 * (np.asarray(x).shape[1] + 8) * U * magnitude(x, t, n, m, mask)


def f_longdouble(x, t, n, m, mask, angle_deg):
    """f at angle_deg (N, T) in extended precision."""
    re, im, mk = _pair_parts(x, t, n, m, mask, np.longdouble)
    arg = np.asarray(angle_deg, np.longdouble)[:, :, None] * (PI_LD / 180) * mk.astype(np.longdouble)
    return (re * np.cos(arg) + im * np.sin(arg)).sum(axis=2)


def theta_grid(n_theta, symmetry=1):
    return np.linspace(0, 360 / symmetry, n_theta, endpoint=False)


def coefficients(x, t, n, m, mask):
    """c_m as (N, T, M + 1) real and imaginary parts, M the largest selected |m| (at least 0)."""
    re, im, mk = _pair_parts(x, t, n, m, mask)
    ia, _, _ = pairs(n, m)
    sel = np.asarray(mask, bool)[ia]
    top = int(mk[sel].max()) if sel.any() else 0
    cr = np.stack([re[:, :, mk == q].sum(axis=2) for q in range(top + 1)], axis=2)
    ci = np.stack([im[:, :, mk == q].sum(axis=2) for q in range(top + 1)], axis=2)
    return cr, ci


def _eval(cr, ci, deg):
    q = np.arange(cr.shape[2])
    arg = np.deg2rad(deg)[:, :, None] * q
    c, s = np.cos(arg), np.sin(arg)
    p = cr * c + ci * s
    return p.sum(axis=2), (q * (ci * c - cr * s)).sum(axis=2), -(q * q * p).sum(axis=2)


def grid_values(cr, ci, n_theta, symmetry=1):
    theta = theta_grid(n_theta, symmetry)
    arg = np.multiply.outer(np.deg2rad(theta), np.arange(cr.shape[2]))
    return cr @ np.cos(arg).T + ci @ np.sin(arg).T, theta      # (N, T, n_theta)


def key_values(t, mask, key):
    sq = (np.asarray(t, float)[:, np.asarray(mask, bool)] ** 2).sum(axis=1)
    return sq if key == "distance" else 1.0 / np.sqrt(sq)


def best_of(score, kv, key):
    return (kv[None] - 2 * score).argmin(axis=1) if key == "distance" else (score * kv[None]).argmax(axis=1)


def align_statement(x, t, n, m, mask=None, n_theta=360, symmetry=1, refine=True, key="distance", newton=3):
    """-> angle (N, T), score (N, T), best (N), grid values (N, T, n_theta)."""
    mask = np.ones(len(n), bool) if mask is None else np.asarray(mask, bool)
    cr, ci = coefficients(x, t, n, m, mask)
    grid, theta = grid_values(cr, ci, n_theta, symmetry)
    j0 = grid.argmax(axis=2)
    th0 = theta[j0]
    fmax = np.take_along_axis(grid, j0[:, :, None], axis=2)[:, :, 0]
    angle, score = th0.copy(), fmax.copy()
    if refine:
        period = 360 / symmetry
        step = period / n_theta
        th = th0.copy()
        for _ in range(newton):
            _, f1, f2 = _eval(cr, ci, th)
            go = f2 < 0
            with np.errstate(divide="ignore", invalid="ignore"):
                nxt = np.clip(th - np.rad2deg(f1 / f2), th0 - step, th0 + step)
            th = np.where(go & np.isfinite(nxt), nxt, th)
        th = np.where(th < 0, th + period, th)
        th = np.where(th >= period, th - period, th)
        f, _, _ = _eval(cr, ci, th)
        keep = f >= fmax
        angle, score = np.where(keep, th, th0), np.where(keep, f, fmax)
    best = best_of(score, key_values(t, mask, key), key).astype(np.int32)
    return angle, score, best, grid


def rotate_longdouble(x, n, m, angles_deg):
    ia, ib, mk = pairs(n, m)
    x = np.asarray(x, np.longdouble)
    out = x.copy()
    arg = np.asarray(angles_deg, np.longdouble)[:, None] * (PI_LD / 180) * mk.astype(np.longdouble)
    c, s = np.cos(arg), np.sin(arg)
    a, b = x[:, ia], x[:, ib]
    rot = mk > 0
    out[:, ia[rot]] = (a * c + b * s)[:, rot]
    out[:, ib[rot]] = (b * c - a * s)[:, rot]
    return out


def rotate_bound(x, n, m, angles_deg):
    ia, ib, mk = pairs(n, m)
    x = np.abs(np.asarray(x, float))
    mag = x[:, ia] + np.where(mk > 0, x[:, ib], 0)
    per_pair = mag * (8 + 2 * mk[None] * np.abs(np.deg2rad(np.asarray(angles_deg, float)))[:, None]) * U
    out = np.zeros_like(x)
    out[:, ia] = per_pair
    out[:, ib] = per_pair
    return out


def rotate_numpy(x, n, m, angles_deg):
    return rotate_longdouble(x, n, m, angles_deg).astype(np.float64)


def kmeans_aligned_numpy(X, n, m, k, init, max_iter=50, tol=1e-4, m_select=None, symmetry=1):
    """The NumPy twin of clustering.kmeans_aligned: same control flow on the statement above."""
    X = np.asarray(X, float)
    mask = select_mask(m, m_select)
    templates = np.array(init, float)
    tol_abs = float(np.mean(np.var(X, axis=0)) * tol)
    at = np.arange(len(X))

    def assign(tm):
        angle, score, best, _ = align_statement(X, tm, n, m, mask, 360, symmetry, True, "distance")
        return best, angle[at, best], score[at, best]

    labels, strict, n_iter = None, False, 0
    for n_iter in range(1, max_iter + 1):
        new, angles, own = assign(templates)
        if labels is not None and np.array_equal(new, labels):
            strict = True
            break
        labels = new
        Y = rotate_numpy(X, n, m, angles)
        new_t = templates.copy()
        for c in range(k):
            if (labels == c).any():
                new_t[c] = Y[labels == c].mean(axis=0)
        shift = ((new_t - templates) ** 2).sum()
        templates = new_t
        if shift <= tol_abs:
            break
    if not strict:
        labels, angles, own = assign(templates)
    inertia = float(((X[:, mask] ** 2).sum(axis=1) + key_values(templates, mask, "distance")[labels] - 2 * own).sum())
    return labels, templates, angles, inertia, n_iter


# ---- shared inputs ----------------------------------------------------------------------------------------------------
N_GRID = (1, 63, 64, 65, 257, 1000)
NMAX_GRID = (0, 1, 4, 8, 12, 13)
T_GRID = (1, 2, 5, 9)
NTHETA_GRID = (1, 2, 7, 360, 361)
# name -> (m_select, symmetry).  The (0, 3, 6) selection leaves a 3-fold f: on a 360-degree grid whose n_theta is a multiple of
# 3 its maximum is attained three times over, equal up to rounding, and "the first maximum" is then decided by the last bit.
# Such an f is what `symmetry` is for, so that selection is searched with symmetry=3 (a 120-degree grid: one maximum).
SELECTS = {"all": (None, 1), "m036": ((0, 3, 6), 3), "m0": ((0,), 1)}
_cache = {}


def case_inputs(n_max):
    """(rows (1000, P), templates (9, P), n, m) of the grid tests: seeded normal moments; sub-cases take leading slices."""
    if n_max not in _cache:
        n, m = labels(n_max)
        rng = np.random.RandomState(1000 + n_max)
        _cache[n_max] = (rng.standard_normal((1000, len(n))), rng.standard_normal((9, len(n))), n, m)
    return _cache[n_max]


def near_tie(grid, bound):
    """Pairs whose top two grid values lie within twice the bound (n_theta >= 2)."""
    top = np.sort(grid, axis=2)[:, :, -2:]
    return top[:, :, 1] - top[:, :, 0] <= 2 * bound


def rotated_pairs(n_max, count, seed, m_keep=None):
    """``count`` random templates and one exact rotation of each (by zmoments.rotate) -> (rows, templates, alpha, n, m)."""
    from mtflearn_amd import zmoments
    n, m = labels(n_max)
    if m_keep is not None:
        keep = np.isin(np.abs(m), m_keep)
        n, m = n[keep], m[keep]
    rng = np.random.RandomState(seed)
    t = rng.standard_normal((count, len(n)))
    alpha = rng.uniform(0, 360, count)
    rows = np.stack([zmoments(t[i:i + 1], n, m).rotate(alpha[i]).to_real().data[0] for i in range(count)])
    return rows, t, alpha, n, m


def circular_gap(a, b, period=360.0):
    d = np.abs(a - b) % period
    return np.minimum(d, period - d)


def planted(seed=7, per_class=300, n_max=6):
    """3 random templates, ``per_class`` rows each at random angles plus noise of 1 % of |t|; init = one row per class."""
    n, m = labels(n_max)
    rng = np.random.RandomState(seed)
    t = rng.standard_normal((3, len(n)))
    truth = np.repeat(np.arange(3), per_class)
    clean = rotate_numpy(t[truth], n, m, rng.uniform(0, 360, len(truth)))
    X = clean + rng.standard_normal(clean.shape) * (0.01 * np.linalg.norm(t, axis=1)[truth] / np.sqrt(len(n)))[:, None]
    order = rng.permutation(len(truth))
    X, truth = X[order], truth[order]
    init = np.stack([X[np.flatnonzero(truth == c)[0]] for c in range(3)])
    return X, truth, init, n, m
