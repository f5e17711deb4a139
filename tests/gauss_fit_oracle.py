"""The Gaussian fit of include/zernike_hip.h ("Gaussian fits of key points") stated in NumPy, one window at a time: written from
the header's text, not from the kernel.  Plain float64 NumPy sums (pairwise, in pixel order), NumPy's ``exp`` and
``np.linalg.cholesky``: the device joins its sums in another order and has its own ``exp``, so the two agree to rounding, not
bit for bit.  ``fit_window`` is the header's loop, ``fit_points`` the host function's conventions around it."""
import numpy as np

CONVERGED, MAX_ITER, STALLED, NOT_FINITE = 0, 1, 2, 3
N_PARAMS = {"circular": 5, "elliptical": 7}


def disk_mask(size):
    r = size // 2
    d2 = np.add.outer((np.arange(size) - r) ** 2, (np.arange(size) - r) ** 2)
    return d2 <= r * r


def fitted_mask(size, mode):
    return disk_mask(size) if mode == "disk" else np.ones((size, size), bool)


def corners(pts, size):
    return np.rint(np.asarray(pts)).astype(int) - size // 2


def windows(frame, pts, size):
    first = corners(pts, size)
    return np.array([frame[y:y + size, x:x + size] for x, y in first], dtype=np.float64).reshape(len(first), size, size)


def unpack(p, model):
    """``(A, x0, y0, a, b, c, g)`` of a parameter vector of either model."""
    if model == "elliptical":
        return tuple(p)
    return p[0], p[1], p[2], p[3], 0.0, p[3], p[4]


def model_and_jacobian(p, model, col, row):
    A, x0, y0, a, b, c, g = unpack(p, model)
    dx, dy = col - x0, row - y0
    e = np.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy) / 2)
    f = g + A * e
    cols = [e, A * e * (a * dx + b * dy), A * e * (b * dx + c * dy)]
    if model == "elliptical":
        cols += [-A * e * dx * dx / 2, -A * e * dx * dy, -A * e * dy * dy / 2]
    else:
        cols += [-A * e * (dx * dx + dy * dy) / 2]
    cols += [np.ones_like(e)]
    return f, np.stack(cols, axis=1)


def sums(p, model, col, row, values):
    f, jac = model_and_jacobian(p, model, col, row)
    r = values - f
    return jac.T @ jac, jac.T @ r, float(r @ r)


def admissible(p, model, size):
    if not np.isfinite(p).all():
        return False
    _, x0, y0, a, b, c, _ = unpack(p, model)
    return bool(a > 0 and c > 0 and a * c - b * b > 0 and -0.5 <= x0 <= size - 0.5 and -0.5 <= y0 <= size - 0.5)


def shape_of(a, b, c):
    """``(sigma_major, sigma_minor, theta)`` of the precision matrix ``[[a, b], [b, c]]``, by the header's formulas."""
    l2 = (a + c) / 2 + np.sqrt(((a - c) / 2) ** 2 + b * b)
    l1 = (a * c - b * b) / l2
    return 1 / np.sqrt(l1), 1 / np.sqrt(l2), np.arctan2(0.0 - 2 * b, c - a) / 2


def fit_window(window, model="elliptical", mode=None, sigma0=None, tol=1e-10, max_iter=100):
    """The header's loop on one ``size x size`` float64 window: ``(p, rss, iterations, status)`` with ``p`` in window
    coordinates (NaN for status 3)."""
    size = window.shape[0]
    keep = fitted_mask(size, mode)
    row, col = (v[keep].astype(np.float64) for v in np.mgrid[:size, :size])
    values = np.asarray(window, np.float64)[keep]
    n = N_PARAMS[model]
    if not np.isfinite(values).all():
        return np.full(n, np.nan), np.nan, 0, NOT_FINITE
    sigma0 = size / 4 if sigma0 is None else sigma0
    lo, hi = values.min(), values.max()
    centre = float(size // 2)
    p = np.array([hi - lo, centre, centre, 1 / sigma0 ** 2] + ([0.0, 1 / sigma0 ** 2] if model == "elliptical" else []) + [lo])
    if lo == hi:
        return p, 0.0, 0, STALLED
    jtj, jtr, rss = sums(p, model, col, row, values)
    lam, it = 1e-3, 0
    while True:
        if it == max_iter:
            return p, rss, it, MAX_ITER
        it += 1
        accepted = False
        try:
            with np.errstate(all="ignore"):
                m = jtj + lam * np.diag(np.diag(jtj))
                if not np.isfinite(m).all():
                    raise np.linalg.LinAlgError
                factor = np.linalg.cholesky(m)
                delta = np.linalg.solve(factor.T, np.linalg.solve(factor, jtr))
                trial = p + delta
                if admissible(trial, model, size):
                    t_jtj, t_jtr, t_rss = sums(trial, model, col, row, values)
                    accepted = bool(t_rss <= rss)
        except np.linalg.LinAlgError:
            pass
        if accepted:
            p, jtj, jtr, rss = trial, t_jtj, t_jtr, t_rss
            lam = max(lam / 10, 1e-12)
            if (np.abs(delta) <= tol * (np.abs(p) + 1)).all():
                return p, rss, it, CONVERGED
        else:
            lam = lam * 10
            if lam > 1e12:
                return p, rss, it, STALLED


def fit_points(pts, frame, size, model="elliptical", mode=None, sigma=None, tol=1e-10, max_iter=100):
    """``(params (N, 8), iterations, status)`` of the windows of ``pts`` (no border clearing), columns as the library writes
    them: x, y, amplitude, sigma_major, sigma_minor, theta, background, rss.  ``p`` (N, n_params) comes fourth."""
    first = corners(pts, size)
    n = N_PARAMS[model]
    out, raw = np.empty((len(first), 8)), np.empty((len(first), n))
    its, status = np.empty(len(first), np.int32), np.empty(len(first), np.int32)
    for k, w in enumerate(windows(frame, pts, size)):
        p, rss, its[k], status[k] = fit_window(w, model, mode, sigma, tol, max_iter)
        raw[k] = p
        if status[k] == NOT_FINITE:
            out[k] = np.nan
            continue
        A, x0, y0, a, b, c, g = unpack(p, model)
        major, minor, theta = shape_of(a, b, c) if model == "elliptical" else (1 / np.sqrt(a), 1 / np.sqrt(a), 0.0)
        out[k] = (first[k, 0] + x0, first[k, 1] + y0, A, major, minor, theta, g, rss)
    return out, its, status, raw
