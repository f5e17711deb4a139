"""The row passes of csrc/zk_rows.hip, zk_kmeans.hip and zk_mixture.hip (mtflearn_amd.clustering.DeviceRows) stated by another route.

Every pass is written in ``np.longdouble`` (64-bit mantissa on x86: 2^11 times finer than the kernels' float64), in row
chunks so that memory stays small.  Decisions are ordered by (value, index) -- the first minimum / maximum wins, as in
scikit-learn -- and every decision comes back with its margin, so a test can tell a decided label from a lucky one:

* Lloyd label: (second-best - best squared distance) / (|x|^2 + |c_best|^2);
* E-step label: best - second-best weighted log probability (a row is decided when this exceeds a multiple of 2^-53 times
  the magnitude of the terms its quadratic forms are built from, which comes back beside it);
* seed_pick: distance of the draw from the nearest cumulative sum, over the total.

Sums come back with the sum of the absolute values of their terms, so that a bound reads ``c * eps * sum|terms|``.

The ``exact_*`` functions state the same passes for matrices of small dyadic values (integers / 4): every product and sum is
then an integer multiple of 1/16 far below 2^53, float64 arithmetic is exact in ANY order (the BLAS calls below included), and
a kernel's result must be equal, not close.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53                      # unit roundoff of the kernels' float64
CHUNK = 4096


def _chunks(n):
    for r0 in range(0, n, CHUNK):
        yield slice(r0, min(n, r0 + CHUNK))


def _ld(a):
    return np.asarray(a, dtype=LD)


# ---- column statistics ------------------------------------------------------------------------------------------------
def colsum(X):
    """(column sums, column sums of |x|)"""
    s, a = np.zeros(X.shape[1], LD), np.zeros(X.shape[1], LD)
    for c in _chunks(len(X)):
        x = _ld(X[c])
        s += x.sum(axis=0)
        a += np.abs(x).sum(axis=0)
    return s, a


def center_at(X, mean):
    """(column sums of (x - mean)^2, squared norms of the centred rows, number of rows with a non-finite element)"""
    mean = _ld(mean)
    sq, xsq, bad = np.zeros(X.shape[1], LD), np.empty(len(X), LD), 0
    with np.errstate(invalid="ignore", over="ignore"):
        for c in _chunks(len(X)):
            v = (_ld(X[c]) - mean) ** 2
            sq += v.sum(axis=0)
            xsq[c] = v.sum(axis=1)
            bad += int(np.sum(~np.isfinite(X[c]).all(axis=1)))
    return sq, xsq, bad


# ---- k-means++ --------------------------------------------------------------------------------------------------------
def seed_step(X, mean, cand, cand_sq, closest=None):
    """Distance rows (t, N) = min(closest, max(0, |x|^2 - 2 x.c + cand_sq)), their sums (the potentials), and per candidate
    the sum over the rows of the terms' magnitudes |x|^2 + 2 sum_i |x_i c_i| + |cand_sq|."""
    mean, cand, cand_sq = _ld(mean), _ld(cand), _ld(cand_sq)
    t, n = len(cand), len(X)
    dist, mag = np.empty((t, n), LD), np.zeros(t, LD)
    for c in _chunks(n):
        x = _ld(X[c]) - mean
        xs = (x * x).sum(axis=1)
        d = np.maximum((-2 * (cand @ x.T) + cand_sq[:, None]) + xs[None, :], 0)
        if closest is not None:
            d = np.minimum(d, _ld(closest[c])[None, :])
        dist[:, c] = d
        mag += (xs[None, :] + 2 * (np.abs(cand) @ np.abs(x).T) + np.abs(cand_sq)[:, None]).sum(axis=1)
    return dist, dist.sum(axis=1), mag


def seed_pick(closest, vals):
    """searchsorted(cumsum(closest), vals, 'left') clipped to N - 1, and the margin of every draw."""
    cum = np.cumsum(_ld(closest))
    vals = _ld(vals)
    idx = np.minimum(np.searchsorted(cum, vals, side="left"), len(cum) - 1).astype(np.int64)
    gap = np.abs(cum[None, :] - vals[:, None]).min(axis=1) if len(vals) else np.zeros(0, LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        return idx, gap / cum[-1]


# ---- Lloyd ------------------------------------------------------------------------------------------------------------
def lloyd(X, mean, centers, prev_labels=None):
    """One Lloyd pass: (labels, margins, sums (k, D), sums of |terms|, counts, changed)."""
    mean, centers = _ld(mean), _ld(centers)
    n, (k, d) = len(X), centers.shape
    csq = (centers * centers).sum(axis=1)
    labels, margin = np.empty(n, np.int32), np.full(n, np.inf, LD)
    sums, mags, counts = np.zeros((k, d), LD), np.zeros((k, d), LD), np.zeros(k)
    with np.errstate(invalid="ignore"):
        for c in _chunks(n):
            x = _ld(X[c]) - mean
            score = csq[None, :] - 2 * (x @ centers.T)
            score = np.where(np.isnan(score), np.inf, score)                 # a NaN never wins a `<`: label 0
            lab = np.argmin(score, axis=1)                                   # first minimum
            labels[c] = lab
            if k > 1:
                part = np.partition(score, 1, axis=1)
                margin[c] = (part[:, 1] - part[:, 0]) / ((x * x).sum(axis=1) + csq[lab])
            for j in range(k):
                sel = x[lab == j]
                sums[j] += sel.sum(axis=0)
                mags[j] += np.abs(sel).sum(axis=0)
                counts[j] += len(sel)
    prev = np.full(n, -1) if prev_labels is None else prev_labels
    return labels, margin, sums, mags, counts, int(np.sum(labels != prev))


def own_distance(X, mean, centers, labels):
    """(squared distance of every centred row to the centre of its label, sum_i (|x_i| + |mean_i| + |c_i|)^2: the size of
    the terms the differences are formed from)"""
    mean, centers = _ld(mean), _ld(centers)
    out, mag = np.empty(len(X), LD), np.empty(len(X), LD)
    for c in _chunks(len(X)):
        x, cen = _ld(X[c]), centers[labels[c]]
        v = (x - mean) - cen
        out[c] = (v * v).sum(axis=1)
        mag[c] = ((np.abs(x) + np.abs(mean) + np.abs(cen)) ** 2).sum(axis=1)
    return out, mag


# ---- Gaussian mixture -------------------------------------------------------------------------------------------------
def _weighted_log_prob(x, prec_chol, means, log_det, log_w):
    k, d = means.shape
    lp = np.empty((len(x), k), x.dtype)
    mag = np.zeros(len(x), x.dtype)
    const = x.dtype.type(d) * np.log(2 * np.pi * x.dtype.type(1))
    for c in range(k):
        b = means[c] @ prec_chol[c]
        y = x @ prec_chol[c] - b
        lp[:, c] = (-0.5 * (const + (y * y).sum(axis=1)) + log_det[c]) + log_w[c]
        ya = np.abs(x) @ np.abs(prec_chol[c]) + np.abs(b)
        mag = np.maximum(mag, 0.5 * (const + (ya * ya).sum(axis=1)) + abs(log_det[c]) + abs(log_w[c]))
    return lp, mag


def _decide(lp):
    lab = np.argmax(lp, axis=1).astype(np.int32)                             # first maximum
    if lp.shape[1] == 1:
        return lab, np.full(len(lp), np.inf, lp.dtype)
    part = np.partition(lp, lp.shape[1] - 2, axis=1)
    return lab, part[:, -1] - part[:, -2]


def estep(X, prec_chol, means, log_det, log_w, want_resp=True):
    """(sum of log-sum-exp, per row the magnitude of the terms behind it, labels, margins, resp (N, k) or None)

    The magnitude of a row is max_c [0.5 (D log 2pi + sum_j (sum_i |x_i P_ij| + |(mu P)_j|)^2) + |logdet_c| + |logw_c|]: what
    rounding in the quadratic form scales with, the form itself being a difference of such terms."""
    args = [_ld(a) for a in (prec_chol, means, log_det, log_w)]
    n, k = len(X), len(means)
    labels, margin = np.empty(n, np.int32), np.empty(n, LD)
    resp = np.empty((n, k), LD) if want_resp else None
    total, mags = LD(0), np.empty(n, LD)
    for c in _chunks(n):
        lp, mag = _weighted_log_prob(_ld(X[c]), *args)
        labels[c], margin[c] = _decide(lp)
        top = lp.max(axis=1)
        lse = np.log(np.exp(lp - top[:, None]).sum(axis=1)) + top
        total += lse.sum()
        mags[c] = mag
        if want_resp:
            resp[c] = np.exp(lp - lse[:, None])
    return total, mags, labels, margin, resp


def estep_labels(X, prec_chol, means, log_det, log_w, screen=1e-6):
    """Labels, margins and the rows' magnitudes alone, for large N: a float64 pass first (its error is orders below ``screen`` times the magnitude
    of the terms), then the rows it leaves within ``screen`` of a tie again in longdouble."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    labels, margin, mags = np.empty(n, np.int32), np.empty(n, LD), np.empty(n, LD)
    ld_args = [_ld(a) for a in (prec_chol, means, log_det, log_w)]
    for c in _chunks(n):
        lp, mag = _weighted_log_prob(X[c], *[np.asarray(a, dtype=np.float64) for a in (prec_chol, means, log_det, log_w)])
        lab, mar = _decide(lp)
        close = np.flatnonzero(mar < screen * mag)
        if len(close):
            lab[close], m2 = _decide(_weighted_log_prob(_ld(X[c][close]), *ld_args)[0])
            mar = mar.astype(LD)
            mar[close] = m2
        labels[c], margin[c], mags[c] = lab, mar, mag
    return labels, margin, mags


def moments(X, w, shift):
    """sum_r w_r z_r z_r^T with z = [x - shift | 1]  (w None: unit weights), and the same sum of |w_r| |z_r| |z_r|^T."""
    shift = _ld(shift)
    d1 = X.shape[1] + 1
    g, a = np.zeros((d1, d1), LD), np.zeros((d1, d1), LD)
    for c in _chunks(len(X)):
        z = np.concatenate([_ld(X[c]) - shift, np.ones((len(X[c]), 1), LD)], axis=1)
        wc = np.ones(len(z), LD) if w is None else _ld(w[c])
        g += (z * wc[:, None]).T @ z
        a += (np.abs(z) * np.abs(wc)[:, None]).T @ np.abs(z)
    return g, a


def project(X, mean, components):
    mean, comp = _ld(mean), _ld(components)
    y, a = np.empty((len(X), len(comp)), LD), np.empty((len(X), len(comp)), LD)
    for c in _chunks(len(X)):
        x = _ld(X[c]) - mean
        y[c] = x @ comp.T
        a[c] = np.abs(x) @ np.abs(comp).T
    return y, a


def ratio(got, ref, mag):
    """max |got - ref| / (eps * sum|terms|): the figure the bounds of the GPU tests are stated in."""
    got, ref, mag = _ld(got), _ld(ref), _ld(mag)
    err = np.abs(got - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0, err / (EPS * mag))
    return float(np.max(r)) if r.size else 0.0


# ---- exact statements for dyadic matrices --------------------------------------------------------------------------------
# Q is the matrix in units of 1/4 (integers), S the shift and C the centres in the same units.  Everything below is integer-
# valued float64; `headroom` returns the largest sum of |terms| any pass forms, in the finest unit (1/16), which the CPU
# tests hold below 2^53.
def exact_headroom(Q, S, C=None):
    z = np.abs(Q.astype(np.float64) - S).max(axis=0)
    worst = len(Q) * (max(z.max(), 4.0) ** 2)                      # a Gram entry (the constant column is 4 quarter-units)
    if C is not None:
        worst = max(worst, len(Q) * (np.sum(z * z) + 2 * np.max(np.abs(C) @ z) + np.max((C * C).sum(axis=1))))
    return worst


def exact_colsum(Q):
    return Q.sum(axis=0, dtype=np.int64) / 4.0


def exact_center(Q, S):
    z = Q.astype(np.int64) - S.astype(np.int64)
    return (z * z).sum(axis=0) / 16.0, (z * z).sum(axis=1) / 16.0


def exact_seed(Q, S, cand_Q, closest=None):
    """cand_Q: centred candidates in quarter units.  Distance rows (t, N) and potentials."""
    z = Q.astype(np.float64) - S
    cq = np.asarray(cand_Q, dtype=np.float64)
    d = np.maximum(((z * z).sum(axis=1)[None, :] - 2.0 * (cq @ z.T)) + (cq * cq).sum(axis=1)[:, None], 0.0) / 16.0
    if closest is not None:
        d = np.minimum(d, closest[None, :])
    return d, d.sum(axis=1)


def exact_lloyd(Q, S, C, prev_labels=None):
    z = Q.astype(np.float64) - S
    C = np.asarray(C, dtype=np.float64)
    score = (C * C).sum(axis=1)[None, :] - 2.0 * (z @ C.T)
    labels = np.argmin(score, axis=1).astype(np.int32)
    onehot = (labels[:, None] == np.arange(len(C))[None, :]).astype(np.float64)
    prev = np.full(len(Q), -1) if prev_labels is None else prev_labels
    return labels, (onehot.T @ z) / 4.0, onehot.sum(axis=0), int(np.sum(labels != prev))


def exact_own_distance(Q, S, C, labels):
    v = (Q.astype(np.float64) - S) - np.asarray(C, dtype=np.float64)[labels]
    return (v * v).sum(axis=1) / 16.0


def exact_moments(Q, S, labels=None, component=None):
    """Gram matrix of [x - shift | 1] over the rows whose label is `component` (all rows when labels is None)."""
    z = np.concatenate([Q.astype(np.float64) - S, np.full((len(Q), 1), 4.0)], axis=1)
    if labels is not None:
        z = z[labels == component]
    return (z.T @ z) / 16.0


def exact_project(Q, S, comp_Q):
    return ((Q.astype(np.float64) - S) @ np.asarray(comp_Q, dtype=np.float64).T) / 16.0
