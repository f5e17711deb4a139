"""An independent host statement of what ``mtflearn_amd.graph.estimate_d`` and ``features.refine_points`` compute, for the
goldens (tests/make_golden_refine.py) and the CPU tests (tests/test_refine_reference_cpu.py).

TEST INFRASTRUCTURE, written from the definitions, not from the code under test: the neighbour distances are scikit-learn's
(``NearestNeighbors(12, algorithm='ball_tree')``, the reference's query), the histogram is ``np.histogram``, Li's tolerance is
``np.unique`` and its means are ``np.mean``.  The two thresholds are the published algorithms as scikit-image states them (Otsu:
256 bins over the sample's range, the bin centre that maximises the between-class variance; Li: the iteration of
``threshold_li`` from the mean, ending when two iterates differ by no more than half the smallest gap between distinct values).
scikit-image itself is not installed here, so parity with it is unpinned.

Also here: ``kernel_bin_rule``, NumPy's own binning rule as the device applies it value by value (the CPU test holds it to
``np.histogram``), and ``sequential_refine``, the row-major float64 statement of the centroid sums (held bit-equal to the SciPy
route of the host ``center_of_mass_refine``)."""
import numpy as np

KS = tuple(range(2, 13))


def knn(pts):
    from sklearn.neighbors import NearestNeighbors
    return NearestNeighbors(n_neighbors=KS[-1], algorithm="ball_tree").fit(pts).kneighbors(pts)[0]


def otsu(d):
    """``(threshold, counts)``; counts is None when all values are equal (that value is the threshold)."""
    if d.min() == d.max():
        return d.flat[0], None
    counts, edges = np.histogram(d, bins=256)
    centers = (edges[:-1] + edges[1:]) / 2
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    m1 = np.cumsum(counts * centers) / w1
    m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
    return centers[np.argmax(w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2)], counts


def li(d):
    """``(threshold, iterations, margin)``: ``margin`` is how close, relative to the tolerance, any ``|t - t_prev|`` of the run
    came to the tolerance (a run that stops within rounding of that boundary pins nothing)."""
    if d.min() == d.max():
        return d.flat[0], 0, np.inf
    low = d.min()
    v = d - low
    tolerance = np.min(np.diff(np.unique(v))) / 2
    t, t_prev, iterations, margin = np.mean(v), -2 * tolerance, 0, np.inf
    with np.errstate(all="ignore"):
        while True:
            margin = min(margin, abs(abs(t - t_prev) - tolerance) / tolerance)
            if not abs(t - t_prev) > tolerance:
                break
            t_prev = t
            iterations += 1
            fore = v > t_prev
            mean_fore, mean_back = np.mean(v[fore]), np.mean(v[~fore])
            if mean_back == 0:
                break
            t = (mean_back - mean_fore) / (np.log(mean_back) - np.log(mean_fore))
    return t + low, iterations, margin


def estimate(pts, threshold, dd=None):
    """The reference's rule (graph/vnn.py:18-40) with the thresholds above; every part of it, as a dict."""
    dd = knn(pts) if dd is None else dd
    ts, scores, counts, iterations, margins = [], [], [], [], []
    for k in KS:
        d = dd[:, 1:k].ravel()
        if threshold == "otsu":
            t, c = otsu(d)
            counts.append(np.zeros(256, np.int64) if c is None else c)
        else:
            t, it, margin = li(d)
            iterations.append(it)
            margins.append(margin)
        ts.append(t)
        scores.append((np.count_nonzero(d > t) / len(d)) * (np.count_nonzero(d <= t) / len(d)))
    best = int(np.argmax(scores))
    return {"dd": dd, "ts": np.array(ts), "scores": np.array(scores), "t": float(ts[best]), "k": KS[best],
            "counts": np.array(counts), "iterations": np.array(iterations), "margins": np.array(margins)}


def kernel_bin_rule(d, first, last):
    """The 256-bin counts of ``d`` under the rule csrc/zk_np_bins.h applies to one value at a time: index
    ``(v - first) / (last - first) * 256`` truncated, 256 folded into 255, one down when ``v < edges[index]``, one up when
    ``v >= edges[index + 1]`` outside the last bin; ``edges = np.linspace(first, last, 257)``."""
    edges = np.linspace(first, last, 257)
    idx = (((d - first) / (last - first)) * 256.0).astype(np.int64)
    idx[idx == 256] = 255
    idx[d < edges[idx]] -= 1
    idx[(d >= edges[idx + 1]) & (idx != 255)] += 1
    return np.bincount(idx, minlength=256)


def sequential_refine(data, pts, size, mode):
    """The centroids as the kernel states them: a pixel belongs to the largest label whose box covers it; a point sums, in
    row-major order and in float64, the pixels it owns (disk mode: only those inside its own disk) -- value, value * float(row),
    value * float(col), each product rounded once."""
    owner = np.zeros(data.shape, np.int64)
    for label, (px, py) in enumerate(pts, start=1):
        owner[py - size:py + size + 1, px - size:px + size + 1] = label
    out = np.empty((len(pts), 2))
    with np.errstate(all="ignore"):
        for label, (px, py) in enumerate(pts, start=1):
            s, sr, sc = np.float64(0), np.float64(0), np.float64(0)
            for row in range(py - size, py + size + 1):
                for col in range(px - size, px + size + 1):
                    if owner[row, col] != label:
                        continue
                    if mode == "disk" and (row - py) ** 2 + (col - px) ** 2 > size ** 2:
                        continue
                    v = np.float64(data[row, col])
                    s, sr, sc = s + v, sr + v * np.float64(row), sc + v * np.float64(col)
            out[label - 1] = sc / s, sr / s
    return out
