"""Test-local oracle of mtflearn_amd.denoise: the two denoisers of the reference's ``denoise`` subpackage and the four window
operations of csrc/zk_denoise.hip as plain NumPy / SciPy / scikit-learn on a MATERIALISED window matrix.  Written from the
behaviour of the reference functions (what they return for what input), not from their text; it is the checker, never the
product."""
import numpy as np
from sklearn.utils.extmath import randomized_svd


def origins(extent, patch, step):
    """Window origins along an axis: 0, step, 2 step, ... below the last possible origin, which always closes the list."""
    last = extent - patch
    out = list(range(0, last, step))
    if not out or out[-1] != last:
        out.append(last)
    return np.array(out, dtype=np.int64)


def window_matrix(frame, ph, pw, ii, jj):
    """A (len(ii) * len(jj), ph * pw) float64: row a * len(jj) + b is the window at (ii[a], jj[b]), flattened row-major."""
    f = np.asarray(frame, dtype=np.float64)
    return np.stack([f[i:i + ph, j:j + pw].ravel() for i in ii for j in jj])


def apply(frame, ph, pw, ii, jj, q, mean=None):
    a = window_matrix(frame, ph, pw, ii, jj)
    return (a - mean) @ q if mean is not None else a @ q


def apply_t(frame, ph, pw, ii, jj, y):
    return window_matrix(frame, ph, pw, ii, jj).T @ y


def moments(frame, ph, pw):
    """Mean and covariance (divided by N - 1, by 1 for a single window) of every dense window."""
    h, w = np.shape(frame)
    a = window_matrix(frame, ph, pw, range(h - ph + 1), range(w - pw + 1))
    mean = a.mean(axis=0)
    c = a - mean
    return mean, (c.T @ c) / max(a.shape[0] - 1, 1)


def overlap_add(patches, shape, ph, pw, ii, jj):
    """Sum of the (N, ph * pw) patches laid at their origins over the number of patches on each pixel (0 / 0 -> NaN)."""
    acc = np.zeros(shape)
    cover = np.zeros(shape)
    for p, (i, j) in zip(np.asarray(patches).reshape(-1, ph, pw), [(i, j) for i in ii for j in jj]):
        acc[i:i + ph, j:j + pw] += p
        cover[i:i + ph, j:j + pw] += 1.0
    with np.errstate(invalid="ignore"):
        return acc / cover


def reconstruct(shape, ph, pw, ii, jj, y, v=None, mean=None):
    patches = y @ v if v is not None else np.asarray(y).reshape(len(y), -1)
    if mean is not None:
        patches = patches + mean
    return overlap_add(patches, shape, ph, pw, ii, jj)


def denoise_svd(frame, patch_size, n_components, extraction_step=None):
    """(clean, s): rank-n_components randomized SVD (scikit-learn's, global random state) of the window matrix, overlap-added."""
    ph, pw = (patch_size, patch_size) if np.isscalar(patch_size) else patch_size
    step = max(1, int(ph / 4)) if extraction_step is None else extraction_step
    h, w = np.shape(frame)
    ii, jj = origins(h, ph, step), origins(w, pw, step)
    a = window_matrix(frame, ph, pw, ii, jj)
    u, s, vt = randomized_svd(a, n_components, random_state=None)
    return overlap_add((u * s) @ vt, (h, w), ph, pw, ii, jj), s


def denoise_svd_memory_view(frame, p, n_components=None, threshold=0.9):
    """(recon, explained_variance_ratio, n_components): PCA of every dense p x p window, projected and overlap-added."""
    h, w = np.shape(frame)
    ii, jj = np.arange(h - p + 1), np.arange(w - p + 1)
    a = window_matrix(frame, p, p, ii, jj)
    mean, cov = moments(frame, p, p)
    vals, vecs = np.linalg.eigh(cov)
    vals = vals[::-1]
    total = vals.sum()
    ratio = vals / total if not np.isclose(total, 0.0) else np.zeros_like(vals)
    if n_components is None:
        n_components = int(np.sum(np.cumsum(ratio) < threshold) + 1) if np.any(ratio != 0) else 1
    n_components = max(1, min(int(n_components), vecs.shape[1]))
    top = vecs[:, -n_components:]
    return overlap_add(((a - mean) @ top) @ top.T + mean, (h, w), p, p, ii, jj), ratio, n_components
