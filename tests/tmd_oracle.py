"""NumPy statement of what TMDImageSimulator.simulate computes, written from the description of the reference
(datasets/_tmd_simulator.py, scipy.ndimage.gaussian_filter, scipy.signal.fftconvolve) and not from the device code.

    delta          one species' float32 delta image: np.add.at at the rounded positions, ascending index;
    scales         the float32 scale of every atom of a species from the stored vacancies and dopants -- the reference's
                   indexing (a global site index used inside the species' array) or the consistent one;
    exact_image    E: per species the exact float64 separable convolution with g[j] = exp(-j^2 / 2 sigma^2), |j| <= ksize // 2,
                   zeros outside the frame, times A, summed over species with no float32 rounding anywhere;
    gauss_image    use_fft=False restated pass by pass: axis 0 then axis 1 with 'reflect', each pass summed in float64 in
                   correlate1d's order (t = c w[0]; t += (left + right) w[j], j = r .. 1) and stored as float32, then
                   float32(A) * blurred and the sum over species in float32.
"""
import numpy as np


def delta(size, positions, scales):
    img = np.zeros(size, dtype=np.float32)
    h, w = size
    xi = np.round(positions[:, 0]).astype(int)
    yi = np.round(positions[:, 1]).astype(int)
    keep = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    np.add.at(img, (yi[keep], xi[keep]), np.asarray(scales, dtype=np.float32)[keep])
    return img


def scales(n_atoms, label, vacancies, dopants, global_indices=None):
    """``global_indices``: None for the reference's behaviour; else the ascending global site indices of this species, and a
    stored index marks the atom at its place in them."""
    out = np.ones(n_atoms, dtype=np.float32)
    for entries in (vacancies, dopants):
        for entry_label, index, scale in entries:
            if entry_label != label:
                continue
            if global_indices is not None:
                hits = np.flatnonzero(np.asarray(global_indices) == index)
                if len(hits) == 0:
                    continue
                index = int(hits[0])
            if 0 <= index < n_atoms:
                out[index] = scale
    return out


def fft_half_kernel(sigma):
    half = (int(6 * sigma) | 1) // 2
    return np.exp(-np.arange(half + 1, dtype=np.float64) ** 2 / (2 * sigma ** 2))


def gauss_half_kernel(sigma):
    """Half of scipy.ndimage's normalised Gaussian kernel at truncate 4.0, centre first."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return phi[radius:]


def _pass(array, w, axis, mode):
    """One symmetric correlation along ``axis`` in float64, correlate1d's order of operations."""
    r = len(w) - 1
    a = np.moveaxis(np.asarray(array, dtype=np.float64), axis, -1)
    n = a.shape[-1]
    pad = [(0, 0)] * (a.ndim - 1) + [(r, r)]
    ext = np.pad(a, pad, mode="symmetric") if mode == "reflect" else np.pad(a, pad, mode="constant")
    t = ext[..., r:r + n] * w[0]
    for j in range(r, 0, -1):
        t = t + (ext[..., r - j:r - j + n] + ext[..., r + j:r + j + n]) * w[j]
    return np.moveaxis(t, -1, axis)


def exact_species(mask, sigma, A):
    g = fft_half_kernel(sigma)
    return A * _pass(_pass(mask, g, 0, "zeros"), g, 1, "zeros")


def exact_image(masks, params):
    """E.  ``masks``: the species' delta images; ``params``: their ``{'sigma', 'A'}``."""
    return sum(exact_species(m, p['sigma'], p['A']) for m, p in zip(masks, params))


def gauss_species(mask, sigma, A):
    w = gauss_half_kernel(sigma)
    first = _pass(mask.astype(np.float32), w, 0, "reflect").astype(np.float32)
    second = _pass(first, w, 1, "reflect").astype(np.float32)
    return np.float32(A) * second


def gauss_image(masks, params):
    total = np.zeros(masks[0].shape, dtype=np.float32)
    for m, p in zip(masks, params):
        total += gauss_species(m, p['sigma'], p['A'])
    return total


def fft_bound(E, n_species):
    """(S / 2) spacing32(peak) + 1e-12 peak: each of the S float32 accumulations rounds once."""
    peak = float(np.max(E))
    return 0.5 * n_species * float(np.spacing(np.float32(peak))) + 1e-12 * peak
