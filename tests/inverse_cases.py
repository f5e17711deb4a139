"""Shared by tests/test_inverse_cpu.py and tests/test_gpu_inverse.py: the synthesis tables of ``ZPs.inverse_transform`` restated with
NumPy alone from the project's own basis, patches that lie exactly in the span of the basis, and the derived error bounds."""
import functools
import warnings

import numpy as np

U = 2.0 ** -53   # unit roundoff of float64


@functools.lru_cache(maxsize=None)
def zps(size, n_max):
    from mtflearn_amd import ZPs
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # n_max > size / 2 is a case here, not a mistake
        return ZPs(n_max=n_max, size=size)


def basis(z):
    return z.polynomials.reshape(len(z.n), -1)


def area(z):
    return np.pi * z.size * z.size / 4.0


def gram(z):
    b = basis(z)
    return b @ b.T / area(z)


def selection(z, m_select):
    if m_select is None:
        return np.ones(len(z.m))
    return np.isin(np.abs(z.m), np.abs(np.asarray(list(m_select)))).astype(np.float64)


def numpy_table(z, method, m_select=None):
    """``G^-1 diag(s) B`` by ``numpy.linalg.solve`` (LU, not the product's Cholesky) or ``diag(s) B``."""
    picked = basis(z) * selection(z, m_select)[:, None]
    return np.linalg.solve(gram(z), picked) if method == "lstsq" else picked


def span_patches(z, n, seed):
    """``(C, X)``: standard-normal coefficients ``(n, P)`` and the patches ``X = C B`` ``(n, size, size)``."""
    c = np.random.default_rng(seed).standard_normal((n, len(z.n)))
    return c, (c @ basis(z)).reshape(n, z.size, z.size)


def sum_bound(c, t):
    """Elementwise rounding bound of ``c @ t`` against another evaluation of the same sum: ``4 (P + 4) u (|c| @ |t|)``, P-term sums
    in any order on both sides (each within ``gamma_P ~ P u`` of the exact sum, doubled, with room for the fused products)."""
    return 4 * (c.shape[1] + 4) * U * (np.abs(c) @ np.abs(t))


def m_partition(z):
    """A partition of the ``|m|`` values of the set into three groups."""
    ms = np.unique(np.abs(z.m))
    return [tuple(ms[ms % 3 == r]) for r in range(3) if np.any(ms % 3 == r)]
