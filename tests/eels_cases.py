"""Shared inputs and the case table of the EELS baseline tests (tests/test_eels_cpu.py, tests/test_gpu_eels.py,
tests/make_golden_eels.py).  Inputs are seeded and regenerated, never stored: a power-law tail, four Gaussian edges, Poisson
counts -- integer-valued float64 below 2^16, so the float32 and uint16 casts of a case hold exactly the same numbers and share
its golden (the reference run on the float64 cast of the same input).

Shapes are the smallest at which the kernel can go wrong, not the workload's own: L = 3 and 5 make the boundary rows of the
penalty overlap, 7 is below one prefetch block, 33 / 64 / 257 leave a remainder of it or none; N = 1, 63, 64, 65, 130 and a
(5, 13) grid cover a lone lane, partial waves and more than one workgroup.  L and N are paired, not crossed (the golden file
has to stay small); airPLS starts at L = 33 because at L = 7 the reference itself goes singular or runs to itermax.
"""
import numpy as np

SHAPES = [(3, (1,)), (3, (65,)), (5, (63,)), (5, (5, 13)), (7, (64,)), (7, (130,)), (33, (1,)), (33, (130,)), (33, (5, 13)),
          (64, (65,)), (257, (1,))]

# name -> (method, keyword arguments, smallest L)
CONFIGS = {
    "als": ("als", {}, 3),
    "als_stiff": ("als", {"lam": 1e5, "p": 0.01}, 3),
    "arpls": ("arpls", {}, 3),
    "airpls1": ("airpls", {"porder": 1}, 33),
    "airpls2": ("airpls", {"porder": 2}, 33),
    "airpls3": ("airpls", {"porder": 3}, 33),
    "snip": ("snip", {"niter": 10}, 3),
    "snip_deep": ("snip", {"niter": 200}, 3),      # niter > L / 2 at every L of the table
}
DTYPES = (np.float64, np.float32, np.uint16)


def shape_id(L, grid):
    return f"L{L}xN{'x'.join(str(g) for g in grid)}"


def cases():
    """``(key, config name, L, grid)`` of every golden entry."""
    return [(f"{name}/{shape_id(L, grid)}", name, L, grid) for name, (_, _, lmin) in CONFIGS.items() for L, grid in SHAPES if L >= lmin]


def spectra(L, n, seed):
    """``(L, n)`` float64 Poisson counts: every spectrum its own power law (amplitude 3e4 .. 5.5e4 at the first channel, falling by
    4^-0.3 .. 4^-1 over the range) and four Gaussian edges of its own heights, so that the iteration counts of a batch differ.
    The counts stay high (relative noise below 1 %) because airPLS stops on ``|sum d[d < 0]| < 0.001 sum |x|``: with noisier
    spectra its first-order runs end at itermax, which is not pinned."""
    rng = np.random.RandomState(seed)
    e = (np.arange(L, dtype=np.float64) + 0.5) / L
    amp = rng.uniform(3e4, 5.5e4, n)
    expo = rng.uniform(0.3, 1.0, n)
    lam = amp[None, :] * (1.0 + 3.0 * e[:, None]) ** (-expo[None, :])
    for centre in (0.2, 0.4, 0.6, 0.8):
        height = amp * rng.uniform(0.05, 0.3, n)
        width = rng.uniform(0.015, 0.04, n)
        lam += height[None, :] * np.exp(-0.5 * ((e[:, None] - centre) / width[None, :]) ** 2)
    counts = rng.poisson(lam).astype(np.float64)
    assert counts.max() < 2 ** 16          # the uint16 cast of a case is exact
    return counts


def cube(L, grid):
    """The ``(L,) + grid`` float64 cube of a table shape (energy-major, the native layout)."""
    n = int(np.prod(grid))
    # + 1: at seed 1000 L + n one spectrum of (7, 130) makes the reference's dense Cholesky in arPLS fail (not positive definite)
    return spectra(L, n, seed=1000 * L + n + 1).reshape((L,) + tuple(grid))
