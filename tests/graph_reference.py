"""Independent extended-precision statements of what ``csrc/zk_graph.hip`` computes on the device -- TEST INFRASTRUCTURE.

Nothing here imports the product or ``oracle/``.  ``correlation_knn`` states the neighbour search (``knn_mfma_kernel``,
``knn_kernel``, ``knn_merge_kernel``) and ``affinities`` the bisection of ``affinity_kernel`` by plain ``np.longdouble``
routes of their own, and each also returns how far its decisions are from flipping: ``gap`` (the closest two distinct
distances among the ranks that decide a row's list) and ``margin`` (the closest any visited bisection step came to the
1e-5 tolerance).  A test that first requires ``gap`` and ``margin`` to be far above the device's rounding may then ask
for exact indices and exact betas on every row, with no row left out.

The second half builds the inputs of ``tests/test_gpu_graph_kernels.py`` and lists its cases;
``tests/test_graph_reference_cpu.py`` checks the references against scikit-learn and ``oracle/manifold_oracle.py`` and
holds ``gap > GAP_MIN`` / ``margin > MARGIN_MIN`` on every one of those inputs without a GPU.
"""
import functools
import hashlib
from collections import namedtuple

import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TOLERANCE = 1e-5          # the bisection's tolerance on |sum - target|
N_STEPS = 100
GAP_MIN = 1e-11           # two orders above the 1e-13 the device's distances are held to
MARGIN_MIN = 1e-9         # the device's float64 sum of < 64 terms <= 1 is within ~1e-14 of the extended-precision one
K_MAX = 64                # the library's limit on n_neighbors

Knn = namedtuple("Knn", "ind dist gap")
Affinities = namedtuple("Affinities", "P beta steps converged margin")


# ------------------------------------------------------------------------------------------------ the two references
def unit_rows(X):
    """Rows centred and scaled to unit length in extended precision; a row whose centred norm is 0 becomes zeros."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    C = X - X.mean(axis=1, keepdims=True)
    norm = np.sqrt((C * C).sum(axis=1, keepdims=True))
    return np.where(norm > 0, C / np.where(norm > 0, norm, LD(1)), LD(0))


def _ranked(X, keep):
    """The first ``keep`` (index, distance) of every row ordered by (distance, index), distances in extended precision."""
    Z = unit_rows(X)
    dist = LD(1) - np.einsum("if,jf->ij", Z, Z)          # self included
    order = np.argsort(dist, axis=1, kind="stable")[:, :keep]      # stable: equal distances keep the smaller index first
    return order, np.take_along_axis(dist, order, axis=1)


def _cut(order, dist, k):
    step = np.diff(dist[:, :k + 1], axis=1)               # ranks 0..k: rank k is the first one left out (absent when k = N)
    step = np.where(step > 0, step, LD(np.inf))           # exactly equal distances are no gap: the index rule decides them
    gap = step.min(axis=1, initial=LD(np.inf)).astype(np.float64)
    return Knn(np.ascontiguousarray(order[:, :k], dtype=np.int64), dist[:, :k].astype(np.float64), gap)


def correlation_knn(X, k):
    """The ``k`` nearest rows of every row of ``X`` under ``1 - corr`` (self included), ordered by (distance, index):
    ``Knn(ind, dist, gap)`` with ``dist`` rounded to float64 and ``gap`` the smallest difference between consecutive
    distinct distances among ranks 0..k of each row (inf where there is none)."""
    X = np.asarray(X)
    if not 1 <= k <= X.shape[0]:
        raise ValueError("need 1 <= k <= n_samples")
    return _cut(*_ranked(X, k + 1), k)


_ranked_cache = {}


def knn(X, k):
    """``correlation_knn`` with the ranking of ``X`` computed once for every ``k <= K_MAX`` (keyed by content)."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    key = (X.shape, hashlib.sha1(X.tobytes()).hexdigest())
    if key not in _ranked_cache:
        _ranked_cache[key] = _ranked(X, K_MAX + 1)
    if not 1 <= k <= min(K_MAX, X.shape[0]):
        raise ValueError("need 1 <= k <= min(64, n_samples)")
    return _cut(*_ranked_cache[key], k)


def affinities(dist, perplexity, local_connectivity):
    """``calculate_asymmetric_Pij`` on the (N, k) neighbour distances: per row the bisection for beta with
    ``sum_j>=1 exp(-max(d_j - rho, 0) beta) = log2(perplexity)`` to 1e-5, at most 100 steps, beta kept after the last
    update where it never gets there.  Beta and ``max(d - rho, 0)`` are float64 (doubling and halving are exact, and a
    float64 difference is what goes into the exponent); products, ``exp`` and sums are extended precision.

    Returns ``Affinities(P, beta, steps, converged, margin)``: ``P`` float64 with the machine-epsilon floor and a zero
    first column, ``steps`` the number of sums evaluated (1..100), ``converged`` whether one of them met the tolerance,
    ``margin`` the minimum over those sums of ``| |sum - target| - 1e-5 |``."""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    if not 0 <= local_connectivity < k:
        raise ValueError("need 0 <= local_connectivity < k")
    v = np.maximum(dist - dist[:, [local_connectivity]], 0.0)
    target = np.log2(np.float64(perplexity))
    lo, hi, beta = np.zeros(n), np.full(n, np.inf), np.ones(n)
    steps, converged, margin = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.full(n, np.inf)
    active = np.arange(n)
    for _ in range(N_STEPS):
        if not active.size:
            break
        b = beta[active]
        total = np.exp(-(v[active, 1:].astype(LD) * b[:, None].astype(LD))).sum(axis=1)
        off = np.abs(total - LD(target))
        steps[active] += 1
        margin[active] = np.minimum(margin[active], np.abs(off - LD(TOLERANCE)).astype(np.float64))
        done = off < LD(TOLERANCE)
        converged[active[done]] = True
        above = total - LD(target) > 0
        up, down = active[~done & above], active[~done & ~above]
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
        hi[down] = beta[down]
        beta[down] = (beta[down] + lo[down]) / 2.0
        active = active[~done]
    P = np.exp(-(v.astype(LD) * beta[:, None].astype(LD))).astype(np.float64)
    P[P < EPS] = EPS
    P[:, 0] = 0.0
    return Affinities(P, beta, steps, converged, margin)


def affinity_bound(dist, local_connectivity, ref):
    """Per element, what ``|P - P_ref|`` may be for a float64 ``exp(-fl(v beta))``: ``(4 + v beta) 2^-52 P_ref`` -- the
    argument's rounding moves the result by ``v beta 2^-53`` of itself, the rest allows an ``exp`` good to 1-2 ulp and
    the reference's own rounding to float64.  Zero (exact equality) for the first column and for elements on the
    machine-epsilon floor."""
    dist = np.asarray(dist, dtype=np.float64)
    v = np.maximum(dist - dist[:, [local_connectivity]], 0.0)
    with np.errstate(over="ignore"):
        bound = (4.0 + v * ref.beta[:, None]) * 2.0 ** -52 * ref.P
    bound[ref.P == EPS] = 0.0
    bound[:, 0] = 0.0
    return bound


# -------------------------------------------------------------------------------------------------- the dispatch
def mfma_instance(d, k):
    """(K, NS) of the ``knn_mfma_kernel<K, NS, 1>`` that ``zk_rows_knn_correlation`` launches for ``d <= 96`` features
    and ``k <= 16`` neighbours (restated from the dispatch, not imported)."""
    ns = 2 if d <= 8 else 4 if d <= 16 else 8 if d <= 32 else (d + 15) // 16 * 4
    return (10 if k <= 10 else 16), ns


MFMA_INSTANCES = {(K, NS) for K in (10, 16) for NS in (2, 4, 8, 12, 16, 20, 24)}


def stage_rows(d):
    """Candidate rows per LDS stage of the matrix-core kernel: 16 SB, SB = 4 up to NS = 12 and 2 above."""
    return 64 if mfma_instance(d, 1)[1] <= 12 else 32


def part_bounds(n, d, parts):
    """First candidate row of every part of the matrix-core search (the kernel's t_lo per blockIdx.y)."""
    n_stages = (n + 63) // 64 * 64 // stage_rows(d)
    return [n_stages * p // parts * stage_rows(d) for p in range(parts)]


def scalar_wave_span(n):
    """Candidates per wave of ``knn_kernel<16, 4>``: ``((Np / 8 + 3) / 4) 8`` with ``Np`` = n rounded up to 8."""
    np8 = (n + 7) // 8 * 8
    return (np8 // 8 + 3) // 4 * 8


# ---------------------------------------------------------------------------------------------------- the inputs
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def offset_rows(n, d, seed):
    """Distinct random rows with a per-feature offset (what the existing neighbour tests draw)."""
    rng = np.random.default_rng(seed)
    return _frozen(rng.standard_normal((n, d)) + rng.standard_normal(d))


# (n, d, k) of the matrix-core search.  D: both sides of every NS boundary; k: both sides of the K boundary.  Every D
# meets every k at N = 17 and 65 (one row into the second block of 16 / the second tile of 64), N = k = 16, one row short
# of a tile, a full tile and 129 (three tiles, one row in the last) once each, and N = 1000 with the longest list of
# either K -- so each of the 14 (K, NS) runs below 64 rows, at 64 or 65, and at 1000.
MFMA_DS = (8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96)
MFMA_CASES = ([(n, d, k) for d in MFMA_DS for n in (17, 65) for k in (1, 10, 11, 16)]
              + [case for d in MFMA_DS for case in ((16, d, 16), (63, d, 10), (64, d, 11), (129, d, 1))]
              + [(1000, d, k) for d in MFMA_DS for k in (10, 16)])
MFMA_SEED = 101

# ZK_KNN_PARTS settings per shape (None = unset); the largest part count each shape allows is n_stages / 16
PARTS_CASES = [((2100, 40, 102), (None, 1, 2)), ((1600, 50, 103), (1, 2, 3, 16))]
PARTS_KS = (10, 16)

# knn_kernel<16, 4> (ZK_KNN_SCALAR=1): at N = 8, 9 three of the four wave ranges are empty, at 63 / 65 the last is short
SCALAR_KS = (1, 9, 16)
SCALAR_SHAPES = [(n, d) for n in (8, 9, 63, 65, 200, 1000, 2100) for d in (3, 45, 96) if n * n * d <= 2.5e8]
SCALAR_SEEDS = {(1000, 3): 1000, (2100, 3): 1043}        # D = 3 leaves a circle: the default seed has pairs closer than GAP_MIN
SCALAR_SEED = 104
# knn_kernel<32, 1> and <64, 1> (k > 16): both ends of each list length, N = k (every row is everybody's neighbour)
WIDE_KS = (17, 32, 33, 64)
WIDE_DS = (5, 91)
WIDE_SEED = 105


def wide_shapes(k):
    return [(n, d) for n in (k, k + 1, 130, 777) for d in WIDE_DS]


def scalar_rows(n, d):
    return offset_rows(n, d, SCALAR_SEEDS.get((n, d), SCALAR_SEED))


# runs of identical rows planted in distinct random rows, (start, length).  Twenty rows cannot lie inside one block of
# 16, so that case is a run of 12; every other run has 20 rows and straddles what its comment names.
TIE_N = 2100
TIE_DS = (40, 50)         # SB = 4 (stages of 64 rows) and SB = 2 (stages of 32)
TIE_KS = (9, 16)
TIE_RUNS = [(28, 20),     # the first stage boundary of SB = 2 (row 32)
            (60, 20),     # the first stage boundary of SB = 4 (row 64)
            (98, 12),     # inside the block 96..111: all four lane groups, three of the four q
            (160, 20),    # from the first row of a block into the next
            (201, 20),    # across a block boundary (208) inside one stage
            (518, 20),    # the first wave range of knn_kernel<16, 4> ends at 528
            (1014, 20),   # D = 40: two parts meet at row 1024
            (1046, 20),   # D = 50: two parts meet at row 1056, which is also where the second wave range ends
            (1574, 20),   # the third wave range ends at 1584
            (2080, 20)]   # the last rows: the tail stage, with padding rows behind them
TIE_SEED = 106


@functools.lru_cache(maxsize=None)
def tie_rows(d):
    X = np.array(offset_rows(TIE_N, d, TIE_SEED + d))
    for start, length in TIE_RUNS:
        X[start:start + length] = X[start]
    return _frozen(X)


# rows without variation: (value planted, index); -1 is the last row.  0.1 and 1e-3 are not dyadic: their float64 mean
# over D features need not be the value itself.
CONSTANT_SHAPES = ((130, 12), (1000, 45))
CONSTANT_ROWS = ((0.0, 0), (1.0, 15), (-2.5, 16), (0.1, 63), (1e-3, -1))
CONSTANT_KS = (9, 16, 17, 40)      # with ZK_KNN_SCALAR=1 as well for the first two: every kernel family
CONSTANT_SEED = 107


@functools.lru_cache(maxsize=None)
def constant_rows(n, d):
    X = np.array(offset_rows(n, d, CONSTANT_SEED))
    for value, at in CONSTANT_ROWS:
        X[at] = value
    return _frozen(X)


def constant_index(n):
    return [at % n for _, at in CONSTANT_ROWS]


AFFINITY_SHAPES = ((1000, 20), (130, 45))
AFFINITY_KS = (2, 5, 17, 40)
# Every matrix takes the full cross of the settings.  A bisection that converges passes through |sum - target| of the
# order of the tolerance, halving as it goes, so about one row-setting in 7 000 comes within MARGIN_MIN = 1e-9 of it:
# about every second seed clears the 6 000 row-settings of the 130-row matrix, about one in forty the 56 000 of the
# 1000-row one (261 is the first from 200 up).
AFFINITY_SEEDS = {(1000, 20): 261, (130, 45): 108}


def affinity_rows(n, d):
    return offset_rows(n, d, AFFINITY_SEEDS[n, d])


def affinity_settings(k):
    """(perplexity, local_connectivity) for k neighbours: the full cross of perplexity 1.5, k / 2, k, 3 k and
    local_connectivity 0, 1, 3, k - 1 (where below k)."""
    perplexities = sorted({1.5, k / 2, float(k), 3.0 * k})
    connectivities = sorted({lc for lc in (0, 1, 3, k - 1) if 0 <= lc < k})
    return [(p, lc) for p in perplexities for lc in connectivities]


def surely_exhausts(k, perplexity, local_connectivity):
    """Whether no beta can bring the sum within the tolerance of log2(perplexity): the ``local_connectivity`` terms at or
    below rho are 1 each whatever beta is, and k - 1 terms cannot add up to more than k - 1."""
    target = np.log2(perplexity)
    return local_connectivity > target + 2 * TOLERANCE or k - 1 < target - 2 * TOLERANCE


def affinity_cases():
    """(n, d, k, settings) of every affinity run."""
    return [(n, d, k, affinity_settings(k)) for n, d in AFFINITY_SHAPES for k in AFFINITY_KS]
