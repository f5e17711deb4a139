"""GPU tests of mtflearn_amd.eels (csrc/zk_eels.hip) over the case table of tests/eels_cases.py.

Tolerances (derived before any run, from the reference's own error and the number format):

* Whittaker solve: the condition-free backward error, evaluated on the host in ``np.longdouble``,
  ``eta = ||A z - W x||_inf / (||A||_inf ||z||_inf + ||W x||_inf) <= 1e-14``.  A band LDL^T / Cholesky of half-bandwidth
  k <= 3 is backward stable with a constant of a few (k + 1) units of roundoff; 1e-14 is about 90 u.
* Baselines against the reference: ``max|got - golden| <= max(1e-12, 20 ref_vs_oracle) max|y|`` per case, ``ref_vs_oracle`` read
  from the golden file (the distance between the reference's sparse LU / dense Cholesky and LAPACK's band Cholesky on the same
  systems), never from the code under test.
* SNIP: elementwise ``|got - golden| <= 1e-12 (|golden| + 1)``: at 4e4 counts the inverse map amplifies an error in the
  transformed value by about 5e5, a few ulp there is about 1e-14 relative; the bound leaves about 100x for the device's
  log / exp.
* Iteration counts (the one discrete output) equal the golden's; everything said to be bit for bit is compared with
  ``assert_array_equal``.

Every case prints its measured distance before it asserts (``pytest -s`` shows them; profiles/eels.txt records them).
"""
import os
import warnings

import numpy as np
import pytest

import eels_cases as ec
import eels_oracle as eo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = {"als": "baseline_als", "arpls": "baseline_arpls", "airpls": "baseline_airpls", "snip": "baseline_snip"}


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "eels_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def eels():
    from mtflearn_amd import eels as module
    return module


def run(eels, method, data, axis=0, **kw):
    """``(baseline, iterations or None)``; no spectrum of the table may reach itermax, so a RuntimeWarning is an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        if method in ("arpls", "airpls"):
            return getattr(eels, FN[method])(data, axis=axis, return_info=True, **kw)
        return getattr(eels, FN[method])(data, axis=axis, **kw), None


def check(name, key, got, iters, cube, golden):
    method = ec.CONFIGS[name][0]
    ref = golden[f"{key}/ref"]
    assert got.dtype == np.float64 and got.shape == ref.shape
    if method == "snip":
        excess = np.abs(got - ref) / (np.abs(ref) + 1)
        print(f"{key}: max |got - golden| / (|golden| + 1) = {excess.max():.2e}")
        assert (excess <= 1e-12).all(), key
        return
    scale = np.abs(cube).max()
    bound = max(1e-12, 20 * float(golden[f"{key}/ref_vs_oracle"]))
    dist = np.abs(got - ref).max() / scale
    print(f"{key}: max |got - golden| / max|y| = {dist:.2e} (bound {bound:.2e}, ref_vs_oracle {float(golden[f'{key}/ref_vs_oracle']):.2e})")
    if iters is not None:
        assert iters.dtype == np.int32
        np.testing.assert_array_equal(iters, golden[f"{key}/iters"], err_msg=key)
    assert dist <= bound, key


@pytest.mark.parametrize("name", list(ec.CONFIGS))
def test_parity_with_the_reference(eels, golden, name):
    """Every shape of the table in float64, float32 and uint16 on ``axis=0`` of ``(L, H, W)``, and ``axis=-1`` of ``(N, L)``."""
    method, kw, lmin = ec.CONFIGS[name]
    for L, grid in ec.SHAPES:
        if L < lmin:
            continue
        key = f"{name}/{ec.shape_id(L, grid)}"
        cube = ec.cube(L, grid)
        first = None
        for dtype in ec.DTYPES:
            got, iters = run(eels, method, cube.astype(dtype), **kw)
            check(name, f"{key}", got, iters, cube, golden)
            if first is None:
                first = got
            else:
                np.testing.assert_array_equal(got, first)          # the casts are exact, so the three runs are one computation
        rows = np.ascontiguousarray(np.moveaxis(cube, 0, -1))       # (grid..., L)
        got, iters = run(eels, method, rows, axis=-1, **kw)
        np.testing.assert_array_equal(np.moveaxis(got, -1, 0), first)
        if iters is not None:
            np.testing.assert_array_equal(iters, golden[f"{key}/iters"])
        if len(grid) == 2:                                          # the energy axis in the middle: (H, L, W)
            mid = np.ascontiguousarray(np.moveaxis(cube, 0, 1))
            np.testing.assert_array_equal(np.moveaxis(run(eels, method, mid, axis=1, **kw)[0], 1, 0), first)


@pytest.mark.parametrize("k", [1, 2, 3])
def test_whittaker_backward_error(eels, k):
    rng = np.random.RandomState(k)
    worst = 0.0
    for L in (k + 1, 5, 7, 33, 64, 257):
        for lam in (1e2, 1e5):
            x = ec.spectra(L, 70, 50 + L)
            w = rng.uniform(0.05, 1.0, x.shape)
            w[:, ::7] = (rng.uniform(size=(L, 10)) > 0.5) + 1e-3     # near-binary masks, the reference's use
            z = eels.WhittakerSmooth(x, w, lam, differences=k)
            shared = w[:, 0].copy()
            z1 = eels.WhittakerSmooth(x, shared, lam, differences=k)
            for j in range(0, 70, 9):
                worst = max(worst, eo.backward_error(x[:, j], w[:, j], lam, k, z[:, j]), eo.backward_error(x[:, j], shared, lam, k, z1[:, j]))
            np.testing.assert_array_equal(z1[:, 0], z[:, 0])
            rows = eels.WhittakerSmooth(np.ascontiguousarray(x.T), np.ascontiguousarray(w.T), lam, differences=k, axis=-1)
            np.testing.assert_array_equal(rows.T, z)
    print(f"differences {k}: worst backward error {worst:.2e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("name", ["als", "arpls", "airpls2", "snip"])
def test_a_spectrum_alone_equals_itself_in_a_batch(eels, name):
    method, kw, lmin = ec.CONFIGS[name]
    cube = ec.cube(33, (130,))
    batch, iters = run(eels, method, cube, **kw)
    for j in (0, 63, 64, 129):
        one, it1 = run(eels, method, cube[:, j].copy(), **kw)
        assert one.shape == (33,) and one.dtype == np.float64
        np.testing.assert_array_equal(one, batch[:, j])
        if iters is not None:
            assert it1.shape == () and int(it1) == int(iters[j])


@pytest.mark.parametrize("name", ["als_stiff", "arpls", "airpls1", "airpls3", "snip_deep"])
def test_two_runs_and_two_chunkings_agree(eels, name):
    """A cap of one byte cuts the spectra into chunks of 64 (the least), the default leaves one chunk."""
    method, kw, lmin = ec.CONFIGS[name]
    cube = ec.cube(33, (130,))
    a, ia = run(eels, method, cube, **kw)
    b, ib = run(eels, method, cube, **kw)
    eels.set_scratch_bytes(1)
    try:
        c, ic = run(eels, method, cube, **kw)
        rows, _ = run(eels, method, np.ascontiguousarray(cube.T), axis=-1, **kw)
    finally:
        eels.set_scratch_bytes(0)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(a, rows.T)
    if ia is not None:
        np.testing.assert_array_equal(ia, ib)
        np.testing.assert_array_equal(ia, ic)


@pytest.mark.parametrize("name", ["als", "arpls", "airpls2", "snip"])
def test_resident_call_equals_the_host_call(eels, name):
    from mtflearn_amd import _native, resident
    method, kw, lmin = ec.CONFIGS[name]
    cube = ec.cube(33, (5, 13)).astype(np.float32)
    host, iters = run(eels, method, cube, **kw)
    dev = _native.DeviceArray.from_numpy(cube, _native.default_device())
    sig, base, it = resident.baseline_device(dev, method, return_signal=True, return_info=True, **kw)
    assert isinstance(base, _native.DeviceArray) and base.dtype == np.float64
    np.testing.assert_array_equal(base.numpy(), host)
    np.testing.assert_array_equal(sig.numpy(), cube.astype(np.float64) - host)
    if iters is not None:
        np.testing.assert_array_equal(it.numpy(), iters)
    import torch
    t = torch.from_numpy(np.ascontiguousarray(np.moveaxis(cube, 0, -1))).cuda()
    tb = resident.baseline_device(t, method, axis=-1, **kw)
    assert tb.is_cuda and tb.dtype == torch.float64
    np.testing.assert_array_equal(np.moveaxis(tb.cpu().numpy(), -1, 0), host)


@pytest.mark.parametrize("method", ["snip", "als", "arpls", "airpls"])
def test_remove_baseline_returns_signal_and_baseline(eels, method):
    cube = ec.cube(64, (65,)).astype(np.uint16)
    data = cube.astype(np.float64)
    signal, baseline = eels.remove_baseline(cube, method=method)
    np.testing.assert_array_equal(baseline, run(eels, method, cube)[0])
    np.testing.assert_array_equal(signal, data - baseline)          # one IEEE subtraction, on the device
    assert (np.abs(signal + baseline - data) <= 2.0 ** -52 * (np.abs(data) + np.abs(baseline))).all()
    s2, b2 = eels.remove_baseline(np.ascontiguousarray(cube.T), method=method, axis=1)
    np.testing.assert_array_equal(b2.T, baseline)
    np.testing.assert_array_equal(s2.T, signal)


def test_features_alias_is_snip(eels):
    from mtflearn_amd import features
    y = ec.cube(257, (1,))[:, 0]
    np.testing.assert_array_equal(features.baseline_correction(y, niter=24), eels.baseline_snip(y, niter=24))
    np.testing.assert_array_equal(features.baseline_correction(y), eels.baseline_snip(y))


def test_itermax_is_reported_once_per_call(eels):
    """One solve is never enough here: every spectrum takes all itermax = 1 solves, and one RuntimeWarning says how many."""
    cube = ec.cube(33, (130,))
    with pytest.warns(RuntimeWarning, match="130 of 130 spectra") as rec:
        base, iters = eels.baseline_airpls(cube, itermax=1, return_info=True)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    assert (iters == 1).all()
    np.testing.assert_array_equal(base, eels.WhittakerSmooth(cube, np.ones(33), 100, differences=1))
