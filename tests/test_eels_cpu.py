"""CPU checks of mtflearn_amd.eels: the host statement (tests/eels_oracle.py) against the goldens captured from the reference,
the conditions that keep the golden cases meaningful, the C ABI table, and every argument check -- all of which run before
any device call, so they hold on a machine without a GPU.  The licence of tests/test_gpu_eels.py."""
import os
import re

import numpy as np
import pytest

import eels_cases as ec
import eels_oracle as eo
from mtflearn_amd import _native, eels, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EELS_SYMBOLS = ["zk_eels_snip", "zk_eels_snip_dev", "zk_eels_pls", "zk_eels_pls_dev", "zk_eels_set_chunk"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "eels_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", list(ec.CONFIGS))
def test_oracle_meets_the_goldens(golden, name):
    """The statement reproduces the reference within the recorded distance (it is where that distance came from), and its
    iteration counts are the stored ones.  SNIP in float64 is NumPy on both sides: equal."""
    method, kw, lmin = ec.CONFIGS[name]
    for L, grid in ec.SHAPES:
        if L < lmin or L * int(np.prod(grid)) > 4500:      # the larger batches are the maker's job (seconds each here)
            continue
        key = f"{name}/{ec.shape_id(L, grid)}"
        cube = ec.cube(L, grid)
        base, iters, *_ = eo.over_axis(eo.METHODS[method], cube, 0, **kw)
        dist = np.abs(base - golden[f"{key}/ref"]).max() / np.abs(cube).max()
        assert dist <= float(golden[f"{key}/ref_vs_oracle"]) * (1 + 1e-12) + 0.0, key
        np.testing.assert_array_equal(iters, golden[f"{key}/iters"])
        if method == "snip":
            np.testing.assert_array_equal(base, golden[f"{key}/ref"])


def test_golden_cases_are_meaningful(golden):
    varied = False
    for key, name, L, grid in ec.cases():
        method = ec.CONFIGS[name][0]
        assert golden[f"{key}/ref"].shape == (L,) + tuple(grid) and golden[f"{key}/iters"].shape == tuple(grid)
        assert golden[f"{key}/ref"].dtype == np.float64 and golden[f"{key}/iters"].dtype == np.int32
        assert float(golden[f"{key}/ref_vs_oracle"]) <= 1e-8, key
        if method == "airpls":
            assert (golden[f"{key}/iters"] < 100).all(), key
        if method == "arpls":
            varied |= len(np.unique(golden[f"{key}/iters"])) > 1
        if method == "als":
            assert float(golden[f"{key}/als_gap"]) >= 1e-9, key
    assert varied
    assert {L for L, _ in ec.SHAPES} == {3, 5, 7, 33, 64, 257}
    assert {g for _, g in ec.SHAPES} == {(1,), (63,), (64,), (65,), (130,), (5, 13)}


def test_case_inputs_are_exact_in_every_tested_dtype():
    for L, grid in ec.SHAPES:
        cube = ec.cube(L, grid)
        for dtype in ec.DTYPES:
            np.testing.assert_array_equal(cube.astype(dtype).astype(np.float64), cube)


def test_backward_error_statement_on_the_host_solver():
    """The criterion of the GPU test, applied to LAPACK's band Cholesky: far inside 1e-14."""
    rng = np.random.RandomState(0)
    for k in (1, 2, 3):
        x = ec.spectra(33, 1, 5)[:, 0]
        w = rng.uniform(0.05, 1.0, 33)
        assert eo.backward_error(x, w, 1e4, k, eo.whittaker(x, w, 1e4, k)) <= 1e-14


def test_eels_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = _native.load()
    for sym in EELS_SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    for mode in ("WHITTAKER", "ALS", "ARPLS", "AIRPLS"):
        assert re.search(rf"#define ZK_EELS_{mode}\s+{getattr(_native, 'EELS_' + mode)}\b", header)
    from mtflearn_amd import distributed, resident
    assert callable(resident.baseline_device) and distributed.baseline_device is resident.baseline_device
    assert set(eels.__all__) == {"baseline_als", "baseline_snip", "baseline_arpls", "baseline_airpls", "WhittakerSmooth", "remove_baseline",
                                 "set_scratch_bytes"}
    assert "baseline_correction" in features.__all__
    import mtflearn_amd
    assert "mtflearn_amd.eels" in mtflearn_amd.__doc__


def test_every_refusal_comes_before_any_device_call():
    """Each bad argument is a ValueError although no device may be present (a device error would be a RuntimeError)."""
    y = ec.spectra(16, 4, 1)
    bad = [
        lambda: eels.baseline_als(y[:2]),                                   # L < 3
        lambda: eels.baseline_arpls(y[:2]),
        lambda: eels.baseline_airpls(y[:1], porder=1),                      # L < porder + 1
        lambda: eels.baseline_airpls(y[:3], porder=3),
        lambda: eels.WhittakerSmooth(y[:2], np.ones(2), 10.0, differences=2),
        lambda: eels.baseline_airpls(y, porder=0),
        lambda: eels.baseline_airpls(y, porder=4),
        lambda: eels.baseline_airpls(y, porder=1.5),
        lambda: eels.WhittakerSmooth(y, np.ones(16), 10.0, differences=4),
        lambda: eels.baseline_als(y, lam=0),
        lambda: eels.baseline_als(y, lam=-1.0),
        lambda: eels.baseline_arpls(y, lam=np.inf),
        lambda: eels.baseline_airpls(y, lam=np.nan),
        lambda: eels.WhittakerSmooth(y, np.ones(16), 0.0),
        lambda: eels.baseline_als(y, p=0.0),
        lambda: eels.baseline_als(y, p=1.0),
        lambda: eels.baseline_als(y, p=np.nan),
        lambda: eels.baseline_als(y, niter=-1),
        lambda: eels.baseline_snip(y, niter=-1),
        lambda: eels.baseline_arpls(y, itermax=0),
        lambda: eels.baseline_airpls(y, itermax=0),
        lambda: eels.WhittakerSmooth(y, np.ones(15), 10.0),                 # w of the wrong shape
        lambda: eels.WhittakerSmooth(y, np.ones((4, 16)), 10.0),
        lambda: eels.baseline_snip(y, axis=2),
        lambda: eels.baseline_snip(np.float64(3.0)),
        lambda: eels.baseline_snip(np.zeros((0, 4))),
        lambda: eels.remove_baseline(y, method="poly"),
        lambda: eels.remove_baseline(y[:2], method="als"),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"refusal {k} did not raise")
    with pytest.raises(TypeError, match="als"):
        eels.remove_baseline(y, method="als", porder=2)
    with pytest.raises(TypeError):
        eels.baseline_snip(y.astype(np.complex128))
    from mtflearn_amd import resident
    fake = _native.DeviceArray((2, 4), np.float64, 0, _base=object(), _ptr=4096)
    with pytest.raises(ValueError):
        resident.baseline_device(fake, "als")
    with pytest.raises(ValueError):
        resident.baseline_device(fake, "snip", axis=3)
    with pytest.raises(ValueError):
        resident.baseline_device(fake, "airpls", porder=7)


def test_good_arguments_fail_loudly_without_a_device():
    y = ec.spectra(16, 4, 1)
    if _native.device_count() > 0:
        assert eels.baseline_snip(y).shape == y.shape       # with a device the same call simply runs
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            eels.baseline_snip(y)
