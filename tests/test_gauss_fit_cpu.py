"""What can be said about the Gaussian fit without a GPU: every argument refusal comes before the library is even loaded, the
two entry points are declared, built and bound, the NumPy oracle of tests/gauss_fit_oracle.py reaches SciPy's converged
minimisers stored in tests/golden/gauss_fit.npz within the stored ``d0``, and the header's (a, b, c) -> (sigma, theta) formulas
are ``numpy.linalg.eigh``'s."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gauss_fit_cases as gc
import gauss_fit_oracle as go
import make_golden_gauss_fit as mg
from conftest import ROOT


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "gauss_fit.npz")) as f:
        return {k: f[k] for k in f.files}


REFUSALS = '''
import numpy as np, pytest
from mtflearn_amd import _native, features
from mtflearn_amd.features import KeyPoints, GaussianFit
data = np.zeros((32, 40), np.float32)
ok = np.array([[10.0, 12.0]])
fit = features.gaussian_fit_points
for frame, pts, size, kw, what in (
        (data.astype(np.int32), ok, 7, {}, "float32 or float64"), (data.astype(np.float16), ok, 7, {}, "float32 or float64"),
        (data[None], ok, 7, {}, "2-D"), (data, np.array([10.0, 12.0, 3.0]), 7, {}, r"\\(N, 2\\)"),
        (data, np.array([[1 + 2j, 3]]), 7, {}, "real points"), (data, ok, 2, {}, "size"), (data, ok, 33, {}, "size"),
        (data, ok, 7.5, {}, "size"), (data, np.array([[np.nan, 12.0]]), 7, {}, "finite"), (data, np.array([[np.inf, 12.0]]), 7, {}, "finite"),
        (data, ok, 7, {"model": "round"}, "model"), (data, ok, 7, {"mode": "ring"}, "mode"), (data, ok, 8, {"mode": "disk"}, "odd size"),
        (data, ok, 3, {"mode": "disk"}, "fitted pixels"), (data, ok, 3, {"mode": "disk", "model": "circular"}, "fitted pixels"),
        (data, ok, 7, {"sigma": 0.0}, "sigma"), (data, ok, 7, {"sigma": np.nan}, "sigma"), (data, ok, 7, {"tol": -1.0}, "tol"),
        (data, ok, 7, {"tol": np.inf}, "tol"), (data, ok, 7, {"max_iter": 0}, "max_iter"), (data, ok, 7, {"max_iter": 2.5}, "max_iter"),
        (data, ok, 7, {"max_iter": 10001}, "max_iter"),
        (data, np.array([[2.0, 12.0]]), 7, {"clear": False}, "inside the frame"), (data, np.array([[10.0, 29.0]]), 7, {"clear": False}, "inside the frame"),
        (data, np.array([[37.0, 12.0]]), 7, {"clear": False}, "inside the frame")):
    with pytest.raises(ValueError, match=what):
        fit(pts, frame, size, **kw)
with pytest.raises(ValueError, match="2\\\\^24"):
    fit(np.broadcast_to(np.array([[4, 4]], np.int32), (2 ** 24, 2)), data, 3)
for pts in (np.empty((0, 2)), [], np.array([[1, 1], [39, 31]])):                      # empty, or all cleared
    for model in ("circular", "elliptical"):
        got = fit(pts, data, 5, model=model)
        assert isinstance(got, GaussianFit) and got._fields == ("xy", "amplitude", "sigma", "theta", "background", "rss", "iterations",
                                                                 "status", "kept")
        assert got.xy.shape == (0, 2) and got.sigma.shape == (0, 2) and got.amplitude.shape == got.theta.shape == got.rss.shape == (0,)
        assert got.xy.dtype == np.float64 and got.iterations.dtype == got.status.dtype == np.int32 and got.kept.dtype == np.int64
assert fit(np.empty((0, 2)), data, 3, mode=None).xy.shape == (0, 2)                   # 9 pixels against 7 parameters: allowed
kp = KeyPoints(np.array([[1, 1]]), data, 7)
assert kp.fit_gaussians().xy.shape == (0, 2) and kp.fit_gaussians(size=5, model="circular").kept.shape == (0,) and len(kp.pts) == 0
assert _native._lib is None, "an argument check loaded the library"
print("refusals ok")
'''


def test_every_refusal_precedes_the_first_device_call():
    """In a fresh interpreter: each refused argument is a ValueError naming it, empty input gives empty arrays, and
    ``_native._lib`` is still unloaded afterwards."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "motif-learn_amd"), os.environ.get("PYTHONPATH", "")]))
    done = subprocess.run([sys.executable, "-c", REFUSALS], env=env, capture_output=True, text=True)
    assert done.returncode == 0 and "refusals ok" in done.stdout, done.stdout + done.stderr


def test_the_entry_points_are_declared_listed_bound_and_exported():
    import ctypes
    from mtflearn_amd import _native, features, resident
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_native.LIB_PATH)
    for sym in ("zk_gauss_fit", "zk_gauss_fit_points_dev"):
        decl = re.search(rf"\bint {sym}\(([^;]*)\);", header)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    for name, value in (("CIRCULAR", 0), ("ELLIPTICAL", 1), ("BOX", 0), ("DISK", 1), ("CONVERGED", 0), ("MAX_ITER", 1), ("STALLED", 2),
                        ("NOT_FINITE", 3)):
        assert re.search(rf"#define ZK_GAUSS_{name}\s+{value}\b", header) and getattr(_native, f"GAUSS_{name}") == value, name
    assert (go.CONVERGED, go.MAX_ITER, go.STALLED, go.NOT_FINITE) == (0, 1, 2, 3)
    makefile = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bzk_gauss_fit\.hip\b", makefile, flags=re.M)
    assert "gaussian_fit_points" in features.__all__ and features.gaussian_fit_points is features.keypoints.gaussian_fit_points
    assert "gaussian_fit_device" not in resident.__all__ and callable(resident.gaussian_fit_device)
    assert "resident.gaussian_fit_device" in resident.gaussian_fit_device.__doc__
    assert lib.zk_abi_version() == 2


def test_the_generator_reproduces_the_golden_file(golden):
    fresh = mg.build()
    assert sorted(fresh) == sorted(golden)
    for key, value in fresh.items():
        assert golden[key].dtype == value.dtype and np.array_equal(golden[key], value), key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gauss_fit.npz")) < 2 ** 18


def test_the_oracle_reaches_scipys_minimisers_within_d0(golden):
    """Every point of every parity case converges (status 0, within max_iter = 100) and lies within the stored ``d0`` of the
    stored SciPy minimiser; ``d0`` sits above ``tol`` = 1e-10 as the last step bounds the distance only up to the linear
    convergence factor under noise, and far below anything a user would see."""
    d0 = float(golden["d0"])
    assert 0 < d0 < 1e-7 and int(golden["most_iterations"]) <= 100
    names = tuple(gc.parity_cases())
    assert len(names) == 36
    worst = 0.0
    for name, (frame, pts, size, model, mode) in gc.parity_cases().items():
        params, its, status, _ = go.fit_points(pts, frame, size, model, mode)
        assert (status == go.CONVERGED).all() and len(pts) == 16, name
        worst = max(worst, gc.scaled_distance(mg.compared(params), golden[f"{name}/scipy"]))
    assert worst <= d0
    assert {c[0].dtype.name for c in gc.parity_cases().values()} == {"float32", "float64"}


def test_recovery_cases_hold_what_they_say(golden):
    for model in gc.MODELS:
        frame, pts, truth = gc.recovery_case(model)
        first = go.corners(pts, gc.RECOVERY_SIZE)
        assert first.min() >= 0 and (first + gc.RECOVERY_SIZE).max() <= 64
        assert np.abs(truth[:, :2] - pts).max() <= 0.4 and float(golden[f"recovery/{model}/oracle_error"]) < 1e-12
    thetas = gc.recovery_case("elliptical")[2][:, 5]
    assert (np.abs(thetas) < 0.05).sum() >= 2 and (np.abs(np.abs(thetas) - np.pi / 2) < 0.05).sum() == 2 and (np.abs(thetas) == np.pi / 4).sum() == 2


def test_sigma_and_theta_are_the_eigen_decomposition():
    rng = np.random.default_rng(3)
    for _ in range(200):
        s1, s2 = np.sort(rng.uniform(0.5, 6.0, 2))[::-1]
        theta = rng.uniform(-np.pi / 2, np.pi / 2)
        a, b, c = gc.precision(s1, s2, theta)
        major, minor, angle = go.shape_of(a, b, c)
        values, vectors = np.linalg.eigh(np.array([[a, b], [b, c]]))
        assert abs(major - 1 / np.sqrt(values[0])) <= 1e-12 * major and abs(minor - 1 / np.sqrt(values[1])) <= 1e-12 * minor
        axis = vectors[:, 0]                                                             # the major axis: the smallest eigenvalue
        assert abs(abs(axis @ np.array([np.cos(angle), np.sin(angle)])) - 1) <= 1e-9
        assert abs(major - s1) <= 1e-12 * s1 and abs(minor - s2) <= 1e-12 * s2 and -np.pi / 2 < angle <= np.pi / 2
        assert abs(angle - theta) <= 1e-9 / (s1 - s2 + 1e-3) or abs(abs(angle - theta) - np.pi) <= 1e-9 / (s1 - s2 + 1e-3)
    assert go.shape_of(0.25, 0.0, 1.0) == (2.0, 1.0, 0.0)                                # major axis along x
    major, minor, angle = go.shape_of(1.0, 0.0, 0.25)                                    # along y: +pi/2, never -pi/2
    assert (major, minor) == (2.0, 1.0) and angle == np.pi / 2
    assert go.shape_of(0.5, 0.0, 0.5)[2] == 0.0                                          # round: the angle is 0
