"""Writes tests/golden/gauss_fit.npz: for every parity case of tests/gauss_fit_cases.py the result of the NumPy oracle
(tests/gauss_fit_oracle.py) and SciPy's converged minimiser started from it, and for the recovery cases the error the oracle
itself shows against the known truth.  Run on the CPU: ``python tests/make_golden_gauss_fit.py``.

Every point of every parity case must end with status 0 in the oracle (asserted).  ``d0`` is the largest distance
``|oracle - scipy| / (|scipy| + 1)`` over the compared columns ``x, y, A, a, b, c, g, rss`` of all cases; the GPU tests hold the
device to ``max(100 * d0, 1e-12)`` against SciPy's minimisers in the same measure."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauss_fit_cases as gc          # noqa: E402
import gauss_fit_oracle as go         # noqa: E402


def compared(params):
    """Library columns (x, y, A, sigma_major, sigma_minor, theta, g, rss) -> (x, y, A, a, b, c, g, rss): the precision-matrix form
    is well conditioned where the column is round, the angle is not."""
    a, b, c = gc.precision(params[:, 3], params[:, 4], params[:, 5])
    return np.stack([params[:, 0], params[:, 1], params[:, 2], a, b, c, params[:, 6], params[:, 7]], axis=1)


def scipy_minimiser(window, model, mode, p):
    from scipy.optimize import least_squares
    size = window.shape[0]
    keep = go.fitted_mask(size, mode)
    row, col = (v[keep].astype(np.float64) for v in np.mgrid[:size, :size])
    values = window[keep]
    fit = least_squares(lambda q: go.model_and_jacobian(q, model, col, row)[0] - values, p,
                        jac=lambda q: go.model_and_jacobian(q, model, col, row)[1], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return fit.x, float(fit.fun @ fit.fun)


def build():
    out, d0, most = {}, 0.0, 0
    for name, (frame, pts, size, model, mode) in gc.parity_cases().items():
        params, its, status, raw = go.fit_points(pts, frame, size, model, mode)
        assert (status == go.CONVERGED).all(), (name, status)
        first = go.corners(pts, size)
        want = np.empty((len(pts), 8))
        for k, w in enumerate(go.windows(frame, pts, size)):
            q, rss = scipy_minimiser(w, model, mode, raw[k])
            A, x0, y0, a, b, c, g = go.unpack(q, model)
            want[k] = (first[k, 0] + x0, first[k, 1] + y0, A, a, b, c, g, rss)
        d0 = max(d0, gc.scaled_distance(compared(params), want))
        most = max(most, int(its.max()))
        out[f"{name}/oracle"], out[f"{name}/iterations"], out[f"{name}/scipy"] = params, its, want
    out["d0"], out["most_iterations"] = np.float64(d0), np.int32(most)
    for model in gc.MODELS:
        frame, pts, truth = gc.recovery_case(model)
        params, _, status, _ = go.fit_points(pts, frame, gc.RECOVERY_SIZE, model)
        assert (status == go.CONVERGED).all(), (model, status)
        out[f"recovery/{model}/oracle_error"] = np.float64(gc.recovery_error(params, truth))
    return out


if __name__ == "__main__":
    made = build()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gauss_fit.npz")
    np.savez_compressed(path, **made)
    print(f"{path}: {len(made)} arrays, {os.path.getsize(path)} bytes, d0 = {made['d0']:.3g}, most iterations {made['most_iterations']}, "
          + ", ".join(f"{m} recovery error {made[f'recovery/{m}/oracle_error']:.3g}" for m in gc.MODELS))
