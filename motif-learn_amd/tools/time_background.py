#!/usr/bin/env python3
"""Times background removal (zk_background_*) against the host computations of the reference's workflow.

Frames: honeycomb_frame(n) plus a ramp (1.5 across x, 0.5 down y), float32, at the parameters
suggest_background_parameters picks for the frame.  For each method: the median of whole calls from a NumPy frame (upload
and download included) and from a resident frame (distributed.remove_background_device on a DeviceArray; every call ends
in a stream synchronise).  Host side, timed once: SciPy's grey_opening and the reference's baseline loop on SciPy; the
rolling ball by the test-local restatement (tests/background_oracle.py; scikit-image is not installed) on a 256 x 256 crop,
scaled to the frame by pixel count and labelled so.  Every device result is checked against its host counterpart (the
rolling ball on the crop and on sampled pixels).

Usage: python motif-learn_amd/tools/time_background.py [--reps 5] [--sizes 2048 4096] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "motif-learn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from scipy import ndimage  # noqa: E402

from mtflearn_amd import _native  # noqa: E402
from mtflearn_amd import background as bg  # noqa: E402
from mtflearn_amd.distributed import remove_background_device  # noqa: E402
from mtflearn_amd.synthetic import honeycomb_frame  # noqa: E402
import background_oracle as bo  # noqa: E402

FP64_PEAK = 78.6e12      # MI355X vector FP64, FLOP/s (spec); one add and one min per tap counted as 2 FLOP
CROP = 256


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def once_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def ramped(n):
    frame = honeycomb_frame(n, n, seed=n).astype(np.float64)
    yy, xx = np.mgrid[0:n, 0:n]
    return (frame + 1.5 * xx / n + 0.5 * yy / n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert _native.device_count() > 0, "time_background.py needs a HIP device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("background removal timing: medians of %d whole calls after 2 warm-ups; host side timed once" % a.reps)
    say("%-11s %-13s %9s %11s %11s %13s %9s  %s" % ("frame", "method", "param", "numpy ms", "resident ms", "host ms",
                                                   "host/res", "host side"))
    for n in a.sizes:
        frame = ramped(n)
        params = bg.suggest_background_parameters(frame)
        dev = _native.DeviceArray.from_numpy(frame)
        for method, key in (("opening", "opening_size"), ("baseline", "baseline_sigma"), ("rolling_ball", "rolling_ball_radius")):
            p = params[key]
            if method == "opening":
                host_fn = lambda: bg.remove_background_opening(frame, p)  # noqa: E731
            elif method == "baseline":
                host_fn = lambda: bg.remove_background_baseline(frame, p)  # noqa: E731
            else:
                host_fn = lambda: bg.remove_background_rolling_ball(frame, p)  # noqa: E731
            t_np = median_ms(host_fn, a.reps)
            t_res = median_ms(lambda: remove_background_device(dev, method, p), a.reps)
            _, got = host_fn()
            if method == "opening":
                t_host, want = once_ms(lambda: ndimage.grey_opening(frame, size=(p, p)))
                assert np.array_equal(got, want)
                label = "scipy grey_opening"
            elif method == "baseline":
                if n <= 2048:
                    t_host, want = once_ms(lambda: bo.baseline(frame, p, 10, gauss=ndimage.gaussian_filter))
                    assert np.array_equal(got, want)
                    label = "reference loop on scipy"
                else:                              # one round timed, scaled to the 10 rounds
                    t_round, want = once_ms(lambda: bo.baseline(frame, p, 1, gauss=ndimage.gaussian_filter))
                    assert np.array_equal(bg.estimate_background_baseline(frame, p, 1), want)
                    t_host = 10 * t_round
                    label = "reference loop on scipy, 1 round x 10 (scaled)"
            else:
                crop = frame[:CROP, :CROP]
                t_crop, want = once_ms(lambda: bo.rolling_ball(crop, p))
                assert np.array_equal(bg.estimate_background_rolling_ball(crop, p), want)
                rng = np.random.default_rng(n)
                pts = rng.integers(0, n, (64, 2))
                assert np.array_equal(got[pts[:, 0], pts[:, 1]], bo.rolling_ball_at(frame, p, pts))
                t_host = t_crop * (n * n) / (CROP * CROP)
                label = "restatement on %d^2 crop x %d (scaled)" % (CROP, (n * n) // (CROP * CROP))
            say("%-11s %-13s %9s %11.3f %11.3f %13.1f %8.0fx  %s" % ("%d^2 f32" % n, method, p, t_np, t_res, t_host,
                                                                    t_host / t_res, label))
            if method == "rolling_ball":
                taps = int(np.isfinite(bo.ball_diff(p)).sum()) * n * n
                # float32 frame: float32 arithmetic; the float64 rate comes from a float64 copy
                dev64 = _native.DeviceArray.from_numpy(frame.astype(np.float64))
                t64 = median_ms(lambda: remove_background_device(dev64, method, p), a.reps)
                say("%-11s %-13s %9s %11s %11.3f   %.3g taps: %.2f Ttap/s f32, %.2f Ttap/s f64 = %.1f %% of the FP64 "
                    "vector peak (2 FLOP per tap, 78.6 TFLOP/s spec, whole call)"
                    % ("%d^2 f64" % n, method, p, "", t64, taps, taps / t_res / 1e9, taps / t64 / 1e9,
                       100.0 * 2 * taps / (t64 * 1e-3) / FP64_PEAK))
        say("  %d^2 parameters: %s" % (n, params))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
