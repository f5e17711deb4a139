#!/usr/bin/env python3
"""Times local_max (zk_local_max / zk_local_max_dev) against the host restatement of the reference's workflow.

Frames: honeycomb_frame(n) + 10 % Gaussian noise (float32).  For each size and min_distance: the median of whole calls
from a NumPy frame (upload included) and from a resident frame (local_max_device on a DeviceArray), and the host
restatement (tests/local_max_oracle.py: scipy 3 x 3 maxima + the greedy loop over a cKDTree, one thread) timed once.
Then the 509-peak ramp: time and suppression launches.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats -- python tools/time_local_max.py --quick`` run.

Usage: python motif-learn_amd/tools/time_local_max.py [--reps 20] [--quick] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "motif-learn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from mtflearn_amd import _native  # noqa: E402
from mtflearn_amd.distributed import local_max_device  # noqa: E402
from mtflearn_amd.features import local_max  # noqa: E402
from mtflearn_amd.synthetic import honeycomb_frame  # noqa: E402
import local_max_oracle as lmo  # noqa: E402


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="2048^2 at r=5 and the ramp only, 5 repetitions, no host timing")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    lib = _native.load()
    sizes, radii, reps = ((2048,), (5.0,), 5) if a.quick else ((512, 2048, 4096), (3.0, 5.0, 8.0), a.reps)
    emit(f"local_max timing: whole-call medians of {reps} calls after 3 warm-up calls; host restatement timed once")
    emit(f"{'frame':>10s} {'r':>4s} {'cand':>8s} {'kept':>7s} {'launches':>8s} {'numpy ms':>9s} {'resident ms':>11s} "
         f"{'host ms':>9s} {'host/resident':>13s}")
    for n in sizes:
        rng = np.random.default_rng(n)
        frame = honeycomb_frame(n, seed=7) + np.float32(0.1) * rng.standard_normal((n, n), dtype=np.float32)
        dev = _native.DeviceArray.from_numpy(frame)
        n_cand = int(lmo.candidate_mask(frame).sum())
        for r in radii:
            pts = local_max(frame, r)
            launches = lib.zk_local_max_last_launches()
            t_np = median_ms(lambda: local_max(frame, r), reps)
            t_dev = median_ms(lambda: local_max_device(dev, r), reps)
            if a.quick:
                t_host = float("nan")
            else:
                t0 = time.perf_counter()
                host = lmo.local_max_raster(frame, r)
                t_host = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(host, pts), "device and host restatement disagree"
            emit(f"{n:>5d}^2 f32 {r:4.1f} {n_cand:8d} {len(pts):7d} {launches:8d} {t_np:9.3f} {t_dev:11.3f} {t_host:9.1f} "
                 f"{t_host / t_dev:12.0f}x")
        dev.close()
    ramp = np.zeros((3, 2 * 509 + 3))
    ramp[1, 1:2 * 509:2] = np.arange(1, 510, dtype=np.float64)
    got = local_max(ramp, 3.0)
    launches = lib.zk_local_max_last_launches()
    dev = _native.DeviceArray.from_numpy(ramp)
    t_dev = median_ms(lambda: local_max_device(dev, 3.0), reps)
    t0 = time.perf_counter()
    host = lmo.local_max_raster(ramp, 3.0)
    t_host = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(host, got)
    emit(f"ramp (509 rising peaks 2 px apart, r=3): kept {len(got)}, {launches} suppression launches, "
         f"resident {t_dev:.3f} ms, host restatement {t_host:.1f} ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
