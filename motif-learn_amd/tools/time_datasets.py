#!/usr/bin/env python3
"""Times HoneyCombLattice.to_image (zk_render_gaussians_dev) against the host statements of the same frame.

For each size (l = 12, sigma = 3): the median of whole calls that return a NumPy frame (``to_image``: coordinates on the host,
render, download) and of whole calls that leave the frame resident (``honeycomb_image_device`` followed by a device
synchronise); the lattice coordinates are cached by the lattice object after the first call, as in the reference.  Then, on
the same host: tests/datasets_oracle.py's NumPy statement of the gather, timed once on a SMALLER frame whose size is printed
(it evaluates the whole frame per point and is not scaled to the larger sizes), and ``synthetic.honeycomb_frame(noise=False)``,
the project's older host generator, at the full size.

Usage: python motif-learn_amd/tools/time_datasets.py [--reps 20] [--sizes 2048 4096] [--oracle-size 256] [--out FILE]
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
from mtflearn_amd.datasets import HoneyCombLattice  # noqa: E402
from mtflearn_amd.distributed import honeycomb_image_device  # noqa: E402
from mtflearn_amd.synthetic import honeycomb_frame  # noqa: E402
import datasets_oracle  # noqa: E402


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--oracle-size", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    lib = _native.load()
    device = _native.default_device()

    def resident(lat):
        honeycomb_image_device(lat)
        _native.check(lib.zk_device_synchronize(device), "zk_device_synchronize")

    emit(f"datasets timing: HoneyCombLattice(l=12).to_image(), float32, whole-call medians of {a.reps} calls after 3 warm-up calls, "
         "each ending in a synchronise; host statements timed once")
    emit(f"{'frame':>8s} {'points':>8s} {'numpy-out ms':>12s} {'resident ms':>11s} {'synthetic.honeycomb_frame ms':>28s}")
    for n in a.sizes:
        lat = HoneyCombLattice(size=n, l=12, seed=0)
        n_pts = len(lat._render_lists(None, 1.0, 0.5)[1])
        t_np = median_ms(lambda: lat.to_image(), a.reps)
        t_dev = median_ms(lambda: resident(lat), a.reps)
        t0 = time.perf_counter()
        honeycomb_frame(n, n, l=12.0, seed=0, noise=False)
        t_syn = (time.perf_counter() - t0) * 1e3
        emit(f"{n:>6d}^2 {n_pts:8d} {t_np:12.3f} {t_dev:11.3f} {t_syn:28.1f}")
    m = a.oracle_size
    lat = HoneyCombLattice(size=m, l=12, seed=0)
    sigma, pts, amps = lat._render_lists(None, 1.0, 0.5)
    t0 = time.perf_counter()
    ref, k = datasets_oracle.render(np.zeros((m, m), np.float32), pts, amps, sigma, 3.0)
    t_oracle = (time.perf_counter() - t0) * 1e3
    got = lat.to_image()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    emit(f"NumPy statement of the gather (tests/datasets_oracle.py) at {m}^2, {len(pts)} points: {t_oracle:.1f} ms on this host; "
         f"device against it: max|delta| {err:.3e} (bound {datasets_oracle.tolerance(ref, k):.3e}, k = {k})")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
