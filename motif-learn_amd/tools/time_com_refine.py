#!/usr/bin/env python3
"""Whole-call times of ``features.com_refine_points`` (NumPy to NumPy) and ``distributed.com_refine_device`` (resident) on the key
points of honeycomb lattices (bond length 12 px, the point sets of tools/time_refine.py) at window sizes 9 and 24, Li and Otsu,
beside the host statement on the same input and the same machine.  scikit-image is not installed where this runs, so the host
statement is the route of tests/make_golden_com_refine.py (the reference's per-window loop with the thresholds of
tests/thresholds_reference.py and ``scipy.ndimage.center_of_mass``), run once.  Medians of ``--reps`` whole calls, each ending in
a device synchronise, after one warm-up.  Not kernel times.

Every size is a process of its own under its own ``timeout``; the first one that fails ends the run.

Usage:  python motif-learn_amd/tools/time_com_refine.py [--sizes 2048 4096] [--reps 20] [--no-host] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "tests"), HERE):
    sys.path.insert(0, os.path.abspath(p))

WINDOWS = (9, 24)


def step(size, reps, host):
    import torch
    from mtflearn_amd import distributed, features
    from mtflearn_amd.features.keypoints import clear_border
    from time_refine import inputs, median_ms
    frame, keep, _ = inputs(size)
    d_frame = torch.from_numpy(frame).cuda()
    lines = []
    for window in WINDOWS:
        pts = np.ascontiguousarray(clear_border(keep, frame.shape, window))
        d_pts = torch.from_numpy(pts).cuda()
        for rule in (None, "otsu"):
            xy, _, it = features.com_refine_points(pts, frame, window, rule, return_thresholds=True)
            np_ms, np_min = median_ms(lambda: features.com_refine_points(pts, frame, window, rule), reps, torch.cuda.synchronize)
            dev_ms, dev_min = median_ms(lambda: distributed.com_refine_device(d_frame, d_pts, window, rule), reps, torch.cuda.synchronize)
            line = (f"size {size:5d} window {window:2d} {rule or 'li':4s}: {len(pts):6d} points | com_refine_points NumPy to NumPy {np_ms:8.2f} ms "
                    f"(min {np_min:.2f}) | com_refine_device resident {dev_ms:7.3f} ms (min {dev_min:.3f}) | Li iterations {it.min()} .. {it.max()}, "
                    f"mean {it.mean():.1f}")
            if host:
                import make_golden_com_refine as mg
                import warnings
                t0 = time.perf_counter()
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    want = mg.build_case(frame, pts, window, rule or "li")
                line += (f" | host statement {1e3 * (time.perf_counter() - t0):9.1f} ms | largest difference of the points "
                         f"{np.nanmax(np.abs(xy - want[0])):.2e} px, iteration counts equal: {np.array_equal(it, want[2])}")
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step-size", type=int, default=None, help="run one size in this process (what the driver starts under timeout)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step_size:
        for line in step(args.step_size, args.reps, not args.no_host):
            print("RESULT " + line, flush=True)
        return 0
    lines = [f"com_refine_points / com_refine_device, whole calls, median of {args.reps} after one warm-up, each ending in a device synchronise; "
             "host clock; profiler off; key points of a jittered honeycomb, l = 12, on a frame of uniform noise (float32); every size a process "
             "of its own.  Not kernel times."]
    status = 0
    for size in args.sizes:
        cmd = ["timeout", "-k", "10", "560", sys.executable, os.path.abspath(__file__), "--step-size", str(size), "--reps", str(args.reps)] + \
              (["--no-host"] if args.no_host else [])
        run = subprocess.run(cmd, capture_output=True, text=True)
        got = [l[7:] for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        lines += got
        print("\n".join(got), flush=True)
        if run.returncode != 0:                                          # a failure ends the run: nothing more is started on the GPU
            lines.append(f"size {size} ended with status {run.returncode}; the run stops here\n{run.stderr[-2000:]}")
            print(lines[-1], flush=True)
            status = 1
            break
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
