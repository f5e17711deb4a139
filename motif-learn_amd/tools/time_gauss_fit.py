#!/usr/bin/env python3
"""Times of ``features.gaussian_fit_points`` (NumPy to NumPy, whole call) and ``resident.gaussian_fit_device`` (resident) for
10^3, 10^4 and 10^5 key points at window sizes 7, 11 and 21, both models, on a 2048 x 2048 float32 frame, beside the NumPy oracle
of tests/gauss_fit_oracle.py and a ``scipy.optimize.least_squares`` loop on a sample of the same points on the host (one thread
each, scaled to the point count).

The frame of a window size is a square lattice of equal Gaussians of pitch ``size + 1`` (sigma ``size / 5``, amplitude 1,
background 0.1, one sub-pixel offset) plus Gaussian noise of 0.02, so every window holds one column; the key points are its
integer sites, repeated in order up to the point count.  Resident times are HIP-event times around ``--reps`` calls on the
current stream, each call ending in the library's own stream synchronise (the error flag), divided by the count; whole-call times
are the host clock around a call that ends in a device synchronise.  Medians after one warm-up.  Not kernel times: the resident
call holds one fill, one kernel and one 4-byte read-back.

The FP64 rate is counted from the source, not from counters: an evaluation costs 100 (elliptical) or 62 (circular) float64
additions and multiplications a fitted pixel with ``exp`` counted as ONE operation, a fit makes ``iterations + 1`` evaluations at
most (a trial that is not admissible skips its own), so the figure is an upper bound of that count over the resident time, against
the 78.6 TFLOP/s FP64 vector peak DESIGN.md quotes.  It is a whole-call rate, not the kernel's share of peak.

Every window size is a process of its own under its own ``timeout``; the first one that fails ends the run.

Usage:  python motif-learn_amd/tools/time_gauss_fit.py [--sizes 7 11 21] [--counts 1000 10000 100000] [--reps 10] [--no-host] [--out FILE]
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

FRAME = 2048
OPS = {"elliptical": 100, "circular": 62}
PEAK = 78.6e12
HOST_SAMPLE = 200


def inputs(size):
    """``(frame float32 (2048, 2048), sites int32 (N, 2))``."""
    pitch = size + 1
    yy, xx = np.mgrid[:pitch, :pitch].astype(np.float64)
    cx, cy, s = pitch // 2 + 0.3, pitch // 2 - 0.2, size / 5
    tile = 0.1 + np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    reps = FRAME // pitch + 1
    frame = np.tile(tile, (reps, reps))[:FRAME, :FRAME] + np.random.default_rng(size).normal(0, 0.02, (FRAME, FRAME))
    k = np.arange(1, FRAME // pitch - 1)
    sites = np.array([(pitch * i + pitch // 2, pitch * j + pitch // 2) for j in k for i in k], dtype=np.int32)
    return frame.astype(np.float32), sites


def event_ms(call, reps):
    import torch
    call()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        end.record()
        end.synchronize()
        times.append(start.elapsed_time(end))
    return float(np.median(times)), min(times)


def step(size, counts, reps, host):
    import torch
    from mtflearn_amd import features, resident
    from time_refine import median_ms
    frame, sites = inputs(size)
    d_frame = torch.from_numpy(frame).cuda()
    lines = []
    for model in ("elliptical", "circular"):
        for n in counts:
            pts = np.ascontiguousarray(sites[np.arange(n) % len(sites)])
            d_pts = torch.from_numpy(pts).cuda()
            fit = features.gaussian_fit_points(pts, frame, size, model=model, clear=False)
            np_ms, np_min = median_ms(lambda: features.gaussian_fit_points(pts, frame, size, model=model, clear=False), reps, torch.cuda.synchronize)
            dev_ms, dev_min = event_ms(lambda: resident.gaussian_fit_device(d_frame, d_pts, size, model=model), reps)
            ops = float((fit.iterations.astype(np.float64) + 1).sum()) * size * size * OPS[model]
            line = (f"size {size:2d} {model:10s} {n:6d} points ({len(sites)} sites): gaussian_fit_points NumPy to NumPy {np_ms:8.2f} ms (min {np_min:.2f}, "
                    f"host clock) | gaussian_fit_device resident {dev_ms:8.3f} ms (min {dev_min:.3f}, HIP events) | status 0: {int((fit.status == 0).sum())}, "
                    f"iterations {fit.iterations.min()} .. {fit.iterations.max()}, mean {fit.iterations.mean():.1f} | at most {ops / 1e9:.2f} GFLOP counted: "
                    f"{ops / (dev_ms * 1e-3) / 1e12:.2f} TFLOP/s = {ops / (dev_ms * 1e-3) / PEAK:.3f} of the FP64 vector peak")
            if host and n == counts[0]:
                import gauss_fit_oracle as go
                import make_golden_gauss_fit as mg
                sample = pts[:HOST_SAMPLE]
                t0 = time.perf_counter()
                want = go.fit_points(sample, frame, size, model)[0]
                oracle_s = time.perf_counter() - t0
                windows = go.windows(frame, sample, size)
                t0 = time.perf_counter()
                for w in windows:                                                # SciPy from the fit's own start
                    p0 = [w.max() - w.min(), size // 2, size // 2, 16 / size ** 2] + ([0.0, 16 / size ** 2] if model == "elliptical" else []) + [w.min()]
                    mg.scipy_minimiser(w, model, None, np.array(p0, dtype=np.float64))
                scipy_s = time.perf_counter() - t0
                table = np.column_stack([fit.xy, fit.amplitude, fit.sigma, fit.theta, fit.background, fit.rss])[:len(sample)]
                line += (f" | host, one thread, {len(sample)} points: NumPy oracle {1e3 * oracle_s / len(sample):.2f} ms a point, SciPy least_squares(lm) "
                         f"{1e3 * scipy_s / len(sample):.2f} ms a point; device against the oracle {np.abs(table[:, :2] - want[:, :2]).max():.2e} px")
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[7, 11, 21])
    ap.add_argument("--counts", type=int, nargs="*", default=[1000, 10000, 100000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step-size", type=int, default=None, help="run one window size in this process (what the driver starts under timeout)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step_size:
        for line in step(args.step_size, args.counts, args.reps, not args.no_host):
            print("RESULT " + line, flush=True)
        return 0
    lines = [f"gaussian_fit_points / gaussian_fit_device on a {FRAME} x {FRAME} float32 frame, median of {args.reps} after one warm-up; whole calls by the "
             "host clock around a call ending in a device synchronise, resident calls by HIP events around the call (which ends in the library's "
             "stream synchronise); profiler off; tol 1e-10, max_iter 100, the box; every window size a process of its own.  Not kernel times."]
    status = 0
    for size in args.sizes:
        cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step-size", str(size), "--reps", str(args.reps),
               "--counts"] + [str(c) for c in args.counts] + (["--no-host"] if args.no_host else [])
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
