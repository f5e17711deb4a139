#!/usr/bin/env python3
"""Whole-call times of ``features.refine_points`` / ``distributed.refine_points_device`` and of ``graph.estimate_d`` on the key
points of honeycomb frames (bond length 12 px, the point sets of tools/time_vnn.py), beside the host routes on the same input
and the same machine: ``KeyPoints.refine`` (the Python paint loop and ``scipy.ndimage.center_of_mass``) and
tests/thresholds_reference.py (scikit-learn's ball tree, ``np.histogram``, ``np.unique``).  Medians of ``--reps`` whole calls,
each ending in a device synchronise, after one warm-up; the host routes run once.  Not kernel times.

Every GPU step is a process of its own under its own ``timeout``; the steps are chained and the first one that fails ends the
run.  With ``--launch-traces SIZE:DB ...`` the kernel dispatches per call and the time of the owner-image pass (the memset and
``paint_kernel``) are read from ``rocprofv3 --kernel-trace`` databases of runs made as ``--step refine_trace --size SIZE`` (two
calls each; tracing is a run of its own, never the timed one).

Usage:  python motif-learn_amd/tools/time_refine.py [--sizes 2048 4096] [--reps 20] [--no-host] [--launch-traces SIZE:DB ...]
                                                    [--out FILE]
        (--sizes with no value: only summarise the traces)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "tests")):
    sys.path.insert(0, os.path.abspath(p))

STEPS = (("refine", 420), ("estimate", 420), ("knn", 180))        # (name, seconds allowed per size)


def inputs(size):
    """``(frame float32 (size, size), key points int32 (N, 2), points float64 (N, 2))``: the jittered honeycomb of
    tests/regions_cases.py, rounded and border-cleared as ``KeyPoints`` does; the frame is noise (only its size matters here)."""
    import regions_cases as rc
    from mtflearn_amd.features.keypoints import clear_border
    pts = rc.honeycomb(size, 12.0, 11)
    keep = clear_border(np.unique(np.rint(pts).astype(np.int32), axis=0), (size, size), 7)
    frame = np.random.default_rng(size).random((size, size), dtype=np.float32)
    return frame, np.ascontiguousarray(keep), pts


def median_ms(call, reps, sync):
    call()
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times)), 1e3 * min(times)


def step_refine(size, reps, host):
    import torch
    from mtflearn_amd import distributed, features
    frame, keep, _ = inputs(size)
    d_frame, d_pts = torch.from_numpy(frame).cuda(), torch.from_numpy(keep).cuda()
    lines = []
    for mode in (None, "disk"):
        np_ms, np_min = median_ms(lambda: features.refine_points(frame, keep, size=3, mode=mode), reps, torch.cuda.synchronize)
        dev_ms, dev_min = median_ms(lambda: distributed.refine_points_device(d_frame, d_pts, size=3, mode=mode), reps, torch.cuda.synchronize)
        line = (f"size {size:5d} r = 3 {'disk' if mode else 'box ':4s}: {len(keep):6d} points | refine_points NumPy to NumPy {np_ms:8.2f} ms "
                f"(min {np_min:.2f}) | refine_points_device resident {dev_ms:7.3f} ms (min {dev_min:.3f})")
        if host:
            kp = features.KeyPoints(keep.astype(np.float64), frame, 7)
            t0 = time.perf_counter()
            try:
                kp.refine(r=3, mode=mode)
                same = np.array_equal(kp.pts, features.refine_points(frame, keep, size=3, mode=mode), equal_nan=True)
                line += f" | host KeyPoints.refine {1e3 * (time.perf_counter() - t0):9.1f} ms | device == host: {same}"
            except OverflowError:
                line += " | host KeyPoints.refine: not measured (its uint8 disk stamp overflows from the 256th point on)"
        lines.append(line)
    return lines


def step_refine_trace(size, reps, host):
    import torch
    from mtflearn_amd import distributed
    frame, keep, _ = inputs(size)
    d_frame, d_pts = torch.from_numpy(frame).cuda(), torch.from_numpy(keep).cuda()
    for _ in range(2):
        distributed.refine_points_device(d_frame, d_pts, size=3)
    torch.cuda.synchronize()
    return [f"size {size}: two traced calls of refine_points_device"]


def step_estimate(size, reps, host):
    import torch
    from mtflearn_amd import distributed
    _, _, pts = inputs(size)
    d_pts = torch.from_numpy(pts).cuda()
    lines = []
    for method in ("otsu", "li"):
        got = distributed.estimate_d_device(d_pts, threshold=method, return_k=True)
        ms, best = median_ms(lambda: distributed.estimate_d_device(d_pts, threshold=method), reps, torch.cuda.synchronize)
        line = f"size {size:5d} {method:4s}: {len(pts):6d} points | estimate_d_device resident {ms:8.2f} ms (min {best:.2f}), t = {got[0]:.6f} at k = {got[1]}"
        if host:
            import thresholds_reference as ref
            t0 = time.perf_counter()
            want = ref.estimate(pts, method)
            line += (f" | host statement {1e3 * (time.perf_counter() - t0):9.1f} ms, t = {want['t']:.6f} at k = {want['k']} | relative difference "
                     f"{abs(got[0] - want['t']) / want['t']:.2e}")
        lines.append(line)
    return lines


def step_knn(size, reps, host):
    import torch
    from ctypes import c_void_p
    from mtflearn_amd import _native
    _, _, pts = inputs(size)
    d_pts = torch.from_numpy(pts).cuda()
    dd = torch.empty((len(pts), 12), dtype=torch.float64, device="cuda")
    lib = _native.load()
    call = lambda: _native.check(lib.zk_knn_distances_dev(0, c_void_p(d_pts.data_ptr()), _native.ZK_F64, len(pts), 12, c_void_p(dd.data_ptr()),
                                                          c_void_p(0)), "zk_knn_distances_dev")
    ms, best = median_ms(call, reps, torch.cuda.synchronize)
    return [f"size {size:5d}: {len(pts):6d} points | zk_knn_distances_dev alone (binning, sort and search; working buffers allocated and freed inside) "
            f"{ms:7.3f} ms (min {best:.3f})"]


def trace_summary(db, calls=2):
    """Dispatches per call and the owner-image pass (fill and ``paint_kernel``) against ``centroid_kernel`` in a rocprofv3 database."""
    import sqlite3
    with sqlite3.connect(db) as con:
        total = con.execute("select count(*) from kernels").fetchone()[0]
        ms = lambda like: (con.execute(f"select sum(end - start) / 1e6 from kernels where name like '%{like}%'").fetchone()[0] or 0.0) / calls
        return total / calls, ms("paint_kernel"), ms("fill"), ms("centroid_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 4096], help="none: only summarise --launch-traces")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--step", default=None, help="run one step in this process (what the driver starts under timeout)")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--launch-traces", nargs="*", default=[], metavar="SIZE:DB")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        for line in globals()[f"step_{args.step}"](args.size, args.reps, not args.no_host):
            print("RESULT " + line, flush=True)
        return 0
    lines = [f"refine_points / estimate_d, whole calls, median of {args.reps} after one warm-up, each ending in a device synchronise; host clock; "
             "profiler off; jittered honeycomb, l = 12; every step a process of its own.  Not kernel times."]
    for size in args.sizes:
        for step, seconds in STEPS:
            cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--step", step, "--size", str(size),
                   "--reps", str(args.reps)] + (["--no-host"] if args.no_host else [])
            run = subprocess.run(cmd, capture_output=True, text=True)
            got = [l[7:] for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            lines += got
            print("\n".join(got), flush=True)
            if run.returncode != 0:                                      # a failure ends the run: nothing more is started on the GPU
                lines.append(f"step {step} at size {size} ended with status {run.returncode}; the run stops here\n{run.stderr[-2000:]}")
                print(lines[-1], flush=True)
                if args.out:
                    open(args.out, "w").write("\n".join(lines) + "\n")
                return 1
    for item in args.launch_traces:
        size, db = item.split(":", 1)
        per_call, paint, fill, centroid = trace_summary(db)
        lines.append(f"size {int(size):5d}: {per_call:.1f} kernel dispatches per refine_points_device call (rocprofv3 --kernel-trace, a run of its own, two "
                     f"calls); owner-image pass: fill {fill:.3f} ms + paint_kernel {paint:.3f} ms, centroid_kernel {centroid:.3f} ms under the tracer")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
