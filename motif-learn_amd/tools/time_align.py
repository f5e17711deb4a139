#!/usr/bin/env python3
"""Times of ``zmoments.align`` / ``rotate_each`` (csrc/zk_align.hip) on one MI355X.

Per n_max (8, 12) at N = 2^20 rows, T = 8 templates, n_theta = 360, refine on and off:
  kernel      HIP events around ``zk_align_rows_dev`` on torch's current stream, median (and minimum) of ``--reps`` >= 10 launches
              after one warm-up, with the mean shader clock over the timed launches (``_native.ClockMonitor``); as FMA/s of the
              grid stage's 2 N T n_theta n_max fused multiply-adds against the FP64 vector peak (78.6 TFLOP/s = 39.3 TFMA/s at
              2.4 GHz) and against the same peak at the measured clock.
  resident    whole ``resident.align_device`` call, output allocation included, ending in a device synchronise; host clock.
  NumPy       whole ``zmoments.align`` call, NumPy in, NumPy out; host clock.
  host        the NumPy statement (tests/align_cases.py) on ``--host-rows`` rows of the same input, as rows per second.
``rotate_rows`` at the same shapes: kernel time and GB/s of its 16 N P bytes, beside the box's 16-B-per-lane copy rate from
``zk_hbm_probe`` (what bench.py prints as ``roofline.this_box``).  No counters are collected here: what binds the kernel is
not measured by this tool.

Usage:  python motif-learn_amd/tools/time_align.py [--reps 11] [--out profiles/align.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..", "tests")))

ROWS, TEMPLATES, N_THETA = 1 << 20, 8, 360
PEAK_TFMA, PEAK_GHZ = 39.3, 2.4


def median_ms(call, reps, sync):
    call()
    sync()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        sync()
        times.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(times)), float(min(times))


def event_ms(launch, reps):
    import torch
    from mtflearn_amd import _native
    launch()
    torch.cuda.synchronize()
    times = []
    stream = torch.cuda.current_stream()
    with _native.ClockMonitor(0, max_ms=1500.0) as mon:
        for _ in range(reps):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            launch()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
        stream.synchronize()
    return float(np.median(times)), float(min(times)), mon.ghz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import align_cases as ac
    from mtflearn_amd import _native, resident, zmoments
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"zmoments.align / rotate_each on {torch.cuda.get_device_name(0)}: N = {ROWS}, T = {TEMPLATES}, n_theta = {N_THETA}; kernel times "
        "from HIP events, whole calls on the host clock ending in a device synchronise; medians after one warm-up; profiler off; "
        "no counters collected (what binds the kernels is unmeasured).")
    nbytes = 4 << 30
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ms_copy = _native.hbm_probe(0, src.data_ptr(), nbytes, dst_ptr=dst.data_ptr())
    copy_rate = 2 * nbytes / ms_copy / 1e6
    say(f"this box, zk_hbm_probe 16-B-per-lane copy over 4 GiB: {copy_rate:.0f} GB/s read + written")
    del src, dst
    stream = torch.cuda.current_stream().cuda_stream
    for n_max in (8, 12):
        n, m = ac.labels(n_max)
        rng = np.random.default_rng(n_max)
        x, t = rng.standard_normal((ROWS, len(n))), rng.standard_normal((TEMPLATES, len(n)))
        xd = torch.from_numpy(x).cuda()
        angle = torch.empty((ROWS, TEMPLATES), dtype=torch.float64, device="cuda")
        score = torch.empty_like(angle)
        best = torch.empty(ROWS, dtype=torch.int32, device="cuda")
        z = zmoments._adopt(x, n, m)
        for refine in (True, False):
            spec = _native.AlignSpec(n, m, t, None, N_THETA, 1, 3 if refine else 0, "distance")
            launch = lambda: _native.align_rows_dev(0, xd.data_ptr(), ROWS, spec, angle.data_ptr(), score.data_ptr(), best.data_ptr(), stream)
            k_med, k_min, ghz = event_ms(launch, args.reps)
            fma = 2.0 * ROWS * TEMPLATES * N_THETA * n_max
            rate = fma / k_med / 1e9
            head = f"n_max {n_max:2d} (P {len(n):3d}) refine {'on ' if refine else 'off'}:"
            say(f"{head} kernel {k_med:8.3f} ms median (min {k_min:.3f}) of {args.reps} at {ghz:.2f} GHz | grid stage {fma / 1e9:.1f} GFMA -> "
                f"{rate:.2f} TFMA/s = {100 * rate / PEAK_TFMA:.0f} % of the FP64 vector peak ({PEAK_TFMA} TFMA/s at {PEAK_GHZ} GHz), "
                f"{100 * rate / (PEAK_TFMA * ghz / PEAK_GHZ):.0f} % of it at the measured clock")
            r_med, r_min = median_ms(lambda: resident.align_device(xd, n, m, t, refine=refine), args.reps, torch.cuda.synchronize)
            n_med, n_min = median_ms(lambda: z.align(t, refine=refine), 3, torch.cuda.synchronize)
            sub = x[:args.host_rows]
            h_med, _ = median_ms(lambda: ac.align_statement(sub, t, n, m, None, N_THETA, 1, refine), 3, lambda: None)
            say(f"{head} whole call resident {r_med:8.3f} ms (min {r_min:.3f}) of {args.reps} | NumPy to NumPy {n_med:8.2f} ms (min {n_min:.2f}) of 3 | "
                f"NumPy statement on this host: {len(sub)} rows in {h_med:.1f} ms = {len(sub) / h_med * 1e3:.3e} rows/s (kernel: "
                f"{ROWS / k_med * 1e3:.3e} rows/s, {ROWS / k_med / (len(sub) / h_med):.0f}x)")
        ad = angle[:, 0].contiguous()
        out = torch.empty_like(xd)
        launch = lambda: _native.rotate_rows_dev(0, xd.data_ptr(), ROWS, n, m, ad.data_ptr(), out.data_ptr(), stream)
        k_med, k_min, ghz = event_ms(launch, args.reps)
        moved = 16.0 * ROWS * len(n)
        say(f"n_max {n_max:2d} rotate_rows: kernel {k_med:8.3f} ms median (min {k_min:.3f}) of {args.reps} at {ghz:.2f} GHz | {moved / 1e9:.2f} GB "
            f"(16 N P) -> {moved / k_med / 1e6:.0f} GB/s, {100 * moved / k_med / 1e6 / copy_rate:.0f} % of this box's copy rate")
        del xd, out, angle, score, best
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
