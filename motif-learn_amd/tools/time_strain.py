#!/usr/bin/env python3
"""Times of mtflearn_amd.strain on one GPU (profiles/strain.txt): float32 frames of 2048^2 and 4096^2, B = 1 and B = 32, with and
without a reference rectangle.

Per size:

* whole resident calls (``resident.gpa_device``) by HIP events on the stream and whole NumPy-to-NumPy calls (``strain.gpa``) by
  the wall clock; one warm-up pass (plans, allocations, the pinned pool), then ``--passes`` timed ones; minimum, median, maximum.
  The calls allocate and free their fields inside the timed window: that is what a caller pays;
* the fused strain kernel alone: the entry point has no event of its own around the kernel, so its time comes from a pass of its
  own -- ``rocprofv3 --kernel-trace --stats -- python tools/time_strain.py --trace-only`` -- whose kernel statistics
  ``--kernel-csv`` reads; without it the kernel's own time is reported as unmeasured.  Its algorithmic bytes (two complex planes
  read once, 32 B, and six float64 planes written, 48 B, per pixel) per second are quoted against the copy rate of this box
  (``zk_hbm_probe`` on 1 GiB, read + written bytes: the figure ``roofline.this_box`` of bench.py carries);
* the NumPy statement of the oracle (tests/strain_oracle.py) on this host, one frame.

    python tools/time_strain.py [--passes 5] [--small-only] [--kernel-csv kernel_stats.csv]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))

G = np.array([[0.0, 1 / 16], [1 / 16 * np.sqrt(3) / 2, -1 / 32]])
KERNEL_BYTES = 32 + 48                                       # per pixel: both planes in, four maps and two amplitudes out


def frames_of(n, b):
    y, x = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    bump = 0.4 * np.exp(-((y - 0.6 * n) ** 2 + (x - 0.55 * n) ** 2) / (2 * (n / 12) ** 2))
    frame = sum(np.cos(2 * np.pi * (gy * y + gx * (x - bump))) for gy, gx in G).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(frame, (b, n, n)))


def event_timed(torch, call, passes):
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(passes):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return np.min(times), np.median(times), np.max(times)


def wall_timed(call, passes):
    call()
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t0))
    return np.min(times), np.median(times), np.max(times)


def kernel_rows(path):
    """``{kernel name: (calls, total ns)}`` of the kernel statistics of a ``rocprofv3 --kernel-trace --stats`` run."""
    with open(path) as f:
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--kernel-csv", default=None)
    ap.add_argument("--trace-only", action="store_true", help="one resident 2048^2 call and nothing else: the run to put under rocprofv3")
    args = ap.parse_args()
    import torch
    from mtflearn_amd import _native, resident, strain
    import strain_oracle as so

    _native.load()
    _native.require_device()
    if args.trace_only:
        dev = torch.from_numpy(frames_of(2048, 1)).cuda()
        for _ in range(3):
            resident.gpa_device(dev, G, reference=(64, 512, 64, 512))
        torch.cuda.synchronize()
        return
    print(f"library {_native.LIB_PATH}; device {torch.cuda.get_device_name(0)}; CPUs of this process {len(os.sched_getaffinity(0))}")
    src = torch.zeros(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    copy = 2 * (1 << 30) / _native.hbm_probe(0, src.data_ptr(), 1 << 30, dst.data_ptr()) / 1e6
    del src, dst
    print(f"copy rate of this box (zk_hbm_probe, 1 GiB, read + written): {copy:.0f} GB/s")
    fmt = lambda t: f"min {t[0]:9.3f}  median {t[1]:9.3f}  max {t[2]:9.3f} ms"
    for n in (2048,) if args.small_only else (2048, 4096):
        reference = (n // 32, n // 4, n // 32, n // 4)
        for b in (1, 32):
            host = frames_of(n, b)
            dev = torch.from_numpy(host).cuda()
            print(f"{b} x {n}^2 float32")
            for ref in (None, reference):
                r = event_timed(torch, lambda: resident.gpa_device(dev, G, reference=ref), args.passes)
                what = "no reference" if ref is None else "reference    "
                print(f"  gpa_device  {what}  {fmt(r)}   {b * n * n / r[1] / 1e6:8.2f} Gpixel/s")
                if b * n * n <= 32 * 2048 * 2048:            # 32 x 4096^2 would hold 26 GB of results on the host
                    h = wall_timed(lambda: strain.gpa(host, G, reference=ref), max(2, args.passes // 2))
                    print(f"  gpa (NumPy) {what}  {fmt(h)}")
            del dev
        t0 = time.perf_counter()
        so.gpa(host[0], G, reference=reference)
        print(f"  NumPy oracle, one frame with a reference: {1e3 * (time.perf_counter() - t0):.1f} ms on this host")
    if args.kernel_csv:
        for name, (calls, total) in kernel_rows(args.kernel_csv).items():
            if "strain_kernel" in name:
                ms = total / calls / 1e6
                rate = 2048 * 2048 * KERNEL_BYTES / ms / 1e6
                print(f"strain_kernel alone, 2048^2, {calls} launches (rocprofv3 --kernel-trace --stats): {ms:.3f} ms, {rate:.0f} GB/s algorithmic"
                      + (f", {100 * rate / copy:.0f} % of the box's copy rate {copy:.0f} GB/s" if copy else ""))
    else:
        print("strain_kernel alone: unmeasured in this run (no --kernel-csv)")


if __name__ == "__main__":
    main()
