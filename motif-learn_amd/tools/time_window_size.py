#!/usr/bin/env python3
"""Times of the Fourier window-size estimators on one GPU (profiles/window_size.txt): whole calls, NumPy in, NumPy out.

Per case, wall clock around the call (every entry point is blocking); two warm-up passes, then ``--passes`` (at least 20)
timed ones; minimum, median, maximum:

* ``get_characteristic_length_fft`` and ``get_characteristic_length`` on one 512^2 frame, one 2048^2 frame and a
  (64, 512, 512) stack;
* the same stack as 64 single-frame calls of this build (two paths of the same code against each other: information, not a
  bar);
* ``angular_average`` at 2048^2 (360 bins, masked);
* beside each, the NumPy / SciPy restatement of tests/window_size_cases.py on this box's host (one pass for the large cases).

Every case runs in a child process of its own under a time limit, so a case that hangs ends alone.

    python tools/time_window_size.py [--passes 20] [--case NAME]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))

CASES = ["frame512", "frame2048", "stack64x512", "angular2048"]
LIMIT = {"frame512": 300, "frame2048": 420, "stack64x512": 600, "angular2048": 300}   # seconds: the host restatement dominates


def timed(call, passes, warm=2):
    for _ in range(warm):
        call()
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return np.array(times)


def show(times):
    return f"min {times.min():9.3f} median {np.median(times):9.3f} max {times.max():9.3f} ms"


def host(call, passes=1):
    return show(timed(call, passes, warm=0))


def run_case(case, passes):
    import window_size_cases as wc
    from mtflearn_amd import _native
    from mtflearn_amd.features import window_size as ws
    _native.load()
    _native.require_device()
    if case == "angular2048":
        data = wc.angular_input((2048, 2048))
        t = timed(lambda: ws.angular_average(data), passes)
        print(f"angular_average 2048^2, 360 bins, masked      {show(t)}")
        print(f"  host restatement (NumPy), one pass          {host(lambda: wc.angular_average(data))}", flush=True)
        return
    if case == "stack64x512":
        stack = np.stack([wc.frame((512, 512), 6.0 + 0.1 * b, b) for b in range(64)])
        for name, fn, ref in (("get_characteristic_length_fft", ws.get_characteristic_length_fft, lambda f: wc.get_characteristic_length_fft(f)[0]),
                              ("get_characteristic_length", ws.get_characteristic_length, lambda f: wc.get_characteristic_length(f)[0])):
            whole = timed(lambda: fn(stack), passes)
            single = timed(lambda: [fn(f) for f in stack], passes)
            same = np.array_equal(np.asarray(fn(stack), dtype=np.float64), np.asarray([fn(f) for f in stack], dtype=np.float64))
            print(f"{name} (64, 512, 512), one call       {show(whole)}")
            print(f"  the same as 64 single-frame calls           {show(single)}   ratio of the medians {np.median(single) / np.median(whole):5.2f}; equal results: {same}")
            t0 = time.perf_counter()
            ref(stack[0])
            one = (time.perf_counter() - t0) * 1e3
            print(f"  host restatement, one frame                 {one:9.1f} ms -> {one * 64 / 1e3:7.2f} s for the stack", flush=True)
        return
    side = 512 if case == "frame512" else 2048
    img = wc.frame((side, side), 8.0, 3)
    host_passes = 3 if side == 512 else 1
    t = timed(lambda: ws.get_characteristic_length_fft(img), passes)
    print(f"get_characteristic_length_fft {side}^2            {show(t)}   -> {ws.get_characteristic_length_fft(img)}")
    print(f"  host restatement (NumPy / SciPy)            {host(lambda: wc.get_characteristic_length_fft(img), host_passes)}")
    t = timed(lambda: ws.get_characteristic_length(img), passes)
    print(f"get_characteristic_length {side}^2                {show(t)}   -> {ws.get_characteristic_length(img)}")
    print(f"  host restatement (NumPy / SciPy)            {host(lambda: wc.get_characteristic_length(img), host_passes)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--case", choices=CASES, default=None, help="run one case in this process (what the parent starts)")
    args = ap.parse_args()
    passes = max(20, args.passes)
    if args.case:
        run_case(args.case, passes)
        return 0
    from mtflearn_amd import _native
    print(f"library {_native.LIB_PATH}; float64 frames; host CPUs available: {len(os.sched_getaffinity(0))}; {passes} timed passes", flush=True)
    for case in CASES:
        rc = subprocess.call(["timeout", "-k", "10", str(LIMIT[case]), sys.executable, os.path.abspath(__file__), "--passes", str(passes),
                              "--case", case])
        if rc != 0:
            print(f"case {case} ended with status {rc}: nothing further is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
