#!/usr/bin/env python3
"""Times of mtflearn_amd.registration on one GPU (profiles/registration.txt): float32 stacks of B = 32 frames of 512^2 and
2048^2, upsample = 100, reference frame 0.

Per stack:

* whole resident calls by HIP events on the stream: ``estimate_shifts_device`` at ``upsample = 100`` and at ``upsample = 1``, and
  ``register_stack_device`` (order 3, 'grid-wrap'); one warm-up pass (plans, allocations), then ``--passes`` timed ones; minimum,
  median, maximum.  The calls allocate and free their fields inside the timed window: that is what a caller pays;
* the upsampled-DFT stage (twiddle tables, the two complex products, the second peak search) as the difference of the two
  ``estimate_shifts_device`` medians -- the entry point has no event of its own around the stage -- and its share of the FP64
  vector peak: ``B S W (8 H + 4 S)`` flops (a complex multiply-add is 8, the real part of one 4) over that time against
  ``--peak-tflops`` (default 78.6, MI355X vector FP64);
* the NumPy statement of the oracle (tests/registration_oracle.py) on this host for ``--oracle-frames`` frames, scaled to B.

    python tools/time_registration.py [--passes 5] [--small-only] [--oracle-frames 2]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))

B, UPSAMPLE = 32, 100


def stack_of(n, seed):
    """B drifted copies of one band-limited noise frame, float32."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, n))
    spectrum = np.fft.fft2(base)
    ky, kx = np.fft.fftfreq(n)[:, None], np.fft.fftfreq(n)[None, :]
    drift = rng.uniform(-4, 4, (B, 2))
    drift[0] = 0
    return np.stack([np.real(np.fft.ifft2(spectrum * np.exp(-2j * np.pi * (ky * s[0] + kx * s[1])))) for s in drift]).astype(np.float32)


def timed(torch, call, passes):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--oracle-frames", type=int, default=2)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    args = ap.parse_args()
    import torch
    from mtflearn_amd import _native, resident
    import registration_oracle as ro

    _native.load()
    _native.require_device()
    print(f"library {_native.LIB_PATH}; device {torch.cuda.get_device_name(0)}; CPUs of this process {len(os.sched_getaffinity(0))}")
    for n in (512,) if args.small_only else (512, 2048):
        host = stack_of(n, n)
        stack = torch.from_numpy(host).cuda()
        fmt = lambda t: f"min {t[0]:9.3f}  median {t[1]:9.3f}  max {t[2]:9.3f} ms"
        fine = timed(torch, lambda: resident.estimate_shifts_device(stack, upsample=UPSAMPLE), args.passes)
        coarse = timed(torch, lambda: resident.estimate_shifts_device(stack, upsample=1), args.passes)
        whole = timed(torch, lambda: resident.register_stack_device(stack, upsample=UPSAMPLE), args.passes)
        s = (3 * UPSAMPLE + 1) // 2
        flops = B * s * n * (8 * n + 4 * s)
        stage = fine[1] - coarse[1]
        print(f"{B} x {n}^2 float32, upsample {UPSAMPLE} (S = {s})")
        print(f"  estimate_shifts_device upsample {UPSAMPLE:3d}  {fmt(fine)}")
        print(f"  estimate_shifts_device upsample   1  {fmt(coarse)}")
        print(f"  register_stack_device                {fmt(whole)}")
        print(f"  upsampled-DFT stage (difference of the medians) {stage:.3f} ms: {flops / 1e9:.1f} GFLOP, "
              f"{flops / stage / 1e9:.2f} TFLOP/s, {100 * flops / stage / 1e9 / args.peak_tflops:.1f} % of {args.peak_tflops} TFLOP/s")
        k = max(1, min(args.oracle_frames, B - 1))
        t0 = time.perf_counter()
        want, _ = ro.estimate_shifts(host[:k + 1].astype(np.float64), upsample=UPSAMPLE)
        per_frame = (time.perf_counter() - t0) / (k + 1)
        got = resident.estimate_shifts_device(stack, upsample=UPSAMPLE).shift.cpu().numpy()[:k + 1]
        print(f"  NumPy oracle {per_frame * 1e3:.1f} ms per frame on this host, {per_frame * B:.2f} s for {B}; "
              f"shifts of the first {k + 1} frames unequal to it: {np.count_nonzero(got != want)}")


if __name__ == "__main__":
    main()
