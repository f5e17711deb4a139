#!/usr/bin/env python3
"""Times the denoise module (zk_windows_* and the public calls) on honeycomb_frame(n) float32 frames at 32 px.

Per operation: the median host-clock time of the device-resident call (zk_windows_*_dev on a resident frame and resident
operands; every such call ends in a stream synchronise inside the library, so the host clock brackets the kernels plus one
launch and one synchronise), with the algorithmic FLOPs and the rate they give.  Per public call: the median wall time from
a NumPy frame to a NumPy result.  The host path of the reference (tests/denoise_oracle.py: the materialised window matrix,
scikit-learn's randomized_svd, a Python overlap-add) is timed once on a crop and named as one.  Neither HIP events nor the
shader clock are taken: the device calls synchronise inside the library, so an event pair around one would bracket the same
uploads and waits as the host clock does; rates are therefore printed only for calls of 5 ms or more.

Every step runs in a child process of its own under a time limit; the first failure ends the run.

Usage: python motif-learn_amd/tools/time_denoise.py [--reps 5] [--out FILE]        (the driver)
       python motif-learn_amd/tools/time_denoise.py --step NAME [--reps 5]          (one step, what the driver starts)
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "motif-learn_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

P, K, L = 32, 8, 18          # patch edge, components, columns of the randomized factors (k + 10)
# step name -> (time limit in seconds, frame edge, grid step or None for the default p / 4)
STEPS = {"ops_2048_default": (240, 2048, None), "ops_2048_step1": (300, 2048, 1), "ops_4096_default": (300, 4096, None),
         "ops_4096_step1": (420, 4096, 1), "call_2048_default": (300, 2048, None), "call_4096_default": (300, 4096, None),
         "call_2048_step1": (360, 2048, 1),
         "view_2048": (420, 2048, 1), "host_crop_1024": (300, 1024, None)}


def median_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def run_step(name, reps):
    import denoise_oracle as do
    import mtflearn_amd
    from mtflearn_amd import _denoise_svd as sv
    from mtflearn_amd import _native, denoise
    from mtflearn_amd.synthetic import honeycomb_frame
    _, n, step = STEPS[name]
    frame = honeycomb_frame(n, seed=7)
    st = max(1, P // 4) if step is None else step
    label = f"{n}^2 f32, {P} px, step {st}"
    if name.startswith("host_crop"):
        threads = os.environ.get("OMP_NUM_THREADS", "unset")
        np.random.seed(0)
        t0 = time.perf_counter()
        do.denoise_svd(frame.astype(np.float64), P, K)
        print(f"host path on a {n}^2 CROP (materialised matrix + sklearn randomized_svd + Python overlap-add, OMP_NUM_THREADS={threads}): "
              f"{(time.perf_counter() - t0) * 1e3:.0f} ms, once")
        return
    if name.startswith("call"):
        def call():
            np.random.seed(0)
            mtflearn_amd.denoise_svd(frame, P, K, extraction_step=step, verbose=False)
        if step == 1:                                   # 4 M windows: every (N, 18) factor is 0.6 GB over PCIe and through LAPACK
            t0 = time.perf_counter()
            call()
            print(f"denoise_svd({label}, k {K}), NumPy in / NumPy out: {(time.perf_counter() - t0) * 1e3:.0f} ms, once, no warm-up")
            return
        print(f"denoise_svd({label}, k {K}), NumPy in / NumPy out: {median_ms(call, reps):.1f} ms (median of {reps})")
        return
    if name.startswith("view"):
        t = median_ms(lambda: denoise.denoise_svd_memory_view(frame, P, K), max(1, reps // 2))
        print(f"denoise_svd_memory_view({n}^2 f32, {P} px, k {K}), NumPy in / NumPy out: {t:.1f} ms")
        dev = _native.DeviceArray.from_numpy(frame)
        win = sv._Windows(dev, (P, P), np.arange(n - P + 1), np.arange(n - P + 1))
        t = median_ms(win.moments_dev, reps)
        flop = 2.0 * (2 * P - 1) * P * n * n
        print(f"  zk_windows_moments_dev: {t:.2f} ms; {flop / 1e9:.1f} GFLOP by shifts ({flop / t / 1e9:.2f} TFLOP/s), "
              f"{2.0 * win.n * win.d ** 2 / 1e12:.2f} TFLOP as a plain product")
        return
    dev = _native.DeviceArray.from_numpy(frame)
    ii = do.origins(n, P, st)
    win = sv._Windows(dev, (P, P), ii, ii)
    rng = np.random.default_rng(0)
    q = _native.DeviceArray.from_numpy(rng.standard_normal((win.d, L)))
    y = win.apply_dev(q, L)
    yk = _native.DeviceArray.from_numpy(rng.standard_normal((win.n, K))) if win.n * K < 1 << 27 else win.apply_dev(
        _native.DeviceArray.from_numpy(rng.standard_normal((win.d, K))), K)
    v = _native.DeviceArray.from_numpy(rng.standard_normal((K, win.d)))
    flop = 2.0 * win.n * win.d * L
    print(f"{label}: N {win.n}, D {win.d}; medians of {reps}")
    for what, fn, f in (("zk_windows_apply_dev   (l 18)", lambda: win.apply_dev(q, L), flop),
                        ("zk_windows_apply_t_dev (l 18)", lambda: win.apply_t_dev(y, L), flop),
                        ("zk_windows_reconstruct_dev (k 8)", lambda: win.reconstruct_dev(yk, K, v),
                         2.0 * K * n * n * (-(-P // st)) ** 2)):
        t = median_ms(fn, reps)
        # below a few ms the host clock sees the two origin-list uploads and the synchronisations, not the kernel: no rate then
        rate = f"{f / t / 1e9:6.2f} TFLOP/s" if t >= 5.0 else "(launch / synchronise bound: no rate)"
        print(f"  {what}: {t:9.2f} ms  {f / 1e9:8.1f} GFLOP  {rate}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", default=None, choices=sorted(STEPS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, a.reps)
        return 0
    lines = []
    for name, (limit, _, _) in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        print(r.stdout, end="", flush=True)
        lines.append(r.stdout)
        if r.returncode != 0:                       # nothing more is started on the GPU after a failure
            print(f"step {name} ended with status {r.returncode}; stopping\n{r.stderr[-2000:]}", flush=True)
            lines.append(f"step {name} ended with status {r.returncode}; stopped\n")
            break
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(lines))
    return 0 if r.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
