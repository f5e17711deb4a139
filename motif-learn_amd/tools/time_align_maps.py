#!/usr/bin/env python3
"""Times of the alignment maps (``ZPs.align_maps`` / ``resident.align_maps_device``, csrc/zk_align.hip) on one MI355X.

Per frame (2048^2 and 4096^2 float32), ZPs(n_max 8, size 32), T = 4 templates, n_theta = 360, refined, HIP events on torch's
current stream, median (and minimum) of ``--reps`` >= 10 after one warm-up, with the mean shader clock over the timed launches
(``_native.ClockMonitor``):
  (a) planes   ``zk_align_planes_dev`` alone on resident (P, H, W) moments; as FMA/s of the scan's T 2 NM n_theta fused
               multiply-adds per pixel (NM = 8) against the FP64 vector peak (78.6 TFLOP/s = 39.3 TFMA/s at 2.4 GHz) and against
               the same peak at the measured clock; beside it the rows kernel on the transposed copy (the expectation: equal).
  (b) maps     ``resident.align_maps_device`` whole, into preallocated whole-frame maps: dense transform into the scratch matrix
               band by band + the planes kernel per band.
  (c) parent   the only route before the maps existed: ``frame_moments_device(full=...)``, a contiguous transpose to (HW, P), then
               ``zk_align_rows_dev``; its three parts timed separately.
Peak device memory of (b) and (c): torch's peak allocation over one call (operands and results) plus, for (b), the library's
scratch matrix, which torch does not see (its size is computed: min(1 GiB, 8 P H W) bytes).  No counters are collected here.

Usage:  python motif-learn_amd/tools/time_align_maps.py [--reps 11] [--out profiles/align_maps.txt]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

SIZE, N_MAX, NM, TEMPLATES, N_THETA = 32, 8, 8, 4, 360
PEAK_TFMA, PEAK_GHZ = 39.3, 2.4


def event_ms(launch, reps):
    import torch
    from mtflearn_amd import _native
    launch()
    torch.cuda.synchronize()
    times, clocks = [], []
    stream = torch.cuda.current_stream()
    for _ in range(reps):                               # one clock monitor per launch: a monitor lives 2 s at the most
        with _native.ClockMonitor(0, max_ms=2000.0) as mon:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            launch()
            stop.record()
            stop.synchronize()
            times.append(start.elapsed_time(stop))
            stream.synchronize()
        clocks.append(mon.ghz)
    return float(np.median(times)), float(min(times)), float(np.mean(clocks))


def peak_gib(call):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    keep = call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    del keep
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--sides", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    from mtflearn_amd import ZPs, _native, resident
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    zps = ZPs(N_MAX, SIZE)
    plan = zps._device_plan()
    P = len(zps.n)
    rng = np.random.default_rng(0)
    t = rng.standard_normal((TEMPLATES, P))
    spec = zps._align_spec(t, None, N_THETA, 1, True, "distance")
    say(f"alignment maps on {torch.cuda.get_device_name(0)}: ZPs({N_MAX}, {SIZE}) (P = {P}), float32 frames, T = {TEMPLATES}, n_theta = "
        f"{N_THETA}, refined; HIP events, medians after one warm-up, profiler off; no counters collected.")
    for side in args.sides:
        h = w = side
        px = h * w
        image = torch.from_numpy(rng.random((h, w), dtype=np.float32)).cuda()
        stream = torch.cuda.current_stream().cuda_stream
        head = f"{side}^2:"
        fma = float(px) * TEMPLATES * 2 * NM * N_THETA
        # ---- (c) the parent's route, part by part
        full = torch.empty((P, h, w), dtype=torch.float64, device="cuda")
        c1 = event_ms(lambda: resident.frame_moments_device(plan, image, full=full), args.reps)
        rows = torch.empty((px, P), dtype=torch.float64, device="cuda")
        c2 = event_ms(lambda: rows.copy_(full.view(P, px).t()), args.reps)
        angle_r = torch.empty((px, TEMPLATES), dtype=torch.float64, device="cuda")
        score_r = torch.empty_like(angle_r)
        best = torch.empty(px, dtype=torch.int32, device="cuda")
        c3 = event_ms(lambda: _native.align_rows_dev(0, rows.data_ptr(), px, spec, angle_r.data_ptr(), score_r.data_ptr(), best.data_ptr(), stream),
                      args.reps)
        del rows, angle_r, score_r
        # ---- (a) the planes kernel alone on the resident moments
        angle = torch.empty((TEMPLATES, h, w), dtype=torch.float64, device="cuda")
        score = torch.empty_like(angle)
        norm2 = torch.empty((h, w), dtype=torch.float64, device="cuda")
        best2 = best.view(h, w)
        a = event_ms(lambda: _native.align_planes_dev(0, full.data_ptr(), px, px, spec, angle.data_ptr(), score.data_ptr(), best.data_ptr(),
                                                      norm2.data_ptr(), px, stream), args.reps)
        del full
        rate = fma / a[0] / 1e9
        say(f"{head} (a) planes kernel {a[0]:8.3f} ms median (min {a[1]:.3f}) of {args.reps} at {a[2]:.2f} GHz | scan {fma / 1e9:.1f} GFMA -> "
            f"{rate:.2f} TFMA/s = {100 * rate / PEAK_TFMA:.0f} % of the FP64 vector peak ({PEAK_TFMA} TFMA/s at {PEAK_GHZ} GHz), "
            f"{100 * rate / (PEAK_TFMA * a[2] / PEAK_GHZ):.0f} % of it at the measured clock | rows kernel on the transposed copy "
            f"{c3[0]:8.3f} ms (min {c3[1]:.3f}) at {c3[2]:.2f} GHz: planes / rows = {a[0] / c3[0]:.3f}")
        # ---- (b) the banded frame route, whole
        maps = (angle, score, best2, norm2)
        b = event_ms(lambda: resident.align_maps_device(plan, image, t, full=maps), args.reps)
        say(f"{head} (b) align_maps_device {b[0]:8.3f} ms median (min {b[1]:.3f}) of {args.reps} at {b[2]:.2f} GHz")
        total_c = c1[0] + c2[0] + c3[0]
        say(f"{head} (c) parent route {total_c:8.3f} ms = moments {c1[0]:.3f} (min {c1[1]:.3f}) + transpose {c2[0]:.3f} (min {c2[1]:.3f}) + "
            f"align_rows {c3[0]:.3f} (min {c3[1]:.3f}) | (b) / (c) = {b[0] / total_c:.3f}, (c) - (b) = {total_c - b[0]:.3f} ms "
            f"(transpose: {c2[0]:.3f} ms)")
        del angle, score, norm2, best, best2, maps
        # ---- peak memory of one whole call of either route
        scratch = min(1 << 30, 8 * P * px) / 2 ** 30
        peak_b = peak_gib(lambda: resident.align_maps_device(plan, image, t))

        def parent():
            mom = resident.frame_moments_device(plan, image)
            r = mom.view(P, px).t().contiguous()
            return resident.align_device(r, zps.n, zps.m, t)

        peak_c = peak_gib(parent)
        say(f"{head} peak device memory of one call: (b) {peak_b:.2f} GiB of tensors + {scratch:.2f} GiB scratch = {peak_b + scratch:.2f} GiB | "
            f"(c) {peak_c:.2f} GiB | 8 P H W = {8 * P * px / 2 ** 30:.2f} GiB")
        del image
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
