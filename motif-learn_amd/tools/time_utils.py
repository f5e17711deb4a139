#!/usr/bin/env python3
"""Times mtflearn_amd.utils (zk_image_stats / zk_image_order_stats / zk_image_map) against the host NumPy statements.

Frames: honeycomb_frame(n), float32, with one hot pixel (so that percentile_clip clips).  For percentile_clip and
normalize_image ("minmax"): the median of whole calls from a NumPy frame (upload and download included), of whole calls on a
resident frame (distributed.*_device on a DeviceArray; every call ends in a stream synchronise), and of the host NumPy
statement on this machine's CPU (restated below: four np.percentile, two np.median and np.clip; min, max and one expression).
Every device result is checked against the host statement, bit for bit.  Last line: percentile_clip_device on a constant
frame, where every element counts the same histogram bin in every sweep.

Usage: python motif-learn_amd/tools/time_utils.py [--reps 20] [--sizes 2048 4096] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "motif-learn_amd")):
    sys.path.insert(0, p)

from mtflearn_amd import _native, utils  # noqa: E402
from mtflearn_amd.distributed import normalize_image_device, percentile_clip_device  # noqa: E402
from mtflearn_amd.synthetic import honeycomb_frame  # noqa: E402


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def host_percentile_clip(x, low=1.0, high=99.0):
    """The statistics percentile_clip needs and the clip, as NumPy statements on a float32 frame."""
    flat = x.reshape(-1)
    stats = [flat.max(), flat.min(), np.percentile(flat, high), np.percentile(flat, low)]
    med = np.median(flat)
    stats += [med, np.median(np.abs(flat - med)), np.percentile(flat, 25), np.percentile(flat, 75)]
    return np.clip(x, float(stats[3]), float(stats[2])), stats


def host_normalize(x, eps=1e-8, vmin=0.0, vmax=1.0):
    x_min, x_max = x.min(), x.max()
    return vmin + (x - x_min) * (vmax - vmin) / ((x_max - x_min) + eps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 runs"
    assert _native.device_count() > 0, "time_utils.py needs a HIP device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("mtflearn_amd.utils timing: medians of %d whole calls after 2 warm-ups (host statement: %d)" % (a.reps, max(3, a.reps // 4)))
    say("%-11s %-16s %11s %12s %10s %10s" % ("frame", "function", "numpy ms", "resident ms", "host ms", "host/res"))
    for n in a.sizes:
        frame = honeycomb_frame(n, n, seed=n)
        frame[n // 3, n // 2] = 40.0
        dev = _native.DeviceArray.from_numpy(frame)
        host_reps = max(3, a.reps // 4)

        want, _ = host_percentile_clip(frame)
        got, did_clip, _ = utils.percentile_clip(frame)
        res, did_clip_dev, _ = percentile_clip_device(dev)
        assert did_clip and did_clip_dev and np.array_equal(got, want) and np.array_equal(res.numpy(), want)
        t_np = median_ms(lambda: utils.percentile_clip(frame), a.reps)
        t_res = median_ms(lambda: percentile_clip_device(dev), a.reps)
        t_host = median_ms(lambda: host_percentile_clip(frame), host_reps, warmup=1)
        say("%-11s %-16s %11.3f %12.3f %10.1f %9.0fx" % ("%d^2 f32" % n, "percentile_clip", t_np, t_res, t_host, t_host / t_res))

        want = host_normalize(frame)
        assert np.array_equal(utils.normalize_image(frame), want) and np.array_equal(normalize_image_device(dev).numpy(), want)
        t_np = median_ms(lambda: utils.normalize_image(frame), a.reps)
        t_res = median_ms(lambda: normalize_image_device(dev), a.reps)
        t_host = median_ms(lambda: host_normalize(frame), host_reps, warmup=1)
        say("%-11s %-16s %11.3f %12.3f %10.1f %9.0fx" % ("%d^2 f32" % n, "normalize_image", t_np, t_res, t_host, t_host / t_res))

    n = a.sizes[0]
    random_dev = _native.DeviceArray.from_numpy(honeycomb_frame(n, n, seed=n))
    const_dev = _native.DeviceArray.from_numpy(np.full((n, n), 0.375, np.float32))
    t_random = median_ms(lambda: percentile_clip_device(random_dev), a.reps)
    t_const = median_ms(lambda: percentile_clip_device(const_dev), a.reps)
    say("%d^2 f32 percentile_clip_device, resident: lattice frame %.3f ms, constant frame (one bin per sweep) %.3f ms = %.2fx"
        % (n, t_random, t_const, t_const / t_random))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
