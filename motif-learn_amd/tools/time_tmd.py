#!/usr/bin/env python3
"""Times of mtflearn_amd.resident.tmd_frames_device on one GPU (profiles/tmd.txt): a stack of default-parameter
TMDImageSimulator frames (``--frames`` x ``--size``^2, a = 30, angles spread over 0 .. 60 degrees, a few random defects each),
in both modes.

Per mode, wall clock around the call (``zk_tmd_render_dev`` uploads its points, takes its scratch and synchronises its stream
before it returns, so the wall clock is the honest figure); two warm-up passes, then ``--passes`` (at least 10) timed ones;
minimum, median, maximum:

* host preparation: the lattices, labels, scales and half kernels of all simulators (NumPy, one thread);
* the device call with the masks kept (delta stage + blur stage, nothing allocated for the delta images);
* the delta stage alone: the same call without weights (memset, link, sum);
* blur stage = the difference of the medians;
* the device call without masks (it then allocates the delta images itself);
* a plain device copy (``zk_hbm_probe``, 16 B per lane) of the stages' algorithmic bytes, taken in the same process.  Delta stage,
  per species and pixel: 4 B set, 4 B read, 4 B written.  Blur stage: 4 B read per species and pixel (the halo and the taps are
  served by the caches and not counted), 4 B written per pixel;
* the NumPy statement of tests/tmd_oracle.py for ONE frame on this box's host, times the number of frames.

    python tools/time_tmd.py [--frames 64] [--size 1024] [--passes 10]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))


def timed(call, passes):
    for _ in range(2):
        call()
    times = []
    for _ in range(passes):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return np.array(times)


def show(times):
    return f"min {times.min():9.3f} median {np.median(times):9.3f} max {times.max():9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    passes = max(10, args.passes)
    import tmd_oracle as to
    from mtflearn_amd import _native, datasets

    _native.load()
    _native.require_device()
    dev = _native.default_device()
    n, size = args.frames, args.size
    pixels = n * size * size
    print(f"library {_native.LIB_PATH}; {n} x {size}^2 float32 frames, 2 species; host CPUs available: {len(os.sched_getaffinity(0))}")
    for use_fft in (True, False):
        sims = []
        for b in range(n):
            sim = datasets.TMDImageSimulator(size=(size, size), theta=60.0 * b / n, use_fft=use_fft)
            sim.add_random_vacancies('X', 3, 3, seed=b)
            sim.add_random_dopants('TM', 4, seed=b)
            sims.append(sim)

        def prepare():
            layers = []
            for b, sim in enumerate(sims):
                layers += [(b,) + layer[1:] for layer in sim._layers()]
            return layers

        host = timed(prepare, passes)
        layers = prepare()
        atoms = sum(len(layer[1]) for layer in layers)
        radii = sorted({len(layer[3]) - 1 for layer in layers})
        out = _native.DeviceArray((n, size, size), np.float32, dev)
        masks = _native.DeviceArray((len(layers), size, size), np.float32, dev)
        both = timed(lambda: datasets._tmd_render_device(out, masks, layers, True, use_fft), passes)
        delta = timed(lambda: datasets._tmd_render_device(None, masks, layers, False, use_fft), passes)
        alone = timed(lambda: datasets._tmd_render_device(out, None, layers, True, use_fft), passes)
        delta_bytes, blur_bytes = 12 * 2 * pixels, (4 * 2 + 4) * pixels
        copies = []
        for total in (delta_bytes, blur_bytes):
            src = _native.DeviceArray((total // 2,), np.uint8, dev)
            dst = _native.DeviceArray((total // 2,), np.uint8, dev)
            copies.append(_native.hbm_probe(dev, src.data_ptr(), src.numel(), dst.data_ptr(), reps=passes))
            del src, dst
        blur_ms = np.median(both) - np.median(delta)
        frame = out.numpy()[0]
        mask0 = masks.numpy()[:2]
        del out, masks
        t0 = time.perf_counter()
        params = [sims[0].species_params[s] for s in ("TM", "X")]
        coords = sims[0]._cached_coords
        own = [to.delta((size, size), coords[s], sims[0]._scales(s, len(coords[s]), False)) for s in ("TM", "X")]
        ref = to.exact_image(own, params) if use_fft else to.gauss_image(own, params)
        oracle_s = time.perf_counter() - t0
        if use_fft:
            agree = f"max |frame 0 - E| = {np.abs(frame - ref).max():.2e} (bound {to.fft_bound(ref, 2):.2e})"
        else:
            agree = f"frame 0 equal to the oracle bit for bit: {np.array_equal(frame, ref)}"
        print(f"use_fft={use_fft}: {atoms} atoms on the frames, kernel radii {radii}; masks of frame 0 equal to the oracle: "
              f"{np.array_equal(mask0, np.stack(own))}; {agree}")
        print(f"  host preparation                 {show(host)}")
        print(f"  device call, masks kept          {show(both)}")
        print(f"  delta stage alone                {show(delta)}   {delta_bytes / 1e9:6.3f} GB -> {delta_bytes / np.median(delta) / 1e6:6.0f} GB/s at the "
              f"median; plain copy of the same bytes {copies[0]:8.3f} ms = {delta_bytes / copies[0] / 1e6:6.0f} GB/s")
        print(f"  blur stage (difference)          {blur_ms:9.3f} ms at the medians            {blur_bytes / 1e9:6.3f} GB -> {blur_bytes / blur_ms / 1e6:6.0f} GB/s; "
              f"plain copy of the same bytes {copies[1]:8.3f} ms = {blur_bytes / copies[1] / 1e6:6.0f} GB/s")
        print(f"  device call, no masks            {show(alone)}")
        print(f"  oracle (NumPy, host), one frame  {oracle_s * 1e3:9.1f} ms -> {oracle_s * n:7.1f} s for {n} frames", flush=True)


if __name__ == "__main__":
    main()
