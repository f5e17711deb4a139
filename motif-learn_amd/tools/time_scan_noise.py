#!/usr/bin/env python3
"""Times of mtflearn_amd.denoise.apply_scan_noise on one GPU (profiles/scan_noise.txt): float32 stacks of 4 x 1024^2 and
16 x 2048^2, orders 1 and 3, mode 'reflect', jx = jy = 1.

Per stack and order:

* the kernels alone, by HIP events around ``zk_scan_resample_dev`` with the caller's scratch (nothing is allocated and nothing
  synchronises inside the timed window): two warm-up passes, then ``--passes`` (at least 10) timed ones; minimum, median, maximum;
* the algorithmic bytes per pixel over that time, beside the rate of a plain device copy of the same number of bytes taken in
  the same process (``zk_hbm_probe``, 16 B per lane).  Order 1: the float32 sample in and out, 8 B.  Order 3: row prefilter
  4 in + 8 out, column prefilter 8 + 8, gather 8 in + 4 out, 40 B.  The taps of a pixel's neighbours and the Z (H + W) shifts
  are served by the caches and not counted;
* the whole host call NumPy to NumPy (upload through the staging ring, kernels, download), best of ``--repeat``;
* SciPy's time for the reference's call on this box's host: ``map_coordinates`` on the whole 3-D stack with three float64
  coordinate cubes, single-threaded (SciPy's ndimage has no threads; the CPUs this process may use are printed).

    python tools/time_scan_noise.py [--passes 10] [--repeat 2] [--small-only] [--no-scipy]
"""
import argparse
import os
import sys
import time
from ctypes import c_void_p

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

BYTES_PER_PIXEL = {1: 4 + 4, 3: (4 + 8) + (8 + 8) + (8 + 4)}


def stack_of(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(256, 4096, size=shape).astype(np.float32)


def scipy_call(images, dx, dy, order, mode):
    """The reference's function body on given draws."""
    from scipy.ndimage import map_coordinates
    z, y, x = np.meshgrid(*(np.arange(n) for n in images.shape), indexing="ij")
    coords = np.array([z, y + dy[:, None, :], x + dx[:, :, None]])
    return map_coordinates(images, coords, order=order, mode=mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    passes = max(10, args.passes)
    import torch
    from mtflearn_amd import _native, denoise

    lib = _native.load()
    _native.require_device()
    dev = _native.default_device()
    print(f"library {_native.LIB_PATH}")
    print(f"host CPUs available to this process: {len(os.sched_getaffinity(0))}; scipy.ndimage.map_coordinates runs on one thread")
    shapes = [(4, 1024, 1024)] + ([] if args.small_only else [(16, 2048, 2048)])
    mode = "reflect"
    code = _native.RESAMPLE_MODES[mode]
    denoise.apply_scan_noise(stack_of((1, 64, 64), 0), jx=1, jy=1, seed=0, order=3, mode=mode)       # loads the code objects
    for shape in shapes:
        z, h, w = shape
        pixels = z * h * w
        images = stack_of(shape, 7)
        dx, dy = denoise._jitter(11, shape, 1, 1)
        t_img, t_dx, t_dy = torch.from_numpy(images).cuda(), torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
        t_out = torch.empty_like(t_img)
        scratch = torch.empty(16 * pixels, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ptr = lambda t: c_void_p(t.data_ptr())
        for order in (1, 3):
            total = BYTES_PER_PIXEL[order] * pixels
            src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            copy_ms = _native.hbm_probe(dev, src.data_ptr(), src.numel(), dst.data_ptr(), reps=passes)
            del src, dst

            def launch():
                _native.check(lib.zk_scan_resample_dev(dev, ptr(t_img), _native.ZK_F32, z, h, w, ptr(t_dx), ptr(t_dy), order, code, ptr(t_out),
                                                       ptr(scratch), scratch.numel(), c_void_p(stream)), "zk_scan_resample_dev")

            for _ in range(2):
                launch()
            torch.cuda.synchronize()
            times = []
            for _ in range(passes):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                torch.cuda.synchronize()
                times.append(a.elapsed_time(b))
            times = np.array(times)
            host = np.inf
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                out = denoise.apply_scan_noise(images, jx=1, jy=1, seed=11, order=order, mode=mode)
                host = min(host, time.perf_counter() - t0)
            same = np.array_equal(out, t_out.cpu().numpy())
            del out
            if args.no_scipy:
                cpu = "not measured"
            else:
                t0 = time.perf_counter()
                scipy_call(images, dx, dy, order, mode)
                cpu = f"{time.perf_counter() - t0:8.2f} s"
            print(f"{shape} order {order} | kernels (HIP events, {passes} passes) min {times.min():8.3f} median {np.median(times):8.3f} max "
                  f"{times.max():8.3f} ms | {BYTES_PER_PIXEL[order]} B/pixel = {total / 1e9:6.3f} GB -> {total / times.min() / 1e6:6.0f} GB/s at the "
                  f"minimum | plain copy of the same bytes {copy_ms:8.3f} ms = {total / copy_ms / 1e6:6.0f} GB/s | whole host call "
                  f"{host * 1e3:9.1f} ms (equal to the resident result: {same}) | SciPy, 3-D call, one thread: {cpu}", flush=True)
        del t_img, t_out, scratch


if __name__ == "__main__":
    main()
