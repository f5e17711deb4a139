#!/usr/bin/env python3
"""Times of ``ZPs.inverse_transform`` (csrc/zk_synth.hip) on one MI355X.

Per shape (size, n_max), row count and output type:
  kernel      HIP events around ``zk_synth_apply_dev`` on torch's current stream, median (and minimum) of ``--reps`` >= 10 launches
              after one warm-up; algorithmic bytes N (K^2 s_out + 8 P) over that time.
  resident    whole ``distributed.inverse_transform_device`` call on resident coefficients, output allocation included, ending in a
              device synchronise; host clock.
  NumPy       whole ``ZPs.inverse_transform`` call, NumPy array in, NumPy array out; host clock.
  host        NumPy's ``C @ T`` on this host with the same table, on ``--host-rows`` rows (the full product at 2^20 rows of 64 px
              takes minutes), as rows per second.
and once per run the bare stream rates of this box from ``zk_hbm_probe`` (what bench.py prints as ``roofline.this_box``): LDS-DMA
read stream and a 16-B-per-lane copy over 4 GiB.

``--pmc-case SIZE N_MAX ROWS DTYPE`` only launches that case's kernel a few times: the workload of a counter pass
(``rocprofv3 --pmc ... -- python time_inverse.py --pmc-case 32 8 1048576 float64``), which is a run of its own.

Usage:  python motif-learn_amd/tools/time_inverse.py [--reps 11] [--out profiles/inverse.txt]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

SHAPES = ((32, 8), (64, 12))
ROWS = (1 << 20, 1000)


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


def kernel_ms(synth, coeffs, out, code, reps):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    launch = lambda: synth.apply_dev(coeffs.data_ptr(), coeffs.shape[0], out.data_ptr(), code, stream)
    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return float(np.median(times)), float(min(times))


def case(z, rows, dtype, reps, host_rows, say):
    import torch
    from mtflearn_amd import _native, distributed
    size, p = z.size, len(z.n)
    px, item = size * size, np.dtype(dtype).itemsize
    entry = z._synthesis_entry("lstsq", None)
    synth = z._synthesis_device(entry)
    coeffs = np.random.default_rng(rows + size).standard_normal((rows, p))
    d_coeffs = torch.from_numpy(coeffs).cuda()
    d_out = torch.empty((rows, px), dtype=torch.float64 if item == 8 else torch.float32, device="cuda")
    k_med, k_min = kernel_ms(synth, d_coeffs, d_out, _native.dtype_code(np.dtype(dtype)), reps)
    check = slice(0, min(rows, 64))
    err = np.abs(d_out[check].cpu().numpy().astype(np.float64) - coeffs[check] @ entry["table"]).max()
    nbytes = rows * (px * item + 8 * p)
    head = f"({size:2d}, {z.n_max:2d}) {rows:8d} rows {np.dtype(dtype).name}:"
    say(f"{head} kernel {k_med:9.4f} ms median (min {k_min:.4f}) of {reps} | {nbytes / 1e9:7.3f} GB algorithmic -> "
        f"{nbytes / k_med / 1e6:7.1f} GB/s | {2.0 * rows * px * p / k_med / 1e9:7.2f} TFLOP/s FP64 (2 N K^2 P) | "
        f"first rows against NumPy: max |diff| {err:.1e}")
    del d_out
    r_med, r_min = median_ms(lambda: distributed.inverse_transform_device(z, d_coeffs, dtype=dtype), reps, torch.cuda.synchronize)
    whole_reps = 3 if rows * px * item > (1 << 30) else reps
    try:
        n_med, n_min = median_ms(lambda: z.inverse_transform(coeffs, dtype=dtype), whole_reps, torch.cuda.synchronize)
        whole = f"NumPy to NumPy {n_med:10.2f} ms (min {n_min:.2f}) of {whole_reps}"
    except (MemoryError, RuntimeError) as exc:
        whole = f"NumPy to NumPy not measured ({type(exc).__name__}: {exc})"
    _native.pinned.trim()
    sub = coeffs[:min(rows, host_rows)]
    table = entry["table"]
    h_med, _ = median_ms(lambda: (sub @ table).astype(dtype, copy=False), 3, lambda: None)
    say(f"{head} whole call resident {r_med:9.3f} ms (min {r_min:.3f}) of {reps} | {whole} | NumPy C @ T on this host: "
        f"{len(sub)} rows in {h_med:.2f} ms = {len(sub) / h_med * 1e3:.3e} rows/s (kernel: {rows / k_med * 1e3:.3e} rows/s)")


def this_box(say):
    import torch
    from mtflearn_amd import _native
    nbytes = 4 << 30
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ms_read = _native.hbm_probe(0, src.data_ptr(), nbytes)
    ms_copy = _native.hbm_probe(0, src.data_ptr(), nbytes, dst_ptr=dst.data_ptr())
    say(f"this box, zk_hbm_probe over 4 GiB (HIP events): LDS-DMA read stream {nbytes / ms_read / 1e6:.0f} GB/s, 16-B-per-lane copy "
        f"{2 * nbytes / ms_copy / 1e6:.0f} GB/s read + written ({nbytes / ms_copy / 1e6:.0f} GB/s of stores beside as many loads)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--host-rows", type=int, default=1 << 14)
    ap.add_argument("--pmc-case", nargs=4, metavar=("SIZE", "N_MAX", "ROWS", "DTYPE"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    from mtflearn_amd import ZPs, _native
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    if args.pmc_case:
        size, n_max, rows = (int(v) for v in args.pmc_case[:3])
        dtype = np.dtype(args.pmc_case[3])
        z = ZPs(n_max=n_max, size=size)
        synth = z._synthesis_device(z._synthesis_entry("lstsq", None))
        d_coeffs = torch.from_numpy(np.random.default_rng(0).standard_normal((rows, len(z.n)))).cuda()
        d_out = torch.empty((rows, size * size), dtype=torch.float64 if dtype.itemsize == 8 else torch.float32, device="cuda")
        for _ in range(3):
            synth.apply_dev(d_coeffs.data_ptr(), rows, d_out.data_ptr(), _native.dtype_code(dtype), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return 0
    say(f"ZPs.inverse_transform (method lstsq, all terms) on {torch.cuda.get_device_name(0)}; kernel times from HIP events, whole calls on "
        f"the host clock ending in a device synchronise; medians after one warm-up; profiler off.")
    this_box(say)
    for size, n_max in SHAPES:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            z = ZPs(n_max=n_max, size=size)
        table = z._synthesis_entry("lstsq", None)["table"]
        say(f"({size}, {n_max}): P = {len(z.n)}, K^2 = {size * size}, table {table.nbytes / 1024:.0f} KiB, cond(G) = "
            f"{z._synthesis_entry('lstsq', None)['cond']:.3g}")
        for rows in ROWS:
            for dtype in (np.float64, np.float32):
                case(z, rows, dtype, args.reps, args.host_rows, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
