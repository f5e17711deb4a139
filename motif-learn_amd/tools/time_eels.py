#!/usr/bin/env python3
"""Times of mtflearn_amd.eels on one GPU (profiles/eels.txt): every estimator on a (1024, 256, 256) float32 cube and on a
(2048, 64, 64) one (the small scan is 64 waves on a 256-CU chip: latency-bound by construction, measured and stated as such).

Per estimator and cube: the whole call NumPy to NumPy; the resident call (host clock around a call that ends in a stream
synchronisation) and its device time from HIP events; the solves actually run; the algorithmic bytes of those solves over the
device time, beside this box's measured copy rate (zk_hbm_probe, 16 B per lane); and the host statement (tests/eels_oracle.py)
timed on 64 spectra of the same cube and SCALED to the cube -- stated as scaled.

Algorithmic bytes per sample and solve, K the difference order (float64 planes; what the sweeps of csrc/zk_eels.hip read and
write): forward y + previous z or w + K + 1 factor planes out; backward K + 1 planes in + z out (+ y for the statistics);
arPLS's weight sweep y + z + w in + w out.  SNIP: one plane in, one out per pass (the two neighbour reads hit the caches).

    python tools/time_eels.py [--small-only] [--methods als,snip,...] [--repeat 2]

The prefetch depth is compile-time (ZK_EELS_PF in csrc/zk_eels.hip); another depth is timed by building the library with
-DZK_EELS_PF=<n> and pointing MTFLEARN_AMD_LIB at it.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))

KW = {"als": {}, "arpls": {}, "airpls": {"porder": 1}, "snip": {}}
ORDER = {"als": 2, "arpls": 2, "airpls": 1}


def bytes_per_solve(method, k):
    if method == "als":
        return 8 + 8 + 8 * (k + 1) + 8 * (k + 1) + 8
    if method == "airpls":
        return 8 + 8 + 8 * (k + 1) + 8 * (k + 1) + 8 + 8
    return 8 + 8 + 8 * (k + 1) + 8 * (k + 1) + 8 + 8 + 32


def cube_of(shape, seed):
    """Power law, four edges, Poisson counts, float32 (exact), built plane by plane to keep the host footprint small."""
    rng = np.random.RandomState(seed)
    L, n = shape[0], int(np.prod(shape[1:]))
    e = ((np.arange(L) + 0.5) / L)[:, None]
    amp, expo = rng.uniform(3e4, 5.5e4, n)[None, :], rng.uniform(0.3, 1.0, n)[None, :]
    out = np.empty((L, n), np.float32)
    step = 64
    for c0 in range(0, L, step):
        ee = e[c0:c0 + step]
        lam = amp * (1.0 + 3.0 * ee) ** (-expo)
        for centre in (0.2, 0.4, 0.6, 0.8):
            lam += 0.15 * amp * np.exp(-0.5 * ((ee - centre) / 0.03) ** 2)
        out[c0:c0 + step] = rng.poisson(lam)
    return out.reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--methods", default="snip,als,arpls,airpls")
    ap.add_argument("--repeat", type=int, default=2)
    args = ap.parse_args()
    import torch
    import eels_oracle as eo
    from mtflearn_amd import _native, eels, resident

    _native.load()
    _native.require_device()
    dev = _native.default_device()
    print(f"library {_native.LIB_PATH}")
    probe = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(probe)
    ms = _native.hbm_probe(dev, probe.data_ptr(), probe.numel(), dst.data_ptr())
    copy_rate = 2 * probe.numel() / ms / 1e6                    # bytes per ms -> GB/s
    print(f"copy rate of this box (zk_hbm_probe, 256 MiB, read + write): {copy_rate:.0f} GB/s")
    del probe, dst
    shapes = [(2048, 64, 64)] + ([] if args.small_only else [(1024, 256, 256)])
    warm = cube_of((256, 8, 8), 1)
    for method in args.methods.split(","):
        eels.remove_baseline(warm, method=method, **KW[method])
    for shape in shapes:
        cube = cube_of(shape, 7)
        L, n = shape[0], shape[1] * shape[2]
        t = torch.from_numpy(cube).cuda()
        for method in args.methods.split(","):
            kw = KW[method]
            best = {"host": np.inf, "resident": np.inf, "device": np.inf}
            for _ in range(args.repeat):
                t0 = time.perf_counter()
                fn = getattr(eels, "baseline_" + method)
                out = fn(cube, return_info=True, **kw) if method in ("arpls", "airpls") else fn(cube, **kw)
                best["host"] = min(best["host"], time.perf_counter() - t0)
                del out
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                res = resident.baseline_device(t, method, return_info=True, **kw)
                b.record()
                torch.cuda.synchronize()
                best["resident"] = min(best["resident"], time.perf_counter() - t0)
                best["device"] = min(best["device"], a.elapsed_time(b) / 1e3)
            iters = res[1].cpu().numpy() if res[1] is not None else None
            del res
            if method == "snip":
                solves, total = 10.0, 16.0 * 10 * L * n
                what = "10 passes"
            else:
                if iters is None:
                    iters = np.full(n, 10)
                solves = float(iters.mean())
                total = float(iters.sum()) * L * bytes_per_solve(method, ORDER[method])
                what = f"solves mean {solves:.2f} max {int(iters.max())}"
            sample = cube.reshape(L, n)[:, :: max(1, n // 64)][:, :64].astype(np.float64)
            t0 = time.perf_counter()
            for j in range(sample.shape[1]):
                eo.METHODS[method](sample[:, j], **kw)
            oracle = (time.perf_counter() - t0) / sample.shape[1] * n
            print(f"{shape} {method:7s} whole call {best['host'] * 1e3:9.2f} ms | resident {best['resident'] * 1e3:9.2f} ms | device (HIP events) "
                  f"{best['device'] * 1e3:9.2f} ms | {what} | algorithmic {total / 1e9:8.1f} GB -> {total / best['device'] / 1e9:7.0f} GB/s "
                  f"(copy rate {copy_rate:.0f}) | host statement, 64 spectra SCALED to the cube: {oracle:9.1f} s", flush=True)
        del t


if __name__ == "__main__":
    main()
