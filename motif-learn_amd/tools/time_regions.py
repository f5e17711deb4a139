#!/usr/bin/env python3
"""Whole-call times of ``distributed.find_regions_device`` on jittered honeycombs (bond length 12 px), beside the host oracle
(tests/regions_oracle.py, a linear-time walk in Python) on the same input, whose result the device's must equal exactly.

Usage:  python motif-learn_amd/tools/time_regions.py [--sizes 512 2048 4096] [--reps 7] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "tests")):
    sys.path.insert(0, os.path.abspath(p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import regions_cases as rc
    import regions_oracle as oracle
    from mtflearn_amd import distributed, graph
    lines = [f"find_regions_device, whole call (two phases, counts read back), median of {args.reps} after one warm-up; "
             f"device {torch.cuda.get_device_name(0)}; jittered honeycomb, l = 12"]
    for size in args.sizes:
        pts = rc.honeycomb(size, 12.0, 11)
        ijs = rc.bonds(pts, 1.3 * 12.0)
        gap, edge = rc.conditioning(pts, ijs)
        t0 = time.perf_counter()
        ref = oracle.regions(pts, ijs)
        t_oracle = time.perf_counter() - t0
        d_pts, d_ijs = torch.from_numpy(pts).cuda(), torch.from_numpy(ijs).cuda()
        got = distributed.find_regions_device(d_pts, d_ijs)
        equal = (all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(got[:3], ref[:3])) and
                 got[3].cpu().numpy().tobytes() == ref[3].tobytes() and
                 oracle.symmetrised(got[4].cpu().numpy()) == oracle.symmetrised(ref[4]))
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            distributed.find_regions_device(d_pts, d_ijs)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        graph.find_regions(pts, ijs)
        t_host_call = time.perf_counter() - t0
        lines.append(f"size {size:5d}: {len(pts):6d} nodes {len(ijs):7d} directed bonds {len(ref[2]):6d} polygons "
                     f"(min angle gap {gap:.1e}) | device {1e3 * float(np.median(times)):8.2f} ms (min {1e3 * min(times):.2f}) | "
                     f"find_regions from host arrays incl. the object array {1e3 * t_host_call:8.1f} ms | host oracle {1e3 * t_oracle:9.1f} ms | "
                     f"device == oracle: {equal}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all("device == oracle: True" in line for line in lines[1:]) else 1


if __name__ == "__main__":
    sys.exit(main())
