#!/usr/bin/env python3
"""Whole-call times of ``distributed.vnn_graph_device`` on jittered honeycombs (bond length 12 px, the inputs of
tools/time_regions.py), beside the host route on the same input: ``scipy.spatial.Voronoi`` of the padded points plus the sparse
steps of the reference's ``vnn_graph`` restated with NumPy / SciPy, on the CPU of the same machine.  The two pair lists are
compared (recorded, not asserted: on a point set nobody conditioned, a fraction may sit within rounding of the threshold).
Also recorded: the shader and memory clocks ``rocm-smi --showclocks`` reports before and after the timed loops, the device's
ridge lengths against the qhull goldens of tests/vnn_cases.py, and, with ``--launch-traces SIZE:DB ...``, the kernel dispatches
per call counted in ``rocprofv3 --kernel-trace`` databases of runs made as ``--sizes SIZE --reps 1 --no-host --no-accuracy``
(two calls each; tracing is a run of its own, never the timed one).

Usage:  python motif-learn_amd/tools/time_vnn.py [--sizes 512 2048 4096] [--reps 7] [--no-host] [--no-accuracy]
                                                 [--launch-traces SIZE:DB ...] [--out FILE]
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "..", "tests")):
    sys.path.insert(0, os.path.abspath(p))


def host_route(pts, dmax, threshold=0.1):
    """qhull and the reference's sparse steps; ``(pairs, seconds in Voronoi, seconds after it)``."""
    from scipy.sparse import coo_matrix
    from scipy.spatial import Voronoi
    from mtflearn_amd.graph import add_corner_points
    t0 = time.perf_counter()
    vor = Voronoi(add_corner_points(pts))
    t1 = time.perf_counter()
    rv, rp, n = np.asarray(vor.ridge_vertices), np.asarray(vor.ridge_points), len(pts)
    d = vor.vertices[rv[:, 0]] - vor.vertices[rv[:, 1]]
    e = vor.points[rp[:, 0]] - vor.points[rp[:, 1]]
    keep = (np.hypot(e[:, 0], e[:, 1]) < dmax) & (rv >= 0).all(axis=1)
    length, rp = np.hypot(d[:, 0], d[:, 1])[keep], rp[keep]
    m = coo_matrix((np.concatenate([length, length]), (np.concatenate([rp[:, 0], rp[:, 1]]), np.concatenate([rp[:, 1], rp[:, 0]]))),
                   shape=(n + 4, n + 4)).tocsr()
    sums = np.asarray(m.sum(axis=1)).ravel()
    m = m.tocoo()
    kept = (m.data / sums[m.row] >= threshold) & (m.row < n) & (m.col < n)
    pairs = np.unique(np.concatenate([np.stack([m.row[kept], m.col[kept]], 1), np.stack([m.col[kept], m.row[kept]], 1)]), axis=0)
    return pairs.astype(np.int64), t1 - t0, time.perf_counter() - t1


def clocks():
    """The sclk / mclk lines of ``rocm-smi --showclocks`` for the first device (read only), or why there are none."""
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
    except Exception as e:                                               # noqa: BLE001 -- a missing tool is recorded, not fatal
        return f"not read ({type(e).__name__})"
    keep = [line.split(":", 1)[-1].strip() for line in out.splitlines() if "GPU[0]" in line and ("sclk" in line or "mclk" in line)]
    return "; ".join(keep) if keep else "not reported"


def launches_per_call(db, calls=2):
    """Kernel dispatches in a rocprofv3 database (its ``kernels`` view) over the ``calls`` calls the traced run made; the
    runtime's own copy and fill kernels count, they are part of the call."""
    import sqlite3
    with sqlite3.connect(db) as con:
        total = con.execute("select count(*) from kernels").fetchone()[0]
        cells = con.execute("select max(end - start) / 1e6 from kernels where name like '%cell_kernel%'").fetchone()[0]
    return total / calls, cells


def accuracy():
    """Largest difference between the device's ridge lengths and the qhull goldens over the cases of tests/vnn_cases.py, in
    units of each case's median edge length; and whether every pair list is the golden's."""
    import torch
    import vnn_cases as vc
    from mtflearn_amd import distributed
    with np.load(os.path.join(HERE, "..", "..", "tests", "golden", "vnn_golden.npz")) as f:
        golden = {k: f[k] for k in f.files}
    worst, where, same = 0.0, "", True
    for name, (pts, _, _) in vc.cases().items():
        ijs, ridge, _ = (a.cpu().numpy() for a in distributed.voronoi_neighbours_device(torch.from_numpy(pts.copy()).cuda()))
        same = same and np.array_equal(ijs, golden[f"{name}/nb_ijs"])
        if same and len(ridge):
            err = float(np.abs(ridge - golden[f"{name}/nb_ridge"]).max() / golden[f"{name}/a"])
            worst, where = (err, name) if err > worst else (worst, where)
    return worst, where, same, float(golden["d0"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 2048, 4096])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--launch-traces", nargs="*", default=[], metavar="SIZE:DB")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import regions_cases as rc
    from mtflearn_amd import distributed
    lines = [f"vnn_graph_device, whole call (two phases, row counts read back), median of {args.reps} after one warm-up; "
             f"device {torch.cuda.get_device_name(0)}; jittered honeycomb, l = 12, dmax = 1.3 l, threshold = 0.1",
             "conditions: points resident as a float64 torch tensor; the call runs both phases, allocates and frees every working buffer "
             "inside it, reads the error flags and row counts back (two stream synchronisations) and allocates the result; host clock "
             "around the call with a device synchronise on both sides; profiler off.  Not kernel times.",
             f"clocks before the timed loops (rocm-smi --showclocks, device 0): {clocks()}"]
    for size in args.sizes:
        pts = rc.honeycomb(size, 12.0, 11)
        dmax = 1.3 * 12.0
        d_pts = torch.from_numpy(pts).cuda()
        got = distributed.vnn_graph_device(d_pts, dmax).cpu().numpy()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            distributed.vnn_graph_device(d_pts, dmax)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        line = (f"size {size:5d}: {len(pts):6d} points {len(got):7d} directed bonds | device {1e3 * float(np.median(times)):8.2f} ms "
                f"(min {1e3 * min(times):.2f})")
        if not args.no_host:
            ref, t_qhull, t_sparse = host_route(pts, dmax)
            line += (f" | host route {1e3 * (t_qhull + t_sparse):9.1f} ms (scipy.spatial.Voronoi {1e3 * t_qhull:.1f}, sparse steps "
                     f"{1e3 * t_sparse:.1f}) | device == host route: {np.array_equal(got, ref)}")
        lines.append(line)
        print(line, flush=True)
    lines.append(f"clocks after the timed loops: {clocks()}")
    for item in args.launch_traces:
        size, db = item.split(":", 1)
        per_call, cell_ms = launches_per_call(db)
        lines.append(f"size {int(size):5d}: {per_call:.1f} kernel dispatches per call (rocprofv3 --kernel-trace, a run of its own, two calls; the "
                     f"runtime's copy and fill kernels included); the longest, cell_kernel, {cell_ms:.2f} ms under the tracer")
    if not args.no_accuracy:
        worst, where, same, d0 = accuracy()
        lines.append(f"accuracy: voronoi_neighbours_device against the qhull goldens on the {len(__import__('vnn_cases').NAMES)} cases of "
                     f"tests/vnn_cases.py: pairs equal: {same}; ridge lengths differ by at most {worst:.2e} a ({where}), a = the case's median "
                     f"edge length; qhull against the brute-force oracle differs by d0 = {d0:.2e} a")
    for line in lines[len(lines) - 2 - len(args.launch_traces):]:
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
