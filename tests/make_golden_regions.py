#!/usr/bin/env python3
"""Generate tests/golden/regions_golden.npz from the REFERENCE's ``mtflearn/graph`` (``find_regions.py`` and ``utils.py``).

TEST INFRASTRUCTURE, run where a checkout of the reference is (``MTFLEARN_REFERENCE``, default: ``reference`` next to this
repository).  The two files import only NumPy and SciPy and each other; they are loaded by path under a stand-in package, so
``planar_graph.py`` (h5py, matplotlib through its mixins) is never imported.  No reference source is copied; the fixture is data
(integer and float arrays only).

Inputs are not stored: tests/regions_cases.py regenerates them.  Per case the file holds ``offsets`` / ``vertices`` / ``ks`` (the
polygons ``find_regions`` returned, in its order), ``centers`` (the reference's own expression, ``nodes[region].mean(axis=0)``
per polygon) and ``adjacency``.  The adjacency is NOT the output of the reference's ``_get_regions_graph_edges`` (that function
lives in the module that cannot be imported here): it is what that function is documented to give -- for every bond that two
polygon sides share, the pair of polygons -- computed here by counting, for every polygon side (v[t], v[t + 1]), the sides on
the same unordered bond, keeping the bonds met exactly twice, and stored sorted and in both directions.

Usage:  python tests/make_golden_regions.py
"""
import importlib.util
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("MTFLEARN_REFERENCE") or os.path.join(HERE, "..", "..", "reference")
OUT = os.path.join(HERE, "golden", "regions_golden.npz")
sys.path.insert(0, HERE)


def import_reference():
    sys.dont_write_bytecode = True
    folder = os.path.join(REF, "mtflearn", "graph")
    pkg = types.ModuleType("ref_graph")
    pkg.__path__ = [folder]
    sys.modules["ref_graph"] = pkg
    mods = {}
    for name in ("utils", "find_regions"):
        spec = importlib.util.spec_from_file_location(f"ref_graph.{name}", os.path.join(folder, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def shared_bonds(polys):
    """Pairs of polygons on the two sides of a bond, both directions, sorted: ``(2 A', 2)`` int64."""
    sides = {}
    for f, p in enumerate(polys):
        p = [int(v) for v in p]
        for a, b in zip(p, p[1:] + p[:1]):
            sides.setdefault((min(a, b), max(a, b)), []).append(f)
    pairs = {(f, g) for both in sides.values() if len(both) == 2 for f, g in (both, both[::-1])}
    return np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)


def main():
    import regions_cases as rc
    find_regions = import_reference()["find_regions"].find_regions
    out = {}
    inputs = dict(rc.cases())
    inputs.update({name: rc.kernel_cases()[name] for name in rc.GOLDEN_KERNEL_NAMES})     # the kernel-level cases it can reach
    for name, (pts, ijs) in inputs.items():
        t0 = time.perf_counter()
        polys = find_regions(pts, ijs)
        seconds = time.perf_counter() - t0
        polys = [np.asarray(p).astype(np.int64) for p in polys]
        ks = np.array([len(p) for p in polys], dtype=np.int64)
        out[f"{name}/offsets"] = np.concatenate([[0], np.cumsum(ks)]).astype(np.int64)
        out[f"{name}/vertices"] = np.concatenate(polys).astype(np.int64) if polys else np.empty(0, np.int64)
        out[f"{name}/ks"] = ks
        out[f"{name}/centers"] = np.array([pts[p.astype(int)].mean(axis=0) for p in polys], dtype=np.float64).reshape(-1, 2)
        out[f"{name}/adjacency"] = shared_bonds(polys)
        sizes = dict(zip(*np.unique(ks, return_counts=True)))
        print(f"{name}: {len(pts)} nodes, {len(ijs)} pairs -> {len(polys)} polygons {sizes}, reference {seconds:.3f} s")
        if name in rc.EXPECTED_FACES:
            assert len(polys) == rc.EXPECTED_FACES[name], (name, len(polys))
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
