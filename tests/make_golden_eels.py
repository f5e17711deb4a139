#!/usr/bin/env python3
"""Generate tests/golden/eels_golden.npz from the REFERENCE's ``mtflearn/eels/_baseline_correction.py``.

TEST INFRASTRUCTURE, run where the reference checkout is (REF below).  The file is loaded by path.  It uses ``np`` without
importing it, so it cannot be called as shipped: ``module.np = numpy`` is set after loading.  No reference source is copied;
the fixture is data (arrays only).

Inputs are not stored: tests/eels_cases.py regenerates them.  Per case ``<config>/<shape>`` the file holds

* ``.../ref``            the reference's baselines, one spectrum at a time, on the float64 cube;
* ``.../iters``          the solves each spectrum took in the host statement (tests/eels_oracle.py), int32 -- the reference does
                         not expose them;
* ``.../ref_vs_oracle``  ``max|ref - oracle| / max|y|``: the distance between two backward-stable solves of the same systems,
                         which scales the tolerance of the GPU parity test.

Asserted here, because the cases mean nothing otherwise: every airPLS spectrum converges before itermax in the statement; at
least one arPLS batch has spectra with different iteration counts; over all ALS iterations ``min|y - z| >= 1e-9 max|y|`` (no
hard-threshold weight sits on a rounding edge; stored as ``.../als_gap``).

Usage:  python tests/make_golden_eels.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "golden", "eels_golden.npz")
sys.path.insert(0, HERE)


def import_reference():
    sys.dont_write_bytecode = True
    path = os.path.join(REF, "mtflearn", "eels", "_baseline_correction.py")
    spec = importlib.util.spec_from_file_location("ref_baseline_correction", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.np = np                       # the file uses np without importing it
    return mod


def main():
    import eels_cases as ec
    import eels_oracle as eo
    ref = import_reference()
    ref_fn = {"als": ref.baseline_als, "arpls": ref.baseline_arpls, "airpls": ref.baseline_airpls, "snip": ref.baseline_snip}
    out, arpls_varied, worst = {}, False, {}
    for key, name, L, grid in ec.cases():
        method, kw, _ = ec.CONFIGS[name]
        cube = ec.cube(L, grid)
        flat = cube.reshape(L, -1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            golden = np.stack([np.asarray(ref_fn[method](flat[:, j].copy(), **kw), np.float64).reshape(L) for j in range(flat.shape[1])],
                              axis=1).reshape(cube.shape)
        base, iters, *rest = eo.over_axis(eo.METHODS[method], cube, 0, **kw)
        scale = np.abs(cube).max()
        dist = float(np.abs(golden - base).max() / scale)
        assert np.isfinite(golden).all() and np.isfinite(base).all(), key
        out[f"{key}/ref"] = golden
        out[f"{key}/iters"] = iters.astype(np.int32)
        out[f"{key}/ref_vs_oracle"] = np.float64(dist)
        worst[name] = max(worst.get(name, 0.0), dist)
        if method == "airpls":
            assert (iters < 100).all(), f"{key}: an airPLS spectrum ran to itermax"
        if method == "arpls":
            arpls_varied |= len(np.unique(iters)) > 1
        if method == "als":
            gap = float((rest[0] / np.abs(flat).max(axis=0).reshape(grid)).min())
            assert gap >= 1e-9, f"{key}: |y - z| came within {gap:.2e} max|y| of a hard threshold"
            out[f"{key}/als_gap"] = np.float64(gap)
    assert arpls_varied, "no arPLS batch has spectra with different iteration counts"
    np.savez_compressed(OUT, **out)
    for name, dist in worst.items():
        print(f"{name:10s} largest ref_vs_oracle {dist:.2e}")
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
