#!/usr/bin/env python3
"""Generate tests/golden/align_maps_golden.npz: the patches of the end-to-end alignment-map tests, drawn by the REFERENCE's
``mtflearn/datasets/_generate_data_gn.py`` (pure NumPy; the package's own generator renders on the GPU, and
tests/test_align_maps_cpu.py runs without one).

TEST INFRASTRUCTURE, run where the reference checkout is (REF below).  No reference source is copied; the fixture is data: one
24 x 24 float64 patch per entry of align_maps_cases.PATCHES.

Usage:  python tests/make_golden_align_maps.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "golden", "align_maps_golden.npz")
sys.path.insert(0, HERE)


def main():
    import align_maps_cases as mc
    sys.dont_write_bytecode = True
    path = os.path.join(REF, "mtflearn", "datasets", "_generate_data_gn.py")
    spec = importlib.util.spec_from_file_location("ref_generate_data_gn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {name: np.asarray(mod.generate_data_gn(size=mc.SIZE, **kw), dtype=np.float64) for name, kw in mc.PATCHES.items()}
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
