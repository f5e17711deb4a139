#!/usr/bin/env python3
"""Generate tests/golden/tmd_golden.npz from the REFERENCE's ``mtflearn/datasets/_tmd_simulator.py``.

TEST INFRASTRUCTURE, run where a checkout of the reference is: its path is the one argument (or ``MTFLEARN_REFERENCE``).  The
file is loaded by path under a stub module name, so neither the reference's package ``__init__`` files nor their optional
dependencies are imported.  No reference source is copied; the fixture is data (arrays only).

Per case of ``tmd_cases.CASES`` the file holds the host side after ``simulate`` (``<case>/...``, see ``tmd_cases.host_record``;
``pts_all`` in full up to ``PTS_ALL_IN_FULL`` sites, its SHA-256 always), and per mode (``fft`` / ``gauss``) the float32 image
``<case>/<mode>/image``, the delta images ``<case>/<mode>/masks`` (S, H, W) and ``<case>/<mode>/species``: the order in which THIS
run of the reference walked its unordered set of species, which is the order of the masks and of the float32 accumulation.
``<case>/fft/e_ref`` is ``max |image - E|`` with E the exact float64 convolution of the recorded masks (tests/tmd_oracle.py):
how far the reference's single-precision transform is from what it approximates.

Usage:  python tests/make_golden_tmd.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def import_reference(root):
    sys.dont_write_bytecode = True
    path = os.path.join(root, "mtflearn", "datasets", "_tmd_simulator.py")
    spec = importlib.util.spec_from_file_location("ref_tmd_simulator", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import tmd_cases as tc
    import tmd_oracle as to
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MTFLEARN_REFERENCE")
    if not root:
        sys.exit(__doc__)
    ref = import_reference(root)
    out = {}
    for name in tc.CASES:
        for mode, use_fft in tc.MODES.items():
            sim = tc.build(ref.TMDImageSimulator, name, use_fft)
            image, masks = sim.simulate(return_masks=True)
            species = list(masks)                       # the order of this run's walk
            assert image.dtype == np.float32 and sorted(species) == sorted(tc.species_of(name)), (name, mode)
            out[f"{name}/{mode}/image"] = image
            out[f"{name}/{mode}/masks"] = np.stack([masks[s] for s in species])
            out[f"{name}/{mode}/species"] = np.array(species, dtype="U8")
            if use_fft:
                E = to.exact_image([masks[s] for s in species], [tc.params_of(name, s) for s in species])
                out[f"{name}/fft/e_ref"] = np.array(np.abs(image.astype(np.float64) - E).max())
                print(f"case {name}: e_ref = {float(out[f'{name}/fft/e_ref']):.3e} at peak {E.max():.4f}, species order {species}")
            record = tc.host_record(sim)
            for key, value in record.items():
                if f"{name}/{key}" in out:              # the host side does not depend on the mode
                    assert np.array_equal(out[f"{name}/{key}"], value), (name, key)
                out[f"{name}/{key}"] = value
    np.savez_compressed(tc.GOLDEN, **out)
    size = os.path.getsize(tc.GOLDEN)
    assert size < 300 * 1024, f"{tc.GOLDEN} is {size} bytes"
    print(f"wrote {tc.GOLDEN}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
