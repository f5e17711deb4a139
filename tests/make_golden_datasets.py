#!/usr/bin/env python3
"""Generate tests/golden/datasets_golden.npz from the REFERENCE's ``mtflearn/datasets`` (``_tapered_gaussian.py``,
``_honeycomb_lattice.py``, ``_zps_test_data.py``, ``_generate_data_gn.py``, ``_noise_models.py``).

TEST INFRASTRUCTURE, run where the reference checkout is (REF below).  The five files import only NumPy and each other; they
are loaded by path under a stand-in package, so the rest of the reference's ``datasets/__init__.py`` is never imported.  No
reference source is copied; the fixture is data (arrays and scalars only).

Inputs are not stored: tests/datasets_cases.py regenerates them.  Frames are at most 96 x 96 and patches 33 x 33.

The script also confirms, with the reference's renderer and tests/local_max_oracle.py, the statement the ground-truth test of
tests/test_gpu_datasets.py makes about the device chain (every interior lattice site has exactly one detected point within
1 px and every interior detected point has a site within 1 px), at the parameters in datasets_cases.TRUTH.

Usage:  python tests/make_golden_datasets.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "golden", "datasets_golden.npz")
sys.path.insert(0, os.path.join(HERE, "..", "motif-learn_amd"))
sys.path.insert(0, HERE)


def import_reference():
    sys.dont_write_bytecode = True
    folder = os.path.join(REF, "mtflearn", "datasets")
    pkg = types.ModuleType("ref_datasets")
    pkg.__path__ = [folder]
    sys.modules["ref_datasets"] = pkg
    mods = {}
    for name in ("_tapered_gaussian", "_honeycomb_lattice", "_zps_test_data", "_generate_data_gn", "_noise_models"):
        spec = importlib.util.spec_from_file_location(f"ref_datasets.{name}", os.path.join(folder, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods


def truth_statement(points, sites, size, margin):
    """(interior sites without exactly one point within 1 px, interior points without a site within 1 px, and how many of
    each there are); interior: farther than ``margin`` from the border."""
    def interior(p):
        return (p[:, 0] > margin) & (p[:, 0] < size - 1 - margin) & (p[:, 1] > margin) & (p[:, 1] < size - 1 - margin)
    d = np.hypot(sites[:, None, 0] - points[None, :, 0], sites[:, None, 1] - points[None, :, 1])
    s_in, p_in = interior(sites), interior(points)
    bad_sites = int((((d <= 1.0).sum(axis=1) != 1) & s_in).sum())
    bad_points = int(((d.min(axis=0) > 1.0) & p_in).sum())
    return bad_sites, bad_points, int(s_in.sum()), int(p_in.sum())


def main():
    import datasets_cases as dc
    ref = import_reference()
    atg = ref["_tapered_gaussian"].add_tapered_gaussian
    Lattice = ref["_honeycomb_lattice"].HoneyCombLattice
    noise = ref["_noise_models"]
    out = {}
    for name, case in dc.render_cases().items():
        for dtype in dc.DTYPES:
            out[f"render/{name}/{np.dtype(dtype).name}"] = atg(dc.case_frame(case, dtype), case["pts"], case["sigma"], case["amps"],
                                                              case["r_factor"])
    for name, amplitudes in dc.ORDER_AMPLITUDES.items():
        case = dc.order_case(amplitudes)
        out[f"order/{name}"] = atg(dc.case_frame(case, np.float32), case["pts"], case["sigma"], case["amps"], case["r_factor"])
    assert out["order/big_one_minus"][5, 6] != out["order/big_minus_one"][5, 6], "the two orders must differ"
    for name, (ctor, kw) in dc.LATTICES.items():
        lat = Lattice(**ctor)
        out[f"lattice/{name}/image"] = lat.to_image(**kw)
        out[f"lattice/{name}/coords_A"], out[f"lattice/{name}/coords_B"] = lat._coords_A, lat._coords_B
        out[f"lattice/{name}/points_A"], out[f"lattice/{name}/points_B"] = lat.get_points()
    lat = Lattice(size=40, l=7.5, angle=3.0, random_shift=False)
    lat.set_angle(-21.0)
    out["lattice/set_angle/points_A"], out["lattice/set_angle/points_B"] = lat.get_points()
    for name, kw in dc.PATCHES.items():
        out[f"patches/{name}"] = ref["_zps_test_data"].get_zps_test_patches(**kw)
    for name, kw in dc.DATA_GN.items():
        out[f"data_gn/{name}"] = ref["_generate_data_gn"].generate_data_gn(**kw)
    img = dc.noise_image()
    out["noise/poisson"], out["noise/poisson_counts"] = noise.apply_poisson_noise(img, 50.0, return_counts=True, seed=3)
    out["noise/gaussian"] = noise.add_gaussian_noise(img, sigma=0.2, seed=4)
    out["noise/poisson_gaussian"] = noise.apply_poisson_gaussian_noise(img, 80.0, 0.05, seed=5)
    out["noise/mle"] = np.float64(noise.estimate_counts_per_pixel_mle(out["noise/poisson"], img))
    out["noise/mle_mask"] = np.float64(noise.estimate_counts_per_pixel_mle(out["noise/poisson"], img, mask=img > 0.5, s_min=0.1))

    # the ground-truth statement, on the CPU, with the reference's renderer and the project's local_max oracle
    from local_max_oracle import local_max_raster as local_max_oracle
    lat = Lattice(**dc.TRUTH["lattice"])
    frame = lat.to_image()
    sites = np.concatenate(lat.get_points())
    points = np.asarray(local_max_oracle(frame, dc.TRUTH["min_distance"]), dtype=np.float64).reshape(-1, 2)
    margin = 3 * (lat.l / 4.0) + 1
    bad_sites, bad_points, n_sites, n_points = truth_statement(points, sites, lat.size, margin)
    print(f"ground truth at {dc.TRUTH}: {n_sites} interior sites, {n_points} interior points, {bad_sites} sites and "
          f"{bad_points} points off")
    assert bad_sites == 0 and bad_points == 0 and n_sites > 100

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
