#!/usr/bin/env python3
"""Generate tests/golden/scan_noise_golden.npz from the REFERENCE's ``mtflearn/denoise/_noise_models.py``.

TEST INFRASTRUCTURE, run where a checkout of the reference is: its path is the one argument (or ``MTFLEARN_REFERENCE``).  The
file is loaded by path under a stub module name, so neither the reference's package ``__init__`` files nor their optional
dependencies are imported.  No reference source is copied; the fixture is data (arrays only).

Per shape of ``scan_noise_cases.GOLDEN_SHAPES`` the file holds the float64 input (``<shape>/images``; its float32 cast is exact),
the seeds of the jitters (``<shape>/seeds``) and the draws as the reference forms them (``<shape>/dx`` (J, Z, H), ``<shape>/dy``
(J, Z, W)), and per dtype one array ``<shape>/<dtype>`` (P, J, Z, H, W) of the reference's outputs for the 3-D stack, in the
input's dtype: axis 0 runs over ``scan_noise_cases.GOLDEN_PAIRS``, axis 1 over ``GOLDEN_JITTERS`` (one array per dtype keeps
the archive's per-entry overhead out of the size budget; ``scan_noise_cases.golden_output`` indexes it).
Orders 0 and 1 with all six modes, order 3 with 'mirror' and 'grid-wrap'.  No order 3 'reflect' case is recorded: there the
reference's 3-D call is not the interpolant it documents on short axes (see ``apply_scan_noise``'s docstring).

Usage:  python tests/make_golden_scan_noise.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "scan_noise_golden.npz")
sys.path.insert(0, HERE)


def import_reference(root):
    sys.dont_write_bytecode = True
    path = os.path.join(root, "mtflearn", "denoise", "_noise_models.py")
    spec = importlib.util.spec_from_file_location("ref_noise_models", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_draws(seed, shape, jx, jy):
    """The draws as the reference's function body forms them (restated here: the function does not return them)."""
    z, h, w = shape
    rng = np.random.default_rng(seed=seed)
    dx = rng.normal(0, 1, (z, h, 1)) * jx
    dy = rng.normal(0, 1, (z, 1, w)) * jy
    return dx.reshape(z, h), dy.reshape(z, w)


def main():
    import scan_noise_cases as sc
    root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("MTFLEARN_REFERENCE")
    if not root:
        sys.exit(__doc__)
    ref = import_reference(root)
    out = {}
    jitters = list(enumerate(sc.GOLDEN_JITTERS))
    for shape in sc.GOLDEN_SHAPES:
        sid = sc.shape_id(shape)
        out[f"{sid}/images"] = sc.images(shape)
        out[f"{sid}/seeds"] = np.array([sc.seed_of(shape, k) for k, _ in jitters], dtype=np.int64)
        draws = [reference_draws(sc.seed_of(shape, k), shape, jx, jy) for k, (jx, jy) in jitters]
        out[f"{sid}/dx"], out[f"{sid}/dy"] = np.stack([d[0] for d in draws]), np.stack([d[1] for d in draws])
        for dtype in sc.DTYPES:
            stack = sc.images(shape).astype(dtype)
            results = np.empty((len(sc.GOLDEN_PAIRS), len(jitters)) + shape, dtype=dtype)
            for p, (order, mode) in enumerate(sc.GOLDEN_PAIRS):
                for k, (jx, jy) in jitters:
                    got = ref.apply_scan_noise(stack, jx=jx, jy=jy, seed=sc.seed_of(shape, k), order=order, mode=mode)
                    assert got.dtype == stack.dtype and got.shape == stack.shape and np.isfinite(got).all(), (shape, dtype, order, mode, k)
                    results[p, k] = got
            out[f"{sid}/{np.dtype(dtype).name}"] = results
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 300 * 1024, f"{OUT} is {size} bytes"
    print(f"wrote {OUT}: {len(out)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
