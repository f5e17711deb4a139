#!/usr/bin/env python3
"""Generate tests/golden/utils_golden.npz from the REFERENCE's ``mtflearn/utils`` (``_clip_image.py``,
``_preprocessing_image.py``).

TEST INFRASTRUCTURE, run where the reference checkout is (REF below).  ``_clip_image.py`` imports only NumPy and is loaded
by path; ``_preprocessing_image.py`` also imports ``disk`` and ``white_tophat`` from ``skimage.morphology`` for ``remove_bg``,
which is not ported: scikit-image is not installed, so empty stand-in modules are registered for the import and never
called.  No reference source is copied; the fixture is data (arrays and scalars only).

Inputs are not stored: tests/utils_cases.py regenerates them.  Every ``info`` dictionary is stored as its key list and its
values (``info_arrays``); the clipped image once per input (it does not depend on the method when a method clips).

Usage:  python tests/make_golden_utils.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "golden", "utils_golden.npz")
sys.path.insert(0, os.path.join(HERE, "..", "motif-learn_amd"))
sys.path.insert(0, HERE)


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def import_reference():
    sys.dont_write_bytecode = True
    sk = types.ModuleType("skimage")
    skm = types.ModuleType("skimage.morphology")
    skm.disk = skm.white_tophat = None
    sk.morphology = skm
    sys.modules["skimage"], sys.modules["skimage.morphology"] = sk, skm
    utils = os.path.join(REF, "mtflearn", "utils")
    return (load_by_path("ref_clip_image", os.path.join(utils, "_clip_image.py")),
            load_by_path("ref_preprocessing_image", os.path.join(utils, "_preprocessing_image.py")))


def main():
    from utils_cases import CLIP_METHODS, MODES, golden_inputs, info_arrays
    clip, prep = import_reference()
    images = golden_inputs()
    out = {}
    for name in ("hot", "clean", "u8", "f64", "const"):
        img = images[name]
        for mode in MODES if name != "const" else ("minmax",):      # l1 / l2: only to print the distance to the reference
            out[f"{name}/normalize/{mode}"] = prep.normalize_image(img, mode=mode)
        for method in CLIP_METHODS:
            clipped, did_clip, info = clip.percentile_clip(img, method=method)
            assert clipped.dtype == np.float32 and info["did_clip"] == did_clip
            keys, values = info_arrays(info)
            out[f"{name}/clip/{method}/keys"], out[f"{name}/clip/{method}/values"] = keys, values
            if method == "auto":
                out[f"{name}/clip/out"] = clipped
        if name == "hot":
            assert all(out[f"hot/clip/{m}/values"][0] == 1.0 for m in CLIP_METHODS), "the hot pixel must trip every test"
        if name == "clean":
            assert all(out[f"clean/clip/{m}/values"][0] == 0.0 for m in CLIP_METHODS), "no test may fire without it"
    for name in ("hot", "u8", "f64"):
        out[f"{name}/standardize"] = prep.standardize_image(images[name])
    out["clean/normalize/minmax_-1_2"] = prep.normalize_image(images["clean"], mode="minmax", vmin=-1.0, vmax=2.0)
    out["hot/clip/low5_high90/out"], _, info = clip.percentile_clip(images["hot"], low=5.0, high=90.0, method="mad")
    out["hot/clip/low5_high90/keys"], out["hot/clip/low5_high90/values"] = info_arrays(info)
    out["clean/value_clip"] = clip.value_clip(images["clean"], 0.2, 0.7)
    for name in ("nonfinite", "clean", "const"):
        out[f"{name}/robust/minmax"] = prep.normalize_image_robust(images[name], mode="minmax")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
