#!/usr/bin/env python3
"""Generate tests/golden/com_refine.npz on the CPU.

TEST INFRASTRUCTURE.  Inputs are not stored, tests/com_refine_cases.py regenerates them from seeds.

Per case and threshold (``li``, ``otsu``): ``<name>/<threshold>/t`` the threshold of every window, ``<name>/<threshold>/it`` Li's
iteration counts (zeros for Otsu) and ``<name>/<threshold>/xy`` the refined points.  The route is the reference's ``com_refine``
taken literally -- cut the window, threshold it, zero what lies below, ``scipy.ndimage.center_of_mass``, subtract ``size / 2``,
swap to (x, y), add the point -- with two things said here: the window is widened to float64 first (the thresholds are defined
on the float64 window), and the thresholds are those of tests/thresholds_reference.py, since scikit-image is not installed
here (parity with it is unpinned).

Conditioning asserted here for the parity cases, with NO window left out: every Li run keeps a margin of at least 1e-6 (no loop
test comes within 1e-6, relative, of the tolerance: a run that stops within rounding of it pins nothing), and no pixel lies
within 1e-9 of the window's range from its threshold (such a pixel could fall on either side of it).

Usage:  python tests/make_golden_com_refine.py
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "motif-learn_amd"))

import com_refine_cases as cc             # noqa: E402
import thresholds_reference as ref        # noqa: E402

LI_MARGIN = 1e-6
PIXEL_MARGIN = 1e-9


def refine_window(w, size, threshold):
    """One window of the reference's loop: ``(centroid moved by size / 2 as (x, y), threshold, iterations, margin)``."""
    from scipy import ndimage
    if threshold == "otsu":
        t, it, margin = ref.otsu(w)[0], 0, np.inf
    else:
        t, it, margin = ref.li(w)
    w = w.copy()
    w[w < t] = 0
    return np.subtract(ndimage.center_of_mass(w), size / 2)[::-1], t, it, margin


def build_case(frame, pts, size, threshold):
    n = len(pts)
    moved, ts, its, margins, nearest = np.empty((n, 2)), np.empty(n), np.zeros(n, np.int32), np.empty(n), np.empty(n)
    for k, w in enumerate(cc.windows(frame, pts, size)):
        moved[k], ts[k], its[k], margins[k] = refine_window(w, size, threshold)
        span = w.max() - w.min()
        nearest[k] = np.abs(w - ts[k]).min() / span if span > 0 else np.inf
    return moved + pts, ts, its, margins, nearest


def build(verbose=False):
    out = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for name, (frame, pts, size) in cc.cases().items():
            for threshold in cc.THRESHOLDS:
                xy, ts, its, margins, nearest = build_case(frame, pts, size, threshold)
                if name in cc.PARITY:
                    assert np.isfinite(xy).all() and np.isfinite(ts).all(), (name, threshold)
                    assert margins.min() >= LI_MARGIN, (name, threshold, "a Li run stops within 1e-6 of the tolerance boundary", margins.min())
                    assert nearest.min() >= PIXEL_MARGIN, (name, threshold, "a pixel lies within 1e-9 of the range from its threshold", nearest.min())
                out[f"{name}/{threshold}/xy"], out[f"{name}/{threshold}/t"], out[f"{name}/{threshold}/it"] = xy, ts, its
                if verbose:
                    print(f"{name} {threshold}: {frame.dtype} {frame.shape}, {len(pts)} windows of {size}, iterations {its.min()} .. {its.max()}, "
                          f"margin {margins.min():.3g}, nearest pixel {nearest.min():.3g}, {int(np.isnan(xy).any(axis=1).sum())} without a centroid")
    return out


def main():
    arrays = build(True)
    path = os.path.join(HERE, "golden", "com_refine.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
