#!/usr/bin/env python3
"""Generate tests/golden/window_size_golden.npz from the REFERENCE's window-size code (build container only, CPU).

TEST INFRASTRUCTURE.  ``mtflearn/features/_window_size.py`` and ``_fft_related.py`` are loaded under stub packages, as
oracle/make_golden_pickers.py does.  ``skimage.transform.warp_polar`` is a stand-in over
``oracle.pickers_oracle.warp_polar_linear`` with warp_polar's defaults (radius: the half diagonal, output (360, ceil(radius)),
``center=`` accepted), so the two ``get_characteristic_length*`` functions are the reference's own lines over the restated
resampling: parity-unpinned against scikit-image itself, like ``radial_profile``.  ``skimage.morphology`` is an empty stand-in
that only satisfies an import.  The file holds arrays only: the inputs' outputs of all five functions, the intermediate
centre and cut profile, and ``y`` / ``y2`` / ``ind`` of the FFT route (captured from the reference's own calls of ``baseline_correction`` and
``uniform_filter1d``).  No reference source or bytecode is copied.

The maker refuses to write unless every case keeps the reference alone inside its margins: DC over runner-up >= 2, the
winning ``argmax`` of ``y2`` ahead by >= 1e-6 relative, the first autocorrelation peak above both neighbours by >= 1e-6 of the
profile's range, and no frame left out.

Usage:  python tests/make_golden_window_size.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import window_size_cases as wc  # noqa: E402
from oracle.pickers_oracle import warp_polar_linear  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "golden", "window_size_golden.npz")

CAPTURE = {}


def warp_polar(image, center=None, radius=None, output_shape=None, scaling='linear', **kwargs):
    assert radius is None and output_shape is None and scaling == 'linear' and not kwargs
    h, w = image.shape
    if center is None:
        center = (h / 2 - 0.5, w / 2 - 0.5)
    CAPTURE["centre"] = (int(center[0]), int(center[1]))
    return warp_polar_linear(image, center)


def import_reference():
    sys.dont_write_bytecode = True
    for name in ("mtflearn", "mtflearn.features", "mtflearn.utils"):
        mod = types.ModuleType(name)
        mod.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = mod

    def absent(*a, **k):
        raise RuntimeError("scikit-image is not installed: this stand-in only satisfies the import")
    for name, attrs in (("skimage", {}), ("skimage.transform", {"warp_polar": warp_polar}),
                        ("skimage.morphology", {"disk": absent, "white_tophat": absent})):
        mod = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(mod, k, v)
        sys.modules[name] = mod
    import matplotlib
    matplotlib.use("Agg")
    from mtflearn.features import _window_size, _fft_related
    return _window_size, _fft_related


def main():
    ws, fr = import_reference()
    g = {}
    n_frames = 0

    # the reference's own calls, recorded as they pass
    real_filter, real_find_peaks, real_baseline = ws.uniform_filter1d, ws.find_peaks, ws.baseline_correction

    def baseline_spy(y, niter=10):
        CAPTURE["y"] = np.array(y)                       # the reference's own cut profile, before anything touches it
        return real_baseline(y, niter=niter)

    def filter_spy(y1, size):
        out = real_filter(y1, size=size)
        CAPTURE["y2"] = out
        return out

    def peaks_spy(line):
        CAPTURE["line"] = np.array(line)
        return real_find_peaks(line)
    ws.uniform_filter1d, ws.find_peaks, ws.baseline_correction = filter_spy, peaks_spy, baseline_spy

    for name in wc.IMAGES:
        g[f"{name}/image"] = wc.image(name)
        for key, img in wc.frames_of(name):
            n_frames += 1
            assert wc.dc_ratio(img) >= 2.0, (key, wc.dc_ratio(img))
            g[f"{key}/autocorr"] = ws.compute_autocorrelation(img)
            g[f"{key}/autocorr_raw"] = ws.compute_autocorrelation(img, standardize=False)
            g[f"{key}/spectrum"] = fr.fft_power_spectrum(img)
            # autocorrelation route
            peak = ws.get_characteristic_length(img)
            line = CAPTURE["line"]
            assert wc.peak_margin(line, int(peak)) >= 1e-6, (key, wc.peak_margin(line, int(peak)))
            g[f"{key}/cl_peak"], g[f"{key}/cl_centre"], g[f"{key}/cl_line"] = np.array(int(peak)), np.array(CAPTURE["centre"]), line
            # FFT route
            for use_log in (True, False):
                tag = "log" if use_log else "lin"
                with np.errstate(divide="ignore"):
                    length = ws.get_characteristic_length_fft(img, use_log=use_log, debug=False)
                y, y2 = CAPTURE["y"], CAPTURE["y2"]
                g[f"{key}/fft_{tag}_centre"], g[f"{key}/fft_{tag}_y"] = np.array(CAPTURE["centre"]), y
                if not use_log:
                    # without the logarithm the DC sample dwarfs the profile and the mirrored edge of the running mean
                    # leaves y2[0] and y2[1] equal to rounding: centre and profile are recorded, ind is not a fact
                    continue
                assert wc.argmax_margin(y2) >= 1e-6, (key, tag, wc.argmax_margin(y2))
                g[f"{key}/fft_{tag}_length"], g[f"{key}/fft_{tag}_y2"], g[f"{key}/fft_{tag}_ind"] = np.array(length), y2, np.array(int(np.argmax(y2)))
            length = ws.get_characteristic_length_fft(img, niter=4, size=6, debug=False)      # an even filter, fewer sweeps
            assert wc.argmax_margin(CAPTURE["y2"]) >= 1e-6, key
            g[f"{key}/fft_n4s6_length"], g[f"{key}/fft_n4s6_y2"] = np.array(length), CAPTURE["y2"]
    assert n_frames == sum(1 if len(s) == 2 else s[0] for s, _, _ in wc.IMAGES.values())     # no frame left out

    for shape in wc.ANGULAR_SHAPES + ["spikes"]:
        data = wc.angular_spikes() if shape == "spikes" else wc.angular_input(shape)
        sid = shape if shape == "spikes" else f"{shape[0]}x{shape[1]}"
        g[f"angular/{sid}/input"] = data
        for nb in wc.ANGULAR_BINS:
            for use_mask in (True, False):
                angles, profile = fr.angular_average(data, num_bins=nb, use_mask=use_mask)
                key = f"angular/{sid}/{nb}/{int(use_mask)}"
                g[f"{key}/angles"], g[f"{key}/profile"] = angles, profile
                g[f"{key}/counts"] = wc.angular_average(data, nb, use_mask)[2]

    np.savez_compressed(OUT, **g)
    print("wrote", OUT, len(g), "arrays,", os.path.getsize(OUT), "bytes,", n_frames, "frames")


if __name__ == "__main__":
    main()
