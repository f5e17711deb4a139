"""The rasteriser of mtflearn_amd.datasets as a gather, in plain NumPy: every pixel takes its contributions in ascending point
index, each computed in float64 with one rounding per operation, and a float32 frame rounds after every add.  Written from
the contract in include/zernike_hip.h, not from the kernel.  Also returns ``k``, the largest number of contributions that land
on one pixel, which the float32 criterion of the tests needs."""
import numpy as np


def render(frame, pts, amps, sigma, r_factor=3.0, taper=True):
    """Add the Gaussians to a copy of the 2D ``frame`` (float32 or float64); returns ``(result, k)``.

    ``r_factor > 0``: pixels of [floor(x0 - R), ceil(x0 + R)] x [floor(y0 - R), ceil(y0 + R)] with r <= R receive
    ``A * exp(-0.5 * r^2 / sigma^2)`` times ``1 - 3 t^2 + 2 t^3`` (``t = r / R``) with ``taper``.  ``r_factor <= 0``: every
    pixel receives ``A * exp(-(dx^2 + dy^2) / (2 sigma^2))``."""
    out = np.array(frame, copy=True)
    h, w = out.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    amps = np.broadcast_to(np.asarray(amps, dtype=np.float64), (len(pts),))
    hits = np.zeros((h, w), dtype=np.int64)
    X, Y = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    sigma = float(sigma)
    R = r_factor * sigma
    for (x0, y0), A in zip(pts, amps):                       # ascending point index
        dx, dy = X - x0, Y - y0
        d2 = dx * dx + dy * dy
        if r_factor > 0:
            r = np.sqrt(d2)
            mask = ((X >= np.floor(x0 - R)) & (X <= np.ceil(x0 + R)) & (Y >= np.floor(y0 - R)) & (Y <= np.ceil(y0 + R)) & (r <= R))
            if not mask.any():
                continue
            rm = r[mask]
            wgt = A * np.exp(-0.5 * (rm * rm) / sigma ** 2)
            if taper:
                t = rm / R
                wgt = wgt * (1.0 - 3.0 * t ** 2 + 2.0 * t ** 3)
        else:
            mask = np.ones((h, w), dtype=bool)
            wgt = (A * np.exp(-d2 / (2 * sigma ** 2))).ravel()
        out[mask] = (out[mask].astype(np.float64) + wgt).astype(out.dtype)      # one rounding per add
        hits[mask] += 1
    return out, int(hits.max()) if hits.size else 0


def render_batch(frames, pts, amps, counts, sigma):
    """Uncut Gaussians into a copy of ``frames`` (B, H, W): frame ``b`` takes the next ``counts[b]`` points."""
    out = np.array(frames, copy=True)
    at = 0
    for b, c in enumerate(counts):
        out[b], _ = render(out[b], pts[at:at + c], amps[at:at + c], sigma, r_factor=0.0, taper=False)
        at += c
    return out, max(counts) if len(counts) else 0


def tolerance(ref, k):
    """The criteria of the tests: float64 frames ``1e-12 * max|ref|`` (the project's bound for its float64 image operators; the
    device's exp against NumPy's is the only difference); float32 frames ``k`` float32 spacings at ``max|ref|`` (each add
    rounds once, and a contribution off by a float64 ulp can move that rounding by one spacing)."""
    top = float(np.abs(ref).max()) if ref.size else 0.0
    if ref.dtype == np.float64:
        return 1e-12 * top
    return k * float(np.spacing(np.float32(top)))
