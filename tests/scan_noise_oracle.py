"""The independent CPU statement of ``apply_scan_noise``: SciPy, frame by frame.

``resample`` is ``scipy.ndimage.map_coordinates(frame, [yy + dy[z], xx + dx[z]], order, mode)`` per frame, with one exception.
For ``order=3, mode='reflect'`` SciPy starts its prefilter recursion from a series truncated to the axis length, which on an
axis shorter than about 28 samples is not the interpolant of the half-sample symmetric extension.  There the frame is padded
by ``P = 32 + ceil(max|shift|)`` samples with ``np.pad(mode='symmetric')`` -- the exact extension -- and evaluated with
``order=3, mode='reflect'`` at coordinates shifted by ``P``: no coordinate leaves the padded frame's interior by less than 32
samples, the truncated start is ``|sqrt(3) - 2|^32`` away, below rounding.  tests/test_scan_noise_cpu.py checks that both
forms agree at n = 40 and that this module reproduces the reference's recorded outputs.
"""
import numpy as np
from scipy.ndimage import map_coordinates


def jitter(seed, shape, jx, jy):
    """The reference's draws as ``(dx (Z, H), dy (Z, W))``: both normal draws happen, in this order, whatever the factors."""
    z, h, w = shape
    jx = 0 if jx is None else jx
    jy = 0 if jy is None else jy
    rng = np.random.default_rng(seed=seed)
    dx = rng.normal(0, 1, (z, h, 1)) * jx
    dy = rng.normal(0, 1, (z, 1, w)) * jy
    return dx[:, :, 0].astype(np.float64), dy[:, 0, :].astype(np.float64)


def resample_frame(frame, dx, dy, order, mode, padded=None):
    """One frame: ``dx`` (H,), ``dy`` (W,).  ``padded``: force (True) or forbid (False) the padded form of order 3 'reflect'."""
    h, w = frame.shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cy = yy + dy[None, :]
    cx = xx + dx[:, None]
    if padded is None:
        padded = order == 3 and mode == "reflect"
    if padded:
        p = 32 + int(np.ceil(max(np.abs(dx).max(), np.abs(dy).max())))
        return map_coordinates(np.pad(frame, p, mode="symmetric"), [cy + p, cx + p], order=order, mode="reflect")
    return map_coordinates(frame, [cy, cx], order=order, mode=mode)


def resample(images, dx, dy, order, mode):
    """``out[z, y, x] = S_z(y + dy[z, x], x + dx[z, y])`` of a (Z, H, W) stack, in the stack's dtype."""
    return np.stack([resample_frame(images[z], dx[z], dy[z], order, mode) for z in range(images.shape[0])])
