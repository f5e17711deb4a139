"""Deterministic small frames for the Gaussian fit (mtflearn_amd.features.gaussian_fit_points), built with NumPy alone.

PARITY     64 x 64 frames of 16 overlapping elliptical Gaussians on a jittered 4 x 4 lattice (pitch 12, sigma 1.6 .. 2.4,
           amplitude 0.6 .. 1.4, background 0.1) with Gaussian noise 0, 0.02 and 0.1, as float64 and float32, fitted from the
           integer lattice sites with both models, the box at size 7 and 11 and the disk at size 9.
RECOVERY   float64 frames in which every window holds ONE noise-free Gaussian of known parameters (the frame is the background
           outside the windows): the elliptical ones with their major axis near 0, near pi/2, at 45 degrees and round, the
           circular ones round.
isolated() the same construction for any window size, for the tests of the sizes where the lane mapping changes."""
import numpy as np

MODELS = ("circular", "elliptical")
NOISES = (0.0, 0.02, 0.1)
WINDOWS = (("box", 7), ("box", 11), ("disk", 9))
BACKGROUND = 0.1


def precision(s_major, s_minor, theta):
    """``(a, b, c)`` of a Gaussian with the given widths and major-axis angle (from x towards y)."""
    l1, l2, co, si = 1 / s_major ** 2, 1 / s_minor ** 2, np.cos(theta), np.sin(theta)
    return l1 * co * co + l2 * si * si, (l1 - l2) * si * co, l1 * si * si + l2 * co * co


def gaussian(shape, x0, y0, amplitude, a, b, c, origin=(0, 0)):
    yy, xx = np.mgrid[:shape[0], :shape[1]].astype(np.float64)
    dx, dy = xx + origin[0] - x0, yy + origin[1] - y0
    return amplitude * np.exp(-(a * dx * dx + 2 * b * dx * dy + c * dy * dy) / 2)


def lattice_frame(noise, seed=7):
    """``(frame float64 (64, 64), integer sites (16, 2))``."""
    rng = np.random.default_rng(seed)
    sites = np.array([(14 + 12 * i, 14 + 12 * j) for j in range(4) for i in range(4)], dtype=np.int32)
    frame = np.full((64, 64), BACKGROUND)
    for sx, sy in sites:
        s1, s2 = np.sort(rng.uniform(1.6, 2.4, 2))[::-1]
        a, b, c = precision(s1, s2, rng.uniform(-np.pi / 2, np.pi / 2))
        frame += gaussian(frame.shape, sx + rng.uniform(-0.45, 0.45), sy + rng.uniform(-0.45, 0.45), rng.uniform(0.6, 1.4), a, b, c)
    if noise:
        frame += rng.normal(0.0, noise, frame.shape)
    return frame, sites


def parity_name(dtype, model, mode, size, noise):
    return f"{dtype}_{model}_{mode}{size}_noise{noise:g}"


def parity_cases():
    """name -> ``(frame, pts, size, model, mode)`` with ``mode`` None or 'disk'."""
    out = {}
    for noise in NOISES:
        frame, sites = lattice_frame(noise)
        for dtype in ("float64", "float32"):
            for model in MODELS:
                for mode, size in WINDOWS:
                    out[parity_name(dtype, model, mode, size, noise)] = (frame.astype(dtype), sites, size, model, None if mode == "box" else mode)
    return out


def isolated(size, shapes, seed=11, frame_shape=(64, 64)):
    """A float64 frame with one noise-free Gaussian per window, the windows side by side without overlap:
    ``(frame, pts int32 (N, 2), truth (N, 7))`` with truth columns x, y, amplitude, sigma_major, sigma_minor, theta, background.
    ``shapes`` lists ``(sigma_major, sigma_minor, theta)``."""
    rng = np.random.default_rng(seed)
    frame = np.full(frame_shape, BACKGROUND)
    per_row = frame_shape[1] // size
    pts, truth = [], []
    for k, (s1, s2, theta) in enumerate(shapes):
        cx, cy = (k % per_row) * size, (k // per_row) * size
        assert cy + size <= frame_shape[0], "too many windows for the frame"
        px, py = cx + size // 2, cy + size // 2
        x, y, amp = px + rng.uniform(-0.4, 0.4), py + rng.uniform(-0.4, 0.4), rng.uniform(0.6, 1.4)
        frame[cy:cy + size, cx:cx + size] += gaussian((size, size), x, y, amp, *precision(s1, s2, theta), origin=(cx, cy))
        pts.append((px, py))
        truth.append((x, y, amp, s1, s2, theta, BACKGROUND))
    return frame, np.array(pts, dtype=np.int32), np.array(truth)


RECOVERY_SIZE = 11
RECOVERY_SHAPES = {
    "elliptical": ((2.2, 1.7, 0.02), (2.2, 1.7, -0.02), (2.3, 1.6, np.pi / 2 - 0.02), (2.3, 1.6, -np.pi / 2 + 0.02), (2.1, 1.5, np.pi / 4),
                   (2.1, 1.5, -np.pi / 4), (2.4, 2.0, 1.0), (1.9, 1.9, 0.0)),
    "circular": ((1.6, 1.6, 0.0), (1.9, 1.9, 0.0), (2.2, 2.2, 0.0), (2.4, 2.4, 0.0)),
}


def recovery_case(model):
    return isolated(RECOVERY_SIZE, RECOVERY_SHAPES[model])


def recovery_error(params, truth):
    """The largest ``|got - truth| / (|truth| + 1)`` over x, y, amplitude, both widths, the background, and the angle where the
    truth is not round (the angle of a round Gaussian is arbitrary)."""
    err = np.abs(params[:, [0, 1, 2, 3, 4, 6]] - truth[:, [0, 1, 2, 3, 4, 6]]) / (np.abs(truth[:, [0, 1, 2, 3, 4, 6]]) + 1)
    oval = truth[:, 3] != truth[:, 4]
    angle = np.abs(params[oval, 5] - truth[oval, 5]) / (np.abs(truth[oval, 5]) + 1)
    return max(err.max(), angle.max(initial=0.0))


def scaled_distance(got, want):
    """``max |got - want| / (|want| + 1)``: the measure of the parity bound."""
    return float((np.abs(got - want) / (np.abs(want) + 1)).max(initial=0.0))
