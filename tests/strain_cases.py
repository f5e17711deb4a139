"""The case table of the strain tests: two-cosine lattices ``I(r) = offset + scale (cos(2 pi g1 . (r - u)) + cos(2 pi g2 . (r - u)))``
with a known displacement field ``u``, each the smallest frame at which its path of csrc/zk_strain.hip can go wrong.  A case is
a dict of ``name, frame (or stack), g, sigma, reference, window`` and, where the truth is known, ``grad_u (2, 2)``
(``[j][a] = du_j / dr_a``, 0 = y, 1 = x).  tests/test_strain_cpu.py licenses the table (amplitude floor, sizes)."""
import numpy as np

AMP_FLOOR = 1e-3                    # strain is compared where every stencil amplitude is at least this share of the plane's maximum
FLOOR_SHARE = 0.01                  # ... and at most this share of a case's pixels may lie below it

G_ON_96x128 = np.array([[10 / 96, 4 / 128], [3 / 96, 14 / 128]])       # both on the FFT grid of a 96 x 128 frame
GRAD_U = np.array([[0.010, 0.004], [-0.006, 0.008]])


def lattice(h, w, g, u=None, offset=0.0, scale=1.0, dtype=np.float64):
    """The two-cosine lattice displaced by ``u(y, x) -> (uy, ux)``; integer dtypes are rounded."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    uy, ux = (0.0, 0.0) if u is None else u(y, x)
    g = np.asarray(g, np.float64)
    img = offset + scale * sum(np.cos(2 * np.pi * (g[k][0] * (y - uy) + g[k][1] * (x - ux))) for k in range(2))
    return np.rint(img).astype(dtype) if np.issubdtype(dtype, np.integer) else img.astype(dtype)


def uniform(grad_u, h, w):
    """``u = grad_u (r - centre)``."""
    def u(y, x):
        ry, rx = y - (h - 1) / 2, x - (w - 1) / 2
        return grad_u[0][0] * ry + grad_u[0][1] * rx, grad_u[1][0] * ry + grad_u[1][1] * rx
    return u


def bump(cy, cx, width, ay, ax):
    """A Gaussian displacement bump ``(ay, ax) exp(-|r - c|^2 / (2 width^2))``."""
    def u(y, x):
        e = np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * width ** 2))
        return ay * e, ax * e
    return u


def case(name, frame, g, sigma=None, reference=None, window=None, grad_u=None):
    return dict(name=name, frame=frame, g=np.asarray(g, np.float64), sigma=sigma, reference=reference, window=window, grad_u=grad_u)


def options(c):
    return dict(sigma=c["sigma"], reference=c["reference"], window=c["window"])


def _cases():
    base = lattice(96, 128, G_ON_96x128, uniform(GRAD_U, 96, 128))
    g_off = [[0.151, 0.023], [0.031, 0.137]]
    g_small = [[0.125, 0.05], [-0.0625, 0.125]]
    out = [
        # grid and dtype basics
        case("96x128-f32-ongrid-uniform", base.astype(np.float32), G_ON_96x128, grad_u=GRAD_U),
        case("61x67-f64-offgrid-bump-ref", lattice(61, 67, g_off, bump(38, 40, 7.0, 0.5, -0.4)), g_off, reference=(2, 16, 3, 24)),
        case("4x5-f64", lattice(4, 5, [[0.25, 0.0], [0.0, 0.2]], uniform(GRAD_U, 4, 5)), [[0.25, 0.0], [0.0, 0.2]]),
        # reference rectangles: 5600 pixels are two partials, one pixel, the whole frame (three partials), two frame edges
        case("96x128-ref-large", base, G_ON_96x128, reference=(10, 80, 20, 100)),
        case("96x128-ref-pixel", base, G_ON_96x128, reference=(40, 41, 50, 51)),
        case("96x128-ref-whole", base, G_ON_96x128, reference=(0, 96, 0, 128)),
        case("96x128-ref-edges", base, G_ON_96x128, reference=(0, 30, 98, 128)),
        # a mask that wraps past the Nyquist row, and negative components
        case("64x48-g049", lattice(64, 48, [[0.49, 0.1], [0.1, 0.3]], uniform(GRAD_U / 4, 64, 48)), [[0.49, 0.1], [0.1, 0.3]]),
        case("48x64-g-negative", lattice(48, 64, [[0.12, -0.07], [-0.05, -0.13]], uniform(GRAD_U, 48, 64)), [[0.12, -0.07], [-0.05, -0.13]],
             reference=(8, 40, 8, 56)),
        case("96x128-hann", base, G_ON_96x128, window="hann"),
        # the detector formats
        case("32x40-uint8", lattice(32, 40, g_small, uniform(GRAD_U, 32, 40), 120, 50, np.uint8), g_small),
        case("32x40-uint16", lattice(32, 40, g_small, uniform(GRAD_U, 32, 40), 30000, 12000, np.uint16), g_small),
        case("32x40-int16", lattice(32, 40, g_small, uniform(GRAD_U, 32, 40), -100, 9000, np.int16), g_small, reference=(4, 20, 4, 30)),
    ]
    return out


CASES = _cases()
PHASE_CASES = ["96x128-f32-ongrid-uniform", "61x67-f64-offgrid-bump-ref", "4x5-f64", "64x48-g049", "48x64-g-negative"]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# the stack of the run test: five 32 x 40 float32 frames of different strain; RUN_FRAMES frames fit the budget the test sets
STACK_G = np.array([[0.125, 0.05], [-0.0625, 0.125]])
RUN_FRAMES = 2


def stack_case():
    frames = [lattice(32, 40, STACK_G, uniform(GRAD_U * s, 32, 40), dtype=np.float32) for s in (0.0, 0.5, 1.0, -1.0, 2.0)]
    return dict(name="32x40-f32-B5", frame=np.stack(frames), g=STACK_G, sigma=None, reference=(4, 28, 6, 34), window=None, grad_u=None)


def run_bytes(h, w, frames):
    """The budget that holds exactly ``frames`` frames of a run: a spectrum and two planes of complex float64 each."""
    return frames * h * w * 48


# the lattice of the pick_g test: Gaussian atoms on a rectangular lattice of 8 rows x 16 columns, periodic in the 96 x 128 frame
PICK_G = np.array([[0.0, 1 / 16], [1 / 8, 0.0]])            # strongest first: the longer period is damped less by the atoms' width


def atoms_frame(h=96, w=128, py=8, px=16, width=2.0):
    def comb(n, period):
        d = (np.arange(n)[:, None] - np.arange(0, n, period)[None, :] + n / 2) % n - n / 2
        return np.exp(-d ** 2 / (2 * width ** 2)).sum(axis=1)
    return np.outer(comb(h, py), comb(w, px))
