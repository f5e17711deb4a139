"""The NumPy statement of ``strain.gpa`` (include/zernike_hip.h, "Geometric phase analysis"), written from the contract:
``np.fft`` for the planes, ``np.angle`` of the neighbour products for the phase gradient, ``np.mean`` over the reference
rectangle.  It is the checker of the strain tests, never the product."""
import numpy as np

from registration_oracle import window_of

TWO_PI = 2 * np.pi


def default_sigma(g):
    g = np.asarray(g, np.float64)
    return min(np.hypot(*g[0]), np.hypot(*g[1]), np.hypot(*(g[0] - g[1]))) / 6


def planes(frame, g, sigma, window=None):
    """``H_k (2, H, W)`` complex: ``ifft2(fft2(I w) M_k)``."""
    h, w = frame.shape
    F = np.fft.fft2(np.asarray(frame, np.float64) * window_of(h, w, window))
    out = np.empty((2, h, w), np.complex128)
    for k in range(2):
        dy = np.fft.fftfreq(h)[:, None] - g[k][0]
        dx = np.fft.fftfreq(w)[None, :] - g[k][1]
        dy = dy - np.rint(dy)
        dx = dx - np.rint(dx)
        out[k] = np.fft.ifft2(F * np.exp(-(dy ** 2 + dx ** 2) / (2 * sigma ** 2)))
    return out


def gradient(plane, gk, axis):
    """``dP/dr_axis`` of one plane: ``np.gradient``'s stencil on the wrapped phase, the carrier ``g`` taken out of every product."""
    P = np.moveaxis(plane, axis, 0)
    c1, c2 = np.exp(-1j * TWO_PI * gk[axis]), np.exp(-2j * TWO_PI * gk[axis])
    d = np.empty(P.shape)
    d[1:-1] = np.angle(P[2:] * np.conj(P[:-2]) * c2) / 2
    d[0] = np.angle(P[1] * np.conj(P[0]) * c1)
    d[-1] = np.angle(P[-1] * np.conj(P[-2]) * c1)
    return np.moveaxis(d, 0, axis)


def gpa(frame, g, sigma=None, reference=None, window=None):
    """A dict of ``exx, eyy, exy, rotation (H, W)``, ``amplitude (2, H, W)``, ``g (2, 2)``, ``phase (2, H, W)``, ``planes`` and
    ``grad (2, 2, H, W)`` (``[k][a]``, before the mean is taken out) of one frame."""
    g = np.asarray(g, np.float64)
    sigma = default_sigma(g) if sigma is None else sigma
    h, w = frame.shape
    Hk = planes(frame, g, sigma, window)
    grad = np.array([[gradient(Hk[k], g[k], a) for a in range(2)] for k in range(2)])
    d = grad.copy()
    G = g.copy()
    if reference is not None:
        y0, y1, x0, x1 = reference
        m = d[:, :, y0:y1, x0:x1].mean(axis=(2, 3))
        d -= m[:, :, None, None]
        G = g + m / TWO_PI
    det = G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
    inv = np.array([[G[1, 1], -G[0, 1]], [-G[1, 0], G[0, 0]]]) / det
    e = -np.einsum("jk,kayx->jayx", inv, d) / TWO_PI                    # e[j][a] = du_j / dr_a; 0 = y, 1 = x
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    phase = np.empty((2, h, w))
    for k in range(2):
        t = g[k][0] * y + g[k][1] * x
        t = t - np.floor(t)
        phase[k] = np.angle(Hk[k] * np.exp(-1j * TWO_PI * t))
    return dict(exx=e[1, 1], eyy=e[0, 0], exy=(e[1, 0] + e[0, 1]) / 2, rotation=(e[0, 1] - e[1, 0]) / 2, amplitude=np.abs(Hk), g=G,
                phase=phase, planes=Hk, grad=grad)


def stencil_floor(amplitude):
    """Per pixel the smallest amplitude ratio (to its plane's maximum) over the pixel and its four neighbours, both planes: what
    the error of a phase gradient at that pixel scales with."""
    r = amplitude / amplitude.max(axis=(1, 2), keepdims=True)
    pad = np.pad(r, ((0, 0), (1, 1), (1, 1)), mode="edge")
    near = np.minimum.reduce([pad[:, 1:-1, 1:-1], pad[:, :-2, 1:-1], pad[:, 2:, 1:-1], pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]])
    return near.min(axis=0)
