"""Cases and the NumPy / SciPy restatement of the Fourier window-size estimators (reference features/_window_size.py,
features/_fft_related.py) -- TEST INFRASTRUCTURE shared by tests/make_golden_window_size.py, tests/test_window_size_cpu.py,
tests/test_gpu_window_size.py and tools/time_window_size.py; never imported by the product.

Inputs: a positive offset + a 2-D cosine lattice of period 6-10 px + seeded noise.  With the offset the DC term is the strict
maximum of the spectrum, so the centre of the polar profile does not hang on the last bit of an FFT (the conjugate-twin
hazard, see mtflearn_amd/features/window_size.py).  ``warp_polar`` is ``oracle.pickers_oracle.warp_polar_linear``
(scikit-image is not installed: parity-unpinned against it, like ``radial_profile``).
"""
import numpy as np
from scipy.ndimage import uniform_filter1d
from scipy.signal import correlate, find_peaks

from eels_oracle import snip
from oracle.pickers_oracle import standardize_image, warp_polar_linear

# name -> (shape, periods (one per frame for a stack), dtype)
IMAGES = {
    "sq64": ((64, 64), (8.0,), np.float64),
    "wide48x80": ((48, 80), (7.0,), np.float64),
    "tall80x48": ((80, 48), (9.0,), np.float64),
    "odd63x65": ((63, 65), (6.5,), np.float64),
    "small33x40": ((33, 40), (6.0,), np.float64),
    "f32_64": ((64, 64), (10.0,), np.float32),
    "stack3x48x80": ((3, 48, 80), (6.0, 8.0, 10.0), np.float64),
}
STACK = "stack3x48x80"

ANGULAR_SHAPES = [(17, 17), (16, 24), (31, 20), (130, 129)]
ANGULAR_BINS = [360, 8, 7, 12, 1]


def frame(shape, period, seed):
    rng = np.random.default_rng(seed)
    y, x = np.indices(shape).astype(np.float64)
    k = 2 * np.pi / period
    lattice = np.cos(k * x) * np.cos(k * (0.5 * x + 0.8660254037844386 * y)) + 0.5 * np.cos(k * y)
    return 3.0 + lattice + 0.05 * rng.standard_normal(shape)


def image(name):
    shape, periods, dtype = IMAGES[name]
    seed = 1000 + sorted(IMAGES).index(name)
    if len(shape) == 3:
        return np.stack([frame(shape[1:], p, seed + 17 * b) for b, p in enumerate(periods)]).astype(dtype)
    return frame(shape, periods[0], seed).astype(dtype)


def frames_of(name):
    """(key, 2-D frame) pairs: the image itself, or every frame of the stack."""
    img = image(name)
    return [(name, img)] if img.ndim == 2 else [(f"{name}/{b}", f) for b, f in enumerate(img)]


def angular_input(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    return rng.random(shape) + 0.25


def angular_spikes(shape=(17, 17)):
    """A large value on each of the eight 45-degree directions and at the centre, over zeros."""
    a = np.zeros(shape)
    cy, cx = shape[0] // 2, shape[1] // 2
    for k, (dy, dx) in enumerate([(0, 0), (0, 3), (3, 3), (3, 0), (3, -3), (0, -3), (-3, -3), (-3, 0), (-3, 3)]):
        a[cy + dy, cx + dx] = 1000.0 + k
    return a


# --------------------------------------------------------------------------------------------- the restatement
def compute_autocorrelation(image, standardize=True):
    """``_window_size.py:16-27``."""
    if standardize is True:
        image = standardize_image(image)
    f = np.fft.fft2(image)
    return np.abs(np.fft.fftshift(np.fft.ifft2(f * np.conj(f))))


def fft_power_spectrum(img):
    """``_fft_related.py:4-7``."""
    return np.abs(np.fft.fftshift(np.fft.fft2(img)))


def warp_polar(data, center):
    return warp_polar_linear(data, center)


def cut_profile(data):
    """``_window_size.py:30-33``: ``(centre, line)``."""
    i, j = np.unravel_index(np.argmax(data), data.shape)
    return (int(i), int(j)), warp_polar(data, (i, j)).mean(axis=0)[0:i]


def autocorr_same(image, standardize=True):
    """``_window_size.py:9-13``."""
    if standardize is True:
        image = standardize_image(image)
    return correlate(image, image, mode='same', method='fft')


def get_characteristic_length(image, standardize=True):
    """``_window_size.py:36-46``: ``(peaks[0], centre, line)``; peaks[0] is -1 where the reference raises."""
    centre, line = cut_profile(autocorr_same(image, standardize))
    peaks, _ = find_peaks(line)
    return (int(peaks[0]) if len(peaks) else -1), centre, line


def fft_route(image, niter=10, size=9, use_log=True):
    """``_window_size.py:65-80`` in this project's words: ``(length, centre, y, y2, ind)``.  The SNIP baseline is
    ``eels_oracle.snip`` (the same operation order as the reference's second copy, sums bit-equal)."""
    magnitude = fft_power_spectrum(image)
    centre, y = cut_profile(np.log(magnitude + 1) if use_log else magnitude)
    y2 = uniform_filter1d(y - snip(y, niter=niter)[0], size=size)
    ind = int(np.argmax(y2))
    with np.errstate(divide="ignore"):
        return image.shape[0] / np.int64(ind), centre, y, y2, ind


get_characteristic_length_fft = fft_route


def pixel_angles(shape):
    """Per pixel about ``(h // 2, w // 2)``: ``(angle in degrees in [0, 360), squared radius (integers), inscribed radius)``."""
    cy, cx = shape[0] // 2, shape[1] // 2
    dy, dx = np.indices(shape)
    dy, dx = dy - cy, dx - cx
    return np.degrees(np.arctan2(dy, dx)) % 360, dx * dx + dy * dy, min(cy, cx)


def angular_masks(shape, num_bins, use_mask):
    """``_fft_related.py:32-61``: ``(angles, list of the bins' boolean masks)``; the disk test is the reference's float
    comparison ``sqrt(r2) <= radius``."""
    degrees, r2, radius = pixel_angles(shape)
    inside = np.sqrt(r2) <= radius if use_mask else np.ones(shape, dtype=bool)
    edges = np.linspace(0, 360, num_bins + 1)
    angles = (edges[:-1] + edges[1:]) / 2
    return angles, [(edges[i] <= degrees) & (degrees < edges[i + 1]) & inside for i in range(num_bins)]


def angular_average(power_spectrum, num_bins=360, use_mask=True):
    """``_fft_related.py:12-66``: ``(angles, profile, counts)``."""
    angles, masks = angular_masks(power_spectrum.shape, num_bins, use_mask)
    counts = np.array([int(m.sum()) for m in masks], dtype=np.int64)
    profile = np.array([power_spectrum[m].mean() if n else 0.0 for m, n in zip(masks, counts)])
    return angles, profile, counts


# --------------------------------------------------------------------------------------------- the maker's conditions
def dc_ratio(image):
    """DC magnitude over the largest other magnitude of the spectrum."""
    mag = np.abs(np.fft.fft2(np.asarray(image, dtype=np.float64))).ravel()
    return mag[0] / mag[1:].max()


def argmax_margin(v):
    """Relative lead of the maximum over the runner-up."""
    s = np.sort(np.asarray(v))[::-1]
    return (s[0] - s[1]) / abs(s[0])


def peak_margin(line, peak):
    """Lead of the peak over the higher neighbour, in units of the profile's range."""
    return (line[peak] - max(line[peak - 1], line[peak + 1])) / np.ptp(line)
