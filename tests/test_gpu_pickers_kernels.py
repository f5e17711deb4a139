"""The picker kernels (csrc/zk_pickers.hip) one by one against independent references (tests/pickers_reference.py:
extended-precision FFT, the plain lag sum, SciPy's interpolation), at the shapes where such kernels go wrong: sizes 1
and 2, odd and prime extents, thin images, non-square images, windows in every corner, window counts around the 256
wide blocks, radius counts around the 128 wide block, every item of a batch, float32 next to float64, cuts through a
conjugate pair, plans evicted from the FFT plan cache, medians that fall into ties.

Tolerances.  "Of the maximum" below: the inputs are zero-mean white noise, whose spectrum is flat, so a bound on the
maximum pins every bin.  1e-12 of the maximum for a float64 FFT result is eps * log2(N^2) with about two orders of
margin.  float32 images are widened exactly on the device, so they get the same bound against the reference on the
widened image.  Every test prints its largest error / scale ratio (pytest -s).

Largest ratios observed on an MI355X, each as a fraction of its bound's scale:
  power spectra            1.1e-15 (sizes 31, 97, 255; every taper and both dtypes below that); on the positive image
                           4.3e-06 of the elementwise bound rtol=1e-9 + 1e-12 of the maximum
  autocorrelation          2.6e-15 (ws 31, float32, raw)
  polar profile            the largest of each shape is a 'sum': 2.0e-14 (1 x 9), 3.8e-14 (7 x 5), 4.3e-13 (257 x 131),
                           3.3e-13 (181 x 181), 4.2e-13 (182 x 182), 1.8e-12 (1024 x 1024, bound 1e-11)
  batched polar profiles   1.8e-14
  denoise_fft              9.2e-16 (255 x 257); plan cache 4.4e-16
  wavelet sigma            4.4e-16 absolute
The only ratios above 1e-13 are the 'sum' profiles of the four largest shapes: 360 samples added, each of which differs from
SciPy's interpolation by the rounding of its coordinate (eps times up to ~150, ~700 at 1024 x 1024) times the data's
gradient; with the CPU oracle in place of the device the same cases give 4.4e-13, 3.2e-13, 3.4e-13 and 1.7e-12.

Before that run the 1 x 1 profile with method 'sum' missed its bound at 1.72e-12: polar_profile_kernel added 360 x 1.454
as a plain running sum and ended 22 ulps of the total off.  The kernel now adds with Neumaier compensation and the
reference adds in extended precision, so neither side carries a summation error (that case now gives 0).
"""
import numpy as np
import pytest

import pickers_reference as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def po():
    from oracle import pickers_oracle
    return pickers_oracle


@pytest.fixture(scope="module")
def pk():
    from mtflearn_amd.features import pickers
    return pickers


class Worst:
    """Largest |got - ref| / scale over the comparisons of one test."""

    def __init__(self):
        self.ratio, self.where = 0.0, None

    def check(self, where, got, ref, tol, scale):
        got, ref = np.asarray(got), np.asarray(ref)
        assert got.shape == ref.shape, where
        assert np.all(np.isfinite(got)), where
        ratio = float(np.abs(got - ref).max() / scale) if got.size and scale > 0 else float(np.abs(got - ref).max(initial=0.0))
        if ratio >= self.ratio:
            self.ratio, self.where = ratio, where
        assert ratio <= tol, f"{where}: error {ratio:.3e} of the scale {scale:.3e}, bound {tol:.1e}"


@pytest.fixture
def worst(request):
    w = Worst()
    yield w
    print(f"\n[{request.node.name}] largest error ratio {w.ratio:.3e} at {w.where}")


def corners_and_random(rng, H, W, size, n_random):
    out = [(0, 0), (H - size, W - size), (0, W - size), (H - size, 0)]
    out += [(int(rng.integers(0, H - size + 1)), int(rng.integers(0, W - size + 1))) for _ in range(n_random)]
    return out


# ------------------------------------------------------------------------------------------- zk_power_spectra
PS_SHAPE = (260, 300)
PS_SIZES = (1, 2, 3, 8, 31, 33, 48, 64, 97, 100, 255)
WINDOWS = (None, "hann", "hanning", "hamming", "blackman", "tukey")


@pytest.fixture(scope="module")
def ps_img():
    return np.random.default_rng(31).standard_normal(PS_SHAPE)


def check_spectra(worst, pk, img, size, origins, window, label):
    got = pk._power_spectra(img, size, origins, window)
    ref = pr.power_spectra_ref(img.astype(np.float64), size, origins, pr.window_ref(window, size))
    assert got.shape == ref.shape == (len(origins), size, size)
    for b in range(len(origins)):                        # every item against its own maximum
        worst.check(f"{label} item {b} origin {origins[b]}", got[b], ref[b], 1e-12, ref[b].max())


@pytest.mark.parametrize("size", PS_SIZES)
def test_power_spectra_every_size_in_every_corner(pk, ps_img, worst, size):
    """Non-square image, the four corner windows and three random ones, float64 and float32."""
    origins = corners_and_random(np.random.default_rng(size), *PS_SHAPE, size, 3)
    for dtype in (np.float64, np.float32):
        check_spectra(worst, pk, ps_img.astype(dtype), size, origins, None, f"size {size} {np.dtype(dtype).name}")


@pytest.mark.parametrize("n_windows", (1, 2, 257))
@pytest.mark.parametrize("size", (3, 33, 64))
def test_power_spectra_every_item_of_a_batch(pk, ps_img, worst, size, n_windows):
    """Batch index above 0 in the fill and in the shift (257 windows: more than one block's worth)."""
    rng = np.random.default_rng(100 * size + n_windows)
    origins = [(int(rng.integers(0, PS_SHAPE[0] - size + 1)), int(rng.integers(0, PS_SHAPE[1] - size + 1))) for _ in range(n_windows)]
    check_spectra(worst, pk, ps_img, size, origins, "hann" if n_windows == 2 else None, f"size {size} n {n_windows}")


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("size", (8, 33, 64))
def test_power_spectra_window_functions(pk, ps_img, worst, size, window):
    """Every taper of the reference against its closed form."""
    origins = corners_and_random(np.random.default_rng(size), *PS_SHAPE, size, 3)
    check_spectra(worst, pk, ps_img, size, origins, window, f"size {size} window {window}")
    check_spectra(worst, pk, ps_img.astype(np.float32), size, origins[:2], window, f"size {size} window {window} float32")


def test_power_spectra_window_is_the_whole_image(pk, worst):
    """size == H == W."""
    img = np.random.default_rng(32).standard_normal((97, 97))
    for window in (None, "hann"):
        check_spectra(worst, pk, img, 97, [(0, 0)], window, f"whole image window {window}")


def test_power_spectra_bins_away_from_dc_on_a_positive_image(pk, worst):
    """A positive image, whose DC bin is ~1e4 times the others: elementwise rtol=1e-9 with atol=1e-12 of the maximum,
    so the small bins are compared too."""
    rng = np.random.default_rng(33)
    img = rng.random(PS_SHAPE) + 0.5
    for size in (33, 48):
        origins = corners_and_random(rng, *PS_SHAPE, size, 3)
        for window in (None, "hann"):
            got = pk._power_spectra(img, size, origins, window)
            ref = pr.power_spectra_ref(img, size, origins, pr.window_ref(window, size))
            for b in range(len(origins)):
                bound = 1e-12 * ref[b].max() + 1e-9 * np.abs(ref[b])
                ratio = float((np.abs(got[b] - ref[b]) / bound).max())
                if ratio >= worst.ratio:
                    worst.ratio, worst.where = ratio, f"size {size} window {window} item {b}"
                np.testing.assert_allclose(got[b], ref[b], rtol=1e-9, atol=1e-12 * ref[b].max())


# ------------------------------------------------------------------------------------------- zk_polar_profile
POLAR_SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (257, 131), (181, 181), (182, 182), (1024, 1024)]


@pytest.mark.parametrize("shape", POLAR_SHAPES, ids=lambda s: "%dx%d" % s)
def test_polar_profile_against_scipy_interpolation(pk, worst, shape):
    """Thin, tiny, non-square and production-size maps; R = 128 and 129 around the 128 wide block; data above zero (fill
    value outside the clip range) and spanning zero; the three aggregations; centres in the middle, in two corners and
    off-centre.  Bound 1e-12 of max |data| (1e-11 at 1024 x 1024: what the two CPU statements differ by there, from
    sin / cos of different libraries times the radius times the data's gradient)."""
    h, w = shape
    rng = np.random.default_rng(41)
    tol = 1e-11 if shape == (1024, 1024) else 1e-12
    assert pr.polar_radii(181, 181) == 128 and pr.polar_radii(182, 182) == 129
    centres = list(dict.fromkeys([None, (0, 0), (h - 1, w - 1), (h // 3, (w // 2 + 1) % w)]))
    for kind, data in (("positive", rng.random(shape) + 0.5), ("spanning", rng.standard_normal(shape))):
        scale = np.abs(data).max()
        for center in centres:
            for method in ("max", "mean", "sum"):
                got = pk.radial_profile(data, center=center, method=method)
                ref = pr.radial_profile_ref(data, center, method)
                assert got.shape == (pr.polar_radii(h, w),)
                worst.check(f"{kind} centre {center} {method}", got, ref, tol, scale)


@pytest.mark.parametrize("stack_shape", [(5, 48, 48), (130, 33, 33)], ids=lambda s: "%dx%dx%d" % s)
def test_polar_profiles_batched_entry_item_by_item(pk, worst, stack_shape):
    """_radial_profiles (centre -1, method max, per-item clip range): items alternate between positive-only and
    zero-spanning and change scale by 1e3 from one to the next, each against its own single-item reference."""
    n, h, w = stack_shape
    rng = np.random.default_rng(42)
    stack = np.empty(stack_shape)
    for b in range(n):
        item = rng.random((h, w)) + 0.5 if b % 2 == 0 else rng.standard_normal((h, w))
        stack[b] = item * 1e3 ** (b % 3)
    got = pk._radial_profiles(stack)
    assert got.shape == (n, pr.polar_radii(h, w))
    for b in range(n):
        worst.check(f"item {b}", got[b], pr.radial_profile_ref(stack[b], None, "max"), 1e-12, np.abs(stack[b]).max())


# ------------------------------------------------------------------------------------------- zk_autocorr_mean
AC_SHAPE = (131, 260)


@pytest.fixture(scope="module")
def ac_img():
    return np.random.default_rng(51).standard_normal(AC_SHAPE)


@pytest.mark.parametrize("ws", (2, 3, 8, 31, 33, 50))
def test_autocorr_mean_against_the_direct_lag_sum(pk, ac_img, worst, ws):
    """Odd and even windows (the 'same' crop is centred at ws / 2), corner and random origins, 1 / 2 / 5 windows (300 at
    the small sizes, where the direct sum is cheap), standardised and raw, float64 and float32."""
    rng = np.random.default_rng(ws)
    origins = corners_and_random(rng, *AC_SHAPE, ws, 296)
    img32 = ac_img.astype(np.float32)
    for n in (1, 2, 5, 300) if ws <= 8 else (1, 2, 5):
        org = origins[4:4 + n] if n == 1 else origins[:n]                 # a random origin alone; else the corners first
        for standardize in (True, False):
            ref = pr.autocorr_mean_ref(ac_img, ws, org, standardize)
            worst.check(f"n {n} standardize {standardize} float64", pk._autocorr_mean(ac_img, ws, org, standardize), ref,
                        1e-12, np.abs(ref).max())
            if n == 2 or ws <= 8:
                ref = pr.autocorr_mean_ref(img32.astype(np.float64), ws, org, standardize)
                worst.check(f"n {n} standardize {standardize} float32", pk._autocorr_mean(img32, ws, org, standardize), ref,
                            1e-12, np.abs(ref).max())


def test_autocorr_mean_window_of_one_pixel(pk, ac_img, worst):
    """Window 1, not standardised: the autocorrelation is the pixel squared, averaged over the windows."""
    for org in ([(130, 259)], [(0, 0), (130, 259), (5, 7), (64, 128), (130, 0)]):
        ref = pr.autocorr_mean_ref(ac_img, 1, org, False)
        worst.check(f"{len(org)} windows", pk._autocorr_mean(ac_img, 1, org, False), ref, 1e-12, np.abs(ref).max())


def test_autocorr_mean_one_constant_window_among_valid_ones(pk, ac_img):
    img = ac_img.copy()
    img[40:48, 60:68] = 3.0
    org = [(0, 0), (123, 252), (40, 60), (0, 252), (123, 0), (17, 101)]
    with pytest.raises(ValueError, match="Standard deviation is zero"):
        pr.autocorr_mean_ref(img, 8, org, True)
    with pytest.raises(ValueError, match="Standard deviation is zero"):
        pk._autocorr_mean(img, 8, org, True)
    for dtype in (np.float64, np.float32):                                # not standardised, the same windows are fine
        ref = pr.autocorr_mean_ref(img.astype(dtype).astype(np.float64), 8, org, False)
        np.testing.assert_allclose(pk._autocorr_mean(img.astype(dtype), 8, org, False), ref, rtol=0, atol=1e-12 * np.abs(ref).max())


# ------------------------------------------------------------------------------------------- zk_denoise_fft
DENOISE_SHAPES = [(1, 7), (7, 1), (2, 2), (5, 3), (33, 64), (97, 101), (100, 36), (255, 257)]


def p_for(k, n):
    """A fraction whose ceil(p n) is k whatever the rounding of the product."""
    return 1.0 if k == n else (k - 0.5) / n


def cut_cases(n):
    """k = 1, 2, an odd and an even k next to n / 2, n - 1 and n (p = 1)."""
    return sorted({k for k in (1, 2, n // 2, n // 2 + 1, n - 1, n) if 1 <= k <= n})


def survivors(out, image):
    return int(np.count_nonzero(np.abs(np.fft.fft2(out)) > 1e-9 * np.abs(np.fft.fft2(image)).max()))


def check_denoise(worst, pk, image, k, label):
    """One (image, k): the precondition from the reference's powers alone, then the device result and its survivor count.
    Returns (device result, whether the cut splits a conjugate pair)."""
    ref = pr.denoise_fft_ref(image, p_for(k, image.size))
    assert ref.k == k
    decided, splits = pr.denoise_cut(ref, image.shape)
    assert decided, f"{label}: another power within 1e-9 of the cut -- pick another seed"
    got = pk.denoise_fft(image, p_for(k, image.size))
    worst.check(label, got, ref.out, 1e-12, np.abs(image).max())
    assert survivors(ref.out, image) == k + (1 if splits else 0), label    # the statement about the reference itself
    assert survivors(got, image) == k + (1 if splits else 0), label        # half a pair comes back as two halves
    return got, splits


@pytest.mark.parametrize("shape", DENOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_denoise_fft_thin_prime_and_extreme_cuts(pk, worst, shape):
    """White noise at 1-pixel-thin, prime and mixed-radix extents; k at both ends and on either side of n / 2.  The cut is
    decided by the reference's powers alone (no other power within 1e-9 of it), so the kept set is known: exactly k
    coefficients survive, k + 1 when the cut keeps one half of a conjugate pair."""
    image = np.random.default_rng(61).standard_normal(shape)
    seen_split = False
    for k in cut_cases(image.size):
        seen_split |= check_denoise(worst, pk, image, k, f"k {k} of {image.size}")[1]
    if image.size > 4:
        assert seen_split                                 # an odd and an even k next to each other: one of them splits


def test_denoise_fft_zero_and_constant_images(pk):
    for shape in ((5, 3), (33, 64)):
        for p in (1e-3, 0.5, 1.0):
            assert np.all(pk.denoise_fft(np.zeros(shape), p) == 0)
    for shape in ((33, 64), (97, 101)):
        for c in (2.5, -0.375):
            np.testing.assert_allclose(pk.denoise_fft(np.full(shape, c), 0.01), np.full(shape, c), rtol=0, atol=1e-12)


def test_denoise_fft_plans_evicted_and_transposed(pk, worst):
    """More shapes than the plan cache holds (four), (ny, nx) followed by (nx, ny), then the first shape again: every
    result matches its reference and the repeat equals the first result bit for bit (cuts that split no tie)."""
    rng = np.random.default_rng(62)
    shapes = [(96, 128), (128, 96), (33, 64), (97, 101), (100, 36), (64, 64)]
    images = {s: rng.standard_normal(s) for s in shapes}

    def whole_cut(image):                                 # the first k from n / 10 up whose cut splits no pair
        for k in range(image.size // 10, image.size // 10 + 8):
            decided, splits = pr.denoise_cut(pr.denoise_fft_ref(image, p_for(k, image.size)), image.shape)
            if decided and not splits:
                return k
        raise AssertionError("no whole cut among eight consecutive k")

    first = None
    for s in shapes + [shapes[0]]:
        k = whole_cut(images[s])
        got, splits = check_denoise(worst, pk, images[s], k, f"shape {s} k {k}")
        assert not splits
        if first is None:
            first = got
    np.testing.assert_array_equal(got, first)


# ------------------------------------------------------------------------------------------- zk_wavelet_sigma
def test_wavelet_sigma_on_quantised_images(po, pk):
    """Integer-valued images (four grey levels) as uint8, uint16 and float32, with an odd and with an even count of
    non-zero |dd| coefficients; then images tiled from a 4 x 4 block, whose interior coefficients take only four values,
    so that the median falls deep inside a run of equal keys."""
    rng = np.random.default_rng(71)
    parities, largest = set(), 0.0
    for shape in ((64, 64), (65, 37), (4, 4)):
        for dtype in (np.uint8, np.uint16, np.float32):
            for tiled in (False, True):
                x = rng.integers(0, 4, (4, 4) if tiled else shape)
                if tiled:
                    x = np.tile(x, (shape[0] // 4 + 1, shape[1] // 4 + 1))[:shape[0], :shape[1]]
                x = x.astype(dtype)
                d = np.abs(po.db2_diagonal_details(x))
                if tiled and d.size > 100:
                    assert np.unique(d.round(12)).size < d.size // 4      # ties, and many of them
                parities.add(int(np.count_nonzero(d)) % 2)
                ref, got = po.estimate_sigma(x), pk.estimate_sigma(x)
                largest = max(largest, abs(got - ref))
                assert abs(got - ref) < 1e-13, (shape, dtype, tiled)
    print(f"\n[wavelet sigma] largest |difference| {largest:.3e}")
    assert parities == {0, 1}                             # the median of an odd and of an even count of non-zero values
