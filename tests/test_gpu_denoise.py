"""mtflearn_amd.denoise on the GPU: the four window operations of csrc/zk_denoise.hip against their NumPy form
(tests/denoise_oracle.py), the two denoisers against the goldens captured from the reference and against scikit-learn on the
materialised matrix, the degenerate cases (constant frames, a single window, tiny patches), and the device-resident chain."""
import os
import warnings
from ctypes import c_void_p

import numpy as np
import pytest

import denoise_oracle as do
import make_golden_denoise as mg
import mtflearn_amd
import mtflearn_amd._denoise_svd as svd_mod
import mtflearn_amd.denoise as denoise_pkg
from conftest import ROOT
from mtflearn_amd import _native
from mtflearn_amd.synthetic import honeycomb_frame

pytestmark = pytest.mark.gpu

# Parity of the end-to-end calls: max|got - golden| <= TOL * max|golden|, TOL = max(100 * d0, 1e-12).  d0 = 4.4e-16 is the
# largest relative difference between tests/denoise_oracle.py and the reference over the golden cases (two float64
# evaluations of the same mathematics; measured by tests/make_golden_denoise.py and stored in the fixture), so TOL sits at
# its floor, 1e-12.  The bare operations: elementwise rtol 1e-12 with an absolute floor of 1e-13 * max|result|.
# Worst differences observed on an MI355X, as a fraction of max|golden| (singular values / ratios: relative):
#   denoise_svd   case 0 (8 px, k 3, default step)      1.7e-15   s 8.9e-16
#                 case 1 (12 px, k 4, step 3)           1.3e-15   s 1.6e-15
#                 case 2 (8 px, k 6, step 1)            2.2e-15   s 1.8e-15
#                 case 3 (8 x 12 px, k 4, default step) 3.1e-15   s 1.4e-15
#                 case 4 (8 x 12 px, k 2, step 3)       1.5e-15   s 1.0e-15
#   memory view   case 0 (8 px, k 3)                    8.8e-16   explained_variance_ratio 1.7e-16 absolute
#                 case 1 (8 px, threshold 0.9 -> 5)     9.2e-16   1.7e-16
#                 case 2 (12 px, k 4)                   8.7e-16   1.1e-16
#                 case 3 (8 px, threshold 0.7 -> 3)     8.8e-16   1.7e-16
#   bare operations: 2.5e-15 of max|result| or better (apply, apply_t, moments), 0 (reconstruct)
D0_MEASURED = 4.4e-16
DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "denoise_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def tol(gold):
    assert float(gold["d0"]) <= 2 * D0_MEASURED
    return max(100 * float(gold["d0"]), 1e-12)


@pytest.fixture(scope="module")
def frame(gold):
    f = mg.golden_frame()
    assert mg.frame_digest(f) == str(gold["frame_sha256"])
    return f


def random_frame(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.issubdtype(dtype, np.floating):
        return (rng.random(shape) * 3 - 0.5).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(max(info.min, -3000), min(info.max, 4000), shape).astype(dtype)


def ptr(a):
    return a.ctypes.data_as(c_void_p) if a is not None else None


def grid_args(ii, jj):
    ii, jj = np.ascontiguousarray(ii, np.int32), np.ascontiguousarray(jj, np.int32)
    return ii, jj, (ptr(ii), len(ii), ptr(jj), len(jj))


def op_apply(img, ph, pw, ii, jj, q, mean=None):
    lib = _native.load()
    ii, jj, g = grid_args(ii, jj)
    out = np.empty((len(ii) * len(jj), q.shape[1]))
    _native.check(lib.zk_windows_apply(0, ptr(img), _native.dtype_code(img.dtype), *img.shape, ph, pw, *g, ptr(q), q.shape[1], ptr(mean),
                                       ptr(out)), "zk_windows_apply")
    return out


def op_apply_t(img, ph, pw, ii, jj, y):
    lib = _native.load()
    ii, jj, g = grid_args(ii, jj)
    out = np.empty((ph * pw, y.shape[1]))
    _native.check(lib.zk_windows_apply_t(0, ptr(img), _native.dtype_code(img.dtype), *img.shape, ph, pw, *g, ptr(y), y.shape[1], ptr(out)),
                  "zk_windows_apply_t")
    return out


def op_moments(img, ph, pw):
    lib = _native.load()
    mean, cov = np.empty(ph * pw), np.empty((ph * pw, ph * pw))
    _native.check(lib.zk_windows_moments(0, ptr(img), _native.dtype_code(img.dtype), *img.shape, ph, pw, ptr(mean), ptr(cov)),
                  "zk_windows_moments")
    return mean, cov


def op_reconstruct(shape, ph, pw, ii, jj, y, v=None, mean=None):
    lib = _native.load()
    ii, jj, g = grid_args(ii, jj)
    out = np.empty(shape)
    y = np.ascontiguousarray(y, dtype=np.float64)
    _native.check(lib.zk_windows_reconstruct(0, *shape, ph, pw, *g, ptr(y), 0 if v is None else v.shape[0], ptr(v), ptr(mean), ptr(out)),
                  "zk_windows_reconstruct")
    return out


def close(got, want, what=""):
    """Elementwise rtol 1e-12, absolute floor 1e-13 * max|want|; the figure is printed before it is asserted."""
    want = np.asarray(want)
    scale = np.abs(want).max()
    err = np.abs(got - want)
    print(f"{what}: max|diff| / max|want| = {err.max() / (scale or 1.0):.3e}")
    assert np.all(err <= 1e-12 * np.abs(want) + 1e-13 * scale), what


GRIDS = [  # (shape, (ph, pw), row origins, column origins)
    ((40, 53), (8, 8), do.origins(40, 8, 2), do.origins(53, 8, 2)),
    ((40, 53), (5, 9), do.origins(40, 5, 3), do.origins(53, 9, 3)),                  # the appended last origin
    ((37, 70), (12, 6), [0, 1, 7, 20, 25], [0, 3, 4, 30, 31, 64]),                   # any ascending list
    ((21, 18), (20, 17), [0, 1], [0, 1]),                                             # fewer windows than pixels per window
    ((30, 33), (4, 4), np.arange(27), np.arange(30)),                                 # dense
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [1, 7, 20, 64])
def test_apply_and_apply_t(dtype, l):
    rng = np.random.default_rng(l)
    for k, (shape, (ph, pw), ii, jj) in enumerate(GRIDS):
        img = random_frame(shape, dtype, 10 + k)
        q = np.ascontiguousarray(rng.standard_normal((ph * pw, l)))
        mean = np.ascontiguousarray(rng.standard_normal(ph * pw) + 1.0)
        y = np.ascontiguousarray(rng.standard_normal((len(ii) * len(jj), l)))
        close(op_apply(img, ph, pw, ii, jj, q), do.apply(img, ph, pw, ii, jj, q), f"apply grid {k}")
        close(op_apply(img, ph, pw, ii, jj, q, mean), do.apply(img, ph, pw, ii, jj, q, mean), f"apply centred grid {k}")
        close(op_apply_t(img, ph, pw, ii, jj, y), do.apply_t(img, ph, pw, ii, jj, y), f"apply_t grid {k}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_moments(dtype):
    for k, (shape, patch) in enumerate([((40, 53), (8, 8)), ((33, 47), (5, 9)), ((64, 50), (12, 12)), ((9, 9), (8, 8)),
                                        ((8, 8), (8, 8)), ((30, 20), (12, 3)), ((100, 90), (32, 32) if dtype == np.float64 else (16, 16))]):
        img = random_frame(shape, dtype, 30 + k)
        mean, cov = op_moments(img, *patch)
        want_mean, want_cov = do.moments(img, *patch)
        close(mean, want_mean, f"window mean {shape} {patch}")
        close(cov, want_cov, f"window covariance {shape} {patch}")
        np.testing.assert_array_equal(cov, cov.T)


def test_moments_of_a_frame_with_a_large_offset():
    """The covariance is formed about the frame's mean: an offset a million times the signal costs no digits of the result's scale."""
    img = random_frame((48, 40), np.float64, 3) * 1e-3 + 1e3
    mean, cov = op_moments(img, 6, 6)
    want_mean, want_cov = do.moments(img - 1e3, 6, 6)            # the oracle on the shifted frame: same covariance
    np.testing.assert_allclose(mean, want_mean + 1e3, rtol=1e-14)
    assert np.abs(cov - want_cov).max() <= 1e-9 * np.abs(want_cov).max()        # 1e3 / 1e-3 ... eps of the pixels themselves


@pytest.mark.parametrize("k", [1, 3, 8])
def test_reconstruct(k):
    rng = np.random.default_rng(k)
    for n, (shape, (ph, pw), ii, jj) in enumerate(GRIDS):
        y = rng.standard_normal((len(ii) * len(jj), k))
        v = np.ascontiguousarray(rng.standard_normal((k, ph * pw)))
        mean = rng.standard_normal(ph * pw)
        want = do.reconstruct(shape, ph, pw, ii, jj, y, v, mean)
        got = op_reconstruct(shape, ph, pw, ii, jj, y, v, mean)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))             # pixels under no window: 0 / 0
        ok = ~np.isnan(want)
        close(got[ok], want[ok], f"reconstruct grid {n}")
        batch = rng.standard_normal((len(y), ph, pw))
        got = op_reconstruct(shape, ph, pw, ii, jj, batch)
        want = do.reconstruct(shape, ph, pw, ii, jj, batch)
        close(got[ok], want[ok], f"reconstruct batch grid {n}")
    assert np.isnan(do.reconstruct(GRIDS[2][0], 12, 6, GRIDS[2][2], GRIDS[2][3], np.zeros((30, 1)), np.zeros((1, 72)))).any()


def test_bad_grids_are_refused():
    lib = _native.load()
    img, q, out = np.zeros((20, 20)), np.zeros((16, 2)), np.zeros((4, 2))
    for ii, jj in (([0, 17], [0, 4]), ([4, 0], [0, 4]), ([0, 0], [0, 4]), ([-1, 3], [0, 4])):
        i32, j32, g = grid_args(ii, jj)
        assert lib.zk_windows_apply(0, ptr(img), _native.ZK_F64, 20, 20, 4, 4, *g, ptr(q), 2, None, ptr(out)) != 0
    assert lib.zk_windows_moments(0, ptr(img), _native.ZK_F64, 20, 20, 49, 4, ptr(out), ptr(out)) != 0
    assert lib.zk_windows_moments(0, ptr(img), _native.ZK_F64, 20, 20, 21, 4, ptr(out), ptr(out)) != 0


def test_repeat_runs_are_bit_identical(frame):
    ii, jj = do.origins(96, 8, 2), do.origins(120, 8, 2)
    rng = np.random.default_rng(0)
    q, y = rng.standard_normal((64, 13)), rng.standard_normal((len(ii) * len(jj), 13))
    for fn in (lambda: op_apply(frame, 8, 8, ii, jj, q), lambda: op_apply_t(frame, 8, 8, ii, jj, y), lambda: op_moments(frame, 8, 8)[1],
               lambda: op_reconstruct(frame.shape, 8, 8, ii, jj, y[:, :5], q[:, :5].T.copy())):
        first = fn()
        for _ in range(2):
            np.testing.assert_array_equal(fn(), first)
    np.random.seed(4)
    first = mtflearn_amd.denoise_svd(frame, 8, 3, verbose=False)
    np.random.seed(4)
    np.testing.assert_array_equal(mtflearn_amd.denoise_svd(frame, 8, 3, verbose=False), first)
    a = denoise_pkg.denoise_svd_memory_view(frame, 8, 3)
    b = denoise_pkg.denoise_svd_memory_view(frame, 8, 3)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------- end to end
def svd_case(gold, k):
    step = int(gold[f"svd{k}_step"])
    return (tuple(int(v) for v in gold[f"svd{k}_patch"]), int(gold[f"svd{k}_n_components"]), None if step < 0 else step,
            int(gold[f"svd{k}_seed"]))


def test_denoise_svd_against_the_reference(gold, frame, tol, capsys):
    for k in range(int(gold["n_svd_cases"])):
        patch, n, step, seed = svd_case(gold, k)
        patch_arg = patch[0] if patch[0] == patch[1] else patch
        want, want_s = gold[f"svd{k}_img_clean"], gold[f"svd{k}_s"]
        np.random.seed(seed)
        got, s = mtflearn_amd.denoise_svd(frame, patch_arg, n, extraction_step=step, verbose=False, return_s=True)
        np.random.seed(seed)
        model = mtflearn_amd.DenoiseSVD(frame, n_components=n, patch_size=patch_arg, extraction_step=step)
        assert model.run() is model.img_clean
        np.testing.assert_array_equal(model.img_clean, got)
        np.testing.assert_array_equal(model.s_values, s)
        d = np.abs(got - want).max() / np.abs(want).max()
        with capsys.disabled():
            print(f"denoise_svd case {k}: patch {patch} k {n} step {step}: {d:.3e} of max|golden|, s {np.abs(s / want_s - 1).max():.3e}")
        assert got.dtype == np.float64 and got.shape == frame.shape
        assert d <= tol
        np.testing.assert_allclose(s, want_s, rtol=tol)


def test_denoise_svd_against_scikit_learn_on_the_materialised_matrix(gold, frame, tol):
    from sklearn.utils.extmath import randomized_svd
    for k in range(int(gold["n_svd_cases"])):
        (ph, pw), n, step, seed = svd_case(gold, k)
        st = max(1, int(ph / 4)) if step is None else step
        ii, jj = do.origins(96, ph, st), do.origins(120, pw, st)
        a = do.window_matrix(frame, ph, pw, ii, jj)
        np.random.seed(seed)
        u, s, vt = randomized_svd(a, n, random_state=None)
        want = do.overlap_add((u * s) @ vt, frame.shape, ph, pw, ii, jj)
        np.random.seed(seed)
        got, got_s = mtflearn_amd.denoise_svd(frame, (ph, pw), n, extraction_step=step, verbose=False, return_s=True)
        assert np.abs(got - want).max() <= tol * np.abs(want).max()
        np.testing.assert_allclose(got_s, s, rtol=tol)
        np.testing.assert_allclose(got_s[-1], gold[f"svd{k}_cut"][0], rtol=1e-9)          # and the exact value at the cut


def test_denoise_svd_transposed_case_and_progress_lines(tol, capsys):
    """Fewer windows than pixels per window: scikit-learn factors the transpose, and draws an (N, k + 10) test matrix."""
    from sklearn.utils.extmath import randomized_svd
    img = honeycomb_frame(40, 44, seed=2).astype(np.float64)
    ii, jj = do.origins(40, 24, 6), do.origins(44, 24, 6)
    a = do.window_matrix(img, 24, 24, ii, jj)
    assert 12 < a.shape[0] < a.shape[1]
    exact = np.linalg.svd(a, compute_uv=False)
    assert (exact[1] - exact[2]) / exact[0] >= 1e-3              # the conditioning floor of the golden cases
    np.random.seed(9)
    u, s, vt = randomized_svd(a, 2, random_state=None)
    want = do.overlap_add((u * s) @ vt, img.shape, 24, 24, ii, jj)
    np.random.seed(9)
    got = mtflearn_amd.denoise_svd(img, 24, 2)
    lines = capsys.readouterr().out.splitlines()
    assert [ln for ln in lines if not ln.startswith("done in")] == ["Extracting reference patches...", "Singular value decomposition...",
                                                                      "Reconstructing..."]
    assert sum(ln.startswith("done in") and ln.endswith("s.") for ln in lines) == 3
    assert np.abs(got - want).max() <= tol * np.abs(want).max()


def test_memory_view_against_the_reference(gold, frame, tol, capsys):
    for k in range(int(gold["n_view_cases"])):
        n_in = int(gold[f"view{k}_n_components_in"])
        recon, ratio, n = denoise_pkg.denoise_svd_memory_view(frame, int(gold[f"view{k}_patch"]), n_components=None if n_in < 0 else n_in,
                                                             threshold=float(gold[f"view{k}_threshold"]), show_progress=False)
        want = gold[f"view{k}_recon"]
        d = np.abs(recon - want).max() / np.abs(want).max()
        with capsys.disabled():
            print(f"memory view case {k}: {d:.3e} of max|golden|, ratio {np.abs(ratio - gold[f'view{k}_explained_variance_ratio']).max():.3e}")
        assert n == int(gold[f"view{k}_n_components"]) and isinstance(n, int)
        assert d <= tol
        want_ratio = gold[f"view{k}_explained_variance_ratio"]
        np.testing.assert_allclose(ratio, want_ratio, rtol=tol)


@pytest.mark.parametrize("patch,want_step", [(3, 1), (2, 1), (4, 1), (7, 1), (8, 2), ((9, 4), 2)])
def test_default_step_is_a_quarter_of_the_patch_height_and_never_zero(patch, want_step):
    """Patches under 4 px would give a step of 0: the default is max(1, height // 4), and the call equals the explicit one."""
    rng = np.random.default_rng(12)
    image = rng.random((19, 23))
    np.random.seed(1)
    got = mtflearn_amd.denoise_svd(image, patch, 2, verbose=False)
    np.random.seed(1)
    want = mtflearn_amd.denoise_svd(image, patch, 2, extraction_step=want_step, verbose=False)
    assert got.shape == image.shape and np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape,patch,n_components", [((8, 8), 8, 1), ((8, 8), 8, None), ((11, 7), 7, 3), ((6, 9), 3, None), ((8, 8), 3, None),
                                                      ((8, 8), 3, 2)])
@pytest.mark.parametrize("value", [1.0, 0.3, 0.0, -2.5])
def test_memory_view_of_a_frame_without_variance(shape, patch, n_components, value):
    """A constant frame, down to a single window: the covariance has no variance to share out, so the ratio is all zero (not
    NaN: no division happens, hence no RuntimeWarning), an unset n_components becomes 1, and the frame comes back."""
    image = np.full(shape, value)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        recon, ratio, n = denoise_pkg.denoise_svd_memory_view(image, patch_size=patch, n_components=n_components, show_progress=False)
    np.testing.assert_allclose(recon, image, rtol=1e-14, atol=0)
    assert ratio.shape == (patch * patch,) and not ratio.any()
    assert n == (1 if n_components is None else n_components)


def test_memory_view_single_window_with_variance():
    """One window only: the reference divides its covariance by 1, not by N - 1 = 0; every eigenvalue is zero, one component."""
    image = np.random.default_rng(4).random((6, 6))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        recon, ratio, n = denoise_pkg.denoise_svd_memory_view(image, patch_size=6)
    np.testing.assert_allclose(recon, image, rtol=1e-13)
    assert n == 1 and np.isfinite(ratio).all()


def test_reconstruct_patches_on_a_callers_batch():
    rng = np.random.default_rng(8)
    for shape, patch, step in (((23, 31), (5, 5), 2), ((23, 31), (4, 7), 3), (20, (6, 6), 6)):
        h, w = (shape, shape) if np.isscalar(shape) else shape
        ii, jj = do.origins(h, patch[0], step), do.origins(w, patch[1], step)
        batch = rng.standard_normal((len(ii) * len(jj),) + patch)
        want = do.overlap_add(batch, (h, w), patch[0], patch[1], ii, jj)
        close(denoise_pkg.reconstruct_patches(batch, shape, step), want, f"reconstruct_patches {shape}")
    img = rng.random((23, 31))
    close(denoise_pkg.reconstruct_patches(denoise_pkg.extract_patches(img, 5, 3), img.shape, 3), img, "extract then reconstruct")


@pytest.mark.parametrize("kind", ["native", "torch"])
def test_device_resident_chain(frame, kind):
    from mtflearn_amd import ZPs
    from mtflearn_amd.distributed import (denoise_svd_device, denoise_svd_memory_view_device, local_max_device,
                                          points_moments_device, remove_background_device)
    img32 = frame.astype(np.float32)
    if kind == "torch":
        torch = pytest.importorskip("torch")
        up = lambda a: torch.from_numpy(a).cuda()
        down = lambda t: t.cpu().numpy()
    else:
        up, down = _native.DeviceArray.from_numpy, lambda t: t.numpy()
    for img in (frame, img32):
        np.random.seed(5)
        want, want_s = mtflearn_amd.denoise_svd(img, 8, 3, verbose=False, return_s=True)
        np.random.seed(5)
        got, s = denoise_svd_device(up(img), 8, 3, return_s=True)
        assert type(got) is type(up(img))
        np.testing.assert_array_equal(down(got), want)
        np.testing.assert_array_equal(s, want_s)
        want = denoise_pkg.denoise_svd_memory_view(img, 8)
        got = denoise_svd_memory_view_device(up(img), 8)
        np.testing.assert_array_equal(down(got[0]), want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert got[2] == want[2]
    residual, _ = remove_background_device(got[0], "opening", 15)                      # the next two steps take it as it is
    peaks = down(local_max_device(residual, 5.0))
    assert len(peaks) > 0
    inner = peaks[(peaks.min(axis=1) >= 8) & (peaks[:, 0] < 120 - 8) & (peaks[:, 1] < 96 - 8)].astype(np.int32)
    assert len(inner) > 0
    zps = ZPs(n_max=6, size=16)
    moments = points_moments_device(zps._device_plan(), got[0], up(np.ascontiguousarray(inner)))       # the last link, float64 frame
    host = zps.transform_at(down(got[0]), inner).data
    assert tuple(moments.shape) == host.shape and np.isfinite(down(moments)).all()
    np.testing.assert_allclose(down(moments), host, rtol=1e-9, atol=1e-12 * np.abs(host).max())
    with pytest.raises(ValueError, match="strictly smaller"):
        denoise_svd_device(up(frame), 96, 3)
    cube = up(np.zeros((2, 16, 16)))
    with pytest.raises(ValueError, match="needs a 2D image"):
        denoise_svd_device(cube, 4, 1)
    with pytest.raises(ValueError, match="needs a 2D image"):
        denoise_svd_memory_view_device(cube, 4)


def test_full_size_frame():
    """2048^2 float32, 32 px, default step, 8 components: the operations against the oracle on a 256^2 crop (same code path,
    same grid step), and shape / finiteness / cover at full size."""
    big = honeycomb_frame(2048, 2048, seed=1)
    assert big.dtype == np.float32
    crop = np.ascontiguousarray(big[512:768, 1024:1280])
    ii = do.origins(256, 32, 8)
    rng = np.random.default_rng(2)
    q, y = rng.standard_normal((1024, 18)), rng.standard_normal((len(ii) ** 2, 18))
    close(op_apply(crop, 32, 32, ii, ii, q), do.apply(crop, 32, 32, ii, ii, q), "apply, crop")
    close(op_apply_t(crop, 32, 32, ii, ii, y), do.apply_t(crop, 32, 32, ii, ii, y), "apply_t, crop")
    v = np.ascontiguousarray(q[:, :8].T)
    close(op_reconstruct(crop.shape, 32, 32, ii, ii, y[:, :8], v), do.reconstruct(crop.shape, 32, 32, ii, ii, y[:, :8], v), "reconstruct, crop")
    np.random.seed(3)
    clean, s = mtflearn_amd.denoise_svd(big, 32, 8, verbose=False, return_s=True)
    assert clean.shape == big.shape and clean.dtype == np.float64 and np.isfinite(clean).all()
    assert s.shape == (8,) and np.all(np.diff(s) <= 0) and s[-1] > 0
    jj = do.origins(2048, 32, 8)
    ones = op_reconstruct((2048, 2048), 32, 32, jj, jj, np.ones((len(jj) ** 2, 1)), np.ones((1, 1024)))
    np.testing.assert_array_equal(ones, 1.0)                               # sum of ones over the cover: every pixel covered
