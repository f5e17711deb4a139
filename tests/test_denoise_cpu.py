"""mtflearn_amd.denoise without a GPU: the public names, the argument checks and messages the reference's interface
fixes (cases of this project's own, all before any device call), the randomized SVD restatement against scikit-learn, the test-local oracle (tests/denoise_oracle.py) against the goldens captured from the reference
(tests/make_golden_denoise.py), and the new C symbols of the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_oracle as do
import make_golden_denoise as mg
import mtflearn_amd
import mtflearn_amd._denoise_svd as svd_mod
import mtflearn_amd.denoise as denoise_pkg
from conftest import ROOT
from mtflearn_amd import _native


@pytest.fixture(scope="module")
def gold():
    with np.load(os.path.join(ROOT, "tests", "golden", "denoise_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def frame(gold):
    f = mg.golden_frame()
    assert f.shape == tuple(gold["frame_spec"][:2]) and f.dtype == np.float64
    assert mg.frame_digest(f) == str(gold["frame_sha256"]), "synthetic.honeycomb_frame no longer renders the golden frame"
    return f


# ---------------------------------------------------------------------------------------------- names
def test_denoise_module_exports_explicit_memory_view_name():
    assert hasattr(denoise_pkg, "DenoiseSVD")
    assert hasattr(denoise_pkg, "denoise_svd_memory_view")
    assert not hasattr(denoise_pkg, "denoise_svd")
    for name in ("extract_patches", "low_rank_svd", "reconstruct_patches", "denoise_fft", "apply_poisson_noise"):
        assert callable(getattr(denoise_pkg, name))
    assert set(denoise_pkg.__all__) >= {"DenoiseSVD", "denoise_svd_memory_view", "extract_patches", "denoise_fft", "apply_poisson_noise"}
    from mtflearn_amd.features.pickers import denoise_fft
    assert denoise_pkg.denoise_fft is denoise_fft


def test_top_level_names():
    assert mtflearn_amd.denoise_svd is svd_mod.denoise_svd
    assert mtflearn_amd.DenoiseSVD is svd_mod.DenoiseSVD is denoise_pkg.DenoiseSVD
    assert {"denoise_svd", "DenoiseSVD"} <= set(mtflearn_amd.__all__)
    from mtflearn_amd.distributed import denoise_svd_device, denoise_svd_memory_view_device
    assert callable(denoise_svd_device) and callable(denoise_svd_memory_view_device)


# ---------------------------------------------------------------------------------------------- argument checks (no device)
TOO_LARGE = "patch_size must be strictly smaller than the image dimensions."


@pytest.mark.parametrize("shape,patch", [((8, 8), 8), ((8, 8), 9), ((10, 14), (10, 3)), ((10, 14), (3, 14)), ((10, 14), (4, 20))])
def test_patch_svd_needs_a_patch_smaller_than_the_frame(shape, patch):
    """A patch that fills an axis leaves one origin on it; the reference refuses that, with this message, and so does every
    entry here, before any device call."""
    frame = np.zeros(shape)
    with pytest.raises(ValueError, match=TOO_LARGE):
        mtflearn_amd.denoise_svd(frame, patch, 1, verbose=False)
    with pytest.raises(ValueError, match=TOO_LARGE):
        mtflearn_amd.DenoiseSVD(frame, 1, patch, None).run()


def test_patch_svd_refuses_bad_steps_components_and_shapes():
    frame = np.zeros((16, 16))
    for step in (0, -2):
        with pytest.raises(ValueError, match="extraction_step must be a positive integer."):
            svd_mod.denoise_svd(frame, patch_size=4, n_components=1, extraction_step=step, verbose=False)
    for k in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n_components"):
            svd_mod.denoise_svd(frame, patch_size=4, n_components=k, verbose=False)
    with pytest.raises(ValueError, match="length-2"):
        svd_mod.denoise_svd(frame, patch_size=(4, 4, 4), n_components=1, verbose=False)
    with pytest.raises(ValueError, match="2D"):
        svd_mod.denoise_svd(np.zeros((4, 16, 16)), patch_size=4, n_components=1, verbose=False)


@pytest.mark.parametrize("step", [None, 1, 5])
def test_the_class_runs_whatever_the_module_calls_denoise_svd(monkeypatch, step):
    """``DenoiseSVD.run`` goes through the module attribute ``denoise_svd`` with its four settings and asks for the
    singular values: a stand-in put there sees them and its two results land in ``img_clean`` / ``s_values``."""
    frame = np.arange(30.0).reshape(5, 6)
    seen = []

    def stand_in(*args, **kwargs):
        names = ("img", "patch_size", "n_components", "extraction_step", "verbose", "return_s")
        call = dict(zip(names, args), **kwargs)
        seen.append(call)
        return call["img"] + 1.0, np.array([3.0, 2.0])

    monkeypatch.setattr(svd_mod, "denoise_svd", stand_in)
    model = denoise_pkg.DenoiseSVD(frame, n_components=2, patch_size=(2, 3), extraction_step=step)
    assert (model.patches, model.s_values, model.img_clean) == (None, None, None)
    for verbose in (False, True):
        out = model.run(verbose=verbose)
        np.testing.assert_array_equal(out, frame + 1.0)
        assert model.img_clean is out
        np.testing.assert_array_equal(model.s_values, [3.0, 2.0])
    assert [c["verbose"] for c in seen] == [False, True]
    for c in seen:
        assert c["img"] is frame and c["patch_size"] == (2, 3) and c["n_components"] == 2
        assert c["extraction_step"] == step and c["return_s"] is True


@pytest.mark.parametrize("patch,message", [((2, 3), "supports only square patches"), ((5, 4), "got patch_size=\\(5, 4\\)"),
                                           ((2, 2, 2), "patch_size must be an int or a length-2 tuple."), ((3,), "length-2 tuple"),
                                           (49, "at most 48"), (13, "at most the image dimensions"), (0, "at least 1")])
def test_memory_view_patch_checks(patch, message):
    frame = np.zeros((12, 64)) if patch in (13, 0) else np.zeros((64, 64))
    with pytest.raises(ValueError, match=message):
        denoise_pkg.denoise_svd_memory_view(frame, patch_size=patch, n_components=1, show_progress=False)


def test_memory_view_accepts_an_equal_pair():
    assert denoise_pkg._memory_view_patch((20, 30), (6, 6)) == 6 == denoise_pkg._memory_view_patch((20, 30), 6.0)
    assert denoise_pkg._memory_view_patch((8, 8), 8) == 8                 # a single window is allowed here


def test_patch_start_indices():
    f = svd_mod._patch_start_indices
    np.testing.assert_array_equal(f(20, 4, 4), [0, 4, 8, 12, 16])
    np.testing.assert_array_equal(f(20, 4, 3), [0, 3, 6, 9, 12, 15, 16])          # the last origin is appended
    np.testing.assert_array_equal(f(20, 4, 1), np.arange(17))
    np.testing.assert_array_equal(f(20, 4, 100), [0, 16])
    np.testing.assert_array_equal(f(5, 4, 2), [0, 1])
    for extent, patch, step in ((20, 4, 4), (96, 12, 3), (120, 8, 2), (9, 3, 1), (120, 12, 5)):
        np.testing.assert_array_equal(f(extent, patch, step), do.origins(extent, patch, step))
    for step in (0, -1):
        with pytest.raises(ValueError, match="extraction_step must be a positive integer."):
            f(20, 4, step)
    for patch in (20, 21):
        with pytest.raises(ValueError, match="patch_size must be strictly smaller than the image size."):
            f(20, patch, 1)


def test_extract_patches_is_the_window_matrix():
    rng = np.random.default_rng(3)
    img = rng.random((23, 31))
    for patch, step in ((5, 1), (5, 3), ((4, 7), 2), ((7, 4), 5)):
        ph, pw = (patch, patch) if np.isscalar(patch) else patch
        got = denoise_pkg.extract_patches(img, patch, step)
        want = do.window_matrix(img, ph, pw, do.origins(23, ph, step), do.origins(31, pw, step))
        assert got.shape == (want.shape[0], ph, pw)
        np.testing.assert_array_equal(got.reshape(len(got), -1), want)


def test_apply_poisson_noise_draws_from_the_global_state():
    img = np.linspace(0, 2, 48).reshape(6, 8)
    np.random.seed(11)
    got = denoise_pkg.apply_poisson_noise(img, dose_per_pixel=50)
    np.random.seed(11)
    counts = np.random.poisson(img * 50)
    np.testing.assert_array_equal(got, counts / counts.max() * img.max())
    assert got.dtype == img.dtype and got.max() == img.max()
    zeros = denoise_pkg.apply_poisson_noise(np.zeros((3, 3), np.float32))
    assert zeros.dtype == np.float32 and not zeros.any()


def test_component_selection_follows_the_reference_rules():
    sel = denoise_pkg._select_components
    cov = np.diag([5.0, 1.0, 3.0, 1.0])
    top, ratio, k = sel(cov, None, 0.75)
    np.testing.assert_allclose(ratio, [0.5, 0.3, 0.1, 0.1])
    assert k == 2 and top.shape == (4, 2)                     # cumulated 0.5 < 0.75, 0.8 is not
    assert sel(cov, None, 0.9)[2] == 3
    assert sel(cov, 10, 0.9)[2] == 4 and sel(cov, 0, 0.9)[2] == 1
    top, ratio, k = sel(np.zeros((4, 4)), None, 0.9)           # no variance: no warning, one component, ratio of zeros
    assert k == 1 and not ratio.any() and top.shape == (4, 1)


# ---------------------------------------------------------------------------------------------- oracle against the reference
def test_golden_cases_are_conditioned(gold):
    assert gold["n_svd_cases"] >= 5 and gold["n_view_cases"] >= 3
    for k in range(int(gold["n_svd_cases"])):
        hi, lo = gold[f"svd{k}_cut"]
        assert (hi - lo) / gold[f"svd{k}_s"][0] >= 1e-3
        np.testing.assert_allclose(gold[f"svd{k}_s"][-1], hi, rtol=1e-9)      # the randomized values are the exact ones here
    for k in range(int(gold["n_view_cases"])):
        hi, lo = gold[f"view{k}_cut"]
        ratio, n = gold[f"view{k}_explained_variance_ratio"], int(gold[f"view{k}_n_components"])
        assert (ratio[n - 1] - ratio[n]) / ratio[0] >= 1e-3                  # ratios are eigenvalues over their sum
        np.testing.assert_allclose((hi - lo) / hi, (ratio[n - 1] - ratio[n]) / ratio[n - 1], rtol=1e-9)
    assert 100 * float(gold["d0"]) <= 1e-8


def test_oracle_reproduces_the_reference_denoise_svd(gold, frame):
    worst = 0.0
    for k in range(int(gold["n_svd_cases"])):
        ph, pw = (int(v) for v in gold[f"svd{k}_patch"])
        step = int(gold[f"svd{k}_step"])
        np.random.seed(int(gold[f"svd{k}_seed"]))
        clean, s = do.denoise_svd(frame, (ph, pw), int(gold[f"svd{k}_n_components"]), None if step < 0 else step)
        want = gold[f"svd{k}_img_clean"]
        worst = max(worst, np.abs(clean - want).max() / np.abs(want).max(), np.abs(s - gold[f"svd{k}_s"]).max() / s[0])
    print(f"oracle against the reference, denoise_svd: {worst:.3e}")
    assert worst <= max(100 * float(gold["d0"]), 1e-12)


def test_oracle_reproduces_the_reference_memory_view(gold, frame):
    for k in range(int(gold["n_view_cases"])):
        n_in = int(gold[f"view{k}_n_components_in"])
        recon, ratio, n = do.denoise_svd_memory_view(frame, int(gold[f"view{k}_patch"]), None if n_in < 0 else n_in,
                                                      float(gold[f"view{k}_threshold"]))
        want = gold[f"view{k}_recon"]
        assert n == int(gold[f"view{k}_n_components"])
        assert np.abs(recon - want).max() <= 1e-12 * np.abs(want).max()
        np.testing.assert_allclose(ratio, gold[f"view{k}_explained_variance_ratio"], rtol=1e-12)


def test_oracle_operations_are_consistent():
    """apply / apply_t / reconstruct of the oracle compose to its denoisers; the covariance is NumPy's."""
    rng = np.random.default_rng(5)
    img = rng.random((19, 26))
    ii, jj = do.origins(19, 5, 3), do.origins(26, 7, 3)
    a = do.window_matrix(img, 5, 7, ii, jj)
    q, y = rng.standard_normal((35, 6)), rng.standard_normal((len(a), 4))
    mean = a.mean(axis=0)
    np.testing.assert_allclose(do.apply(img, 5, 7, ii, jj, q, mean), a @ q - mean @ q, rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(do.apply_t(img, 5, 7, ii, jj, y), (y.T @ a).T, rtol=1e-12)
    np.testing.assert_allclose(do.reconstruct(img.shape, 5, 7, ii, jj, a), img, rtol=1e-13)     # averaging equal patches
    mu, cov = do.moments(img, 4, 4)
    dense = do.window_matrix(img, 4, 4, range(16), range(23))
    np.testing.assert_allclose(cov, np.cov(dense, rowvar=False), rtol=1e-11, atol=1e-15)
    np.testing.assert_allclose(mu, dense.mean(axis=0))
    assert np.isnan(do.overlap_add(np.ones((1, 4)), (4, 4), 2, 2, [0], [0])[3, 3])                    # uncovered: 0 / 0


def test_restated_randomized_svd_is_scikit_learns_on_the_same_products(frame):
    """With NumPy products in place of the device's, the restated control flow returns scikit-learn's arrays to the bit:
    same draw from the global state, same LU / QR / SVD calls, same sign rule -- in both orientations."""
    from sklearn.utils.extmath import randomized_svd

    class HostWindows:
        def __init__(self, a):
            self.a, (self.n, self.d) = a, a.shape

        def apply(self, q):
            return self.a @ q

        def apply_t(self, y):
            return self.a.T @ y

    tall = do.window_matrix(frame, 8, 8, do.origins(96, 8, 2), do.origins(120, 8, 2))
    wide = do.window_matrix(frame[:40, :44], 24, 24, do.origins(40, 24, 6), do.origins(44, 24, 6))
    assert tall.shape[0] > tall.shape[1] and wide.shape[0] < wide.shape[1]
    for a, k in ((tall, 3), (tall, 7), (wide, 2)):
        np.random.seed(k)
        got = svd_mod._randomized_svd_windows(HostWindows(a), k)
        np.random.seed(k)
        want = randomized_svd(a, k, random_state=None)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


# ---------------------------------------------------------------------------------------------- the C surface
def test_new_symbols_are_exported_with_the_documented_signatures():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_native.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ["zk_windows_apply", "zk_windows_apply_t", "zk_windows_moments", "zk_windows_reconstruct"]
    for base in names:
        for name in (base, base + "_dev"):
            assert hasattr(lib, name), f"{name} is not exported"
            decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
            assert decl, f"{name} is not declared in include/zernike_hip.h"
            n_args = len([a for a in decl.group(1).split(",") if a.strip()])
            assert n_args == len(_native.SYMBOLS[name][1]), f"{name}: the ctypes table and the header disagree"
            assert ("hip_stream" in decl.group(1)) == name.endswith("_dev")
    assert "zk_denoise.hip" in open(os.path.join(ROOT, "motif-learn_amd", "csrc", "Makefile")).read()
