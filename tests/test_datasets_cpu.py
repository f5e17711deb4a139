"""mtflearn_amd.datasets without a GPU: the NumPy statement of the gather (tests/datasets_oracle.py) against goldens captured from
the reference (tests/make_golden_datasets.py), everything the package computes on the host (lattice coordinates, noise models,
argument checks) against the same goldens, and the new entry points in header, loader table and library."""
import inspect
import os
import re

import numpy as np
import pytest

import datasets_cases as dc
import datasets_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, datasets


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "datasets_golden.npz")) as f:
        return {k: f[k] for k in f.files}


# ------------------------------------------------------------------------------------------------ the oracle is the reference
@pytest.mark.parametrize("name", sorted(dc.render_cases()))
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_oracle_equals_the_reference(golden, name, dtype):
    case = dc.render_cases()[name]
    got, k = oracle.render(dc.case_frame(case, dtype), case["pts"], case["amps"], case["sigma"], case["r_factor"])
    ref = golden[f"render/{name}/{np.dtype(dtype).name}"]
    assert got.dtype == ref.dtype == dtype and k >= 1
    np.testing.assert_array_equal(got, ref)


def test_order_changes_the_reference_and_the_oracle_follows(golden):
    values = {}
    for name, amplitudes in dc.ORDER_AMPLITUDES.items():
        case = dc.order_case(amplitudes)
        got, k = oracle.render(dc.case_frame(case, np.float32), case["pts"], case["amps"], case["sigma"], case["r_factor"])
        np.testing.assert_array_equal(got, golden[f"order/{name}"])
        assert k == 3
        values[name] = got[5, 6]
    assert values["big_one_minus"] == np.float32(0.0) and values["big_minus_one"] == np.float32(1.0)


@pytest.mark.parametrize("name", sorted(dc.PATCHES))
def test_oracle_patches_equal_the_reference(golden, name):
    kw = dict(include_center=True, relative_center_intensity=1)
    kw.update(dc.PATCHES[name])
    size, sigma, center, radius = kw["size"], kw["size"] / 10, kw["size"] / 2, kw["size"] / 3
    for b, rotation in enumerate(np.linspace(0, 2 * np.pi, kw["num_patches"], endpoint=False)):
        pts = [(center, center)] if kw["include_center"] else []
        amps = [kw["relative_center_intensity"]] if kw["include_center"] else []
        for fold in range(kw["n_fold"]):
            angle = fold * (2 * np.pi / kw["n_fold"]) + rotation
            pts.append((center + radius * np.cos(angle), center + radius * np.sin(angle)))
            amps.append(1.0)
        got, _ = oracle.render(np.zeros((size, size), np.float32), pts, amps, sigma, r_factor=0.0, taper=False)
        np.testing.assert_array_equal(got / got.max(), golden[f"patches/{name}"][b])


# ------------------------------------------------------------------------------------------------ the kernel-level inputs
def _oracle(case, dtype=np.float32):
    return oracle.render(dc.case_frame(case, dtype), case["pts"], case["amps"], case["sigma"], case["r_factor"])[0]


@pytest.mark.parametrize("layout", ["consecutive", "spread"])
@pytest.mark.parametrize("L", dc.SEAM_LENGTHS)
def test_order_probes_read_as_stated_and_flip_when_swapped(L, layout):
    """What tests/test_gpu_datasets_kernels.py asserts of the device, in the oracle's float32 model: every probed pixel is 1.0
    (the 1 last) or 0.0 (the 1 second), nothing else is touched, and exchanging the last two points of each triple flips it."""
    case, expect = dc.order_probe_case(L, layout)
    assert len(expect) <= L // 3 and (L >= 3) == bool(expect) and len(case["pts"]) == L
    if L >= 3 * (dc.TILE - 2) ** 2:
        assert len(expect) > 180                                         # nearly every pixel the tile offers
    values = set(v.item() for v in expect.values())
    assert values <= {0.0, 1.0} and (len(expect) < 2 or values == {0.0, 1.0})
    pts = case["pts"]
    assert (pts == np.round(pts)).all() and pts.min() >= dc.TILE + 1 and pts.max() <= 2 * dc.TILE - 2     # boxes stay in the tile
    got = _oracle(case)
    flipped = _oracle(dc.swapped_last_two(case, L, layout))
    rest = np.ones(case["shape"], bool)
    for pixel, value in expect.items():
        assert got[pixel].tobytes() == value.tobytes() and flipped[pixel] == np.float32(1.0) - value, (L, layout, pixel)
        rest[pixel] = False
    assert not got[rest].any() and not flipped[rest].any()
    # the triples reach every window seam of the list
    idx = np.flatnonzero(case["amps"])
    assert all(((idx // 256) == w).any() for w in range(-(-L // 256))) or L < 3


def test_seam_lists_have_exactly_L_entries():
    R = 3.0
    for L in dc.SEAM_LENGTHS:
        pts = dc.seam_random_case(L)["pts"]
        assert len(pts) == L and np.floor(pts - R).min() >= dc.TILE and np.ceil(pts + R).max() <= 2 * dc.TILE - 1


def test_uncut_probe_reads_as_stated():
    case, expect = dc.uncut_probe_case()
    assert case["counts"] == [257, 257, 601, 601, 256, 256] and [e.item() for e in expect] == [1.0, 0.0] * 3
    got, _ = oracle.render_batch(np.zeros(case["shape"], np.float32), case["pts"], case["amps"], case["counts"], case["sigma"])
    assert [got[b][dc.UNCUT_PROBE_PIXEL].tobytes() for b in range(6)] == [e.tobytes() for e in expect]
    swapped = case["amps"].copy()
    for start, idx in zip(np.cumsum([0] + case["counts"][:-1]), [i for i in dc.UNCUT_PROBE_INDICES for _ in range(2)]):
        swapped[start + idx[1]], swapped[start + idx[2]] = swapped[start + idx[2]], swapped[start + idx[1]]
    got, _ = oracle.render_batch(np.zeros(case["shape"], np.float32), case["pts"], swapped, case["counts"], case["sigma"])
    assert [got[b][dc.UNCUT_PROBE_PIXEL].item() for b in range(6)] == [0.0, 1.0] * 3
    # a window walked backwards shows where a whole triple lies inside it: (1e8, -1e8, 1) reads 0.0 from the back
    backwards = case["amps"][-512:-256][::-1]
    got, _ = oracle.render_batch(np.zeros((1, 19, 23), np.float32), case["pts"][:256], backwards, [256], case["sigma"])
    assert got[0][dc.UNCUT_PROBE_PIXEL].item() == 0.0


def test_many_tile_frames_cover_the_scan():
    for shape in dc.MANY_TILES_SHAPES:
        case = dc.many_tiles_case(shape)
        h, w = shape
        tiles_x, tiles_y = -(-w // dc.TILE), -(-h // dc.TILE)
        assert 1024 < tiles_x * tiles_y <= 2048 and len(case["pts"]) == 60
        inside = case["pts"][(case["pts"][:, 0] >= 0) & (case["pts"][:, 0] < w) & (case["pts"][:, 1] >= 0) & (case["pts"][:, 1] < h)]
        tile = (inside[:, 1] // dc.TILE).astype(int) * tiles_x + (inside[:, 0] // dc.TILE).astype(int)
        assert {0, tiles_x * tiles_y - 1, tiles_x - 3, tiles_x - 2, tiles_x - 1} <= set(tile.tolist())
        assert len(set((tile // 2).tolist())) > 25                       # scan lanes with something to add
    assert dc.many_tiles_case((33, 8200))["pts"][:, 0].max() > 8192      # the remainder columns


def test_cut_edge_case_is_exact_at_r_equal_R():
    case = dc.cut_edge_case()
    plain = oracle.render(dc.case_frame(case, np.float64), case["pts"], case["amps"], case["sigma"], case["r_factor"], taper=False)[0]
    tapered = _oracle(case, np.float64)
    (x, y), a = case["pts"][0].astype(int), case["amps"][0]
    for pixel in [(y, x + 3), (y, x - 3), (y + 3, x), (y - 3, x)]:
        assert plain[pixel] == a * np.exp(-4.5) and tapered[pixel].tobytes() == np.float64(0.0).tobytes()
    assert np.count_nonzero(plain) == 29 and np.count_nonzero(tapered) == 25


# ------------------------------------------------------------------------------------------------ host parts of the package
@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_coordinates_equal_the_reference(golden, name):
    ctor, _ = dc.LATTICES[name]
    lat = datasets.HoneyCombLattice(**ctor)
    pts_a, pts_b = lat.get_points()
    np.testing.assert_array_equal(lat._coords_A, golden[f"lattice/{name}/coords_A"])
    np.testing.assert_array_equal(lat._coords_B, golden[f"lattice/{name}/coords_B"])
    np.testing.assert_array_equal(pts_a, golden[f"lattice/{name}/points_A"])
    np.testing.assert_array_equal(pts_b, golden[f"lattice/{name}/points_B"])
    assert lat._coords_A.dtype == np.float64 and lat._coords_A.shape == ((2 * lat.N + 1) ** 2, 2)


def test_set_angle_and_no_shift(golden):
    lat = datasets.HoneyCombLattice(size=40, l=7.5, angle=3.0, random_shift=False)
    assert lat.shift_u1 == 0.0 and lat.shift_u2 == 0.0
    lat.get_points()
    lat.set_angle(-21.0)
    assert lat._coords_A is None and lat.angle_deg == -21.0
    pts_a, pts_b = lat.get_points()
    np.testing.assert_array_equal(pts_a, golden["lattice/set_angle/points_A"])
    np.testing.assert_array_equal(pts_b, golden["lattice/set_angle/points_B"])


def test_render_lists_are_a_then_b_within_reach():
    lat = datasets.HoneyCombLattice(size=96, l=12, seed=0, angle=17)
    sigma, pts, amps = lat._render_lists(None, 1.0, 0.5)
    assert sigma == 3.0 and pts.dtype == np.float64 and pts.shape == (len(amps), 2)
    n_a = int((amps == 1.0).sum())
    assert (amps[:n_a] == 1.0).all() and (amps[n_a:] == 0.5).all() and 0 < n_a < len(amps)
    assert pts.min() >= -9 and pts.max() <= 95 + 9


def test_error_messages_are_the_references():
    with pytest.raises(ValueError, match=r"^Inconsistent 'a' and 'l': got a=20\.0, l=12\.0, but for ideal graphene expect "
                                         r"a≈sqrt\(3\)\*l≈20\.784610\.$"):
        datasets.HoneyCombLattice(l=12, a=20.0)
    assert datasets.HoneyCombLattice(l=12, a=12 * np.sqrt(3.0)).a == 12 * np.sqrt(3.0)
    img = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match="^img must be a 2D array$"):
        datasets.add_tapered_gaussian(np.zeros((2, 2, 2), np.float32), [[0, 0]], 1.0)
    with pytest.raises(ValueError, match=r"^pts must have shape \(N, 2\)$"):
        datasets.add_tapered_gaussian(img, [0.0, 1.0, 2.0], 1.0)
    with pytest.raises(ValueError, match="^If amplitude is array-like, its length must match number of points$"):
        datasets.add_tapered_gaussian(img, [[0, 0], [1, 1]], 1.0, amplitude=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="^sigma must be positive$"):
        datasets.add_tapered_gaussian(img, [[0, 0]], 0.0)
    with pytest.raises(ValueError, match="^counts_per_pixel must be positive.$"):
        datasets.apply_poisson_noise(img, 0)
    with pytest.raises(ValueError, match="^sigma must be non-negative.$"):
        datasets.add_gaussian_noise(img, sigma=-1)
    with pytest.raises(ValueError, match="^counts_per_pixel must be positive.$"):
        datasets.apply_poisson_gaussian_noise(img, -1, 0.1)
    with pytest.raises(ValueError, match="^sigma must be non-negative.$"):
        datasets.apply_poisson_gaussian_noise(img, 1, -0.1)
    with pytest.raises(ValueError, match="^noisy_img and clean_img must have same shape.$"):
        datasets.estimate_counts_per_pixel_mle(img, img[:2])
    with pytest.raises(ValueError, match="^mask must match image shape.$"):
        datasets.estimate_counts_per_pixel_mle(img + 1, img + 1, mask=np.ones((2, 2), bool))
    with pytest.raises(ValueError, match="^No valid pixels to fit counts_per_pixel.$"):
        datasets.estimate_counts_per_pixel_mle(img, img)
    assert datasets.estimate_counts_per_pixel_mle(img + 1, img + 1) == np.inf
    # nothing to draw: no device is asked for
    assert datasets.add_tapered_gaussian(img, np.empty((0, 2)), 1.0) is img and not img.any()


def test_noise_models_equal_the_reference(golden):
    img = dc.noise_image()
    noisy, counts = datasets.apply_poisson_noise(img, 50.0, return_counts=True, seed=3)
    for got, key in ((noisy, "noise/poisson"), (counts, "noise/poisson_counts"), (datasets.add_gaussian_noise(img, sigma=0.2, seed=4), "noise/gaussian"),
                     (datasets.apply_poisson_gaussian_noise(img, 80.0, 0.05, seed=5), "noise/poisson_gaussian")):
        assert got.dtype == golden[key].dtype == np.float32
        np.testing.assert_array_equal(got, golden[key])
    assert datasets.estimate_counts_per_pixel_mle(noisy, img) == golden["noise/mle"]
    assert datasets.estimate_counts_per_pixel_mle(noisy, img, mask=img > 0.5, s_min=0.1) == golden["noise/mle_mask"]


def test_signatures_are_the_references():
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.kind != p.KEYWORD_ONLY]
    E = inspect.Parameter.empty
    assert sig(datasets.add_tapered_gaussian) == [("img", E), ("pts", E), ("sigma", E), ("amplitude", 1), ("r_factor", 3.0)]
    assert sig(datasets.HoneyCombLattice.__init__)[1:] == [("size", 512), ("l", 12.0), ("a", None), ("angle", 0.0), ("random_shift", True),
                                                           ("seed", None), ("jitter", 0.0)]
    assert sig(datasets.HoneyCombLattice.to_image)[1:] == [("sigma", None), ("intensity_A", 1.0), ("intensity_B", 0.5), ("normalize", False)]
    assert sig(datasets.get_zps_test_image) == []
    assert sig(datasets.get_zps_test_patches) == [("size", 64), ("n_fold", 3), ("num_patches", 10), ("include_center", True),
                                                  ("relative_center_intensity", 1)]
    assert sig(datasets.generate_data_gn) == [("size", E), ("n", 6), ("sigma", None), ("include_center", True), ("radius_frac", 0.25),
                                              ("rotation_angle", 0.0)]
    assert sig(datasets.apply_poisson_noise) == [("img", E), ("counts_per_pixel", E), ("return_counts", False), ("seed", None)]
    assert sig(datasets.add_gaussian_noise) == [("img", E), ("sigma", 0.1), ("seed", None)]
    assert sig(datasets.apply_poisson_gaussian_noise) == [("img", E), ("counts_per_pixel", E), ("sigma", E), ("seed", None)]
    assert sig(datasets.estimate_counts_per_pixel_mle) == [("noisy_img", E), ("clean_img", E), ("mask", None), ("s_min", 1e-3)]


# ------------------------------------------------------------------------------------------------ the binding
def test_header_table_and_library_agree():
    header = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    assert re.search(r"#define ZK_ABI_VERSION 2\b", header)
    lib = _native.load()
    for sym in ("zk_render_gaussians", "zk_render_gaussians_dev"):
        assert sym in _native.SYMBOLS and hasattr(lib, sym)
        decl = re.search(rf"\bint {sym}\(([^;]*)\);", header).group(1)
        assert len(_native.SYMBOLS[sym][1]) == decl.count(",") + 1, sym
    makefile = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "Makefile")).read()
    assert "zk_datasets.hip" in makefile and re.search(r"zk_datasets\.o: CXXFLAGS \+= -ffp-contract=off", makefile)


def test_c_abi_rejects_bad_arguments():
    """Argument checks come before any device is touched."""
    lib = _native.load()
    from ctypes import c_void_p
    frame, pts, amps = np.zeros((4, 4), np.float32), np.zeros((1, 2)), np.ones(1)
    p = lambda a: a.ctypes.data_as(c_void_p)
    call = lambda **kw: lib.zk_render_gaussians(0, p(frame), kw.get("dtype", 0), kw.get("h", 4), kw.get("w", 4), kw.get("batch", 1),
                                                p(pts), p(amps), None, 1, kw.get("sigma", 1.0), kw.get("r", 3.0), kw.get("taper", 1), 0)
    for bad in (dict(dtype=2), dict(h=0), dict(sigma=0.0), dict(sigma=float("nan")), dict(r=0.0), dict(r=-1.0), dict(batch=2),
                dict(r=0.0, taper=0, batch=2), dict(r=float("inf"))):
        assert call(**bad) != 0, bad
        assert _native.last_error()
