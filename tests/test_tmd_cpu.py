"""CPU checks of mtflearn_amd.datasets.TMDImageSimulator: the host side (lattice, labels, defect draws) against what the
reference left in tests/golden/tmd_golden.npz, the NumPy oracle (tests/tmd_oracle.py) against the reference's masks and
Gaussian-mode images -- which shows on the CPU that the operation order the kernel copies is the right one -- the conditions
that keep the goldens meaningful, the C ABI table and every argument check, all before any device call.  The licence of
tests/test_gpu_tmd.py."""
import inspect
import os
import re

import numpy as np
import pytest

import tmd_cases as tc
import tmd_oracle as to
from mtflearn_amd import _native, datasets, resident

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["zk_tmd_render", "zk_tmd_render_dev"]


@pytest.fixture(scope="module")
def golden():
    return tc.load_golden()


@pytest.fixture(scope="module")
def sims():
    """One simulator per case with its lattice generated (the host side does not depend on ``use_fft``)."""
    out = {}
    for name in tc.CASES:
        sim = tc.build(datasets.TMDImageSimulator, name, True)
        sim.generate_lattice()
        out[name] = sim
    return out


def oracle_masks(sim, name, species, consistent=False):
    coords = sim._cached_coords
    site_labels = np.tile(np.array([b[2] for b in sim.basis]), len(sim.pts_all) // len(sim.basis))
    masks = []
    for label in species:
        own = np.flatnonzero(site_labels == label) if consistent else None
        masks.append(to.delta(sim.size, coords[label], to.scales(len(coords[label]), label, sim.vacancies, sim.dopants, own)))
    return masks


def test_signatures_and_defaults_are_the_references():
    cls = datasets.TMDImageSimulator
    spec = lambda f: [(p.name, p.default, p.kind) for p in inspect.signature(f).parameters.values()]
    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    E = inspect.Parameter.empty
    assert spec(cls.__init__) == [("self", E, P), ("size", (512, 512), P), ("a", 30, P), ("theta", 0.0, P), ("species_params", None, P),
                                  ("basis", None, P), ("use_fft", True, P)]
    assert spec(cls.add_single_vacancy) == [("self", E, P), ("label", 'X', P), ("index", None, P)]
    assert spec(cls.add_double_vacancy) == [("self", E, P), ("label", 'X', P), ("indices", None, P)]
    assert spec(cls.add_random_vacancies) == [("self", E, P), ("label", 'X', P), ("num_single", 0, P), ("num_double", 0, P), ("seed", None, P)]
    assert spec(cls.add_random_dopants) == [("self", E, P), ("label", 'TM', P), ("num_dopants", 0, P), ("dopant_intensity", 0.8, P),
                                            ("seed", None, P)]
    assert spec(cls.place_atoms_delta) == [("self", E, P), ("positions", E, P), ("scales", E, P)]
    assert spec(cls.gaussian_kernel) == [("self", E, P), ("size", E, P), ("sigma", E, P), ("A", E, P)]
    assert spec(cls.simulate) == [("self", E, P), ("return_masks", False, P), ("consistent_defects", False, K)]
    for name in ("rotation_matrix", "generate_lattice", "get_defect_counts"):
        assert spec(getattr(cls, name)) == [("self", E, P)]
    assert spec(cls.plot) == [("self", E, P), ("img", E, P)] and spec(cls.save) == [("self", E, P), ("img", E, P), ("path", E, P)]
    assert spec(resident.tmd_frames_device) == [("simulators", E, P), ("return_masks", False, P), ("out", None, P),
                                                ("consistent_defects", False, P)]
    sim = cls()
    assert sim.species_params == {'TM': {'sigma': 2.0, 'A': 1.0}, 'X': {'sigma': 1.5, 'A': 0.6}}
    assert sim.basis == [(0.0, 0.0, 'TM'), (1 / 3, 1 / 3, 'X')]
    assert (sim.vacancies, sim.dopants, sim.filtered_indices, sim.pts_all, sim.pts, sim.labels, sim.lbs, sim._cached_coords) == \
        ([], [], {}, None, None, None, None, None)
    with pytest.raises(ValueError, match="Run simulate"):
        sim.get_defect_counts()
    np.testing.assert_array_equal(sim.gaussian_kernel(5, 1.5, 0.6),
                                  0.6 * np.exp(-(np.arange(-2, 3)[None] ** 2 + np.arange(-2, 3)[:, None] ** 2) / (2 * 1.5 ** 2)))
    assert "TMDImageSimulator" in datasets.__all__ and "tmd_frames_device" not in resident.__all__
    left_out = datasets.__doc__.split("Left out:")[1].split("\n\n")[0]
    assert "TMDImageSimulator" not in left_out and "first appearance" in datasets.__doc__ and "consistent_defects" in datasets.__doc__


@pytest.mark.parametrize("name", list(tc.CASES))
def test_host_side_equals_the_reference(golden, sims, name):
    sim = sims[name]
    record = tc.host_record(sim)
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/") and k.split("/")[1] not in tc.MODES}
    assert set(record) == set(want)
    for key, value in want.items():
        assert record[key].dtype == value.dtype or value.dtype.kind == "U", (key, record[key].dtype, value.dtype)
        np.testing.assert_array_equal(record[key], value, err_msg=f"{name}/{key}")
    assert sim.labels.dtype == golden[f"{name}/labels"].dtype               # the reference's string width
    assert sim.pts_all.dtype == np.float64 and sim.pts.flags.c_contiguous
    assert all(type(i) is int for i in sim.filtered_indices[tc.species_of(name)[0]][:5])
    assert list(sim._cached_coords) == tc.species_of(name) == sim._species()
    stacked = np.empty_like(sim.pts_all)
    k = len(sim.basis)
    for pos, (_, _, label) in enumerate(sim.basis):                         # every case's basis names each species once
        stacked[pos::k] = sim._cached_coords[label]
    np.testing.assert_array_equal(stacked, sim.pts_all)


def test_the_rotation_form_is_the_per_site_product(sims):
    """``R @ pos`` site by site, as the reference does it, on the in-frame sites of the rotated cases."""
    for name in ("C", "E"):
        sim = sims[name]
        R = sim.rotation_matrix()
        a1, a2 = sim.a * np.array([1, 0]), sim.a * np.array([0.5, np.sqrt(3) / 2])
        height, width = sim.size
        nx, ny = int(width // sim.a * 2) + 4, int(height // (sim.a * np.sqrt(3) / 2) * 2) + 4
        sites = []
        for i in range(-nx, nx):
            for j in range(-ny, ny):
                base = i * a1 + j * a2
                for dx, dy, _ in sim.basis:
                    sites.append(R @ (base + dx * a1 + dy * a2))
        np.testing.assert_array_equal(np.array(sites), sim.pts_all)


@pytest.mark.parametrize("name", list(tc.CASES))
def test_oracle_reproduces_the_reference(golden, sims, name):
    """The masks in every case; the Gaussian-mode image for up to two species (with three the reference's order is its own)."""
    sim = sims[name]
    for mode in tc.MODES:
        species = list(golden[f"{name}/{mode}/species"])
        masks = oracle_masks(sim, name, species)
        np.testing.assert_array_equal(np.stack(masks), golden[f"{name}/{mode}/masks"], err_msg=f"{name}/{mode}")
    params = [tc.params_of(name, s) for s in species]
    image = to.gauss_image(masks, params)
    assert image.dtype == np.float32
    if len(species) <= 2:
        np.testing.assert_array_equal(image, golden[f"{name}/gauss/image"])
    else:                                                   # the recorded order of the walk reproduces it, too
        np.testing.assert_array_equal(image, golden[f"{name}/gauss/image"])
        assert list(species) != tc.species_of(name)
    E = to.exact_image(masks, params)
    e_ref = np.abs(golden[f"{name}/fft/image"].astype(np.float64) - E).max()
    assert e_ref == float(golden[f"{name}/fft/e_ref"])
    print(f"case {name}: e_ref = {e_ref:.3e}, peak {E.max():.4f}, spacing32(peak) = {np.spacing(np.float32(E.max())):.3e}")
    assert e_ref <= 4e-7 * E.max()                          # a single-precision transform, not a wrong kernel


def test_goldens_are_meaningful(golden, sims):
    # B: a site within 1e-9 of a half-integer x, and rounding half to even differs from rounding half up there
    x = sims["B"].pts[:, 0]
    near = np.abs(x - np.floor(x) - 0.5) < 1e-9
    assert near.any()
    # D: a pixel with three or more atoms whose float32 sum depends on the order
    sim = sims["D"]
    found = 0
    for label in ("TM", "X"):
        atoms = sim._cached_coords[label]
        scales = to.scales(len(atoms), label, sim.vacancies, sim.dopants)
        forward = to.delta(sim.size, atoms, scales)
        backward = to.delta(sim.size, atoms[::-1], scales[::-1])
        counts = to.delta(sim.size, atoms, np.ones(len(atoms)))
        found += int(((forward != backward) & (counts >= 3)).sum())
        assert len(set(scales.tolist())) >= 4
    assert found >= 1
    print(f"case D: {found} pixels of 3+ atoms whose reversed float32 sum differs")
    # C: the reference's index mix-up is visible -- the default and the consistent frames differ, in both modes
    sim = sims["C"]
    assert len(sim.vacancies) == 6 and len(sim.dopants) == 4
    species = tc.species_of("C")
    params = [tc.params_of("C", s) for s in species]
    default, consistent = oracle_masks(sim, "C", species), oracle_masks(sim, "C", species, consistent=True)
    assert not np.array_equal(np.stack(default), np.stack(consistent))
    assert not np.array_equal(to.gauss_image(default, params), to.gauss_image(consistent, params))
    assert np.abs(to.exact_image(default, params) - to.exact_image(consistent, params)).max() > 0.1
    for label in species:                                   # the class's own scales are the oracle's, both ways
        n = len(sim._cached_coords[label])
        own = sim._index_of[label]
        np.testing.assert_array_equal(sim._scales(label, n, False), to.scales(n, label, sim.vacancies, sim.dopants))
        np.testing.assert_array_equal(sim._scales(label, n, True), to.scales(n, label, sim.vacancies, sim.dopants, own))
    # E: the halos the case is there for
    assert len(to.fft_half_kernel(6.0)) - 1 == 18 and len(to.gauss_half_kernel(6.0)) - 1 == 24 > tc.CASES["E"]["size"][0]
    assert os.path.getsize(tc.GOLDEN) < 300 * 1024


def test_layers_handed_to_the_device(sims):
    """Per species, in order of first appearance: the on-frame atoms in order, the amplitude and the oracle's half kernel."""
    for name in tc.CASES:
        for mode, use_fft in tc.MODES.items():
            sim = tc.build(datasets.TMDImageSimulator, name, use_fft)
            layers = sim._layers()
            assert [layer[0] for layer in layers] == tc.species_of(name)
            for label, points, amp, w in layers:
                p = tc.params_of(name, label)
                np.testing.assert_array_equal(w, to.fft_half_kernel(p['sigma']) if use_fft else to.gauss_half_kernel(p['sigma']))
                assert amp == p['A'] and points.dtype == np.float64 and points.shape[1] == 3
                atoms = sim._cached_coords[label]
                scales = to.scales(len(atoms), label, sim.vacancies, sim.dopants)
                np.testing.assert_array_equal(to.delta(sim.size, points[:, :2], points[:, 2]), to.delta(sim.size, atoms, scales))
                assert len(points) <= len(atoms) and len(points) == int(to.delta(sim.size, atoms, np.ones(len(atoms))).sum())


def test_symbols_are_declared_bound_and_built():
    text = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    assert re.search(r"#define ZK_ABI_VERSION 2\b", text)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.load()
    assert lib.zk_abi_version() == 2
    for sym in SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    assert re.search(r"#define ZK_TMD_FFT\s+0\b", header) and re.search(r"#define ZK_TMD_GAUSSIAN\s+1\b", header)
    assert (_native.TMD_FFT, _native.TMD_GAUSSIAN) == (0, 1)
    makefile = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bzk_tmd\.hip\b", makefile, flags=re.M)
    assert re.search(r"^\$\(OBJDIR\)/zk_tmd\.o: CXXFLAGS \+= -ffp-contract=off$", makefile, flags=re.M)
    from mtflearn_amd import distributed
    assert distributed.tmd_frames_device is resident.tmd_frames_device


def test_library_refuses_bad_arguments_without_a_device():
    """Both entry points check everything before they look for a device: ZK_E_BADARG and a message, never 'no device'."""
    lib = _native.load()
    p = lambda a: None if a is None else a.ctypes.data_as(_native.c_void_p)
    frames, masks = np.zeros((2, 4, 5), np.float32), np.zeros((3, 4, 5), np.float32)
    good = dict(frames=frames, masks=masks, dtype=_native.ZK_F32, B=2, H=4, W=5, L=3, layer_frame=np.array([0, 0, 1], np.int32),
                point_offsets=np.array([0, 2, 3, 4], np.int64), points=np.array([[1, 1, 1], [2, 2, .5], [0, 0, 1], [3, 3, 1]], np.float64),
                amps=np.array([1.0, 0.6, 1.0]), weight_offsets=np.array([0, 2, 3, 6], np.int64), weights=np.array([1, .5, 1, 1, .5, .25]),
                mode=_native.TMD_FFT)
    nan_points, inf_weights = good["points"].copy(), good["weights"].copy()
    nan_points[1, 0], inf_weights[4] = np.nan, np.inf
    changes = [dict(dtype=_native.ZK_F64), dict(dtype=7), dict(mode=2), dict(mode=-1), dict(B=0), dict(H=0), dict(W=-1), dict(L=-1),
               dict(frames=None), dict(layer_frame=None), dict(point_offsets=None), dict(points=None), dict(amps=None),
               dict(weights=None), dict(weight_offsets=None), dict(weights=None, weight_offsets=None, masks=None),
               dict(point_offsets=np.array([0, 3, 2, 4], np.int64)),                    # decreasing
               dict(point_offsets=np.array([1, 2, 3, 4], np.int64)),                    # not from 0
               dict(layer_frame=np.array([0, 1, 0], np.int32)),                         # a frame's layers not consecutive
               dict(layer_frame=np.array([0, 0, 2], np.int32)), dict(layer_frame=np.array([-1, 0, 1], np.int32)),
               dict(weight_offsets=np.array([0, 2, 2, 6], np.int64)),                   # a layer without w[0]: r = -1
               dict(weight_offsets=np.array([0, 3, 2, 6], np.int64)),
               dict(weight_offsets=np.array([1, 2, 3, 6], np.int64)),
               dict(points=nan_points), dict(weights=inf_weights), dict(amps=np.array([1.0, np.nan, 1.0]))]
    for change in changes:
        a = {**good, **change}
        tail = (a["dtype"], a["B"], a["H"], a["W"], a["L"], p(a["layer_frame"]), p(a["point_offsets"]), p(a["points"]), p(a["amps"]),
                p(a["weight_offsets"]), p(a["weights"]), a["mode"])
        for name, extra in (("zk_tmd_render", ()), ("zk_tmd_render_dev", (None,))):
            rc = getattr(lib, name)(0, p(a["frames"]), p(a["masks"]), *tail, *extra)
            assert rc == _native.ZK_E_BADARG and "zk_tmd_render" in _native.last_error(), (name, list(change))
    wide = np.ones(962 + 2)
    rc = lib.zk_tmd_render(0, p(frames), None, _native.ZK_F32, 2, 4, 5, 1, p(np.zeros(1, np.int32)), p(np.array([0, 1], np.int64)),
                           p(good["points"]), p(np.ones(1)), p(np.array([0, 962], np.int64)), p(wide), 1)
    assert rc == _native.ZK_E_BADARG and "960" in _native.last_error()


def test_python_refusals_and_the_device_requirement():
    cls = datasets.TMDImageSimulator
    with pytest.raises(ValueError, match="at least one"):
        resident.tmd_frames_device([])
    with pytest.raises(ValueError, match="share one size"):
        resident.tmd_frames_device([cls(size=(8, 8)), cls(size=(8, 9))])
    with pytest.raises(ValueError, match="share one size"):
        resident.tmd_frames_device([cls(size=(8, 8)), cls(size=(8, 8), use_fft=False)])
    three = cls(size=(8, 8), basis=tc.CASES["E"]["basis"])
    with pytest.raises(ValueError, match="same number of species"):
        resident.tmd_frames_device([cls(size=(8, 8)), three], return_masks=True)
    fake = lambda shape, dtype: _native.DeviceArray(shape, dtype, 0, _base=object(), _ptr=4096)
    for out in (np.zeros((1, 8, 8), np.float32), fake((1, 8, 8), np.float64), fake((8, 8), np.float32), fake((2, 8, 8), np.float32)):
        with pytest.raises(ValueError, match="out must be"):
            resident.tmd_frames_device([cls(size=(8, 8))], out=out)
    sim = cls(size=(16, 16), a=6)
    if _native.device_count() > 0:
        assert sim.simulate().shape == (16, 16)
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            sim.simulate()
        with pytest.raises(RuntimeError, match="no HIP device"):
            sim.place_atoms_delta(np.zeros((1, 2)), np.ones(1))
        assert sim.pts is not None and sim.get_defect_counts()         # the lattice and the labels are there all the same
