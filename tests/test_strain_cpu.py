"""CPU tests of mtflearn_amd.strain: what licenses the oracle and the case table of the GPU tests, and everything the package
decides before its first device call.

* truth: on a uniformly strained two-cosine lattice with ``g`` on the FFT grid of a 96 x 128 frame the oracle recovers ``grad u``
  over the central half.  Measured (profiles/strain.txt): 9.94e-4 at the worst pixel and 1.44e-4 for the mean, of strains of
  order 1e-2 -- the second-order terms of a first-order method; the bounds are twice the measured distances.  The unstrained
  lattice gives ``|e| <= 1.54e-8``, the leakage of one spot into the other's mask (6 sigma apart: ``exp(-18) = 1.5e-8``).
* amplitude floor: in every case at most 1 % of the pixels have a stencil amplitude below ``AMP_FLOOR`` of the plane's maximum
  -- a condition on the cases, so that the GPU tests compare strain on (nearly) the whole frame.
"""
import os
import re

import numpy as np
import pytest

import strain_cases as sc
import strain_oracle as so
from conftest import ROOT

MAPS = ("exx", "eyy", "exy", "rotation")
TRUTH_PIXEL, TRUTH_MEAN, UNSTRAINED = 9.94e-4, 1.44e-4, 1.54e-8        # measured, see above


def truth_maps(grad_u):
    e = np.asarray(grad_u)
    return dict(exx=e[1][1], eyy=e[0][0], exy=(e[1][0] + e[0][1]) / 2, rotation=(e[0][1] - e[1][0]) / 2)


def test_oracle_recovers_uniform_strain():
    case = sc.by_name("96x128-f32-ongrid-uniform")
    frame = sc.lattice(96, 128, case["g"], sc.uniform(case["grad_u"], 96, 128))
    got, want = so.gpa(frame, case["g"]), truth_maps(case["grad_u"])
    half = (slice(24, 72), slice(32, 96))
    pixel = max(np.abs(got[k][half] - want[k]).max() for k in MAPS)
    mean = max(abs(got[k][half].mean() - want[k]) for k in MAPS)
    print(f"uniform strain, central half: worst pixel {pixel:.3e}, worst mean {mean:.3e}")
    assert pixel <= 2 * TRUTH_PIXEL and mean <= 2 * TRUTH_MEAN


def test_oracle_reference_removes_a_uniform_strain():
    """A rectangle inside a uniformly strained frame as the reference: the strain goes into ``G`` (the local Bragg vectors
    ``g (1 - grad u)`` to first order), and the maps vanish in the mean over the rectangle.  (Over the whole periodic frame the
    phase winds an integer number of times, so the mean gradient of that rectangle is quantised and says nothing.)"""
    case = sc.by_name("96x128-ref-large")
    y0, y1, x0, x1 = reference = (24, 72, 32, 96)           # the central half: three mask widths from the frame's seam
    got = so.gpa(case["frame"], case["g"], reference=reference)
    free = so.gpa(case["frame"], case["g"])
    assert all(abs(got[k][y0:y1, x0:x1].mean()) <= 1e-15 for k in MAPS)
    local = case["g"] @ (np.eye(2) - sc.GRAD_U)
    print(f"refined G against g (1 - grad u): {np.abs(got['g'] - local).max():.3e}")
    assert np.abs(got["g"] - local).max() <= 1e-4 < np.abs(got["g"] - case["g"]).max() and np.array_equal(free["g"], case["g"])


def test_unstrained_lattice_is_at_the_leakage_level():
    got = so.gpa(sc.lattice(96, 128, sc.G_ON_96x128), sc.G_ON_96x128)
    worst = max(np.abs(got[k]).max() for k in MAPS)
    print(f"unstrained lattice: max |e| {worst:.3e}")
    assert worst <= 2 * UNSTRAINED


def _frames(case):
    return case["frame"] if case["frame"].ndim == 3 else case["frame"][None]


@pytest.mark.parametrize("case", sc.CASES + [sc.stack_case()], ids=lambda c: c["name"])
def test_amplitude_floor(case):
    for frame in _frames(case):
        floor = so.stencil_floor(so.gpa(frame, case["g"], **sc.options(case))["amplitude"])
        share = (floor < sc.AMP_FLOOR).mean()
        print(f"{case['name']}: {share:.4f} of the pixels below the floor, smallest ratio {floor.min():.3e}")
        assert share <= sc.FLOOR_SHARE


def test_cases_are_named_once_and_phase_cases_exist():
    names = [c["name"] for c in sc.CASES]
    assert len(set(names)) == len(names) and set(sc.PHASE_CASES) <= set(names)


def _constant(name):
    text = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "zk_strain.hip")).read()
    m = re.search(rf"constexpr \w+ {name} = (?:\(size_t\))?(\d+)(?: << (\d+))?;", text)
    return int(m.group(1)) << int(m.group(2) or 0)


def test_edge_sizes_reach_what_they_are_for():
    """The sizes of the cases against the constants of csrc/zk_strain.hip: were a constant to change, the cases would quietly
    stop reaching the branches they were chosen for."""
    red, run = _constant("RED_PER_BLOCK"), _constant("RUN_BYTES")
    parts = lambda r: -(-(r[1] - r[0]) * (r[3] - r[2]) // red)
    assert red == 4096 and run == 1 << 30
    assert parts(sc.by_name("96x128-ref-large")["reference"]) == 2 and parts(sc.by_name("96x128-ref-whole")["reference"]) == 3
    assert parts(sc.by_name("96x128-ref-pixel")["reference"]) == 1
    y0, y1, x0, x1 = sc.by_name("96x128-ref-edges")["reference"]
    assert y0 == 0 and x1 == 128
    assert 96 * 128 > 256 and 61 * 67 % 256 and 4 * 5 < 64                          # several blocks, a ragged last block, less than a wave
    stack = sc.stack_case()["frame"]
    b, h, w = stack.shape
    budget = sc.run_bytes(h, w, sc.RUN_FRAMES)
    assert budget // (h * w * 48) == 2 and (b // 2, b % 2) == (2, 1)                # runs of 2 + 2 + 1 under the budget the test sets
    assert run // (h * w * 48) >= b                                                 # ... and one run under the default
    g = sc.by_name("64x48-g049")["g"]
    assert g[0][0] == 0.49 and 0.49 + 3 * so.default_sigma(g) > 0.5                 # the mask reaches past the Nyquist row


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture()
def no_device(monkeypatch):
    """Any device call would come through ``_native.load``: it must not be reached."""
    from mtflearn_amd import _native

    def refuse():
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_native, "load", refuse)


FRAME = np.zeros((8, 8))
G = [[0.25, 0.0], [0.0, 0.25]]


@pytest.mark.parametrize("kwargs, error", [
    (dict(g=[[0.25, 0.0, 0.0], [0.0, 0.25, 0.0]]), ValueError), (dict(g=[0.25, 0.0]), ValueError), (dict(g=[[np.nan, 0.0], [0.0, 0.25]]), ValueError),
    (dict(g=[[np.inf, 0.0], [0.0, 0.25]]), ValueError), (dict(g=[[0.25j, 0.0], [0.0, 0.25]]), ValueError),
    (dict(g=[[0.51, 0.0], [0.0, 0.25]]), ValueError), (dict(g=[[0.25, 0.0], [0.0, -0.6]]), ValueError),
    (dict(g=[[0.0, 0.0], [0.0, 0.25]]), ValueError), (dict(g=[[0.1, 0.2], [0.2, 0.4]]), ValueError),
    (dict(g=[[0.1, 0.2], [0.2, 0.4 + 1e-8]]), ValueError),
    (dict(sigma=0), ValueError), (dict(sigma=-0.1), ValueError), (dict(sigma=np.nan), ValueError), (dict(sigma=np.inf), ValueError),
    (dict(sigma="0.1"), ValueError),
    (dict(reference=(2, 2, 0, 4)), ValueError), (dict(reference=(0, 4, 5, 3)), ValueError), (dict(reference=(0, 9, 0, 4)), ValueError),
    (dict(reference=(-1, 4, 0, 4)), ValueError), (dict(reference=(0, 4, 0, 9)), ValueError), (dict(reference=(0, 4, 0)), ValueError),
    (dict(reference=(0.0, 4.0, 0.0, 4.0)), ValueError),
    (dict(window="hamming"), ValueError),
    (dict(image=np.zeros((3, 8))), ValueError), (dict(image=np.zeros((8, 3))), ValueError), (dict(image=np.zeros((2, 3, 8))), ValueError),
    (dict(image=np.zeros(8)), ValueError), (dict(image=np.zeros((2, 2, 8, 8))), ValueError), (dict(image=np.zeros((0, 8, 8))), ValueError),
    (dict(image=np.broadcast_to(np.float32(0), (4, 16385))), ValueError), (dict(image=np.broadcast_to(np.float32(0), (16385, 4))), ValueError),
    (dict(image=np.zeros((8, 8), np.complex128)), TypeError), (dict(image=np.zeros((2, 8, 8), np.complex64)), TypeError),
])
def test_gpa_argument_errors(no_device, kwargs, error):
    from mtflearn_amd import strain
    kwargs = dict(kwargs)
    image, g = kwargs.pop("image", FRAME), kwargs.pop("g", G)
    with pytest.raises(error):
        strain.gpa(image, g, **kwargs)


@pytest.mark.parametrize("kwargs, error", [
    (dict(image=np.zeros((2, 8, 8))), ValueError), (dict(image=np.zeros((8, 8), np.complex64)), TypeError), (dict(image=np.zeros((3, 8))), ValueError),
    (dict(window="hamming"), ValueError), (dict(dc_radius=-1), ValueError), (dict(dc_radius=np.nan), ValueError),
])
def test_pick_g_argument_errors(no_device, kwargs, error):
    from mtflearn_amd import strain
    kwargs = dict(kwargs)
    with pytest.raises(error):
        strain.pick_g(kwargs.pop("image", FRAME), **kwargs)


def test_default_sigma_is_a_sixth_of_the_shortest_spacing():
    from mtflearn_amd import strain
    g = np.array([[0.3, 0.0], [0.1, 0.1]])
    assert strain.default_sigma(g) == so.default_sigma(g) == np.hypot(0.1, 0.1) / 6


def test_header_and_native_table_agree_on_the_new_names():
    from mtflearn_amd import _native, strain
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zk_[a-z_0-9]+)\s*\(", text))
    for name in ("zk_gpa", "zk_gpa_dev", "zk_gpa_set_run_bytes"):
        assert name in declared and name in _native.SYMBOLS
    for name, value in (("ZK_GPA_WINDOW_NONE", strain._WINDOWS[None]), ("ZK_GPA_WINDOW_HANN", strain._WINDOWS["hann"])):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name
    source = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "zk_strain.hip")).read()
    assert "atomicAdd" not in source                                                # the sums are fixed trees


def test_resident_twin_exists():
    from mtflearn_amd import resident
    assert callable(resident.gpa_device)
