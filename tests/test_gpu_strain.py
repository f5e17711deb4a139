"""GPU tests of mtflearn_amd.strain and its resident twin (csrc/zk_strain.hip) over the case table of tests/strain_cases.py,
against the NumPy statement tests/strain_oracle.py (licensed by tests/test_strain_cpu.py) -- never against the truth:

* the complex planes ``H_k`` (the debug output of ``zk_gpa``) and the amplitudes within 1e-12 of the plane's largest magnitude,
  the project's bound for its FFT-based kernels;
* the refined ``G`` within ``n_roi eps pi / (2 pi)`` (a sum of ``n_roi`` gradients, each at most pi) plus what the plane bound
  leaves in a gradient, ``1e-12 (2 / r) / (2 pi)``, ``r`` the smallest stencil amplitude ratio in the rectangle;
* the strain maps, at the pixels whose stencil amplitudes are all at least ``AMP_FLOOR`` of the plane's maximum, within
  ``1e-12 (2 / r) ||inv(G)||_inf / (2 pi)``, ``r`` the smallest such ratio of the case: ``arg`` of a product of two numbers, each
  off by ``delta / r`` relatively, is off by at most ``2 delta / r``, and the rows of ``inv(G) / 2 pi`` sum those errors;
* ``phase`` (``arg`` of one number: ``1e-12 / r``) with an additional ``2 pi 4 eps (|gy| H + |gx| W)`` for the carrier;
* everything said to be bit for bit is compared with ``assert_array_equal``.

Every case prints its measured distance before it asserts (``pytest -s``; profiles/strain.txt records them).
"""
import functools

import numpy as np
import pytest

import strain_cases as sc
import strain_oracle as so

pytestmark = pytest.mark.gpu

BOUND = 1e-12
EPS = np.finfo(np.float64).eps
MAPS = ("exx", "eyy", "exy", "rotation")


@pytest.fixture(scope="module")
def strain():
    from mtflearn_amd import strain
    return strain


def up(array):
    from mtflearn_amd import _native
    return _native.DeviceArray.from_numpy(np.ascontiguousarray(array), 0)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's answer of a case: computed once, shared by every test that needs it, read-only."""
    case = sc.by_name(name)
    out = so.gpa(case["frame"], case["g"], **sc.options(case))
    for v in out.values():
        v.setflags(write=False)
    return out


def check_frame(name, got, want, g, reference, planes=None):
    """One frame of the device against the oracle's dict, by the bounds of the module docstring."""
    h, w = want["exx"].shape
    scale = np.abs(want["planes"]).max(axis=(1, 2))
    d_amp = (np.abs(got.amplitude - want["amplitude"]).max(axis=(1, 2)) / scale).max()
    print(f"{name}: amplitude {d_amp:.2e} of the plane's maximum")
    assert d_amp <= BOUND
    if planes is not None:
        d_planes = (np.abs(planes - want["planes"]).max(axis=(1, 2)) / scale).max()
        print(f"{name}: planes {d_planes:.2e} of the plane's maximum")
        assert d_planes <= BOUND
    floor = so.stencil_floor(want["amplitude"])
    if reference is None:
        np.testing.assert_array_equal(got.g, g)
    else:
        y0, y1, x0, x1 = reference
        n_roi, r_roi = (y1 - y0) * (x1 - x0), floor[y0:y1, x0:x1].min()
        tol_g = n_roi * EPS * np.pi / (2 * np.pi) + BOUND * (2 / r_roi) / (2 * np.pi)
        d_g = np.abs(got.g - want["g"]).max()
        print(f"{name}: refined G {d_g:.2e} (bound {tol_g:.2e})")
        assert d_g <= tol_g
    keep = floor >= sc.AMP_FLOOR
    r = floor[keep].min()
    tol = BOUND * (2 / r) * np.abs(np.linalg.inv(want["g"])).sum(axis=1).max() / (2 * np.pi)
    worst = max(np.abs(getattr(got, k) - want[k])[keep].max() for k in MAPS)
    print(f"{name}: strain maps {worst:.2e} (bound {tol:.2e}, r {r:.2e}, {keep.mean():.4f} of the pixels compared)")
    assert worst <= tol
    if got.phase is not None:
        centre = want["amplitude"] / want["amplitude"].max(axis=(1, 2), keepdims=True)
        for k in range(2):
            ok = centre[k] >= sc.AMP_FLOOR
            tol_p = BOUND / centre[k][ok].min() + 2 * np.pi * 4 * EPS * (abs(g[k][0]) * h + abs(g[k][1]) * w)
            d = np.abs(np.angle(np.exp(1j * (got.phase[k] - want["phase"][k]))))[ok].max()
            print(f"{name}: phase {k} {d:.2e} (bound {tol_p:.2e})")
            assert d <= tol_p


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c["name"])
def test_gpa(strain, case):
    """Every case of the table: the planes through the debug output, the amplitudes, ``G`` and the four maps; the display phase
    where the case is one of ``PHASE_CASES``."""
    name = case["name"]
    frames, options, _ = strain._checked_host(case["frame"], case["g"], case["sigma"], case["reference"], case["window"])
    maps, amp, g_out, phase, planes = strain._gpa_host(frames, options, name in sc.PHASE_CASES, planes=True)
    got = strain._result(maps, amp, g_out, phase, False)
    assert got.exx.shape == case["frame"].shape and got.amplitude.shape == (2,) + case["frame"].shape and got.g.shape == (2, 2)
    check_frame(name, got, oracle(name), case["g"], case["reference"], planes[0])
    public = strain.gpa(case["frame"], case["g"], return_phase=name in sc.PHASE_CASES, **sc.options(case))
    for a, b in zip(public, got):                            # the debug output changes nothing
        np.testing.assert_array_equal(a, b)


@functools.lru_cache(maxsize=None)
def stack_host():
    from mtflearn_amd import strain
    case = sc.stack_case()
    return strain.gpa(case["frame"], case["g"], return_phase=True, **sc.options(case))


def test_stack_runs(strain):
    """``B = 5`` under a budget of two frames: runs of 2 + 2 + 1 (the tail plans, the per-run offsets of every output); every
    frame equal to its single-frame call and to the default budget, bit for bit."""
    from mtflearn_amd import _native
    case = sc.stack_case()
    b, h, w = case["frame"].shape
    whole = stack_host()
    _native.gpa_set_run_bytes(sc.run_bytes(h, w, sc.RUN_FRAMES))
    try:
        runs = strain.gpa(case["frame"], case["g"], return_phase=True, **sc.options(case))
    finally:
        _native.gpa_set_run_bytes(0)
    assert runs.exx.shape == (b, h, w) and runs.amplitude.shape == (b, 2, h, w) and runs.g.shape == (b, 2, 2)
    for a, c in zip(runs, whole):
        np.testing.assert_array_equal(a, c)
    for k in range(b):
        one = strain.gpa(case["frame"][k], case["g"], return_phase=True, **sc.options(case))
        for a, c in zip(one, runs):
            np.testing.assert_array_equal(a, c[k])
        want = so.gpa(case["frame"][k], case["g"], **sc.options(case))
        check_frame(f"{case['name']} frame {k}", one, want, case["g"], case["reference"])


def test_two_runs_agree(strain):
    case = sc.by_name("61x67-f64-offgrid-bump-ref")
    first = strain.gpa(case["frame"], case["g"], return_phase=True, **sc.options(case))
    second = strain.gpa(case["frame"], case["g"], return_phase=True, **sc.options(case))
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("kind", ["torch", "native"])
def test_resident_equals_host(strain, kind):
    """``resident.gpa_device`` on torch tensors and on ``DeviceArray``s, a stack and a single frame, against the host form."""
    from mtflearn_amd import _device, resident
    case = sc.stack_case()
    if kind == "torch":
        import torch
        to_device = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    else:
        to_device = up
    got = resident.gpa_device(to_device(case["frame"]), case["g"], return_phase=True, **sc.options(case))
    for a, b in zip(got, stack_host()):
        np.testing.assert_array_equal(_device.to_host(a), b)
    single = sc.by_name("32x40-int16")
    frame = to_device(single["frame"])
    got = resident.gpa_device(frame, single["g"], **sc.options(single))
    want = strain.gpa(single["frame"], single["g"], **sc.options(single))
    assert got.phase is None and want.phase is None
    for a, b in zip(got[:6], want[:6]):
        np.testing.assert_array_equal(_device.to_host(a), b)


def test_pick_g_on_a_known_lattice(strain):
    """Gaussian atoms on an 8 x 16 lattice, periodic in the 96 x 128 frame: every Bragg spot sits on a bin, and under the periodic
    Hann window it spreads over its 3 x 3 bins symmetrically (1-D: -1/4, 1/2, -1/4 of the line), so the power centroid is the bin
    itself in exact arithmetic.  The spectrum is within ``1e-12 M`` of exact (the project's FFT bound, ``M`` its largest
    magnitude, the DC line); a power ``P = |F|^2`` of the box is then off by at most ``2 A 1e-12 M`` (``A`` the spot's magnitude),
    the box sum is at least ``A^2``, and the six bins at offset +-1 of an axis move the centroid by at most ``6 x 2e-12 M / A``
    bins, ``/ n`` in cycles per pixel.  ``M / A`` is taken from NumPy's spectrum of the same frame."""
    frame = sc.atoms_frame()
    h, w = frame.shape
    got = strain.pick_g(frame)
    F = np.abs(np.fft.fft2(frame * so.window_of(h, w, "hann")))
    for k in range(2):
        ky, kx = int(round(sc.PICK_G[k][0] * h)), int(round(sc.PICK_G[k][1] * w))
        bound = 6 * 2 * BOUND * F.max() / F[ky, kx] / min(h, w)
        d = np.abs(got[k] - sc.PICK_G[k]).max()
        print(f"pick_g spot {k}: {got[k]} against {sc.PICK_G[k]}: {d:.2e} (bound {bound:.2e})")
        assert d <= bound


def test_rendered_honeycomb(strain):
    """A 256 x 256 ``HoneyCombLattice(l=12)`` frame with ``g`` from ``pick_g``: a real lattice image (atoms, harmonics, a third
    spot family the masks must keep out), against the oracle only."""
    from mtflearn_amd.datasets import HoneyCombLattice
    frame = HoneyCombLattice(size=256, l=12, seed=3).to_image()
    assert frame.shape == (256, 256)
    g = strain.pick_g(frame)
    print(f"honeycomb: pick_g {g.tolist()}")
    reference = (96, 160, 96, 160)
    got = strain.gpa(frame, g, reference=reference, window="hann", return_phase=True)
    want = so.gpa(frame, g, reference=reference, window="hann")
    floor = so.stencil_floor(want["amplitude"])
    print(f"honeycomb: {(floor < sc.AMP_FLOOR).mean():.4f} of the pixels below the floor")
    check_frame("honeycomb-256", got, want, g, reference)
