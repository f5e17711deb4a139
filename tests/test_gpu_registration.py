"""GPU tests of mtflearn_amd.registration and its resident twins (csrc/zk_register.hip) over the case table of
tests/registration_cases.py, against the NumPy statement tests/registration_oracle.py (licensed by
tests/test_registration_cpu.py):

* ``shift`` equal to the oracle's exactly: both are nodes of one grid, ``y0 + (j - off) / upsample`` in float64, and the CPU tests
  hold every case's top-two margin at 1e-9 or more, far above the kernels' error;
* ``peak``, the correlation plane and the upsampled plane within 1e-12 of the plane's largest magnitude, the project's bound for
  its FFT-based kernels;
* everything said to be bit for bit is compared with ``assert_array_equal``.

Every case prints its measured distance before it asserts (``pytest -s``; profiles/registration.txt records them).
"""
import numpy as np
import pytest

import registration_cases as rc
import registration_oracle as ro

pytestmark = pytest.mark.gpu

BOUND = 1e-12


@pytest.fixture(scope="module")
def reg():
    from mtflearn_amd import registration
    return registration


def up(array):
    from mtflearn_amd import _native
    return _native.DeviceArray.from_numpy(np.ascontiguousarray(array), 0)


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c["name"])
def test_estimate_shifts(reg, case):
    got = reg.estimate_shifts(case["stack"], **rc.options(case))
    shift, peak = ro.estimate_shifts(case["stack"], **rc.options(case))
    scale = np.abs(peak).max()
    print(f"{case['name']}: shifts unequal {np.count_nonzero(got.shift != shift)}, peak {np.abs(got.peak - peak).max() / scale:.2e} of max")
    if case["tie"] is not None:
        np.testing.assert_array_equal(got.shift, np.tile(case["tie"], (len(case["stack"]), 1)))
    np.testing.assert_array_equal(got.shift, shift)
    assert np.abs(got.peak - peak).max() <= BOUND * scale


@pytest.mark.parametrize("name", rc.PLANE_CASES)
def test_planes(reg, name):
    """The correlation plane and the upsampled plane themselves, through the debug outputs of ``zk_register_shifts``."""
    case = rc.by_name(name)
    stack, ref, options = reg._checked_host(case["stack"], *(case[k] for k in ("reference", "upsample", "max_shift", "normalization", "window")))
    _, corr, upsampled = reg._estimate_host(stack, ref, options, planes=True)
    for b in range(len(stack)):
        _, _, c, C = ro.planes(case["stack"][b], case["stack"][case["reference"]], case["upsample"])
        dc, dC = np.abs(corr[b] - c).max() / np.abs(c).max(), np.abs(upsampled[b] - C).max() / np.abs(C).max()
        print(f"{name} frame {b}: correlation plane {dc:.2e}, upsampled plane {dC:.2e} of the plane's maximum")
        assert dc <= BOUND and dC <= BOUND


def test_honeycomb(reg):
    stack, answer, max_shift = rc.honeycomb()
    for ms in (None, max_shift):
        got = reg.estimate_shifts(stack, upsample=10, max_shift=ms)
        shift, peak = ro.estimate_shifts(stack, upsample=10, max_shift=ms)
        print(f"honeycomb max_shift={ms}: device {got.shift[1]}, oracle {shift[1]}, true {answer}")
        np.testing.assert_array_equal(got.shift, shift)
        assert np.abs(got.peak - peak).max() <= BOUND * np.abs(peak).max()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=lambda d: np.dtype(d).name)
def test_shift_stack_is_scan_noise_with_constant_rows(reg, dtype):
    from mtflearn_amd import resident
    stack = rc.by_name("32x48-u100-a")["stack"].astype(dtype)
    shifts = np.array([[0.0, 0.0], [1.37, -2.61], [-40.5, 0.25]])
    b, h, w = stack.shape
    dx, dy = np.repeat(-shifts[:, 1:2], h, axis=1), np.repeat(-shifts[:, 0:1], w, axis=1)
    for order, mode in ((3, "grid-wrap"), (1, "reflect"), (0, "constant")):
        want = resident.scan_noise_device(up(stack), up(dx), up(dy), order=order, mode=mode).numpy()
        np.testing.assert_array_equal(reg.shift_stack(stack, shifts, order=order, mode=mode), want)
        np.testing.assert_array_equal(resident.shift_stack_device(up(stack), up(shifts), order=order, mode=mode).numpy(), want)
        assert want.dtype == dtype
    whole = reg.shift_stack(stack, [[0, 0], [2, -3], [-1, 5]], order=0, mode="grid-wrap")
    np.testing.assert_array_equal(whole[1], np.roll(stack[1], (2, -3), axis=(0, 1)))      # the sign: +dy moves the frame down


def test_register_stack_forms_agree(reg):
    import torch
    from mtflearn_amd import resident
    stack, _, _ = rc.end_to_end()
    stack = stack[:5, :33, :47].copy()                                                    # odd extents, more than one block
    host = reg.register_stack(stack, upsample=10, return_aligned=True)
    shifts = reg.estimate_shifts(stack, upsample=10)
    aligned = reg.shift_stack(stack, shifts.shift)
    np.testing.assert_array_equal(host.shifts, shifts.shift)
    np.testing.assert_array_equal(host.peak, shifts.peak)
    np.testing.assert_array_equal(host.aligned, aligned)
    np.testing.assert_array_equal(host.mean, np.add.reduce(aligned, axis=0) / len(stack))
    assert host.mean.dtype == np.float64 and reg.register_stack(stack, upsample=10).aligned is None
    again = reg.register_stack(stack, upsample=10, return_aligned=True)
    native = resident.register_stack_device(up(stack), upsample=10, return_aligned=True)
    tensor = resident.register_stack_device(torch.from_numpy(stack).cuda(), upsample=10, return_aligned=True)
    for other in (again, type(host)(*(a.numpy() for a in native)), type(host)(*(a.cpu().numpy() for a in tensor))):
        for a, b in zip(host, other):
            np.testing.assert_array_equal(a, b)
    est = resident.estimate_shifts_device(up(stack), reference="previous", upsample=10)
    want = reg.estimate_shifts(stack, reference="previous", upsample=10)
    np.testing.assert_array_equal(est.shift.numpy(), want.shift)
    np.testing.assert_array_equal(est.peak.numpy(), want.peak)
    by_array = resident.estimate_shifts_device(up(stack), reference=up(stack[2]), upsample=10)
    np.testing.assert_array_equal(by_array.shift.numpy(), reg.estimate_shifts(stack, reference=2, upsample=10).shift)
    f32 = stack.astype(np.float32)                                                        # a float32 stack is summed in float64
    np.testing.assert_array_equal(reg.register_stack(f32, upsample=10).mean,
                                  np.add.reduce(reg.shift_stack(f32, reg.estimate_shifts(f32, upsample=10).shift).astype(np.float64), axis=0) / len(f32))


def test_end_to_end(reg):
    """N drifted frames in, one clean frame out: a 64 x 64 truth stack of 8 frames, ``order=3``, ``mode='grid-wrap'``."""
    stack, base, answers = rc.end_to_end()
    out = reg.register_stack(stack, upsample=100, order=3, mode="grid-wrap")
    err = rc.wrapped_error(out.shifts, answers, (64, 64)).max()
    registered, plain = np.abs(out.mean - base).max(), np.abs(stack.mean(axis=0) - base).max()
    print(f"end to end: worst shift error {err:.4f} px (bound 0.01); max |mean - frame| registered {registered:.3e}, unregistered {plain:.3e}")
    assert err <= 1.0 / 100 * (1 + 1e-9)
    assert registered < plain
