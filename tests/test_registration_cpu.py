"""CPU tests of mtflearn_amd.registration: what licenses the oracle and the case table of the GPU tests, and everything the
package decides before its first device call.

* truth: on the truth frames the oracle recovers ``-s`` within ``1 / upsample`` per axis (0.5 px at ``upsample = 1``).  The
  grid spacing is ``1 / upsample``; on 7 x 5 white noise the nearest-node error was seen to exceed half a spacing slightly
  (0.0059 at ``upsample = 100``), so a full spacing is the bound.
* margin: every case's top-two margin in its deciding plane, ``(max - second) / |max|``, is at least 1e-9 -- a condition on the
  inputs, so that the device's discrete answer can be required to equal the oracle's.  The tie cases are exempt and are
  checked by index.
"""
import os
import re

import numpy as np
import pytest

import registration_cases as rc
import registration_oracle as ro
from conftest import ROOT


def _frames(case):
    """``(frame, reference frame)`` pairs of a case, as the oracle pairs them."""
    stack, reference = np.asarray(case["stack"], np.float64), case["reference"]
    for b in range(len(stack)):
        if isinstance(reference, str):
            yield stack[b], stack[max(b - 1, 0)]
        elif np.ndim(reference) == 0:
            yield stack[b], stack[reference]
        else:
            yield stack[b], reference


@pytest.mark.parametrize("case", [c for c in rc.CASES if c["truth"] is not None], ids=lambda c: c["name"])
def test_oracle_recovers_truth(case):
    shift, _ = ro.estimate_shifts(case["stack"], **rc.options(case))
    err = rc.wrapped_error(shift, case["truth"], case["stack"].shape[1:])
    bound = 0.5 if case["upsample"] == 1 else 1.0 / case["upsample"]
    print(f"{case['name']}: worst per-axis error {err.max():.4f} px (bound {bound:g})")
    assert err.max() <= bound * (1 + 1e-9)


def _smallest_margin(case):
    """The smallest top-two margin of a case's deciding planes: the coarse plane under its mask, and the upsampled plane.  A
    masked coarse plane of a single sample (``max_shift = 0``) has no second candidate: its margin is ``inf``."""
    opts = rc.options(case)
    opts.pop("reference")
    worst = np.inf
    for b, (frame, ref) in enumerate(_frames(case)):
        if isinstance(case["reference"], str) and b == 0:
            continue                                        # frame 0 of "previous" is pinned to (0, 0), not read from a plane
        _, _, c, C = ro.planes(frame, ref, **opts)
        if opts["max_shift"] is not None:
            ly, lx = np.fft.fftfreq(c.shape[0], 1 / c.shape[0]), np.fft.fftfreq(c.shape[1], 1 / c.shape[1])
            c = c[np.abs(ly) <= opts["max_shift"]][:, np.abs(lx) <= opts["max_shift"]]
        worst = min(worst, np.inf if c.size == 1 else ro.top_two_margin(c), np.inf if C is None else ro.top_two_margin(C))
    return worst


@pytest.mark.parametrize("case", [c for c in rc.CASES if c["tie"] is None], ids=lambda c: c["name"])
def test_margin(case):
    worst = _smallest_margin(case)
    print(f"{case['name']}: smallest top-two margin {worst:.2e}")
    assert worst >= 1e-9


def test_margin_of_a_single_permitted_lag_is_infinite():
    case = rc.edge("72x136-u10-ms0")
    coarse_only = dict(case, upsample=1)
    assert _smallest_margin(coarse_only) == np.inf and np.isfinite(_smallest_margin(case))


@pytest.mark.parametrize("case", [c for c in rc.CASES if c["tie"] is not None], ids=lambda c: c["name"])
def test_ties_take_the_first_index(case):
    shift, _ = ro.estimate_shifts(case["stack"], **rc.options(case))
    np.testing.assert_array_equal(shift, np.tile(case["tie"], (len(case["stack"]), 1)))


# ------------------------------------------------------------------------------------------------ the edge cases
EDGE_IDS = [name for name, _ in rc.EDGE_CASES]
EDGE_TIES = [name for name in EDGE_IDS if name.endswith("-tie")]


def test_edge_cases_are_lazy_and_named_once():
    assert len(set(EDGE_IDS)) == len(EDGE_IDS) and not set(EDGE_IDS) & {c["name"] for c in rc.CASES}
    assert all(callable(make) for _, make in rc.EDGE_CASES)
    assert sorted(EDGE_TIES) == sorted(name for name, make in rc.EDGE_CASES if name.startswith("128x64"))
    for name in EDGE_TIES:
        assert rc.edge(name)["tie"] is not None


@pytest.mark.parametrize("name", [n for n in EDGE_IDS if n not in EDGE_TIES])
def test_edge_margin(name):
    """The margin condition of ``test_margin`` on every edge case that is not a tie, the mask applied to the coarse plane."""
    case = rc.edge(name)
    assert case["tie"] is None
    worst = _smallest_margin(case)
    print(f"{name}: smallest top-two margin {worst:.2e}")
    assert worst >= 1e-9


@pytest.mark.parametrize("name", EDGE_TIES)
def test_edge_ties_take_the_first_index(name):
    case = rc.edge(name)
    shift, _ = ro.estimate_shifts(case["stack"], **rc.options(case))
    np.testing.assert_array_equal(shift, np.tile(case["tie"], (len(case["stack"]), 1)))


@pytest.mark.parametrize("name", ["72x136-u100", "1040x1032-u10", "16x16-u1000-B120-first"])
def test_edge_oracle_recovers_truth(name):
    case = rc.edge(name)
    shift, _ = ro.estimate_shifts(case["stack"], **rc.options(case))
    err = rc.wrapped_error(shift, case["truth"], case["stack"].shape[1:])
    print(f"{name}: worst per-axis error {err.max():.4f} px (bound {1.0 / case['upsample']:g})")
    assert err.max() <= 1.0 / case["upsample"] * (1 + 1e-9)


def _flat_lags(case):
    """The flat index of every frame's coarse peak, without a mask."""
    h, w = case["stack"].shape[1:]
    shift, _ = ro.estimate_shifts(case["stack"], reference=case["reference"], upsample=1)
    return [int(s[0] % h) * w + int(s[1] % w) for s in shift]


def test_the_mask_matters_between_neighbouring_thresholds():
    """The oracle's answers of the mask cases: what is said to differ differs, what is said to be equal is equal."""
    def answer(prefix, ms):
        case = rc.edge(f"{prefix}-ms{ms}")
        return ro.estimate_shifts(case["stack"], **rc.options(case))[0]

    free = ro.estimate_shifts(rc.edge("13x17-u10-ms2")["stack"], upsample=10)[0]
    by = {ms: answer("13x17-u10", ms) for ms in rc.MASKS_13}
    coarse = ro.estimate_shifts(rc.edge("13x17-u10-ms2")["stack"], upsample=1)[0]
    np.testing.assert_array_equal(coarse[1:3], [[3, -1], [1, -3]])      # frame 1 is beyond 2 in y only, frame 2 in x only
    assert (by[2][1] != free[1]).any() and (by[2][2] != free[2]).any()
    np.testing.assert_array_equal(by[2][3:], free[3:])
    np.testing.assert_array_equal(by[2.999], by[2])
    np.testing.assert_array_equal(by[8], free)
    np.testing.assert_array_equal(by[100], free)
    for low, high in ((0, 1), (1, 2), (2, 6)):
        assert (by[low] != by[high]).any(), (low, high)
    free = ro.estimate_shifts(rc.edge("16x12-u10-ms8")["stack"], upsample=10)[0]
    by = {ms: answer("16x12-u10", ms) for ms in rc.MASKS_16x12}
    coarse = ro.estimate_shifts(rc.edge("16x12-u10-ms8")["stack"], upsample=1)[0]
    np.testing.assert_array_equal(coarse[1:], [[-8, -6], [-8, -6]])     # row 8 and column 6: the lags -n / 2 of 16 and 12
    np.testing.assert_array_equal(by[8], free)
    for low, high in ((5, 6), (7, 8)):                                  # 6 admits column 6 and 8 admits row 8; 5 and 7 do not
        assert (by[low] != by[high]).any(), (low, high)


def _constant(name):
    text = open(os.path.join(ROOT, "motif-learn_amd", "csrc", "zk_register.hip")).read()
    m = re.search(rf"constexpr \w+ {name} = (?:\(size_t\))?(\d+)(?: << (\d+))?;", text)
    return int(m.group(1)) << int(m.group(2) or 0)


def test_edge_sizes_reach_what_they_are_for():
    """The sizes of the edge cases against the constants of csrc/zk_register.hip: were a constant to change, the cases would
    quietly stop reaching the branches they were chosen for."""
    red, gt, gk = _constant("RED_PER_BLOCK"), _constant("GT"), _constant("GK")
    field, table, mean = _constant("FIELD_BYTES"), _constant("TABLE_BYTES"), _constant("MEAN_BUDGET")
    parts = lambda h, w: -(-h * w // red)
    assert (red, gt, gk) == (4096, 64, 16)
    assert parts(72, 136) == 3 and 72 * 136 - 2 * red == 1600 and (136 // gt, 136 % gt) == (2, 8) and (72 // gk, 72 % gk) == (4, 8)
    assert [k // red for k in _flat_lags(rc.edge("72x136-u1"))] == [0, 0, 1, 2, 1]
    rows = np.arange(72)
    shut = rows[np.abs(np.fft.fftfreq(72, 1 / 72)) > 10]
    assert shut.min() * 136 <= red and shut.max() * 136 + 135 >= 2 * red - 1          # max_shift = 10 shuts all of partial 1
    assert parts(128, 64) == 2
    assert parts(1040, 1032) == 263 and [k // red for k in _flat_lags(rc.edge("1040x1032-u10"))] == [0, 0, 262]
    assert field // (512 * 512 * 32) == 128                                          # runs of 128 + 2, and of 128 + 1
    s = 1500
    assert table // ((s * (16 + 2 * 16) * 2 + s * s) * 8) == 56                      # runs of 56 + 56 + 8
    chunk = mean // (2100 + 8) & ~255
    assert (chunk, 257 * 511 - chunk) == (127232, 4095)                              # the two pixel chunks of the chunked mean


def test_previous_is_the_running_sum_of_pairwise_answers():
    case = rc.by_name("16x16-u10-previous")
    stack = case["stack"]
    shift, _ = ro.estimate_shifts(stack, **rc.options(case))
    pair = [np.zeros(2)] + [ro.planes(stack[b], stack[b - 1], upsample=case["upsample"])[0] for b in range(1, len(stack))]
    np.testing.assert_array_equal(shift, np.cumsum(pair, axis=0))


def test_honeycomb_needs_max_shift():
    stack, answer, max_shift = rc.honeycomb()
    free, _ = ro.estimate_shifts(stack, upsample=10)
    bound, _ = ro.estimate_shifts(stack, upsample=10, max_shift=max_shift)
    lattice_vector = np.array([-np.sqrt(3.0) * rc.HONEY_L / 2, 1.5 * rc.HONEY_L])        # (dy, dx) of a1's mirror image
    print(f"honeycomb: max_shift=None {free[1]}, max_shift={max_shift} {bound[1]}, true {answer}")
    assert np.abs(bound[1] - answer).max() <= 0.1
    assert np.abs(free[1] - answer).max() > 1.0                      # another lag ...
    assert np.abs(free[1] - (answer - lattice_vector)).max() <= 0.25  # ... the lattice-equivalent one
    for ms in (None, max_shift):
        c = ro.planes(stack[1], stack[0], upsample=10, max_shift=ms)
        assert ro.top_two_margin(c[3]) >= 1e-9


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture()
def no_device(monkeypatch):
    """Any device call of the three functions would come through ``_native.load``: it must not be reached."""
    from mtflearn_amd import _native

    def refuse():
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(_native, "load", refuse)


STACK = np.zeros((3, 8, 8))


@pytest.mark.parametrize("kwargs, error", [
    (dict(stack=np.zeros((8, 8))), ValueError), (dict(stack=np.zeros((2, 3, 8, 8))), ValueError),
    (dict(stack=np.zeros((0, 8, 8))), ValueError), (dict(stack=np.zeros((3, 1, 8))), ValueError),
    (dict(stack=np.zeros((3, 8, 1))), ValueError), (dict(stack=np.zeros((3, 8, 8), np.complex128)), TypeError),
    (dict(reference=3), IndexError), (dict(reference=-4), IndexError), (dict(reference="next"), ValueError),
    (dict(reference=np.zeros((8, 9))), ValueError), (dict(reference=np.zeros((8, 8), np.complex64)), TypeError),
    (dict(upsample=0), ValueError), (dict(upsample=1001), ValueError), (dict(upsample=2.5), ValueError), (dict(upsample=True), ValueError),
    (dict(max_shift=-1), ValueError), (dict(max_shift=np.inf), ValueError), (dict(max_shift=np.nan), ValueError),
    (dict(max_shift="3"), ValueError), (dict(normalization="magnitude"), ValueError), (dict(window="hamming"), ValueError),
])
@pytest.mark.parametrize("function", ["estimate_shifts", "register_stack"])
def test_estimate_argument_errors(no_device, function, kwargs, error):
    from mtflearn_amd import registration
    kwargs = dict(kwargs)
    stack = kwargs.pop("stack", STACK)
    with pytest.raises(error):
        getattr(registration, function)(stack, **kwargs)


@pytest.mark.parametrize("kwargs, error", [
    (dict(order=2), NotImplementedError), (dict(order=6), RuntimeError), (dict(order=1.0), TypeError), (dict(mode="wrap"), NotImplementedError),
    (dict(mode="periodic"), ValueError), (dict(order=3, mode="nearest"), NotImplementedError), (dict(stack=np.zeros((8, 8))), ValueError),
    (dict(stack=np.zeros((0, 8, 8))), ValueError), (dict(stack=np.zeros((3, 8, 8), np.int64)), TypeError),
])
def test_shift_argument_errors(no_device, kwargs, error):
    from mtflearn_amd import registration
    kwargs = dict(kwargs)
    stack = kwargs.pop("stack", STACK)
    with pytest.raises(error):
        registration.shift_stack(stack, np.zeros((len(stack), 2)), **kwargs)
    with pytest.raises(error):
        registration.register_stack(stack, **kwargs)


@pytest.mark.parametrize("shifts", [np.zeros((2, 2)), np.zeros((3, 3)), np.zeros(3), np.full((3, 2), np.nan)])
def test_shift_stack_refuses_bad_shifts(no_device, shifts):
    from mtflearn_amd import registration
    with pytest.raises(ValueError):
        registration.shift_stack(STACK, shifts)


def test_header_and_native_table_agree_on_the_new_names():
    from mtflearn_amd import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zk_[a-z_0-9]+)\s*\(", text))
    for name in ("zk_register_shifts", "zk_register_shifts_dev", "zk_stack_mean", "zk_stack_mean_dev"):
        assert name in declared and name in _native.SYMBOLS
    from mtflearn_amd import registration
    for name, value in (("ZK_REGISTER_REF_INDEX", registration.REF_INDEX), ("ZK_REGISTER_REF_FRAME", registration.REF_FRAME),
                        ("ZK_REGISTER_REF_PREVIOUS", registration.REF_PREVIOUS), ("ZK_REGISTER_NORM_PHASE", registration._NORMALIZATIONS["phase"]),
                        ("ZK_REGISTER_WINDOW_HANN", registration._WINDOWS["hann"])):
        assert re.search(rf"#define\s+{name}\s+{value}\b", text), name


def test_resident_twins_exist():
    from mtflearn_amd import distributed, resident
    for name in ("estimate_shifts_device", "shift_stack_device", "register_stack_device"):
        assert getattr(distributed, name) is getattr(resident, name)
