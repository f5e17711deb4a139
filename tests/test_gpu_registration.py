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
import functools

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


# ---------------------------------------------------------------------------------------------------------------------
# Past one reduction block, one tile and one run (rc.EDGE_CASES; the sizes are held against the constants of
# csrc/zk_register.hip by test_registration_cpu.py::test_edge_sizes_reach_what_they_are_for)
# ---------------------------------------------------------------------------------------------------------------------
EDGE_IDS = [name for name, _ in rc.EDGE_CASES]
RUN_IDS = [name for name in EDGE_IDS if "-B1" in name]
FORMS = {"first": 0, "previous": "previous", "last": -1}


@functools.lru_cache(maxsize=None)
def edge_oracle(name):
    """The oracle's ``(shift, peak)`` of an edge case: computed once, shared by every test that needs it, read-only."""
    case = rc.edge(name)
    shift, peak = ro.estimate_shifts(case["stack"], **rc.options(case))
    shift.setflags(write=False)
    peak.setflags(write=False)
    return shift, peak


@functools.lru_cache(maxsize=None)
def edge_host(name):
    """``estimate_shifts`` of an edge case through the host entry, once."""
    from mtflearn_amd import registration
    case = rc.edge(name)
    got = registration.estimate_shifts(case["stack"], **rc.options(case))
    got.shift.setflags(write=False)
    got.peak.setflags(write=False)
    return got


def peak_distance(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


@pytest.mark.parametrize("name", EDGE_IDS)
def test_edge_estimate_shifts(reg, name):
    """``estimate_shifts`` against the oracle where the code takes the branches that frames of at most 64 x 64 never reach.

    * ``72x136-*``: 9792 samples are 3 partials (4096, 4096, 1600) per frame, the coarse peaks of the five frames in partials 0,
      0, 1, 2, 1: ``argmax_parts_kernel`` with ``stride = 2`` and ``fold_parts`` / ``coarse_kernel`` combine several partials of
      a correlation plane; with ``"phase"`` the multi-block ``part_max`` / ``frame_max_kernel`` path.  ``product_kernel<false>``
      (``T = Ey P``) runs past one column tile, ``blockIdx.x`` 0 .. 2 for ``N = W = 136`` (64 + 64 + 8), with ``K = H = 72``,
      four depth slices and 8.  ``ms10``: rows 11 .. 61 are shut, so all of partial 1 is outside the mask and comes back with
      ``idx = -1`` between two live partials; ``ms3`` at ``upsample = 1`` (the ``last`` branch of ``coarse_kernel`` under a
      mask); ``ms0``: one permitted sample, ``idx = -1`` in partials 1 and 2.
    * ``128x64-*-tie``: every sample of the plane is one float64, the partials of blocks 0 and 1 tie and the smaller flat index
      wins; under ``max_shift = 2`` too.
    * ``1040x1032-*``: 263 partials, so the ``k += 256`` loop of ``fold_parts`` runs twice for lanes 0 .. 6 and the peak of the
      last frame (row 1039, partial 262) is met there; with ``"phase"`` the ``k += 256`` loop of ``frame_max_kernel``.
    * ``13x17-*-ms*``, ``16x12-*-ms*``: ``max_shift`` on frames that are not square: at 2 frame 1 is shut out by the y test alone
      and frame 2 by the x test alone; ``max_shift = 0``; masks wider than the frame (8, 100); 2.999, which is 2; the lag
      ``-n / 2`` of both even extents of 16 x 12, which 8 admits as row 8 and 7 does not, 6 as column 6 and 5 not.
    * ``32x48-u10-int16``: ``ZK_I16``, the ``default:`` branch of the dtype switch of ``launch_widen``, about half the samples
      negative.  ``*-ref-float64``, ``*-ref-int16``: a reference array with ``ref_dtype != dtype``, both ways.
    * ``512x512-u10-B130-*``: ``run_length`` returns 128 (``FIELD_BYTES`` / (32 x 262144)): the loop over runs, 128 + 2 frames,
      ``plan_tail``, the per-run offsets of ``shifts`` and ``peak``; ``previous``: slot 0 is handed from frame 127 to the second
      run; ``last``: the reference is a frame of the second run.
    * ``16x16-u1000-B120-*``: ``run_length`` returns 56 (``TABLE_BYTES`` / 19,152,000): runs of 56 + 56 + 8, the same three forms.
    """
    case = rc.edge(name)
    got = edge_host(name)
    shift, peak = edge_oracle(name)
    print(f"{name}: shifts unequal {np.count_nonzero(got.shift != shift)}, peak {peak_distance(got.peak, peak):.2e} of max")
    if case["tie"] is not None:
        np.testing.assert_array_equal(got.shift, np.tile(case["tie"], (len(case["stack"]), 1)))
    np.testing.assert_array_equal(got.shift, shift)
    assert peak_distance(got.peak, peak) <= BOUND


@pytest.mark.parametrize("name", rc.EDGE_PLANE_CASES)
def test_edge_planes(reg, name):
    """Both planes of every frame of 72 x 136 at ``upsample = 100``: the three partials of ``argmax_parts_kernel``'s
    ``plane_out``, and the (150, 150) plane behind ``product_kernel<false>`` past one column tile (``T`` is 150 x 136: 3 x 3
    tiles, both edges with a remainder)."""
    case = rc.edge(name)
    stack, ref, options = reg._checked_host(case["stack"], *(case[k] for k in ("reference", "upsample", "max_shift", "normalization", "window")))
    _, corr, upsampled = reg._estimate_host(stack, ref, options, planes=True)
    for b in range(len(stack)):
        _, _, c, C = ro.planes(case["stack"][b], case["stack"][case["reference"]], case["upsample"])
        dc, dC = np.abs(corr[b] - c).max() / np.abs(c).max(), np.abs(upsampled[b] - C).max() / np.abs(C).max()
        print(f"{name} frame {b}: correlation plane {dc:.2e}, upsampled plane {dC:.2e} of the plane's maximum")
        assert dc <= BOUND and dC <= BOUND


@pytest.mark.parametrize("name", RUN_IDS)
def test_runs_resident_is_host(reg, name):
    """``resident.estimate_shifts_device`` on the stacks that go in several runs, bit for bit the host call (which
    ``test_edge_estimate_shifts`` holds against the oracle), for the three reference forms: the loop over runs of the ``_dev``
    entry, its per-run offsets of ``shifts`` and ``peak``, the hand-over of slot 0 and the reference in a later run there."""
    from mtflearn_amd import resident
    case = rc.edge(name)
    got = resident.estimate_shifts_device(up(case["stack"]), **rc.options(case))
    host = edge_host(name)
    np.testing.assert_array_equal(got.shift.numpy(), host.shift)
    np.testing.assert_array_equal(got.peak.numpy(), host.peak)


@pytest.fixture(scope="module")
def field_runs():
    """The 130 x 512 x 512 uint8 stack and, per reference form, the oracle's answer and the host call's: each made once."""
    stack, _ = rc.field_runs_stack()
    name = "512x512-u10-B130-{}".format
    return dict(stack=stack, oracle=lambda form: edge_oracle(name(form)), host=lambda form: edge_host(name(form)))


def test_field_runs_tail_of_one_frame(reg, field_runs):
    """129 frames are runs of 128 + 1: the tail takes ``plan_one``, which ``prepare`` made for the reference.  The oracle's
    frames do not depend on one another, so its rows 0 .. 128 of the 130-frame call are the reference; and the device's rows are
    bit for bit those of its 130-frame call, whose tail went through ``plan_tail``."""
    stack = field_runs["stack"][:129]
    got = reg.estimate_shifts(stack, upsample=10)
    shift, peak = field_runs["oracle"]("first")
    print(f"512x512-u10-B129: shifts unequal {np.count_nonzero(got.shift != shift[:129])}, peak {peak_distance(got.peak, peak[:129]):.2e} of max")
    np.testing.assert_array_equal(got.shift, shift[:129])
    assert peak_distance(got.peak, peak[:129]) <= BOUND
    whole = field_runs["host"]("first")
    np.testing.assert_array_equal(got.shift, whole.shift[:129])
    np.testing.assert_array_equal(got.peak, whole.peak[:129])


def test_field_runs_do_not_depend_on_the_run_length(reg, field_runs):
    """"A frame's numbers do not depend on the run length": frames 126 .. 129 as a stack of their own (one run of 4) against
    frame 0 as an array are bit for bit rows 126 .. 129 of the whole call, where they end one run of 128 and fill one of 2."""
    stack = field_runs["stack"]
    got = reg.estimate_shifts(stack[126:], reference=stack[0], upsample=10)
    whole = field_runs["host"]("first")
    np.testing.assert_array_equal(got.shift, whole.shift[126:])
    np.testing.assert_array_equal(got.peak, whole.peak[126:])


def test_field_runs_planes(reg, field_runs):
    """The planes across runs, at ``upsample = 2``: ``corr`` and the upsampled plane of frames 0, 127, 128 and 129 -- the first
    and last frame of the first run and both frames of the second -- against the oracle's.  The host entry: the per-run offsets
    of ``corr`` and ``up`` in the ring's slot and of their copies to the host; the ``_dev`` entry: its per-run offsets
    ``corr_dev + first per`` and ``up_dev + first up_per``."""
    from mtflearn_amd import resident
    stack = field_runs["stack"]
    host_stack, ref, options = reg._checked_host(stack, 0, 2, None, None, None)
    _, corr, upsampled = reg._estimate_host(host_stack, ref, options, planes=True)
    _, corr_dev, up_dev = resident._estimate_shifts_resident(up(stack), _native_code(stack), stack.shape, 0, options, planes=True)
    corr_dev, up_dev = corr_dev.numpy(), up_dev.numpy()
    for b in (0, 127, 128, 129):
        _, _, c, C = ro.planes(stack[b], stack[0], 2)
        for entry, (pc, pC) in (("host", (corr, upsampled)), ("resident", (corr_dev, up_dev))):
            dc, dC = np.abs(pc[b] - c).max() / np.abs(c).max(), np.abs(pC[b] - C).max() / np.abs(C).max()
            print(f"512x512-u2-B130 {entry} frame {b}: correlation plane {dc:.2e}, upsampled plane {dC:.2e} of the plane's maximum")
            assert dc <= BOUND and dC <= BOUND


def _native_code(array):
    from mtflearn_amd import _native
    return _native.dtype_code(array.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# zk_stack_mean on its own
# ---------------------------------------------------------------------------------------------------------------------
MEAN_SHAPES = ((1, 1, 257), (3, 5, 51), (70, 17, 15))       # B = 1; 257 and 255 pixels, no multiples of 256; two blocks and one
MEAN_DTYPES = (np.float32, np.float64, np.uint8, np.uint16, np.int16)


def mean_input(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(shape).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)      # int16: negatives included


@pytest.mark.parametrize("dtype", MEAN_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stack_mean(reg, shape, dtype):
    """``zk_stack_mean`` and ``zk_stack_mean_dev`` called directly: every instantiation of ``mean_kernel`` (the integer ones,
    and ``ZK_I16`` as the ``default:`` branch of ``launch_mean``, were unreached), ``B = 1``, pixel counts that are no multiple
    of 256.  The sum over the frames in ascending order and one division are the same float64 operations in NumPy: equal."""
    from mtflearn_amd import resident
    stack = mean_input(shape, dtype, 300 + len(shape) + shape[0])
    want = np.add.reduce(stack.astype(np.float64), axis=0) / shape[0]
    if dtype is np.int16:
        assert (stack < 0).any()
    np.testing.assert_array_equal(reg._mean_host(stack), want)
    np.testing.assert_array_equal(resident.stack_mean_device(up(stack)).numpy(), want)


def test_stack_mean_in_pixel_chunks(reg):
    """The pixel chunking of the host entry.  A uint8 stack of 2100 frames takes 2100 + 8 = 2108 bytes per pixel, input and
    output; ``zk_chunk_plan(MEAN_BUDGET = 256 MiB, 2108, 256, 257 x 511 = 131327)`` gives floor(268435456 / 2108) = 127341
    rounded down to whole blocks, 127232 pixels, so two chunks of 127232 and 4095 pixels: ``zk_ring_up_2d`` with a device
    pitch (127232) other than the host's (131327), a short last chunk whose rows start mid-frame, the chunk offsets of
    ``out``.  Sums of 2100 bytes are integers below 2^53, exact in any order."""
    stack = np.random.default_rng(310).integers(0, 256, (2100, 257, 511), dtype=np.uint8)
    want = stack.sum(axis=0, dtype=np.float64) / 2100
    got = reg._mean_host(stack)
    print(f"stack mean in chunks: unequal pixels {np.count_nonzero(got != want)} of {want.size}")
    np.testing.assert_array_equal(got, want)


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
