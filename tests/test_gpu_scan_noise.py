"""GPU tests of mtflearn_amd.denoise.apply_scan_noise and resident.scan_noise_device (csrc/zk_resample.hip) over the case
table of tests/scan_noise_cases.py, whose docstring derives the shapes and the tolerances:

* order 0 equal; order 1 float64 within 1e-14 max|frame|; order 3 float64 within 1e-12 max|frame|; float32 output within one
  float32 ulp of the oracle's value, elementwise;
* everything said to be bit for bit is compared with ``assert_array_equal``.

The references are the reference's recorded outputs (tests/golden/scan_noise_golden.npz) and the SciPy statement
(tests/scan_noise_oracle.py), which tests/test_scan_noise_cpu.py licenses against them.  Every case prints its measured
distance before it asserts (``pytest -s`` shows them; profiles/scan_noise.txt records them).
"""
import os

import numpy as np
import pytest

import scan_noise_cases as sc
import scan_noise_oracle as so

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "scan_noise_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def denoise():
    from mtflearn_amd import denoise as module
    return module


def device_call(images, dx, dy, order, mode):
    """``resident.scan_noise_device`` on uploaded operands, result back on the host."""
    from mtflearn_amd import _native, resident
    up = lambda a: _native.DeviceArray.from_numpy(a, 0)
    return resident.scan_noise_device(up(images), up(dx), up(dy), order=order, mode=mode).numpy()


def check(label, got, ref, order, scale, worst):
    measured, bound, unit = sc.distance(got, ref, order, scale)
    worst[0] = max(worst[0], measured)
    assert measured <= bound, f"{label}: {measured:.3e} {unit} (bound {bound:g})"


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_golden_cases(denoise, golden, dtype):
    """The host function with the reference's arguments against the reference's recorded output."""
    worst = {0: [0.0], 1: [0.0], 3: [0.0]}
    for shape, dt, order, mode, k in sc.golden_cases():
        if dt != dtype:
            continue
        stack = golden[f"{sc.shape_id(shape)}/images"].astype(dtype)
        jx, jy = sc.GOLDEN_JITTERS[k]
        got = denoise.apply_scan_noise(stack, jx=jx, jy=jy, seed=sc.seed_of(shape, k), order=order, mode=mode)
        check(f"{shape} {sc.pair_id((order, mode))} j{k}", got, sc.golden_output(golden, shape, dtype, order, mode, k), order,
              np.abs(stack).max(), worst[order])
    print(f"golden {np.dtype(dtype).name}: worst order 0 {worst[0][0]:g} unequal, order 1 {worst[1][0]:.2e}, order 3 {worst[3][0]:.2e}"
          f" ({'float32 ulp' if dtype == np.float32 else 'of max|frame|'})")


@pytest.mark.parametrize("pair", sc.PAIRS, ids=sc.pair_id)
def test_oracle_cases(denoise, pair):
    """Every shape of the table, both float types: the small shapes with a sub-pixel / multi-pixel shift and with 60 on both axes
    (many folds of a line of 1 to 9 samples), (2, 64, 130) with jx and jy from {0, 0.3, 2.5} crossed and 60 on both."""
    order, mode = pair
    for shape in sc.ORACLE_SHAPES:
        images = sc.images(shape)
        scale = np.abs(images).max()
        worst = {np.float64: [0.0], np.float32: [0.0]}
        for k, (jx, jy) in enumerate(sc.BIG_JITTERS if shape == sc.BIG else sc.SMALL_JITTERS):
            dx, dy = so.jitter(sc.seed_of(shape, k), shape, jx, jy)
            for dtype in sc.DTYPES:
                stack = images.astype(dtype)
                got = denoise.apply_scan_noise(stack, jx=jx, jy=jy, seed=sc.seed_of(shape, k), order=order, mode=mode)
                check(f"{shape} {sc.pair_id(pair)} jx {jx} jy {jy} {np.dtype(dtype).name}", got, so.resample(stack, dx, dy, order, mode), order,
                      scale, worst[dtype])
        print(f"{sc.pair_id(pair)} {shape}: worst float64 {worst[np.float64][0]:.2e}, float32 {worst[np.float32][0]:.2e}"
              f" ({'unequal samples' if order == 0 else 'of max|frame| / float32 ulp'})")


@pytest.mark.parametrize("pair", sc.PAIRS, ids=sc.pair_id)
def test_zero_jitter_returns_the_input(denoise, pair):
    order, mode = pair
    for shape in sc.ORACLE_SHAPES:
        for dtype in sc.DTYPES:
            stack = sc.images(shape).astype(dtype)
            got = denoise.apply_scan_noise(stack, jx=0, jy=None, seed=3, order=order, mode=mode)
            if order < 3:
                np.testing.assert_array_equal(got, stack)
            else:
                measured, bound, unit = sc.distance(got, stack, 3, np.abs(stack).max())
                print(f"zero jitter {sc.pair_id(pair)} {shape} {np.dtype(dtype).name}: {measured:.2e} {unit}")
                assert measured <= bound


@pytest.mark.parametrize("pair", [(0, "nearest"), (1, "grid-constant"), (1, "constant"), (3, "reflect"), (3, "mirror"), (3, "grid-wrap")],
                         ids=sc.pair_id)
def test_frames_entry_points_and_run_lengths_agree_bit_for_bit(denoise, pair):
    """Frame k of a stack is the call on that frame alone with its own shifts; the host entry is the resident entry; a budget
    that forces one frame per run changes nothing."""
    from mtflearn_amd import _native
    order, mode = pair
    for shape in [(3, 5, 7), (3, 64, 130)]:
        for dtype in sc.DTYPES:
            stack = sc.images(shape).astype(dtype)
            seed = sc.seed_of(shape, 1)
            dx, dy = so.jitter(seed, shape, 2.5, 1.5)
            whole = denoise.apply_scan_noise(stack, jx=2.5, jy=1.5, seed=seed, order=order, mode=mode)
            resident = device_call(stack, dx, dy, order, mode)
            np.testing.assert_array_equal(resident, whole)
            for k in range(shape[0]):
                np.testing.assert_array_equal(device_call(stack[k:k + 1], dx[k:k + 1], dy[k:k + 1], order, mode)[0], whole[k])
            lib = _native.load()
            _native.check(lib.zk_scan_resample_set_chunk(0, 1), "zk_scan_resample_set_chunk")        # one byte: one frame per run
            try:
                forced_host = denoise.apply_scan_noise(stack, jx=2.5, jy=1.5, seed=seed, order=order, mode=mode)
                forced_resident = device_call(stack, dx, dy, order, mode)
            finally:
                _native.check(lib.zk_scan_resample_set_chunk(0, 0), "zk_scan_resample_set_chunk")
            np.testing.assert_array_equal(forced_host, whole)
            np.testing.assert_array_equal(forced_resident, whole)


def test_caller_scratch_of_one_frame_and_out_argument():
    """``zk_scan_resample_dev`` with the caller's scratch sized for one frame runs frame by frame and gives the same bits; ``out``
    is written in place."""
    from ctypes import c_void_p
    from mtflearn_amd import _native, resident
    shape = (3, 33, 65)
    stack = sc.images(shape)
    dx, dy = so.jitter(9, shape, 2.5, 1.5)
    up = lambda a: _native.DeviceArray.from_numpy(a, 0)
    d_stack, d_dx, d_dy = up(stack), up(dx), up(dy)
    out = _native.DeviceArray(shape, np.float64, 0)
    assert resident.scan_noise_device(d_stack, d_dx, d_dy, order=3, mode="mirror", out=out) is out
    want = out.numpy()
    scratch = _native.DeviceArray((2, 33, 65), np.float64, 0)
    again = _native.DeviceArray(shape, np.float64, 0)
    ptr = lambda a: c_void_p(a.data_ptr())
    _native.check(_native.load().zk_scan_resample_dev(0, ptr(d_stack), _native.ZK_F64, *shape, ptr(d_dx), ptr(d_dy), 3,
                                                      _native.RESAMPLE_MODES["mirror"], ptr(again), ptr(scratch), scratch.nbytes, None),
                  "zk_scan_resample_dev")
    np.testing.assert_array_equal(again.numpy(), want)


@pytest.mark.parametrize("pair", [(1, "reflect"), (3, "grid-wrap")], ids=sc.pair_id)
def test_integer_input_is_the_float64_result_of_its_cast(denoise, pair):
    order, mode = pair
    stack = sc.images((2, 33, 65))
    want = denoise.apply_scan_noise(stack, jx=2.5, jy=1.5, seed=4, order=order, mode=mode)
    for dtype in (np.uint16, np.int16):
        got = denoise.apply_scan_noise(stack.astype(dtype), jx=2.5, jy=1.5, seed=4, order=order, mode=mode)
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
    small = (stack // 16).astype(np.uint8)
    got = denoise.apply_scan_noise(small, jx=2.5, jy=1.5, seed=4, order=order, mode=mode)
    np.testing.assert_array_equal(got, denoise.apply_scan_noise(small.astype(np.float64), jx=2.5, jy=1.5, seed=4, order=order, mode=mode))


def test_torch_operands_stay_on_the_device(denoise):
    torch = pytest.importorskip("torch")
    from mtflearn_amd import resident
    shape = (2, 33, 65)
    stack = sc.images(shape).astype(np.float32)
    dx, dy = so.jitter(6, shape, 1.0, 0.3)
    t = lambda a: torch.from_numpy(a).cuda()
    got = resident.scan_noise_device(t(stack), t(dx), t(dy), order=3, mode="reflect")
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape
    np.testing.assert_array_equal(got.cpu().numpy(), denoise.apply_scan_noise(stack, jx=1.0, jy=0.3, seed=6, order=3, mode="reflect"))
