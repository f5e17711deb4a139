"""CPU checks of mtflearn_amd.denoise.apply_scan_noise: the SciPy statement (tests/scan_noise_oracle.py) against the outputs
recorded from the reference, the jitter draws, the C ABI table and every argument check -- all of which run before any device
call, so they hold on a machine without a GPU.  The licence of tests/test_gpu_scan_noise.py."""
import os
import re

import numpy as np
import pytest

import scan_noise_cases as sc
import scan_noise_oracle as so
from mtflearn_amd import _native, denoise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["zk_scan_resample", "zk_scan_resample_dev", "zk_scan_resample_set_chunk"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "scan_noise_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def test_oracle_reproduces_the_reference(golden):
    """Frame-by-frame SciPy equals the reference's 3-D call: bit for bit at orders 0 and 1, to 1e-14 max|x| at order 3
    ('mirror' and 'grid-wrap', whose prefilter along z is exact and leaves integer z positions alone)."""
    worst = 0.0
    for shape, dtype, order, mode, k in sc.golden_cases():
        sid = sc.shape_id(shape)
        stack = golden[f"{sid}/images"].astype(dtype)
        ref = sc.golden_output(golden, shape, dtype, order, mode, k)
        got = so.resample(stack, golden[f"{sid}/dx"][k], golden[f"{sid}/dy"][k], order, mode)
        assert got.dtype == ref.dtype == np.dtype(dtype)
        if order < 3:
            np.testing.assert_array_equal(got, ref, err_msg=str((shape, dtype, order, mode, k)))
        elif dtype == np.float64:
            dist = np.abs(got - ref).max() / np.abs(stack).max()
            worst = max(worst, dist)
            assert dist <= 1e-14, (shape, dtype, order, mode, k, dist)
        else:                       # two float64 results 1e-14 apart, each rounded once: the same float32 or its neighbour
            ulps, bound, _ = sc.distance(got, ref, 1, 1.0)
            assert ulps <= bound, (shape, dtype, order, mode, k, ulps)
    print(f"order 3, float64: largest |oracle - reference| / max|x| = {worst:.2e}")


def test_golden_file_is_what_the_case_table_says(golden):
    for shape in sc.GOLDEN_SHAPES:
        sid = sc.shape_id(shape)
        np.testing.assert_array_equal(golden[f"{sid}/images"], sc.images(shape))
        np.testing.assert_array_equal(golden[f"{sid}/seeds"], [sc.seed_of(shape, k) for k in range(len(sc.GOLDEN_JITTERS))])
        for dtype in sc.DTYPES:
            assert golden[f"{sid}/{np.dtype(dtype).name}"].shape == (len(sc.GOLDEN_PAIRS), len(sc.GOLDEN_JITTERS)) + shape
            np.testing.assert_array_equal(sc.images(shape).astype(dtype).astype(np.float64), sc.images(shape))
    assert (3, "reflect") not in sc.GOLDEN_PAIRS and len(sc.GOLDEN_PAIRS) == 14 and len(sc.PAIRS) == 15
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "scan_noise_golden.npz")) < 300 * 1024


def test_padded_reflect_form_agrees_with_the_direct_call_on_a_long_axis():
    """At n = 40 SciPy's truncated start is below rounding, so the oracle's padded construction and the direct call agree."""
    frame = sc.images((1, 40, 40))[0]
    dx, dy = so.jitter(5, (1, 40, 40), 2.5, 1.5)
    a = so.resample_frame(frame, dx[0], dy[0], 3, "reflect", padded=True)
    b = so.resample_frame(frame, dx[0], dy[0], 3, "reflect", padded=False)
    dist = np.abs(a - b).max() / np.abs(frame).max()
    print(f"padded vs direct at n = 40: {dist:.2e}")
    assert dist <= 1e-13


def test_draws_equal_the_reference(golden, monkeypatch):
    """The shifts that would be uploaded are the reference's, bit for bit -- also with a zero factor and with None."""
    seen = {}

    def capture(images, dx, dy, order, mode_code):
        seen.update(dx=dx, dy=dy, order=order, mode=mode_code)
        return images

    monkeypatch.setattr(denoise, "_resample_host", capture)
    for shape in sc.GOLDEN_SHAPES:
        sid = sc.shape_id(shape)
        for k, (jx, jy) in enumerate(sc.GOLDEN_JITTERS):
            denoise.apply_scan_noise(sc.images(shape), jx=jx, jy=jy, seed=sc.seed_of(shape, k), order=3, mode="grid-wrap")
            assert seen["dx"].dtype == seen["dy"].dtype == np.float64 and seen["dx"].flags.c_contiguous and seen["dy"].flags.c_contiguous
            np.testing.assert_array_equal(seen["dx"], golden[f"{sid}/dx"][k])
            np.testing.assert_array_equal(seen["dy"], golden[f"{sid}/dy"][k])
            assert (seen["order"], seen["mode"]) == (3, _native.RESAMPLE_MODES["grid-wrap"])
        # jx = 0 still consumes the first draw: dy is the reference's dy of the same seed; None means 0
        jy = sc.GOLDEN_JITTERS[1][1]
        for zero in (0, None):
            dx, dy = denoise._jitter(sc.seed_of(shape, 1), shape, zero, jy)
            np.testing.assert_array_equal(dy, golden[f"{sid}/dy"][1])
            assert dx.shape == shape[:2] and not dx.any()
        dx, dy = denoise._jitter(sc.seed_of(shape, 1), shape, sc.GOLDEN_JITTERS[1][0], None)
        np.testing.assert_array_equal(dx, golden[f"{sid}/dx"][1])
        assert dy.shape == (shape[0], shape[2]) and not dy.any()
        for a, b in zip(denoise._jitter(3, shape, 1.5, 0.5), so.jitter(3, shape, 1.5, 0.5)):
            np.testing.assert_array_equal(a, b)
    assert denoise.apply_scan_noise.__defaults__ == (1, 0, None, 1, "reflect")


def test_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "zernike_hip.h")).read()
    assert re.search(r"#define ZK_ABI_VERSION 2\b", text)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _native.load()
    assert lib.zk_abi_version() == 2
    for sym in SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    for mode, code in _native.RESAMPLE_MODES.items():
        assert re.search(rf"#define ZK_RESAMPLE_{mode.upper().replace('-', '_')}\s+{code}\b", header)
    assert set(_native.RESAMPLE_MODES) == set(sc.MODES)
    from mtflearn_amd import distributed, resident
    assert "apply_scan_noise" in denoise.__all__
    assert callable(resident.scan_noise_device) and distributed.scan_noise_device is resident.scan_noise_device
    assert "apply_scan_noise" in denoise.__doc__


def test_every_refusal_comes_before_any_device_call():
    x = sc.images((2, 5, 7))
    cases = [
        (ValueError, lambda: denoise.apply_scan_noise(x[0])),                               # rank 2
        (ValueError, lambda: denoise.apply_scan_noise(x[None])),                            # rank 4
        (ValueError, lambda: denoise.apply_scan_noise(np.zeros((0, 5, 7)))),
        (ValueError, lambda: denoise.apply_scan_noise(np.zeros((2, 0, 7)))),
        (ValueError, lambda: denoise.apply_scan_noise(np.zeros((2, 5, 0)))),
        (TypeError, lambda: denoise.apply_scan_noise(x.astype(np.int32))),
        (TypeError, lambda: denoise.apply_scan_noise(x.astype(np.complex128))),
        (TypeError, lambda: denoise.apply_scan_noise(x.astype(np.float16))),
        (ValueError, lambda: denoise.apply_scan_noise(x, mode="periodic")),
        (RuntimeError, lambda: denoise.apply_scan_noise(x, order=6)),
        (RuntimeError, lambda: denoise.apply_scan_noise(x, order=-1)),
        (ValueError, lambda: denoise.apply_scan_noise(x, jx=np.inf)),
        (ValueError, lambda: denoise.apply_scan_noise(x, jy=np.nan)),
    ]
    cases += [(NotImplementedError, lambda o=o: denoise.apply_scan_noise(x, order=o)) for o in (2, 4, 5)]
    cases += [(NotImplementedError, lambda m=m: denoise.apply_scan_noise(x, order=3, mode=m)) for m in ("nearest", "grid-constant", "constant")]
    cases += [(NotImplementedError, lambda o=o: denoise.apply_scan_noise(x, order=o, mode="wrap")) for o in (0, 1, 3)]
    for k, (exc, call) in enumerate(cases):
        with pytest.raises(exc) as info:
            call()
        assert type(info.value) is exc, f"refusal {k}: {type(info.value).__name__}"      # RuntimeError would also mean "no device"
    with pytest.raises(RuntimeError, match="spline order not supported"):
        denoise.apply_scan_noise(x, order=7)
    with pytest.raises(NotImplementedError, match="0, 1 and 3"):
        denoise.apply_scan_noise(x, order=2)
    with pytest.raises(NotImplementedError, match="reflect, mirror, grid-wrap"):
        denoise.apply_scan_noise(x, order=3, mode="constant")
    with pytest.raises(NotImplementedError, match="grid-constant"):
        denoise.apply_scan_noise(x, mode="wrap")
    from mtflearn_amd import resident
    fake = lambda shape, dtype=np.float64: _native.DeviceArray(shape, dtype, 0, _base=object(), _ptr=4096)
    stack, dx, dy = fake((2, 5, 7), np.float32), fake((2, 5)), fake((2, 7))
    bad = [
        (ValueError, lambda: resident.scan_noise_device(fake((5, 7)), dx, dy)),
        (ValueError, lambda: resident.scan_noise_device(stack, dy, dx)),                     # swapped shapes
        (ValueError, lambda: resident.scan_noise_device(stack, fake((2, 5), np.float32), dy)),
        (ValueError, lambda: resident.scan_noise_device(stack, dx, dy, out=fake((2, 5, 7), np.float64))),
        (ValueError, lambda: resident.scan_noise_device(stack, np.zeros((2, 5)), dy)),       # a host array
        (TypeError, lambda: resident.scan_noise_device(fake((2, 5, 7), np.uint16), dx, dy)),
        (NotImplementedError, lambda: resident.scan_noise_device(stack, dx, dy, order=3, mode="nearest")),
        (RuntimeError, lambda: resident.scan_noise_device(stack, dx, dy, order=9)),
        (ValueError, lambda: resident.scan_noise_device(stack, dx, dy, mode="nope")),
    ]
    for k, (exc, call) in enumerate(bad):
        with pytest.raises(exc) as info:
            call()
        assert type(info.value) is exc, f"resident refusal {k}: {type(info.value).__name__}"


def test_library_refuses_bad_arguments_without_a_device():
    """The C entry points check their arguments before they look for a device: ZK_E_BADARG and a message."""
    lib = _native.load()
    x = np.zeros((1, 2, 3), dtype=np.float32)
    d = np.zeros(8)
    p = lambda a: a.ctypes.data_as(_native.c_void_p)
    good = dict(dtype=_native.ZK_F32, z=1, h=2, w=3, order=1, mode=0)
    for change in (dict(dtype=7), dict(z=0), dict(h=-1), dict(order=2), dict(order=3, mode=2), dict(mode=6), dict(mode=-1)):
        a = {**good, **change}
        rc = lib.zk_scan_resample(0, p(x), a["dtype"], a["z"], a["h"], a["w"], p(d), p(d), a["order"], a["mode"], p(x))
        assert rc == _native.ZK_E_BADARG and "scan_resample" in _native.last_error(), change
    assert lib.zk_scan_resample(0, None, 0, 1, 2, 3, p(d), p(d), 1, 0, p(x)) == _native.ZK_E_BADARG
    assert lib.zk_scan_resample_dev(0, p(x), 0, 1, 2, 3, p(d), p(d), 3, 0, p(x), p(d), 8, None) == _native.ZK_E_BADARG   # scratch too small
    assert lib.zk_scan_resample_set_chunk(0, -1) == _native.ZK_E_BADARG


def test_good_arguments_fail_loudly_without_a_device():
    x = sc.images((1, 5, 7))
    if _native.device_count() > 0:
        assert denoise.apply_scan_noise(x, seed=1).shape == x.shape       # with a device the same call simply runs
    else:
        with pytest.raises(RuntimeError, match="no HIP device"):
            denoise.apply_scan_noise(x, seed=1)
