"""GPU tests of the alignment maps: the planes kernel of csrc/zk_align.hip against the rows kernel (bit for bit: one body, two
operand layouts) and, independently of it, against the NumPy statement and bounds of tests/align_cases.py; norm2; the banded frame
route against transform + align_map; the routes against each other; the library's refusals; and the planted frame of
tests/align_maps_cases.py end to end (margins licensed by tests/test_align_maps_cpu.py)."""
import warnings
from ctypes import POINTER, c_double, c_int32, c_void_p

import numpy as np
import pytest

import align_cases as ac
import align_maps_cases as mc
from mtflearn_amd import ZPs, _native, zmoments

pytestmark = pytest.mark.gpu

KEYS = ("distance", "cosine")
SENTINEL = -7.25


def _spec(n, m, t, sel, symmetry, n_theta=360, refine=True, key="distance"):
    select = None if sel is None else ac.select_mask(m, sel).astype(np.int32)
    return _native.AlignSpec(n, m, t, select, n_theta, symmetry, 3 if refine else 0, key)


@pytest.mark.parametrize("select", list(ac.SELECTS))
@pytest.mark.parametrize("n_max", ac.NMAX_GRID)
def test_planes_equal_rows_bit_for_bit(n_max, select):
    """align_planes on X.T is align_rows on X, transposed -- compact, and with padded strides on both sides.  The rows results are
    taken once per option set on all 1000 rows (a row's results do not depend on its place in the batch: test_gpu_align.py)."""
    sel, symmetry = ac.SELECTS[select]
    X, Tm, n, m = ac.case_inputs(n_max)
    for t in ac.T_GRID:
        for refine in (True, False):
            for key in KEYS:
                spec = _spec(n, m, Tm[:t], sel, symmetry, 360, refine, key)
                want = _native.align_rows(X, spec)
                for pixels in ac.N_GRID:
                    got = _native.align_planes(np.ascontiguousarray(X[:pixels].T), spec)
                    for u, v in zip(got[:2], want[:2]):
                        np.testing.assert_array_equal(u, v[:pixels].T)
                    np.testing.assert_array_equal(got[2], want[2][:pixels])
                    # plane_stride = pixels + 3 (the padding holds 1e300), out_plane_stride = pixels + 5 (a sentinel, untouched)
                    planes = np.full((len(n), pixels + 3), 1e300)
                    planes[:, :pixels] = X[:pixels].T
                    out = (np.full((t, pixels + 5), SENTINEL), np.full((t, pixels + 5), SENTINEL), np.full(pixels + 2, -9, np.int32),
                           np.full(pixels + 2, SENTINEL))
                    _native.align_planes(planes, spec, n_pixels=pixels, out=out)
                    for u, v in zip(out[:2], want[:2]):
                        np.testing.assert_array_equal(u[:, :pixels], v[:pixels].T)
                        assert (u[:, pixels:] == SENTINEL).all()
                    np.testing.assert_array_equal(out[2][:pixels], want[2][:pixels])
                    np.testing.assert_array_equal(out[3][:pixels], got[3])
                    assert (out[2][pixels:] == -9).all() and (out[3][pixels:] == SENTINEL).all()


def _check_planes(x, t, n, m, sel, symmetry, n_theta, refine, key, tally):
    """The criterion of test_gpu_align.py::_check, on align_planes: nothing here comes from the rows kernel."""
    mask = ac.select_mask(m, sel)
    angle, score, best, _ = _native.align_planes(np.ascontiguousarray(x.T), _spec(n, m, t, sel, symmetry, n_theta, refine, key))
    angle, score = angle.T, score.T
    assert angle.shape == score.shape == (len(x), len(t)) and best.shape == (len(x),)
    bound = ac.score_bound(x, t, n, m, mask)
    _, _, _, grid = ac.align_statement(x, t, n, m, mask, n_theta, symmetry, False, key)
    err = np.abs(score - ac.f_longdouble(x, t, n, m, mask, angle))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    assert (score >= grid.max(axis=2) - bound).all()
    period = 360 / symmetry
    assert ((angle >= 0) & (angle < period)).all()
    np.testing.assert_array_equal(best, ac.best_of(score, ac.key_values(t, mask, key), key))
    if not refine:
        theta = ac.theta_grid(n_theta, symmetry)
        j = np.rint(angle / (period / n_theta)).astype(int)
        np.testing.assert_array_equal(theta[j], angle)
        skip = ac.near_tie(grid, bound) if n_theta > 1 else np.zeros(j.shape, bool)
        np.testing.assert_array_equal(j[~skip], grid.argmax(axis=2)[~skip])
        tally[0] += j.size
        tally[1] += int(skip.sum())


@pytest.mark.parametrize("t", [1, 5])
@pytest.mark.parametrize("n_max", [4, 8, 13])
def test_planes_match_the_statement(n_max, t):
    X, Tm, n, m = ac.case_inputs(n_max)
    tally = [0, 0]
    for pixels in (65, 257):
        for n_theta in ac.NTHETA_GRID:
            for refine in (True, False):
                for key in KEYS:
                    _check_planes(X[:pixels], Tm[:t], n, m, None, 1, n_theta, refine, key, tally)
    print(f"n_max {n_max} T {t}: {tally[1]} of {tally[0]} pairs skipped as near ties ({tally[1] / tally[0]:.2e})")
    assert tally[1] <= 0.01 * tally[0]                  # the cap of test_gpu_align.py


@pytest.mark.parametrize("select", list(ac.SELECTS))
@pytest.mark.parametrize("n_max", ac.NMAX_GRID)
def test_norm2(n_max, select):
    sel, symmetry = ac.SELECTS[select]
    X, Tm, n, m = ac.case_inputs(n_max)
    mask = ac.select_mask(m, sel)
    x = X[:257].copy()
    zero = np.zeros(len(x), bool)
    zero[3::7] = True
    x[np.ix_(zero, mask)] = 0.0                         # pixels whose selection holds no nonzero moment
    _, _, _, norm2 = _native.align_planes(np.ascontiguousarray(x.T), _spec(n, m, Tm[:2], sel, symmetry))
    want = (x[:, mask].astype(np.longdouble) ** 2).sum(axis=1)
    err = np.abs(norm2.astype(np.longdouble) - want)
    bound = (len(n) + 2) * ac.U * want
    print(f"n_max {n_max} {select}: worst norm2 error {float((err[~zero] / bound[~zero]).max()):.3f} of the bound")
    assert (err <= bound).all()
    assert (norm2[zero] == 0).all() and (norm2[~zero] > 0).all()


FRAME_CASES = [(8, 4), (9, 4), (16, 8), (28, 13), (36, 18)]


def _frame(dtype):
    rng = np.random.RandomState(41)
    return rng.standard_normal((37, 41)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("size,n_max", FRAME_CASES)
def test_frame_route_equals_transform_then_align_map(size, n_max, dtype):
    """Bit for bit, borders included, whatever the band: one row, five rows, the whole frame."""
    import torch
    from mtflearn_amd import resident
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        zps = ZPs(n_max, size)
    image = _frame(dtype)
    h, w = image.shape
    P = len(zps.n)
    t = np.random.RandomState(n_max).standard_normal((3, P))
    want = zps.transform(image).align_map(t)
    assert want.angle.shape == want.score.shape == (3, h, w) and want.best.shape == want.norm2.shape == (h, w)
    try:
        for rows in (1, 5, h):
            _native.align_set_band_bytes(rows * P * w * 8)
            got = zps.align_maps(image, t)
            assert got.best.dtype == np.int32
            for u, v in zip(got, want):
                np.testing.assert_array_equal(u, v)
        # a band of rows written in place into whole-frame tensors: exactly those rows, the rest keeps its sentinel
        _native.align_set_band_bytes(5 * P * w * 8)
        plan = zps._device_plan()
        img = torch.from_numpy(image).cuda()
        full = (torch.full((3, h, w), SENTINEL, dtype=torch.float64, device="cuda"), torch.full((3, h, w), SENTINEL, dtype=torch.float64, device="cuda"),
                torch.full((h, w), -9, dtype=torch.int32, device="cuda"), torch.full((h, w), SENTINEL, dtype=torch.float64, device="cuda"))
        assert resident.align_maps_device(plan, img, t, row0=5, n_rows=7, full=full) is full
        torch.cuda.synchronize()
        for a, v, fill in zip(full, want, (SENTINEL, SENTINEL, -9, SENTINEL)):
            a = a.cpu().numpy()
            np.testing.assert_array_equal(a[..., 5:12, :], v[..., 5:12, :])
            assert (a[..., :5, :] == fill).all() and (a[..., 12:, :] == fill).all()
    finally:
        _native.align_set_band_bytes(0)


def test_routes_runs_and_streams_agree_bit_for_bit():
    import torch
    from mtflearn_amd import resident
    zps = ZPs(8, 16)
    image = _frame(np.float32)
    h, w = image.shape
    t = np.random.RandomState(3).standard_normal((5, len(zps.n)))
    first = zps.align_maps(image, t, key="cosine")
    again = zps.align_maps(image, t, key="cosine")
    mom = zps.transform(image)
    planes_host = mom.align_map(t, key="cosine")
    try:
        _native.align_set_host_chunk(1)                 # 256 pixels per chunk of the host planes route
        small = mom.align_map(t, key="cosine")
    finally:
        _native.align_set_host_chunk(0)
    for other in (again, planes_host, small):
        for u, v in zip(first, other):
            np.testing.assert_array_equal(u, v)
    plan = zps._device_plan()
    img = torch.from_numpy(image).cuda()
    res = resident.align_maps_device(plan, img, t, key="cosine")
    band = resident.align_maps_device(plan, img, t, key="cosine", row0=9, n_rows=11)
    md = resident.frame_moments_device(plan, img)
    res_planes = resident.align_planes_device(md, zps.n, zps.m, t, key="cosine")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res_side = resident.align_maps_device(plan, img, t, key="cosine")
        planes_side = resident.align_planes_device(md, zps.n, zps.m, t, key="cosine")
    side.synchronize()
    torch.cuda.synchronize()
    for u, a, b, c, d, e in zip(first, res, res_planes, res_side, planes_side, band):
        for v in (a, b, c, d):
            np.testing.assert_array_equal(u, v.cpu().numpy())
        np.testing.assert_array_equal(u[..., 9:20, :], e.cpu().numpy())
    nd = _native.DeviceArray.from_numpy(np.ascontiguousarray(mom.data))
    res_nd = resident.align_planes_device(nd, zps.n, zps.m, zmoments(t, zps.n, zps.m), key="cosine")
    for u, v in zip(first, res_nd):
        np.testing.assert_array_equal(u, v.numpy())


def test_library_refusals_come_with_a_message_before_any_launch():
    """Arguments chosen to be refused: ZK_E_BADARG and a message, nothing launched."""
    n, m = ac.labels(4)
    lib = _native.load()
    n32, m32 = n.astype(np.int32), m.astype(np.int32)
    bad_n, bad_m = np.delete(n32, 1), np.delete(m32, 1)
    pi, pd = POINTER(c_int32), POINTER(c_double)
    out = np.empty((65, 8))

    def planes_call(nn, mm, cols, T, n_theta, pixels=3, stride=4, out_stride=8, symmetry=1, key=0):
        planes, t = np.ones((cols, stride)), np.ones((T, cols))
        return lib.zk_align_planes(0, planes.ctypes.data_as(c_void_p), pixels, stride, cols, nn.ctypes.data_as(pi), mm.ctypes.data_as(pi),
                                   t.ctypes.data_as(pd), T, None, n_theta, symmetry, 3, key, None, 0, None, out.ctypes.data_as(c_void_p), None,
                                   None, None, out_stride)

    P = len(n)
    for kwargs, word in ((dict(nn=bad_n, mm=bad_m, cols=P - 1, T=2, n_theta=360), "not paired"), (dict(nn=n32, mm=m32, cols=P, T=65, n_theta=360), "64 templates"),
                         (dict(nn=n32, mm=m32, cols=P, T=2, n_theta=0), "n_theta"), (dict(nn=n32, mm=m32, cols=P, T=2, n_theta=7, symmetry=0), "symmetry"),
                         (dict(nn=n32, mm=m32, cols=P, T=2, n_theta=7, key=5), "key"),
                         (dict(nn=n32, mm=m32, cols=P, T=2, n_theta=7, pixels=5, stride=4), "plane_stride"),
                         (dict(nn=n32, mm=m32, cols=P, T=2, n_theta=7, pixels=4, stride=4, out_stride=3), "out_plane_stride")):
        assert planes_call(**kwargs) == _native.ZK_E_BADARG, kwargs
        assert word in _native.last_error(), (word, _native.last_error())
    assert planes_call(n32, m32, P, 2, 7) == 0
    assert planes_call(n32, m32, P, 2, 7, pixels=0, stride=0) == 0         # nothing to do is not an error

    zps = ZPs(4, 8)
    plan = zps._device_plan()
    image = np.ones((9, 10), np.float32)
    t = np.ones((2, P))

    def frame_call(handle=None, T=2, n_theta=7, row0=0, n_rows=9, out_stride=90, dtype=_native.ZK_F32):
        return lib.zk_frame_align(plan._h if handle is None else handle, image.ctypes.data_as(c_void_p), dtype, 9, 10, row0, n_rows,
                                  np.ones((T, P)).ctypes.data_as(pd), T, None, n_theta, 1, 3, 0, None, 0, None,
                                  out.ctypes.data_as(c_void_p), None, None, None, out_stride)

    for kwargs, word in ((dict(handle=c_void_p(None)), "null plan"), (dict(T=65), "64 templates"), (dict(n_theta=0), "n_theta"),
                         (dict(row0=5, n_rows=5), "row band"), (dict(out_stride=89), "out_plane_stride"), (dict(dtype=17), "dtype")):
        assert frame_call(**kwargs) == _native.ZK_E_BADARG, kwargs
        assert word in _native.last_error(), (word, _native.last_error())
    assert frame_call(n_rows=0) == 0
    assert frame_call(out_stride=90, n_rows=4, row0=5) == 0
    with pytest.raises(ValueError, match="64 templates"):
        zps.align_maps(image, np.ones((65, P)))
    del t


def test_planted_frame_end_to_end():
    """The frame of tests/test_align_maps_cpu.py: at the planted centres best is the planted template and the angle lies within the
    CPU-established margin; the peaks of the cosine map are the planted centres."""
    from mtflearn_amd.features import local_max
    zps = ZPs(mc.N_MAX, mc.SIZE)
    n, m, _ = mc.basis()
    t = mc.templates()
    mask = ac.select_mask(m, mc.M_SELECT)
    rows, cols, planted, alpha = mc.centres()
    maps = zps.align_maps(mc.frame(), t, m_select=mc.M_SELECT, symmetry=mc.SYMMETRY, key="cosine")
    np.testing.assert_array_equal(maps.best[rows, cols], planted)
    three = planted == 0
    got = maps.angle[0][rows, cols][three]
    gap = ac.circular_gap(got, alpha[three] % 120, period=120)
    print(f"kernel: angle errors {gap} degree, margin {mc.ANGLE_MARGIN:.4f}")
    assert (gap <= mc.ANGLE_MARGIN).all()
    x = mc.dense_moments()[:, rows, cols].T
    want, _, _, _ = ac.align_statement(x, t, n, m, mask, 360, mc.SYMMETRY, True, "cosine")
    assert ac.circular_gap(got, want[three, 0], period=120).max() <= 1e-6
    moved, stayed, bound = mc.never_moved_away(x[three][:, mask], t[0, mask], n[mask], m[mask], got)
    assert (moved <= stayed + bound).all(), (moved - stayed - bound).max()
    cos = mc.cosine_map(maps.score, maps.norm2, (t[:, mask] ** 2).sum(axis=1))
    assert cos.max() <= 1 + 1e-12
    points = local_max(cos, mc.MIN_DISTANCE, threshold=mc.COSINE_THRESHOLD)
    assert mc.peaks_match_centres(points), points
