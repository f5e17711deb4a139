"""CPU checks of the alignment maps (``zmoments.align_map`` / ``ZPs.align_maps`` / ``zk_align_planes`` / ``zk_frame_align``): the
new symbols, the refusals that come before any device call, the empty input, and -- on the NumPy statement of
tests/align_cases.py alone -- the margins the end-to-end GPU test of tests/test_gpu_align_maps.py then asserts of the kernel."""
import os
import re

import numpy as np
import pytest

import align_cases as ac
import align_maps_cases as mc
from mtflearn_amd import _native, zmoments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_SYMBOLS = ["zk_align_planes", "zk_align_planes_dev", "zk_frame_align", "zk_frame_align_dev", "zk_align_set_band_bytes"]


def test_map_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zernike_hip.h")).read(), flags=re.S)
    lib = _native.load()
    for sym in MAP_SYMBOLS:
        decl = re.search(rf"\bint {sym}\((.*?)\);", header, flags=re.S)
        assert decl and sym in _native.SYMBOLS and hasattr(lib, sym), sym
        assert len(_native.SYMBOLS[sym][1]) == decl.group(1).count(",") + 1, sym
    from mtflearn_amd import ZPs, resident
    from mtflearn_amd.features.moments import AlignMaps
    assert AlignMaps._fields == ("angle", "score", "best", "norm2")
    assert callable(ZPs.align_maps) and callable(zmoments.align_map)
    assert callable(resident.align_planes_device) and callable(resident.align_maps_device)
    for name in ("align_planes", "align_planes_dev", "frame_align", "frame_align_dev", "align_set_band_bytes"):
        assert callable(getattr(_native, name)), name


def test_refusals_come_from_the_host_before_any_device_call():
    n, m = ac.labels(4)
    P = len(n)
    dense = zmoments(np.ones((P, 5, 6)), n, m)
    t = np.ones((2, P))
    with pytest.raises(ValueError, match=r"rows of moments: align\b"):
        zmoments(np.ones((3, P)), n, m).align_map(t)                       # rank-2 data: the message names align
    n1, m1 = np.delete(n, 1), np.delete(m, 1)                              # (1, -1) goes, (1, 1) stays
    with pytest.raises(ValueError, match="not paired"):
        zmoments(np.ones((P - 1, 5, 6)), n1, m1).align_map(np.ones((2, P - 1)))
    with pytest.raises(ValueError, match="64 templates"):
        dense.align_map(np.ones((65, P)))
    with pytest.raises(ValueError, match="n_theta"):
        dense.align_map(t, n_theta=0)
    with pytest.raises(ValueError, match="symmetry"):
        dense.align_map(t, symmetry=0)
    with pytest.raises(ValueError, match="key"):
        dense.align_map(t, key="euclid")
    with pytest.raises(ValueError, match="labels of the rows"):
        dense.align_map(zmoments(np.ones((2, 6)), *ac.labels(2)))
    spec = _native.AlignSpec(n, m, t)
    planes = np.ones((P, 30))
    with pytest.raises(ValueError, match="plane_stride"):
        _native.align_planes(planes, spec, n_pixels=31)
    with pytest.raises(ValueError, match="out_plane_stride"):
        _native.align_planes(planes, spec, out=(np.empty((2, 29)), np.empty((2, 29)), np.empty(30, np.int32), np.empty(30)))
    for call in (lambda: _native.align_planes_dev(0, 0, 31, 30, spec, 0, 0, 0, 0, 31), lambda: _native.align_planes_dev(0, 0, 30, 30, spec, 0, 0, 0, 0, 29)):
        with pytest.raises(ValueError, match="plane_stride"):
            call()
    # align and rotate_each keep refusing dense frames, and now say where to go
    with pytest.raises(ValueError, match="rank-2.*align_map"):
        dense.align(t)
    with pytest.raises(ValueError, match="rank-2"):
        dense.rotate_each(np.zeros(5))
    from mtflearn_amd import ZPs
    zps = ZPs(4, 8)
    for kwargs, word in ((dict(templates=np.ones((65, P))), "64 templates"), (dict(templates=t, n_theta=0), "n_theta"),
                         (dict(templates=t, key="euclid"), "key"), (dict(templates=np.ones((2, P + 1))), "templates must be")):
        with pytest.raises(ValueError, match=word):
            zps.align_maps(np.ones((9, 9)), **kwargs)
    with pytest.raises(ValueError, match="2D image"):
        zps.align_maps(np.ones((2, 9, 9)), t)


def test_empty_input_needs_no_device():
    n, m = ac.labels(4)
    P = len(n)
    spec = _native.AlignSpec(n, m, np.ones((3, P)))
    angle, score, best, norm2 = _native.align_planes(np.empty((P, 0)), spec)
    assert angle.shape == score.shape == (3, 0) and best.shape == norm2.shape == (0,)
    assert angle.dtype == score.dtype == norm2.dtype == np.float64 and best.dtype == np.int32
    angle, score, best, norm2 = _native.align_planes(np.ones((P, 7)), spec, n_pixels=0)     # a stride without pixels
    assert angle.shape == (3, 0) and best.shape == (0,)
    res = zmoments(np.empty((P, 0, 5)), n, m).align_map(np.ones((3, P)))
    assert res.angle.shape == res.score.shape == (3, 0, 5) and res.best.shape == res.norm2.shape == (0, 5)
    assert res.best.dtype == np.int32


def test_fixture_frame_is_what_the_cases_say():
    img = mc.frame()
    assert img.shape == (mc.FRAME, mc.FRAME) and img.dtype == np.float64
    rows, cols, _, _ = mc.centres()
    x = mc.dense_moments()[:, rows, cols].T
    direct = mc.patch_moments(np.stack([mc.patches()[p[0]] for p in mc.PLANTED]))
    np.testing.assert_allclose(x, direct, rtol=0, atol=1e-15)             # a centre's window is the stamped patch


def test_statement_recovers_the_planted_angles_within_the_margin():
    """Of the statement alone; tests/test_gpu_align_maps.py asserts the same margins of the kernel."""
    n, m, _ = mc.basis()
    t = mc.templates()
    rows, cols, planted, alpha = mc.centres()
    mask = ac.select_mask(m, mc.M_SELECT)
    x = mc.dense_moments()[:, rows, cols].T
    angle, score, best, _ = ac.align_statement(x, t, n, m, mask, 360, mc.SYMMETRY, True, "cosine")
    np.testing.assert_array_equal(best, planted)
    three = planted == 0
    gap = ac.circular_gap(angle[three, 0], alpha[three] % 120, period=120)
    print(f"statement: angle errors {gap} degree, margin {mc.ANGLE_MARGIN:.4f}")
    assert (gap <= mc.ANGLE_MARGIN).all()
    moved, stayed, bound = mc.never_moved_away(x[three][:, mask], t[0, mask], n[mask], m[mask], angle[three, 0])
    assert (moved <= stayed + bound).all(), (moved - stayed - bound).max()


def test_statement_cosine_map_peaks_at_the_planted_centres():
    from local_max_oracle import local_max_raster
    n, m, _ = mc.basis()
    t = mc.templates()
    mask = ac.select_mask(m, mc.M_SELECT)
    d = mc.dense_moments()
    X = d.reshape(len(n), -1).T
    _, score, best, _ = ac.align_statement(X, t, n, m, mask, 360, mc.SYMMETRY, True, "cosine")
    norm2 = (X[:, mask] ** 2).sum(axis=1).reshape(mc.FRAME, mc.FRAME)
    cos = mc.cosine_map(score.T.reshape(2, mc.FRAME, mc.FRAME), norm2, (t[:, mask] ** 2).sum(axis=1))
    assert cos.max() <= 1 + 1e-12
    points = local_max_raster(cos, mc.MIN_DISTANCE, threshold=mc.COSINE_THRESHOLD)
    assert mc.peaks_match_centres(points), points
