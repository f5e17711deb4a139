"""The kernels of csrc/zk_datasets.hip past the sizes of tests/test_gpu_datasets.py, against the NumPy statement of the gather
(tests/datasets_oracle.py; tests/test_datasets_cpu.py proves the inputs): the offset scan with more than one tile per lane, the
list sort at every length where it changes (one window, several windows in LDS, the LDS / global-memory seam, either side of a
power of two), the windows of the uncut kernel, and the cut without the taper at ``r == R``.

Criteria: ``datasets_oracle.tolerance`` (float64 ``1e-12 * max|ref|``, float32 ``k`` spacings at ``max|ref|``, ``k`` the most
contributions on one pixel, from the oracle); the order probes are float32 and exact, bit for bit."""
import numpy as np
import pytest

import datasets_cases as dc
import datasets_oracle as oracle
from mtflearn_amd import datasets

pytestmark = pytest.mark.gpu


def close(got, ref, k, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    err, tol = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) if ref.size else 0.0, oracle.tolerance(ref, k)
    print(f"{what}: max|delta| {err:.3e}, bound {tol:.3e} (k = {k})")
    assert err <= tol, (what, err, tol)


def run(case, dtype, taper=True):
    """The case through ``zk_render_gaussians`` (the tapered form through the public function); ``(device result, oracle, k)``."""
    img = dc.case_frame(case, dtype)
    pts, amps = np.ascontiguousarray(case["pts"]), np.ascontiguousarray(np.broadcast_to(case["amps"], len(case["pts"])), dtype=np.float64)
    ref, k = oracle.render(img, pts, amps, case["sigma"], case["r_factor"], taper=taper)
    if taper:
        datasets.add_tapered_gaussian(img, pts, case["sigma"], amps, case["r_factor"])
    else:
        datasets._render_host(img, pts, amps, case["sigma"], case["r_factor"], False)
    return img, ref, k


# ------------------------------------------------------------------------------------------------ the offset scan
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("shape", dc.MANY_TILES_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_more_tiles_than_scan_lanes(shape, dtype):
    """1025 and 1539 tiles: every lane of the scan owns two counts, about half (a third) of the lanes own none, the last owner
    has a ragged share.  A wrong offset sends a tile to another tile's list (or to none), so its pixels miss their points."""
    case = dc.many_tiles_case(shape)
    tiles = -(-shape[0] // dc.TILE) * -(-shape[1] // dc.TILE)
    assert tiles > 1024 and -(-tiles // 1024) == 2
    got, ref, k = run(case, dtype)
    assert np.abs(ref.astype(np.float64) - dc.case_frame(case, dtype)).max() > 0.5          # the points did land
    close(got, ref, k, f"{shape} {np.dtype(dtype).name}")


# ------------------------------------------------------------------------------------------------ the list sort and its windows
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("L", dc.SEAM_LENGTHS)
def test_list_lengths_at_the_seams_random(L, dtype):
    """One list of exactly ``L`` entries (the middle tile of 3 x 3) against the oracle."""
    got, ref, k = run(dc.seam_random_case(L), dtype)
    assert k >= 1
    close(got, ref, k, f"L = {L} {np.dtype(dtype).name}")


@pytest.mark.parametrize("layout", ["consecutive", "spread"])
@pytest.mark.parametrize("L", dc.SEAM_LENGTHS)
def test_list_order_at_the_seams_exact(L, layout):
    """The order of one list of ``L`` entries, read off a float32 frame bit for bit (datasets_cases.order_probe_case): every
    probed pixel is 1.0 or 0.0 by the order of its three points alone, the rule of test_order_of_the_adds_is_the_references.
    The atomics hand out the list slots in arbitrary order, so a wrong exchange of the sort misplaces entries broadly."""
    case, expect = dc.order_probe_case(L, layout)
    assert (len(expect) > 0) == (L >= 3)
    got, ref, _ = run(case, np.float32)
    wrong = [(pixel, float(got[pixel]), float(value)) for pixel, value in expect.items() if got[pixel].tobytes() != value.tobytes()]
    assert not wrong, (L, layout, len(wrong), wrong[:8])
    assert got.tobytes() == ref.tobytes()


# ------------------------------------------------------------------------------------------------ no cutoff: the windows
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_uncut_windows(dtype):
    case = dc.uncut_window_case()
    frames = case["base"].astype(dtype)
    ref, k = oracle.render_batch(frames, case["pts"], case["amps"], case["counts"], case["sigma"])
    offsets = np.concatenate([[0], np.cumsum(case["counts"])]).astype(np.int64)
    got = frames.copy()
    datasets._render_host(got, np.ascontiguousarray(case["pts"]), np.ascontiguousarray(case["amps"]), case["sigma"], 0.0, False, offsets=offsets)
    for b, count in enumerate(case["counts"]):                           # per frame: its own k and its own max|ref|
        close(got[b], ref[b], count, f"uncut, {count} points, {np.dtype(dtype).name}")
    assert case["counts"][0] == 0 and got[0].tobytes() == frames[0].tobytes()


def test_uncut_order_across_the_windows_exact():
    """Triples at indices 254, 255, 256, then 255, 256, 600, then 3, 130, 255 of a frame's point range
    (datasets_cases.uncut_probe_case): the probed pixel is exactly 1.0 or 0.0 by their order.  Only that pixel is compared:
    elsewhere 1e8 * exp(.) cancels against its twin."""
    case, expect = dc.uncut_probe_case()
    offsets = np.concatenate([[0], np.cumsum(case["counts"])]).astype(np.int64)
    got = np.zeros(case["shape"], np.float32)
    datasets._render_host(got, np.ascontiguousarray(case["pts"]), np.ascontiguousarray(case["amps"]), case["sigma"], 0.0, False, offsets=offsets)
    values = [got[b][dc.UNCUT_PROBE_PIXEL] for b in range(len(expect))]
    assert [v.tobytes() for v in values] == [e.tobytes() for e in expect], (values, expect)


# ------------------------------------------------------------------------------------------------ the cut without the taper
@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_cut_without_taper_reaches_r_equal_R(dtype):
    """No other test reaches ``taper = 0`` with a cutoff.  A point on a pixel centre, sigma 1, R = 3: the pixels at distance
    exactly 3 are inside (``r <= R``) and receive ``a * exp(-4.5)``; with the taper they receive exactly +0.0; the next pixels
    along the box edge (distance sqrt(10)) receive nothing either way."""
    case = dc.cut_edge_case()
    (x, y), a = case["pts"][0].astype(int), float(case["amps"][0])
    rim = [(y, x + 3), (y, x - 3), (y + 3, x), (y - 3, x)]
    outside = [(y + 1, x + 3), (y - 1, x - 3), (y + 3, x + 1), (y - 3, x - 1), (y + 3, x + 3)]
    got, ref, k = run(case, dtype, taper=False)
    close(got, ref, k, f"cut, no taper, {np.dtype(dtype).name}")
    for pixel in rim:
        assert abs(float(got[pixel]) - a * np.exp(-4.5)) <= oracle.tolerance(ref, 1) and got[pixel] > 0, pixel
    assert all(got[pixel].tobytes() == dtype(0.0).tobytes() for pixel in outside)
    assert np.count_nonzero(got) == np.count_nonzero(ref) == 29          # the lattice points with dx^2 + dy^2 <= 9
    tapered, ref_t, k = run(case, dtype, taper=True)
    close(tapered, ref_t, k, f"cut, taper, {np.dtype(dtype).name}")
    assert all(tapered[pixel].tobytes() == dtype(0.0).tobytes() for pixel in rim + outside)
    assert np.count_nonzero(tapered) == 25


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_cut_without_taper_on_the_tile_grid(dtype):
    """The same instantiation on the 3 x 5 tile frame of case ``tiles`` (points on the borders, outside, duplicated)."""
    got, ref, k = run(dc.render_cases()["tiles"], dtype, taper=False)
    close(got, ref, k, f"tiles, no taper, {np.dtype(dtype).name}")
