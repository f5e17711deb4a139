"""mtflearn_amd.datasets on the GPU: the rasteriser against goldens captured from the reference (tests/make_golden_datasets.py)
and against the NumPy statement of the gather (tests/datasets_oracle.py), at the shapes where it can go wrong (one pixel, one
row, one column, off the tile grid, lists past the LDS staging, point ranges cut by the budget), the order of the adds exactly,
and the key-point chain against the known sites of a rendered lattice.

Criteria (datasets_oracle.tolerance): float64 frames ``1e-12 * max|ref|``; float32 frames ``k`` float32 spacings at
``max|ref|``, ``k`` the most contributions on one pixel of that case, from the oracle."""
import os

import numpy as np
import pytest

import datasets_cases as dc
import datasets_oracle as oracle
from conftest import ROOT
from mtflearn_amd import _native, datasets, distributed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "datasets_golden.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def cases():
    return dc.render_cases()


@pytest.fixture(scope="module")
def oracles(cases):
    """(result, k) of the NumPy gather per case and dtype, computed once."""
    return {(name, dtype): oracle.render(dc.case_frame(case, dtype), case["pts"], case["amps"], case["sigma"], case["r_factor"])
            for name, case in cases.items() for dtype in dc.DTYPES}


def close(got, ref, k, what=""):
    assert got.dtype == ref.dtype and got.shape == ref.shape, what
    err, tol = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()) if ref.size else 0.0, oracle.tolerance(ref, k)
    print(f"{what}: max|delta| {err:.3e}, bound {tol:.3e} (k = {k})")
    assert err <= tol, (what, err, tol)


def run(case, dtype, **kw):
    img = dc.case_frame(case, dtype)
    out = datasets.add_tapered_gaussian(img, case["pts"], case["sigma"], case["amps"], case["r_factor"], **kw)
    assert out is img
    return out


# ------------------------------------------------------------------------------------------------ goldens and oracle
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("name", sorted(dc.render_cases()))
def test_render_equals_reference_and_oracle(golden, cases, oracles, name, dtype):
    ref, k = oracles[name, dtype]
    got = run(cases[name], dtype)
    close(got, golden[f"render/{name}/{np.dtype(dtype).name}"], k, f"{name} golden")
    close(got, ref, k, f"{name} oracle")


def test_no_points_and_points_out_of_reach_change_nothing():
    base = dc._frame((37, 53), 5).astype(np.float32)
    img = base.copy()
    datasets.add_tapered_gaussian(img, np.empty((0, 2)), 1.0)
    datasets.add_tapered_gaussian(img, [[500.0, 3.0], [-40.0, -40.0], [10.0, 37.0 + 3.5]], 1.0)
    np.testing.assert_array_equal(img, base)


@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("budget", [1, 7, 200])
def test_point_ranges_cut_by_the_budget_change_nothing(cases, oracles, dtype, budget):
    """The budget is an argument: 1 renders point after point, 7 and 200 cut the 80 points (about 4 list entries each) into
    uneven ranges."""
    np.testing.assert_array_equal(run(cases["tiles"], dtype, list_budget=budget), run(cases["tiles"], dtype))
    close(run(cases["tiles"], dtype, list_budget=budget), *oracles["tiles", dtype], f"budget {budget}")


@pytest.mark.parametrize("name", sorted(dc.ORDER_AMPLITUDES))
def test_order_of_the_adds_is_the_references(golden, name):
    """Three points on the centre of pixel (6, 5) with amplitudes 1e8, 1, -1e8 in two orders: there every contribution is exact
    and float32 rounding makes the sum 0 in one order and 1 in the other (tests/test_datasets_cpu.py confirms the references
    differ)."""
    case = dc.order_case(dc.ORDER_AMPLITUDES[name])
    ref, k = oracle.render(dc.case_frame(case, np.float32), case["pts"], case["amps"], case["sigma"], case["r_factor"])
    got = run(case, np.float32)
    assert got[5, 6].tobytes() == ref[5, 6].tobytes() == golden[f"order/{name}"][5, 6].tobytes()
    assert got[5, 6] == np.float32(0.0 if name == "big_one_minus" else 1.0)
    close(got, ref, k, name)


def test_order_inside_long_lists():
    """The same three amplitudes between 3000 weak points on one pixel: the list of that tile is sorted in global memory and
    walked in windows, and the three must still arrive in index order (any other order changes the float32 sum)."""
    rng = np.random.default_rng(8)
    for amplitudes, expect in (((1e8, 1.0, -1e8), 0.0), ((1e8, -1e8, 1.0), 1.0)):
        pts = np.tile([[20.0, 9.0]], (3003, 1))
        amps = np.zeros(3003)
        amps[[100, 1500, 2900]] = amplitudes
        pts[:, 0] += np.where(amps == 0, rng.integers(-2, 3, 3003), 0)      # zero-amplitude points around it: they add 0.0
        got = datasets.add_tapered_gaussian(np.zeros((24, 40), np.float32), pts, 1.0, amps)
        assert got[9, 20] == np.float32(expect)


def test_two_runs_agree_bit_for_bit(cases):
    for dtype in dc.DTYPES:
        assert run(cases["dense"], dtype).tobytes() == run(cases["dense"], dtype).tobytes()


@pytest.mark.parametrize("dtype", dc.DTYPES)
def test_resident_render_equals_the_host_function(cases, dtype):
    case = cases["tiles"]
    host = run(case, dtype)
    dev = _native.DeviceArray.from_numpy(dc.case_frame(case, dtype), _native.default_device())
    out = distributed.render_gaussians_device(dev, case["pts"], case["sigma"], case["amps"], case["r_factor"])
    assert out is dev
    assert out.numpy().tobytes() == host.tobytes()
    import torch
    t = torch.from_numpy(dc.case_frame(case, dtype)).cuda()
    assert distributed.render_gaussians_device(t, case["pts"], case["sigma"], case["amps"], case["r_factor"]) is t
    assert t.cpu().numpy().tobytes() == host.tobytes()


def test_strided_image_is_modified_in_place(cases):
    case = cases["37x53"]
    wide = np.zeros((37, 106), np.float32)
    view = wide[:, ::2]
    view[...] = dc.case_frame(case, np.float32)
    assert datasets.add_tapered_gaussian(view, case["pts"], case["sigma"], case["amps"], case["r_factor"]) is view
    np.testing.assert_array_equal(view, run(case, np.float32))
    assert not wide[:, 1::2].any()


# ------------------------------------------------------------------------------------------------ no cutoff, batched
@pytest.mark.parametrize("dtype", dc.DTYPES)
@pytest.mark.parametrize("batch", [1, 3])
def test_uncut_batches(batch, dtype):
    case = dc.uncut_batch_case(batch)
    frames = case["base"].astype(dtype)
    ref, k = oracle.render_batch(frames, case["pts"], case["amps"], case["counts"], case["sigma"])
    offsets = np.concatenate([[0], np.cumsum(case["counts"])]).astype(np.int64)
    got = frames.copy()
    datasets._render_host(got, np.ascontiguousarray(case["pts"]), np.ascontiguousarray(case["amps"]), case["sigma"], 0.0, False,
                          offsets=offsets)
    close(got, ref, k, f"uncut batch {batch}")
    if batch > 1:
        np.testing.assert_array_equal(got[1], frames[1])        # the frame without points


@pytest.mark.parametrize("name", sorted(dc.PATCHES))
def test_zps_test_patches(golden, name):
    kw = dc.PATCHES[name]
    got = datasets.get_zps_test_patches(**kw)
    k = int(kw.get("include_center", True)) + kw["n_fold"]
    close(got, golden[f"patches/{name}"], k, f"patches {name}")


@pytest.mark.parametrize("name", sorted(dc.DATA_GN))
def test_generate_data_gn(golden, name):
    kw = dc.DATA_GN[name]
    close(datasets.generate_data_gn(**kw), golden[f"data_gn/{name}"], kw["n"] + int(kw.get("include_center", True)), f"data_gn {name}")


# ------------------------------------------------------------------------------------------------ the lattice
@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_images(golden, name):
    ctor, kw = dc.LATTICES[name]
    lat = datasets.HoneyCombLattice(**ctor)
    sigma, pts, amps = lat._render_lists(kw.get("sigma"), 1.0, 0.5)
    _, k = oracle.render(np.zeros((lat.size, lat.size), np.float32), pts, amps, sigma, 3.0)
    got = lat.to_image(**kw)
    close(got, golden[f"lattice/{name}/image"], k, f"lattice {name}")
    dev = distributed.honeycomb_image_device(datasets.HoneyCombLattice(**ctor), **kw)
    assert isinstance(dev, _native.DeviceArray) and dev.numpy().tobytes() == got.tobytes()
    import torch
    t = distributed.honeycomb_image_device(datasets.HoneyCombLattice(**ctor), like=torch.empty(1, device="cuda"), **kw)
    assert t.is_cuda and t.dtype == torch.float32 and t.cpu().numpy().tobytes() == got.tobytes()


def test_zps_test_image_is_a_512_lattice():
    img = datasets.get_zps_test_image()
    assert img.dtype == np.float32 and img.shape == (512, 512) and 0.9 < img.max() < 1.6 and img.min() >= 0.0


def test_key_points_of_a_rendered_lattice_are_its_sites():
    """Ground truth, end to end on the device: HoneyCombLattice(size=192, l=12, seed=5, angle=7) (sigma = 3, no jitter) rendered
    resident, local_max_device with min_distance 5.  Every site of get_points() farther than 3 sigma + 1 = 10 px from the border
    has exactly one detected point within 1 px, and every detected point in that interior has a site within 1 px.
    tests/make_golden_datasets.py confirms the same statement for the reference's renderer with tests/local_max_oracle.py at
    these parameters (155 interior sites, none off)."""
    lat = datasets.HoneyCombLattice(**dc.TRUTH["lattice"])
    frame = distributed.honeycomb_image_device(lat)
    points = distributed.local_max_device(frame, dc.TRUTH["min_distance"]).numpy().astype(np.float64)
    sites = np.concatenate(lat.get_points())
    margin, size = 3 * (lat.l / 4.0) + 1, lat.size

    def interior(p):
        return (p[:, 0] > margin) & (p[:, 0] < size - 1 - margin) & (p[:, 1] > margin) & (p[:, 1] < size - 1 - margin)

    d = np.hypot(sites[:, None, 0] - points[None, :, 0], sites[:, None, 1] - points[None, :, 1])
    s_in, p_in = interior(sites), interior(points)
    assert s_in.sum() > 100 and p_in.sum() > 100
    assert not (((d <= 1.0).sum(axis=1) != 1) & s_in).any()
    assert not ((d.min(axis=0) > 1.0) & p_in).any()
