"""mtflearn_amd.features.refine_points / KeyPoints.refine_gpu / distributed.refine_points_device on the GPU against the goldens
the host ``center_of_mass_refine`` made (tests/make_golden_refine.py) on every case of tests/refine_cases.py.

Criterion: ``(x, y)`` equal bit for bit, NaN exactly where the golden has NaN (a NaN's sign and payload are not pinned).  The
GPU tests read only the goldens: neither SciPy nor scikit-learn is needed here."""
import os

import numpy as np
import pytest

import refine_cases as rc
from conftest import ROOT
from mtflearn_amd import _native, distributed, features, graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "refine_golden.npz")) as f:
        return {k: f[k] for k in f.files}


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


def to_host(a):
    return a.numpy() if isinstance(a, _native.DeviceArray) else a.cpu().numpy()


def resident(a, kind):
    if kind == "native":
        return _native.DeviceArray.from_numpy(a)
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


@pytest.mark.parametrize("name", rc.REFINE_NAMES)
def test_refine_points_is_bit_equal_to_the_host_route(golden, name):
    data, pts, size, mode = rc.refine_cases()[name]
    got = features.refine_points(data, pts, size=size, mode=mode)
    assert same_bits(got, golden[f"{name}/xy"]), name
    assert features.refine_points(data, pts.astype(np.int64), size=size, mode=mode).tobytes() == got.tobytes()


@pytest.mark.parametrize("kind", ("native", "torch"))
@pytest.mark.parametrize("name", ("overlap_one_column_ab_box", "swallowed_by_four_later_disk", "disk_corner_removes_earlier_pixel",
                                  "zero_sums_box", "every_edge_size6_disk", "n65_box", "n3000_disk", "n3000_size6_box"))
def test_refine_points_device_is_bit_equal_to_the_host_route(golden, name, kind):
    data, pts, size, mode = rc.refine_cases()[name]
    out = distributed.refine_points_device(resident(data, kind), resident(pts, kind), size=size, mode=mode)
    assert isinstance(out, _native.DeviceArray) if kind == "native" else out.is_cuda
    assert same_bits(to_host(out), golden[f"{name}/xy"]), name


def test_key_points_of_the_512_frame_and_refine_gpu(golden):
    frame, pts = rc.frame_512(), golden["keypoints_512/pts"]
    for mode in rc.MODES:
        want = golden[f"keypoints_512_{'disk' if mode else 'box'}/xy"]
        assert same_bits(features.refine_points(frame, pts, size=3, mode=mode), want)
        kp = features.KeyPoints(pts.astype(np.float64) + 0.75, frame, 7)          # refine truncates: the same integer points
        assert len(kp.pts) == len(pts)
        kp.refine_gpu(r=3, mode=mode)
        assert same_bits(kp.pts, want)


def test_each_precondition_raises_and_the_next_call_succeeds(golden):
    import torch
    data, pts, size, mode = rc.refine_cases()["isolated_box"]
    height, width = data.shape
    for bad in ([[2, 40]], [[width - 3, 40]], [[30, 2]], [[30, height - 3]], [[-5, 40]], [[30, 10 ** 6]]):
        both = np.concatenate([pts, np.array(bad, np.int32)])
        with pytest.raises(ValueError, match="inside the frame"):
            features.refine_points(data, both, size=3)
        for kind in ("native", "torch"):                                          # checked on the device: nothing is written out of bounds
            with pytest.raises(ValueError, match="leaves the frame"):
                distributed.refine_points_device(resident(data, kind), resident(both, kind), size=3)
    with pytest.raises(ValueError, match="float"):
        features.refine_points((data * 100).astype(np.int32), pts, size=3)
    with pytest.raises(ValueError, match="float"):
        distributed.refine_points_device(torch.zeros(32, 32, dtype=torch.int16).cuda(), resident(pts[:1], "torch"), size=3)
    with pytest.raises(TypeError, match="int32"):
        distributed.refine_points_device(resident(data, "torch"), resident(pts.astype(np.float64), "torch"), size=3)
    with pytest.raises(ValueError, match="2\\^24"):
        distributed.refine_points_device(resident(data, "torch"), torch.zeros((2 ** 24, 2), dtype=torch.int32).cuda(), size=3)
    with pytest.raises(ValueError, match="size"):
        features.refine_points(data, pts, size=65)
    assert same_bits(features.refine_points(data, pts, size=size, mode=mode), golden["isolated_box/xy"])
    assert same_bits(to_host(distributed.refine_points_device(resident(data, "torch"), resident(pts, "torch"), size=size)), golden["isolated_box/xy"])


def test_resident_chain_local_max_refine_estimate_bonds_regions():
    """local_max_device -> refine_points_device -> vnn_graph_device(dmax=None) -> find_regions_device: frame and points stay on
    the device; the refined points equal the host route on the same key points and feed the bonds."""
    import torch
    from mtflearn_amd.features.keypoints import clear_border
    from mtflearn_amd.synthetic import honeycomb_frame
    frame = honeycomb_frame(160, 192, seed=3).astype(np.float32)
    d_frame = torch.from_numpy(frame).cuda()
    d_all = distributed.local_max_device(d_frame, min_distance=3, threshold=float(frame.mean()))
    keep = clear_border(d_all.cpu().numpy(), frame.shape, 7)                       # the border clearing KeyPoints does
    d_pts = torch.from_numpy(np.ascontiguousarray(keep)).cuda()
    assert d_pts.dtype == torch.int32 and len(keep) > 60
    d_xy = distributed.refine_points_device(d_frame, d_pts, size=3)
    assert d_xy.is_cuda and d_xy.dtype == torch.float64 and tuple(d_xy.shape) == (len(keep), 2)
    host = features.refine_points(frame, keep, size=3)
    assert same_bits(d_xy.cpu().numpy(), host) and np.abs(host - keep).max() < 3
    d_ijs = distributed.vnn_graph_device(d_xy, threshold_method="otsu")
    ijs = graph.vnn_graph(host, threshold_method="otsu")
    assert np.array_equal(d_ijs.cpu().numpy(), ijs) and len(ijs) > len(keep)
    got = [a.cpu().numpy() for a in distributed.find_regions_device(d_xy, d_ijs)]
    want = graph._regions_arrays(*graph._check_graph(host, ijs))
    assert (want[2] == 6).sum() > 0 and all(np.array_equal(g, w) for g, w in zip(got, want))
    # the native arrays take the same road
    n_xy = distributed.refine_points_device(_native.DeviceArray.from_numpy(frame), _native.DeviceArray.from_numpy(keep), size=3)
    assert isinstance(n_xy, _native.DeviceArray) and same_bits(n_xy.numpy(), host)
    assert np.array_equal(distributed.vnn_graph_device(n_xy, threshold_method="otsu").numpy(), ijs)
