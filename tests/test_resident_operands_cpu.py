"""What the resident entry points (``mtflearn_amd.resident``, re-exported by ``mtflearn_amd.distributed``) ask of their operands,
checked without a GPU and without the built library: the adapter's dtype table, every refusal each ``*_device`` function makes
before its first device call, and the names ``distributed`` keeps exporting.

A resident operand is faked as a ``DeviceArray`` VIEW at an arbitrary address (a view allocates nothing and frees nothing); CPU
torch tensors serve for "must live on the GPU".  Every call here must raise before anything dereferences the address.
"""
import re
import types

import numpy as np
import pytest
import torch

from mtflearn_amd import _native, distributed as D

ROWS = [(np.float32, 0), (np.float64, 1), (np.uint8, 2), (np.uint16, 3), (np.int16, 4), (np.int32, 5), (np.int64, None)]
FLOAT_NAMES, IMAGE_NAMES = ("float32", "float64"), ("float32", "float64", "uint8", "uint16", "int16")
FLOATS_MESSAGE, IMAGES_MESSAGE = "float32 or float64", "float32, float64, uint8, uint16 or int16"

MOVED = {"patch_moments_device", "frame_moments_device", "frame_maps_device", "normalize_image_device",
         "standardize_image_device", "percentile_clip_device", "local_max_device", "points_moments_device",
         "remove_background_device", "render_gaussians_device", "honeycomb_image_device", "denoise_svd_device",
         "denoise_svd_memory_view_device", "find_regions_device", "voronoi_neighbours_device", "vnn_graph_device",
         "refine_points_device", "com_refine_device", "estimate_d_device", "inverse_transform_device"}
KEPT = {"shard_bounds", "one_gpu_rank_env", "rccl_debug_env", "rccl_transport_summary", "describe_transport", "RcclComm",
        "TorchComm", "DeviceCompute", "sharded_patch_moments", "sharded_frame_moments", "sharded_frame_maps",
        "sharded_frames_moments"}
# the parent's distributed.__all__, entry for entry
PARENT_ALL = (MOVED - {"render_gaussians_device", "honeycomb_image_device"}) | (KEPT - {"rccl_debug_env", "rccl_transport_summary",
                                                                                      "describe_transport"})


def fake(shape, dtype=np.float32, device=0):
    """A resident array that owns nothing: a DeviceArray view."""
    return _native.DeviceArray(shape, dtype, device, _base=object(), _ptr=4096)


def torch_like_on_gpu(shape, dtype):
    """What the kind check reads of a CUDA torch tensor (there is none without a GPU): not a DeviceArray, and on device 0."""
    return types.SimpleNamespace(is_cuda=True, shape=shape, dtype=dtype, device=types.SimpleNamespace(index=0),
                                 is_contiguous=lambda: True)


class Plan:
    device, n_poly = 0, 3


@pytest.fixture(scope="module")
def library_untouched():
    """Yields; afterwards the library must still be unloaded -- meaningful only when it was at the start."""
    was_unloaded = _native._lib is None
    yield
    if was_unloaded:
        assert _native._lib is None, "a refusal came after _native.load()"


# ---------------------------------------------------------------------------------------------------- the dtype table
@pytest.mark.parametrize("dtype,code", ROWS, ids=[np.dtype(d).name for d, _ in ROWS])
def test_every_row_of_the_table_for_both_kinds(dtype, code):
    from mtflearn_amd import _device
    name = np.dtype(dtype).name
    tdtype = getattr(torch, name)
    for array in (fake((3, 2), dtype), torch.zeros((3, 2), dtype=tdtype)):
        assert _device.np_dtype(array) == np.dtype(dtype) and _device.np_dtype(array) is not None
        if code is not None:
            assert _device.code(array, (name,)) == code
        for allowed, message in ((_device.FLOATS, FLOATS_MESSAGE), (_device.IMAGES, IMAGES_MESSAGE)):
            if name in allowed:
                assert _device.code(array, allowed) == code
            else:
                with pytest.raises(TypeError, match=f"{message}, not .*{name}"):
                    _device.code(array, allowed)
    out = _device.empty((2, 3), dtype, torch.zeros(1))                     # the torch branch, on the CPU
    assert out.dtype == tdtype and tuple(out.shape) == (2, 3) and out.device.type == "cpu"
    # the DeviceArray branch hands empty()'s dtype to DeviceArray as it is: the mapping is the view's own
    assert fake((2, 3), dtype).dtype == np.dtype(dtype) and fake((2, 3), dtype).element_size() == np.dtype(dtype).itemsize


def test_the_two_allowed_sets():
    from mtflearn_amd import _device
    assert tuple(_device.FLOATS) == FLOAT_NAMES and tuple(_device.IMAGES) == IMAGE_NAMES
    assert _device.code(torch.zeros(1), _device.FLOATS) == _native.ZK_F32 == D._dtype_code(torch.zeros(1))
    assert _device.code(torch.zeros(1, dtype=torch.float64)) == _native.ZK_F64


@pytest.mark.parametrize("array", [torch.zeros(2, dtype=torch.float16), torch.zeros(2, dtype=torch.bfloat16),
                                   torch.zeros(2, dtype=torch.bool), torch.zeros(2, dtype=torch.complex64), fake((2,), np.int8)],
                         ids=["float16", "bfloat16", "bool", "complex64", "native-int8"])
def test_types_outside_the_table_are_never_read_as_float64(array):
    from mtflearn_amd import _device
    assert _device.np_dtype(array) is None
    with pytest.raises(TypeError, match=FLOATS_MESSAGE):
        _device.code(array, _device.FLOATS)
    with pytest.raises(TypeError, match=IMAGES_MESSAGE):
        _device.code(array)
    with pytest.raises(TypeError, match=FLOATS_MESSAGE):
        D._dtype_code(array)
    with pytest.raises(TypeError, match="int32"):
        _device.points_code(array)


def test_host_copies_and_streams_of_the_adapter():
    from mtflearn_amd import _device
    assert _device.is_native(fake((1,))) and not _device.is_native(torch.zeros(1))
    assert _device.stream_ptr(fake((1,))) == 0 and _device.stream_ptr(torch.zeros(1)) == 0
    back = _device.to_host(_device.from_host(np.arange(6, dtype=np.int16).reshape(2, 3)[:, ::2], torch.zeros(1)))
    assert back.dtype == np.float64 and np.array_equal(back, [[0, 2], [3, 5]])


# ---------------------------------------------------------------------------------------------------- one bad operand per check
GPU = "must live on the GPU"
F32_FRAME, I32_POINTS = fake((48, 48)), fake((14, 2), np.int32)
CPU_FRAME, CPU_POINTS = torch.zeros((48, 48)), torch.zeros((14, 2), dtype=torch.int32)
CUBE = fake((4, 48, 48))

REFUSALS = {
    # the plan-bound entry points
    "patches-cpu": (lambda: D.patch_moments_device(Plan(), torch.zeros((2, 8, 8))), ValueError, "patches " + GPU),
    "patches-int16": (lambda: D.patch_moments_device(Plan(), fake((2, 8, 8), np.int16)), TypeError, FLOATS_MESSAGE + ".*int16"),
    "patches-device": (lambda: D.patch_moments_device(Plan(), fake((2, 8, 8), device=1)), ValueError, "plan was created on device 0"),
    "patches-out-device": (lambda: D.patch_moments_device(Plan(), fake((2, 8, 8)), out=fake((2, 3), np.float64, 1)), ValueError,
                           "out is on cuda:1"),
    "frame-cpu": (lambda: D.frame_moments_device(Plan(), CPU_FRAME), ValueError, "image " + GPU),
    "frame-uint8": (lambda: D.frame_moments_device(Plan(), fake((48, 48), np.uint8)), TypeError, FLOATS_MESSAGE + ".*uint8"),
    "maps-cpu": (lambda: D.frame_maps_device(Plan(), CPU_FRAME, 4), ValueError, "image " + GPU),
    "maps-int32": (lambda: D.frame_maps_device(Plan(), fake((48, 48), np.int32), 4), TypeError, FLOATS_MESSAGE + ".*int32"),
    "moments-cpu-frame": (lambda: D.points_moments_device(Plan(), CPU_FRAME, I32_POINTS), ValueError, "image " + GPU),
    "moments-cpu-points": (lambda: D.points_moments_device(Plan(), F32_FRAME, CPU_POINTS), ValueError, "points " + GPU),
    "moments-int16-frame": (lambda: D.points_moments_device(Plan(), fake((48, 48), np.int16), I32_POINTS), TypeError, FLOATS_MESSAGE),
    "moments-f64-points": (lambda: D.points_moments_device(Plan(), F32_FRAME, fake((14, 2), np.float64)), TypeError,
                           r"points must be an \(N, 2\) int32 array"),
    "moments-f32-points": (lambda: D.points_moments_device(Plan(), F32_FRAME, fake((14, 2), np.float32)), TypeError,   # four bytes wide too
                           r"points must be an \(N, 2\) int32 array"),
    "moments-points-shape": (lambda: D.points_moments_device(Plan(), F32_FRAME, fake((14, 3), np.int32)), TypeError,
                             r"points must be an \(N, 2\) int32 array"),
    "moments-points-device": (lambda: D.points_moments_device(Plan(), F32_FRAME, fake((14, 2), np.int32, 1)), ValueError,
                              "points is on cuda:1"),
    # images of the five formats
    "local-max-rank": (lambda: D.local_max_device(CUBE, 3), ValueError, "local_max_device needs a 2D image, not 3-D"),
    "local-max-cpu": (lambda: D.local_max_device(CPU_FRAME, 3), ValueError, "image " + GPU),
    "local-max-int32": (lambda: D.local_max_device(fake((48, 48), np.int32), 3), TypeError, IMAGES_MESSAGE + ".*int32"),
    "background-rank": (lambda: D.remove_background_device(CUBE, "opening", 3), ValueError, "2D"),
    "background-cpu": (lambda: D.remove_background_device(CPU_FRAME, "opening", 3), ValueError, "image " + GPU),
    "background-int64": (lambda: D.remove_background_device(fake((48, 48), np.int64), "opening", 3), TypeError, IMAGES_MESSAGE + ".*int64"),
    "background-method": (lambda: D.remove_background_device(F32_FRAME, "tophat", 3), ValueError, "method must be one of"),
    "normalize-cpu": (lambda: D.normalize_image_device(CPU_FRAME), ValueError, "image " + GPU),
    "normalize-int32": (lambda: D.normalize_image_device(fake((8, 8, 3), np.int32)), TypeError, "device images must be.*" + IMAGES_MESSAGE),
    "normalize-mode": (lambda: D.normalize_image_device(F32_FRAME, mode="max"), ValueError, "mode must be"),
    "normalize-size": (lambda: D.normalize_image_device(fake((2 ** 16, 2 ** 15))), ValueError, r"between 1 and 2\*\*31 - 1 elements"),
    "standardize-cpu": (lambda: D.standardize_image_device(CPU_FRAME), ValueError, "image " + GPU),
    "standardize-int8": (lambda: D.standardize_image_device(fake((8, 8), np.int8)), TypeError, IMAGES_MESSAGE + ".*int8"),
    "clip-cpu": (lambda: D.percentile_clip_device(CPU_FRAME), ValueError, "image " + GPU),
    "clip-int32": (lambda: D.percentile_clip_device(fake((8, 8), np.int32)), TypeError, IMAGES_MESSAGE),
    "clip-method": (lambda: D.percentile_clip_device(F32_FRAME, method="sigma"), ValueError, "method must be"),
    "clip-percentile": (lambda: D.percentile_clip_device(F32_FRAME, high=101.0), ValueError, "Percentiles must be in the range"),
    "svd-rank": (lambda: D.denoise_svd_device(CUBE, 4, 1), ValueError, "denoise_svd_device needs a 2D image"),
    "svd-cpu": (lambda: D.denoise_svd_device(CPU_FRAME, 4, 1), ValueError, "image " + GPU),
    "svd-int32": (lambda: D.denoise_svd_device(fake((48, 48), np.int32), 4, 1), TypeError, IMAGES_MESSAGE),
    "svd-patch": (lambda: D.denoise_svd_device(F32_FRAME, 48, 1), ValueError, "strictly smaller"),
    "svd-components": (lambda: D.denoise_svd_device(F32_FRAME, 4, 0), ValueError, "n_components"),
    "memory-view-rank": (lambda: D.denoise_svd_memory_view_device(CUBE, 4), ValueError, "denoise_svd_memory_view_device needs a 2D image"),
    "memory-view-cpu": (lambda: D.denoise_svd_memory_view_device(CPU_FRAME, 4), ValueError, "image " + GPU),
    "memory-view-int32": (lambda: D.denoise_svd_memory_view_device(fake((48, 48), np.int32), 4), TypeError, IMAGES_MESSAGE),
    "memory-view-patch": (lambda: D.denoise_svd_memory_view_device(fake((64, 64)), 49), ValueError, "at most 48"),
    # the rasteriser
    "render-rank": (lambda: D.render_gaussians_device(CUBE, [[1.0, 1.0]], 1.0), ValueError, "img must be a 2D array"),
    "render-cpu": (lambda: D.render_gaussians_device(CPU_FRAME, [[1.0, 1.0]], 1.0), ValueError, "image " + GPU),
    "render-int16": (lambda: D.render_gaussians_device(fake((48, 48), np.int16), [[1.0, 1.0]], 1.0), TypeError, FLOATS_MESSAGE + ".*int16"),
    "honeycomb-keyword": (lambda: D.honeycomb_image_device(None, gamma=2), TypeError, "unexpected keyword argument 'gamma'"),
    # the refine pair
    "refine-rank": (lambda: D.refine_points_device(CUBE, I32_POINTS), ValueError, "refine_points_device needs a 2D image, not 3-D"),
    "refine-cpu-frame": (lambda: D.refine_points_device(CPU_FRAME, I32_POINTS), ValueError, GPU),
    "refine-cpu-points": (lambda: D.refine_points_device(F32_FRAME, CPU_POINTS), ValueError, GPU),
    "refine-kinds": (lambda: D.refine_points_device(F32_FRAME, torch_like_on_gpu((14, 2), torch.int32)), ValueError, "of one kind"),
    "refine-devices": (lambda: D.refine_points_device(F32_FRAME, fake((14, 2), np.int32, 1)), ValueError, "on one device"),
    "refine-int16-frame": (lambda: D.refine_points_device(fake((48, 48), np.int16), I32_POINTS), ValueError,
                           "refine_points_device needs a float frame.*int16"),
    "refine-f64-points": (lambda: D.refine_points_device(F32_FRAME, fake((14, 2), np.float64)), TypeError, r"\(N, 2\) int32 array"),
    "refine-points-shape": (lambda: D.refine_points_device(F32_FRAME, fake((14, 3), np.int32)), TypeError, r"\(N, 2\) int32 array"),
    "refine-size": (lambda: D.refine_points_device(F32_FRAME, I32_POINTS, size=65), ValueError, r"size must be in \[0, 64\], not 65"),
    "refine-count": (lambda: D.refine_points_device(F32_FRAME, fake((2 ** 24, 2), np.int32)), ValueError, r"refine_points_device needs len\(points\) < 2\^24"),
    "com-rank": (lambda: D.com_refine_device(CUBE, I32_POINTS, 5), ValueError, "com_refine_device needs a 2D image, not 3-D"),
    "com-cpu-frame": (lambda: D.com_refine_device(CPU_FRAME, I32_POINTS, 5), ValueError, GPU),
    "com-cpu-points": (lambda: D.com_refine_device(F32_FRAME, CPU_POINTS, 5), ValueError, GPU),
    "com-kinds": (lambda: D.com_refine_device(F32_FRAME, torch_like_on_gpu((14, 2), torch.float64), 5), ValueError, "of one kind"),
    "com-devices": (lambda: D.com_refine_device(F32_FRAME, fake((14, 2), np.float64, 1), 5), ValueError, "on one device"),
    "com-uint8-frame": (lambda: D.com_refine_device(fake((48, 48), np.uint8), I32_POINTS, 5), ValueError,
                        "com_refine_device needs a float frame.*uint8"),
    "com-f32-points": (lambda: D.com_refine_device(F32_FRAME, fake((14, 2), np.float32), 5), TypeError, r"\(N, 2\) int32 or float64 array"),
    "com-points-shape": (lambda: D.com_refine_device(F32_FRAME, fake((14,), np.float64), 5), TypeError, r"\(N, 2\) int32 or float64 array"),
    "com-size-small": (lambda: D.com_refine_device(F32_FRAME, I32_POINTS, 1), ValueError, r"size must be an integer in \[2, 64\], not 1"),
    "com-size-fraction": (lambda: D.com_refine_device(F32_FRAME, I32_POINTS, 2.5), ValueError, r"size must be an integer in \[2, 64\]"),
    "com-size-large": (lambda: D.com_refine_device(F32_FRAME, fake((14, 2), np.float64), 65), ValueError, r"size must be an integer in \[2, 64\]"),
    "com-count": (lambda: D.com_refine_device(F32_FRAME, fake((2 ** 24, 2), np.float64), 5), ValueError, r"com_refine_device needs len\(points\) < 2\^24"),
    # points for the Voronoi and kNN kernels
    "voronoi-shape": (lambda: D.voronoi_neighbours_device(fake((14, 3), np.float64)), ValueError, r"points must have shape \(N, 2\), not \(14, 3\)"),
    "voronoi-cpu": (lambda: D.voronoi_neighbours_device(CPU_POINTS), ValueError, "points " + GPU),
    "voronoi-f32": (lambda: D.voronoi_neighbours_device(fake((14, 2), np.float32)), TypeError, "float64 or int32 DeviceArray, not float32"),
    "voronoi-count": (lambda: D.voronoi_neighbours_device(fake((2 ** 26 - 4, 2), np.int32)), ValueError,
                      r"voronoi_neighbours_device needs len\(points\) < 2\^26 - 4"),
    "voronoi-pad": (lambda: D.voronoi_neighbours_device(I32_POINTS, pad=0), ValueError, "pad must be positive"),
    "vnn-dmax": (lambda: D.vnn_graph_device(I32_POINTS, dmax=0.0), ValueError, "dmax must be positive"),
    "vnn-dmax-nan": (lambda: D.vnn_graph_device(I32_POINTS, dmax=float("nan")), ValueError, "dmax must be positive"),
    "vnn-threshold": (lambda: D.vnn_graph_device(I32_POINTS, dmax=1.3, threshold=0.0), ValueError, "threshold must be > 0"),
    "vnn-count": (lambda: D.vnn_graph_device(fake((2 ** 26 - 4, 2), np.float64), dmax=1.3), ValueError, r"vnn_graph_device needs len\(points\) < 2\^26 - 4"),
    "vnn-few-points": (lambda: D.vnn_graph_device(fake((11, 2), np.float64)), ValueError, "n_neighbors = 12, n_samples_fit = 11"),
    "estimate-shape": (lambda: D.estimate_d_device(fake((14,), np.float64)), ValueError, r"points must have shape \(N, 2\)"),
    "estimate-cpu": (lambda: D.estimate_d_device(CPU_POINTS), ValueError, "points " + GPU),
    "estimate-int64": (lambda: D.estimate_d_device(fake((14, 2), np.int64)), TypeError, "float64 or int32 DeviceArray, not int64"),
    "estimate-few-points": (lambda: D.estimate_d_device(fake((11, 2), np.int32)), ValueError, "n_neighbors = 12, n_samples_fit = 11"),
    "estimate-count": (lambda: D.estimate_d_device(fake((2 ** 26, 2), np.float64)), ValueError, r"estimate_d_device needs len\(points\) < 2\^26$"),
    # polygons
    "regions-points-shape": (lambda: D.find_regions_device(fake((5, 3), np.float64), fake((4, 2), np.int64)), ValueError,
                             r"points must have shape \(N, 2\), not \(5, 3\)"),
    "regions-edges-shape": (lambda: D.find_regions_device(fake((5, 2), np.float64), fake((4,), np.int64)), ValueError,
                            r"edges must have shape \(E, 2\), not \(4,\)"),
    "regions-float-edges": (lambda: D.find_regions_device(fake((5, 2), np.float64), torch.zeros((4, 2))), ValueError,
                            "edges must be of an integer type, not torch.float32"),
    "regions-bool-edges": (lambda: D.find_regions_device(fake((5, 2), np.float64), torch.zeros((4, 2), dtype=torch.bool)), ValueError,
                           "edges must be of an integer type"),
    "regions-cpu-points": (lambda: D.find_regions_device(torch.zeros((5, 2)), fake((4, 2), np.int64)), ValueError, "points " + GPU),
    "regions-cpu-edges": (lambda: D.find_regions_device(fake((5, 2), np.float64), torch.zeros((4, 2), dtype=torch.int64)), ValueError, "edges " + GPU),
    "regions-f32-points": (lambda: D.find_regions_device(fake((5, 2), np.float32), fake((4, 2), np.int64)), TypeError,
                           "points must be a float64 DeviceArray, not float32"),
    "regions-i32-edges": (lambda: D.find_regions_device(fake((5, 2), np.float64), fake((4, 2), np.int32)), TypeError,
                          "edges must be a int64 DeviceArray, not int32"),
    "regions-devices": (lambda: D.find_regions_device(fake((5, 2), np.float64), fake((4, 2), np.int64, 1)), ValueError, "same device"),
    "regions-count": (lambda: D.find_regions_device(fake((2 ** 30, 2), np.float64), fake((2 ** 30 - 4, 2), np.int64)), ValueError, r"\+ 4 < 2\^31"),
    "regions-no-points": (lambda: D.find_regions_device(fake((0, 2), np.float64), fake((1, 2), np.int64)), ValueError, "edges without points"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_every_check_refuses_its_operand_before_the_library_is_loaded(case, library_untouched):
    call, exception, message = REFUSALS[case]
    with pytest.raises(exception, match=message):
        call()


@pytest.fixture(scope="module")
def zps():
    from mtflearn_amd import ZPs
    return ZPs(n_max=4, size=9)


def test_inverse_transform_device_refusals(zps, library_untouched):
    p = len(zps.n)
    good = fake((3, p), np.float64)
    inverse = lambda *a, **k: D.inverse_transform_device(zps, *a, **k)
    for bad in (torch.zeros((3, p), dtype=torch.float64), np.zeros((3, p))):
        with pytest.raises(ValueError, match="coeffs_dev must live on the GPU"):
            inverse(bad)
    for bad in (fake((3, p - 1), np.float64), fake((p,), np.float64), fake((3, p), np.float32), fake((3, p), np.int64)):
        with pytest.raises(ValueError, match=rf"coeffs_dev must be an \(N, {p}\) float64 matrix of real Zernike moments"):
            inverse(bad)
    for n_rows in (-1, 4):
        with pytest.raises(ValueError, match="n_rows must be between 0 and 3"):
            inverse(good, n_rows=n_rows)
    with pytest.raises(ValueError, match="dtype must be float64 or float32, not float16"):
        inverse(good, dtype=np.float16)
    with pytest.raises(ValueError, match="method must be 'lstsq' or 'direct'"):
        inverse(good, method="pinv")
    for out in (fake((2, 9, 9), np.float64), fake((3, 9, 9), np.float32), fake((3, 9, 9), np.float64, 1), fake((3, 9, 9), np.int64)):
        with pytest.raises(ValueError, match=r"out must be a contiguous \(3, 9, 9\) array of float64"):
            inverse(good, out=out)
    with pytest.raises(ValueError, match=r"out must be a contiguous \(3, 9, 9\) array of float32"):
        inverse(good, dtype=np.float32, out=fake((3, 9, 9), np.float64))
    with pytest.raises(ValueError, match="coeffs_dev is on cuda:1 but this ZPs computes on device 0"):
        D.inverse_transform_device(zps.to_device(0), fake((3, p), np.float64, 1))


def test_an_out_of_a_type_outside_the_table_is_a_value_error_not_a_key_error(zps, library_untouched):
    """float16 is in no row of the table: ``out`` is refused with the message written for it (it used to die in the lookup)."""
    for dtype in (torch.float16, torch.bfloat16, torch.complex64):
        with pytest.raises(ValueError, match=r"out must be a contiguous \(3, 9, 9\) array of float64"):
            D.inverse_transform_device(zps, fake((3, len(zps.n)), np.float64), out=torch.zeros((3, 9, 9), dtype=dtype))


# ---------------------------------------------------------------------------------------------------- the compatibility surface
def test_distributed_keeps_every_name_and_they_are_the_resident_functions():
    from mtflearn_amd import resident
    assert MOVED == set(resident.__all__) and len(resident.__all__) == len(MOVED)
    assert PARENT_ALL <= set(D.__all__) == MOVED | (KEPT & set(D.__all__)) and len(set(D.__all__)) == len(D.__all__)
    for name in MOVED:
        assert getattr(D, name) is getattr(resident, name), name
    for name in KEPT:
        assert callable(getattr(D, name)) and getattr(D, name).__module__ == "mtflearn_amd.distributed", name
    namespace = {}
    exec("from mtflearn_amd.distributed import *", namespace)
    assert MOVED | PARENT_ALL <= set(namespace)


def test_distributed_keeps_the_private_names_others_read():
    assert D._chunk_bounds(10, 3) == [(0, 3), (3, 6), (6, 10)]
    assert D._current_stream_ptr(torch.zeros(1)) == 0 and D._current_stream_ptr(fake((1,))) == 0
    assert D._dtype_code(fake((1,), np.float64)) == _native.ZK_F64
    with pytest.raises(TypeError, match=re.escape("float32 or float64")):
        D._dtype_code(fake((1,), np.uint8))
