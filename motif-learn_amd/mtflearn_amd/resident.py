"""The single-GPU resident entry points: every ``<name>_device`` function takes operands that already live on the GPU -- torch
tensors or :class:`~mtflearn_amd._native.DeviceArray` -- and returns device arrays of the same kind, so a frame goes from
denoising to polygons without a host copy.

What "a torch tensor or a DeviceArray" means for an operand (element types, allocation, stream, the shared checks) is answered
once, in :mod:`mtflearn_amd._device`; the functions here add what is their own.  torch is used for device memory and streams
only; the arithmetic is ``libzernike_hip.so`` called on raw device pointers.  Every name here is also an attribute of
:mod:`mtflearn_amd.distributed`, where these functions lived first: ``distributed.<name>_device`` remains a valid spelling.
"""
from __future__ import annotations

import warnings
from ctypes import byref, c_int64, c_void_p

import numpy as np

from . import _device, _native
from ._device import FLOATS, is_native, stream_ptr

__all__ = ["patch_moments_device", "frame_moments_device", "frame_maps_device", "normalize_image_device",
           "standardize_image_device", "percentile_clip_device", "local_max_device", "points_moments_device",
           "remove_background_device", "render_gaussians_device", "honeycomb_image_device", "denoise_svd_device",
           "denoise_svd_memory_view_device", "find_regions_device", "voronoi_neighbours_device", "vnn_graph_device",
           "refine_points_device", "com_refine_device", "estimate_d_device", "inverse_transform_device"]


def _empty_f64(shape, like):
    return _device.empty(shape, np.float64, like)


def _check_operand(plan, tensor, what):
    if not tensor.is_cuda:
        raise ValueError(f"{what} must live on the GPU")
    if not tensor.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if tensor.device.index != plan.device:
        raise ValueError(f"{what} is on cuda:{tensor.device.index} but the plan was created on device {plan.device}: "
                         "create the plan on the tensor's device (MTFLEARN_AMD_DEVICE / ZPs.to_device)")


def patch_moments_device(plan: "_native.Plan", patches, out=None):
    """Run the batch kernel on a CUDA/HIP torch tensor ``(N, K, K)`` (float32/float64) on torch's
    current stream; returns the ``(N, n_poly)`` float64 tensor (no host copies)."""
    _check_operand(plan, patches, "patches")
    code = _device.code(patches, FLOATS)
    n = patches.shape[0]
    if out is None:
        out = _empty_f64((n, plan.n_poly), patches)
    else:
        _check_operand(plan, out, "out")
    plan.transform_patches_dev(patches.data_ptr(), code, n, out.data_ptr(), stream_ptr(patches))
    return out


def frame_moments_device(plan: "_native.Plan", image, row0=0, n_rows=None, out=None, full=None):
    """Run the dense kernel for output rows ``[row0, row0+n_rows)`` of a CUDA/HIP torch frame ``(H, W)``.
    Returns ``(n_poly, n_rows, W)`` float64 -- or, with ``full`` (an ``(n_poly, H, W)`` tensor), writes the
    band in place into it and returns ``full``."""
    _check_operand(plan, image, "image")
    code = _device.code(image, FLOATS)
    h, w = image.shape
    n_rows = h - row0 if n_rows is None else n_rows
    stream = stream_ptr(image)
    if full is not None:
        _check_operand(plan, full, "full")
        assert tuple(full.shape) == (plan.n_poly, h, w) and _device.np_dtype(full) == np.float64
        plan.transform_frame_dev(image.data_ptr(), code, h, w, row0, n_rows, full.data_ptr() + row0 * w * 8, stream,
                                 plane_stride=h * w)
        return full
    if out is None:
        out = _empty_f64((plan.n_poly, n_rows, w), image)
    else:
        _check_operand(plan, out, "out")
    plan.transform_frame_dev(image.data_ptr(), code, h, w, row0, n_rows, out.data_ptr(), stream)
    return out


def frame_maps_device(plan: "_native.Plan", image, n_complex, folds=(2, 3, 4, 6), m_unselect=(0, 1), p=2,
                      theta=None, want_abs=True, row0=0, n_rows=None, full=None):
    """Fused frame -> symmetry maps for output rows ``[row0, row0+n_rows)`` of a CUDA/HIP torch frame.
    Returns ``(rot, abs, mirror)`` float64 tensors of shapes ``(len(folds), n_rows, W)``,
    ``(n_complex, n_rows, W)``, ``(n_rows, W)`` (``None`` for outputs not requested).  With
    ``full = (rot_full, abs_full, mirror_full)`` (whole-frame tensors, entries ``None`` where not wanted) the
    band is written in place into them and ``full`` is returned."""
    _check_operand(plan, image, "image")
    code = _device.code(image, FLOATS)
    h, w = image.shape
    n_rows = h - row0 if n_rows is None else n_rows
    stream = stream_ptr(image)
    if full is not None:
        ptr = lambda t: t.data_ptr() + row0 * w * 8 if t is not None else 0
        plan.frame_maps_dev(image.data_ptr(), code, h, w, row0, n_rows, folds if full[0] is not None else None,
                            m_unselect, p, theta if full[2] is not None else None, ptr(full[0]), ptr(full[1]),
                            ptr(full[2]), stream, plane_stride=h * w)
        return full
    mk = lambda planes: _empty_f64((planes, n_rows, w), image)
    rot = mk(len(folds)) if folds is not None and len(folds) else None
    ab = mk(n_complex) if want_abs else None
    mir = _empty_f64((n_rows, w), image) if theta is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    plan.frame_maps_dev(image.data_ptr(), code, h, w, row0, n_rows, folds, m_unselect, p, theta,
                        ptr(rot), ptr(ab), ptr(mir), stream)
    return rot, ab, mir


def local_max_device(image, min_distance, threshold=None):
    """:func:`mtflearn_amd.features.local_max` of a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).  Returns the
    ``(N, 2)`` int32 ``(x, y)`` points as a device array of the same kind, in the layout :func:`points_moments_device`
    reads: the frame never crosses to the host, only the point count does.  Runs on torch's current stream."""
    from .features.peaks import _check_distance, _comparison_threshold
    image, code = _device.resident_frame(image, "local_max_device")
    r = _check_distance(min_distance)
    has_t, t = (0, 0.0) if threshold is None else (1, _comparison_threshold(_device.np_dtype(image), threshold))
    h, w = (int(v) for v in image.shape)
    lib = _native.load()
    stream = c_void_p(stream_ptr(image))
    capacity = max(1024, h * w // 8)                   # kept points of a real frame: a few % of its pixels
    out = _device.empty((capacity, 2), np.int32, image)
    n = c_int64()
    for _ in range(2):                                  # the second pass only when the first guess was short
        _native.check(lib.zk_local_max_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, r, has_t, t,
                                           c_void_p(out.data_ptr()), capacity, byref(n), stream), "zk_local_max_dev")
        if n.value <= capacity:
            break
        capacity = n.value
        out = _device.empty((capacity, 2), np.int32, image)
    n = n.value
    return out[:n]


def points_moments_device(plan: "_native.Plan", image, points, out=None):
    """Moments of the windows centred on device-resident key points (``zk_transform_points_dev``): ``image`` an
    ``(H, W)`` float32 / float64 frame, ``points`` ``(N, 2)`` int32 ``(x, y)`` (what :func:`local_max_device` returns),
    both torch tensors or both :class:`~mtflearn_amd._native.DeviceArray`.  Returns the ``(N, n_poly)`` float64 moments
    on the device -- ``ZPs.transform_at(frame, points)`` with neither the frame nor the points crossing PCIe."""
    _check_operand(plan, image, "image")
    _check_operand(plan, points, "points")
    code = _device.code(image, FLOATS)
    _device.points_code(points)
    h, w = image.shape
    n = int(points.shape[0])
    if out is None:
        out = _empty_f64((n, plan.n_poly), image)
    else:
        _check_operand(plan, out, "out")
        assert tuple(out.shape) == (n, plan.n_poly) and _device.np_dtype(out) == np.float64
    if n:
        plan.transform_points_dev(image.data_ptr(), code, h, w, points.data_ptr(), n, out.data_ptr(), stream_ptr(image))
    return out


def remove_background_device(image, method, parameter, clip=True, **method_kw):
    """:mod:`mtflearn_amd.background` on a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).

    ``method``: ``"opening"`` (``parameter`` = size), ``"rolling_ball"`` (radius) or ``"baseline"`` (sigma; ``num_iters``
    as a keyword, default 10).  Returns ``(residual, background)`` as device arrays of the image's kind, in the image's dtype
    (float64 for the baseline), the same numbers as the host ``remove_background_*``.  Runs on torch's current stream and no
    pixel crosses to the host, so a frame goes to :func:`local_max_device` and :func:`points_moments_device` without PCIe."""
    from .background import _method_parameter
    param = _method_parameter(method, parameter, method_kw)
    image, code = _device.resident_frame(image, "remove_background_device")
    h, w = (int(v) for v in image.shape)
    out_dtype = np.float64 if method == "baseline" else _device.np_dtype(image)
    background = _device.empty((h, w), out_dtype, image)
    residual = _device.empty((h, w), out_dtype, image)
    lib = _native.load()
    args = (image.device.index, c_void_p(image.data_ptr()), code, h, w)
    outs = (int(bool(clip)), c_void_p(background.data_ptr()), c_void_p(residual.data_ptr()), c_void_p(stream_ptr(image)))
    if method == "opening":
        _native.check(lib.zk_background_opening_dev(*args, param[0], param[1], *outs), "zk_background_opening_dev")
    elif method == "rolling_ball":
        _native.check(lib.zk_background_rolling_ball_dev(*args, param, *outs), "zk_background_rolling_ball_dev")
    else:
        (wy, wx), iters = param
        _native.check(lib.zk_background_baseline_dev(*args, wy.ctypes.data_as(c_void_p), len(wy) - 1, wx.ctypes.data_as(c_void_p),
                                                     len(wx) - 1, iters, *outs), "zk_background_baseline_dev")
    return residual, background


def _device_image(image):
    """The :class:`mtflearn_amd.utils._Operand` of a device-resident image of any shape, on torch's current stream."""
    from .utils import _Operand
    image, _ = _device.resident_frame(image, "image", ndim=None)
    return _Operand(image, stream_ptr(image))


def normalize_image_device(image, mode="minmax", eps=1e-8, vmin=0.0, vmax=1.0):
    """:func:`mtflearn_amd.utils.normalize_image` of an image resident on the GPU (a torch tensor or a :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` or ``(H, W, C)``
    of float32 / float64 / uint8 / uint16 / int16).  Returns the float32 result as a device array of the same kind, the same
    numbers as the host function; only the statistics (two floats, a count, three sums) cross to the host.  Runs on torch's
    current stream."""
    from .utils import _check_mode, _normalize_core
    _check_mode(mode)
    return _normalize_core(_device_image(image), mode, float(eps), float(vmin), float(vmax), False)


def standardize_image_device(image):
    """:func:`mtflearn_amd.utils.standardize_image` of an image resident on the GPU (as :func:`normalize_image_device`):
    float32 for a float32 image, float64 otherwise, as a device array of the same kind."""
    from .utils import _standardize_core
    return _standardize_core(_device_image(image))


def percentile_clip_device(image, low=1.0, high=99.0, method="auto", high_ratio_thresh=5.0, mad_k=8.0, iqr_k=3.0, eps=1e-8):
    """:func:`mtflearn_amd.utils.percentile_clip` of an image resident on the GPU (as :func:`normalize_image_device`).  Returns
    ``(out, did_clip, info)`` with ``out`` the float32 image (clipped or not) as a device array of the same kind and ``info``
    the host function's dictionary; only the order statistics (at most 16 floats per call) cross to the host."""
    from .utils import _check_method, _check_percentile, _clip_core
    method = _check_method(method)
    _check_percentile(high)
    _check_percentile(low)
    return _clip_core(_device_image(image), low, high, method, high_ratio_thresh, mad_k, iqr_k, eps)


def render_gaussians_device(frame_dev, pts, sigma, amplitude=1, r_factor=3.0):
    """:func:`mtflearn_amd.datasets.add_tapered_gaussian` into a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64): the tapered Gaussians at the host points
    ``pts`` are added in place and the frame is returned, the same numbers as the host function bit for bit.  Only the points
    cross to the device.  Runs on torch's current stream, which is synchronised before the call returns."""
    from .datasets import _points_and_amplitudes, _render_device
    pts, amps = _points_and_amplitudes(len(frame_dev.shape), pts, sigma, amplitude, r_factor)
    if not frame_dev.is_cuda:
        raise ValueError("image must live on the GPU")
    if not frame_dev.is_contiguous():
        raise ValueError("the frame is added to in place and must be contiguous")
    _device.code(frame_dev, FLOATS)
    if len(pts) and frame_dev.numel():
        _render_device(frame_dev, pts, amps, sigma, r_factor, True)
    return frame_dev


def honeycomb_image_device(lattice, like=None, **to_image_kw):
    """:meth:`mtflearn_amd.datasets.HoneyCombLattice.to_image` with the image left on the GPU: the float32
    ``(size, size)`` frame as a :class:`~mtflearn_amd._native.DeviceArray` on the default device, or, with ``like`` a torch
    tensor (or a DeviceArray), as an array of that kind on that device.  ``to_image_kw``: ``sigma``, ``intensity_A``,
    ``intensity_B``, ``normalize``.  The frame is born on the device and goes on to :func:`remove_background_device`,
    :func:`local_max_device` and :func:`points_moments_device` without a host copy; only the site coordinates go up."""
    from .datasets import _render_device
    from .utils import _Operand, _map, _stats
    unknown = set(to_image_kw) - {"sigma", "intensity_A", "intensity_B", "normalize"}
    if unknown:
        raise TypeError(f"to_image() got an unexpected keyword argument {sorted(unknown)[0]!r}")
    sigma, pts, amps = lattice._render_lists(to_image_kw.get("sigma"), to_image_kw.get("intensity_A", 1.0),
                                             to_image_kw.get("intensity_B", 0.5))
    size = lattice.size
    if like is None or is_native(like):
        _native.load()
        _native.require_device()
        device = _native.default_device() if like is None else like.device.index
        img = _native.DeviceArray.from_numpy(np.zeros((size, size), np.float32), device)
    else:
        import torch
        img = torch.zeros((size, size), dtype=torch.float32, device=like.device)
    if len(pts) and size:
        _render_device(img, pts, amps, sigma, 3.0, True)
    if to_image_kw.get("normalize", False) and size:
        operand = _Operand(img, stream_ptr(img))
        vmax = float(_stats(operand)[1])
        if vmax > 0.0:
            # x / vmax in float64 rounded once is the float32 quotient: 53 bits are more than 2 * 24 + 2
            img = _map(operand, _native.MAP_DIVIDE, [vmax])
    return img


def tmd_frames_device(simulators, return_masks=False, out=None, consistent_defects=False):
    """The frames of a sequence of :class:`mtflearn_amd.datasets.TMDImageSimulator` of one ``size`` and one ``use_fft``, in one
    device call: the ``(B, H, W)`` float32 stack as a :class:`~mtflearn_amd._native.DeviceArray` on the default device, or
    written into ``out`` (a contiguous float32 array of that shape, a DeviceArray or a torch tensor, on whose device and stream
    the call then runs).  With ``return_masks`` also the delta images ``(B, S, H, W)`` of the same kind, species in order of
    first appearance in ``basis`` (every simulator then needs the same number of species).  Every simulator's lattice is
    generated (its ``pts``, ``labels`` and ``lbs`` are set); frame ``b`` is ``simulators[b].simulate()`` bit for bit, whatever
    else is in the batch.  Only the atoms on the frame and the half kernels cross to the device; the stream is synchronised
    before the call returns.  Newer than ``__all__``: reached as ``resident.tmd_frames_device``."""
    from .datasets import _tmd_render_device
    simulators = list(simulators)
    if not simulators:
        raise ValueError("tmd_frames_device needs at least one simulator")
    h, w = (int(v) for v in simulators[0].size)
    use_fft = bool(simulators[0].use_fft)
    if h < 1 or w < 1:
        raise ValueError("the frame size must be positive")
    layers, counts = [], []
    for b, sim in enumerate(simulators):
        if tuple(int(v) for v in sim.size) != (h, w) or bool(sim.use_fft) != use_fft:
            raise ValueError("the simulators of one call share one size and one use_fft")
        own = sim._layers(consistent_defects)
        counts.append(len(own))
        layers += [(b,) + layer[1:] for layer in own]
    if return_masks and len(set(counts)) != 1:
        raise ValueError("return_masks needs the same number of species in every simulator")
    shape = (len(simulators), h, w)
    if out is None:
        _native.load()
        _native.require_device()
        out = _native.DeviceArray(shape, np.float32, _native.default_device())
    elif (not getattr(out, "is_cuda", False) or not out.is_contiguous() or tuple(out.shape) != shape
          or _device.np_dtype(out) != np.float32):
        raise ValueError(f"out must be a contiguous {shape} float32 array on the GPU")
    masks = _device.empty((len(layers), h, w), np.float32, out) if return_masks else None
    _tmd_render_device(out, masks, layers, True, use_fft)
    if not return_masks:
        return out
    mask_shape = (len(simulators), counts[0], h, w)
    if is_native(masks):
        masks = _native.DeviceArray(mask_shape, np.float32, masks.device.index, _base=masks, _ptr=masks.data_ptr())
    else:
        masks = masks.view(mask_shape)
    return out, masks


def _as_dtype_device(array, np_dtype, what):
    """``array`` as a contiguous device array of ``np_dtype``: a torch tensor is converted on the device, a DeviceArray must
    already have the type."""
    if not array.is_cuda:
        raise ValueError(f"{what} must live on the GPU")
    if is_native(array):
        if array.dtype != np_dtype:
            raise TypeError(f"{what} must be a {np.dtype(np_dtype).name} DeviceArray, not {array.dtype}")
        return array
    import torch
    return array.to(getattr(torch, np.dtype(np_dtype).name)).contiguous()


def find_regions_device(points, edges):
    """:func:`mtflearn_amd.graph.find_regions` of points and bonds resident on the GPU: ``points`` ``(N, 2)`` (torch tensor of
    any real type, e.g. what :func:`local_max_device` returns, converted to float64 on the device; or a float64
    :class:`~mtflearn_amd._native.DeviceArray`), ``edges`` ``(E, 2)`` directed index pairs (torch integer tensor, or an int64
    DeviceArray) on the same device.  Returns ``(offsets, vertices, ks, centers, adjacency)`` as device arrays of the same kind:
    polygon ``f`` is ``vertices[offsets[f]:offsets[f + 1]]`` (int64), ``ks`` its size (int64), ``centers`` ``(F, 2)`` float64
    bit-equal to ``nodes[region].mean(axis=0)``, ``adjacency`` ``(A, 2)`` int64 pairs of polygons that share a bond.  Only the
    three counts cross to the host.  The edge values cannot be checked before the launch here: the device checks them, and
    a pair outside ``[0, N)`` or a self-loop raises ``RuntimeError`` (``ZK_E_BADARG``) with nothing computed.  Runs on torch's
    current stream, which is synchronised before the call returns."""
    if len(points.shape) != 2 or points.shape[1] != 2:
        raise ValueError(f"points must have shape (N, 2), not {tuple(points.shape)}")
    if len(edges.shape) != 2 or edges.shape[1] != 2:
        raise ValueError(f"edges must have shape (E, 2), not {tuple(edges.shape)}")
    if not is_native(edges) and (edges.dtype.is_floating_point or edges.dtype.is_complex or str(edges.dtype) == "torch.bool"):
        raise ValueError(f"edges must be of an integer type, not {edges.dtype}")
    points = _as_dtype_device(points, np.float64, "points")
    edges = _as_dtype_device(edges, np.int64, "edges")
    if points.device.index != edges.device.index:
        raise ValueError("points and edges must live on the same device")
    n, e = int(points.shape[0]), int(edges.shape[0])
    if n + e + 4 >= 2 ** 31:
        raise ValueError("find_regions_device needs len(points) + len(edges) + 4 < 2^31")
    if n == 0 and e:
        raise ValueError("edges without points")
    lib = _native.load()
    device, stream = points.device.index, c_void_p(stream_ptr(points))
    state, counts = c_void_p(), (c_int64 * 3)()
    _native.check(lib.zk_find_regions_dev(device, c_void_p(points.data_ptr()), n, c_void_p(edges.data_ptr()), e, byref(state), counts,
                                          None, None, None, None, None, stream), "zk_find_regions_dev")
    f, v, a = (int(c) for c in counts)
    offsets, vertices, ks = (_device.empty(shape, np.int64, points) for shape in ((f + 1,), (v,), (f,)))
    centers, adjacency = _empty_f64((f, 2), points), _device.empty((a, 2), np.int64, points)
    _native.check(lib.zk_find_regions_dev(device, None, 0, None, 0, byref(state), counts, c_void_p(offsets.data_ptr()),
                                          c_void_p(vertices.data_ptr()), c_void_p(ks.data_ptr()), c_void_p(centers.data_ptr()),
                                          c_void_p(adjacency.data_ptr()), stream), "zk_find_regions_dev")
    return offsets, vertices, ks, centers, adjacency


def _resident_points(points, what, spare=0):
    """``(points, ZK_* code)`` of resident ``(N, 2)`` points for ``zk_voronoi_cells_dev`` and ``zk_knn_distances_dev``: float64 or
    int32 as they are, any other real torch type converted to float64 on the device.  ``what`` needs
    ``len(points) < 2^26 - spare``."""
    if len(points.shape) != 2 or points.shape[1] != 2:
        raise ValueError(f"points must have shape (N, 2), not {tuple(points.shape)}")
    if not points.is_cuda:
        raise ValueError("points must live on the GPU")
    if is_native(points):
        if points.dtype not in (np.float64, np.int32):
            raise TypeError(f"points must be a float64 or int32 DeviceArray, not {points.dtype}")
    else:
        import torch
        if points.dtype.is_complex or points.dtype == torch.bool:
            raise ValueError(f"points must be real numbers, not {points.dtype}")
        if points.dtype not in (torch.float64, torch.int32):
            points = points.to(torch.float64)
        points = points.contiguous()
    if int(points.shape[0]) + spare >= 2 ** 26:
        raise ValueError(f"{what} needs len(points) < 2^26" + (f" - {spare}" if spare else ""))
    return points, _device.code(points, ("float64", "int32"))


def _voronoi_device(points, pad, mode, dmax, threshold, stream, what):
    """Both phases of ``zk_voronoi_cells_dev`` on resident points; returns ``(ijs, ridge, edge)`` of the points' kind."""
    points, code = _resident_points(points, what, spare=4)
    if not (np.isfinite(pad) and pad > 0):
        raise ValueError(f"pad must be positive and finite, not {pad}")
    n = int(points.shape[0])
    lengths = mode == _native.VORONOI_NEIGHBOURS
    if n == 0:
        return _device.empty((0, 2), np.int64, points), _empty_f64((0,), points), _empty_f64((0,), points)
    lib = _native.load()
    device = points.device.index
    if stream is None:
        stream = stream_ptr(points)
    stream = c_void_p(int(getattr(stream, "cuda_stream", stream)))
    state, counts = c_void_p(), (c_int64 * 1)()
    _native.check(lib.zk_voronoi_cells_dev(device, c_void_p(points.data_ptr()), code, n, pad, mode, dmax, threshold, byref(state), counts,
                                           None, None, None, stream), "zk_voronoi_cells_dev")
    m = int(counts[0])
    ijs = _device.empty((m, 2), np.int64, points)
    ridge, edge = (_empty_f64((m,), points), _empty_f64((m,), points)) if lengths else (None, None)
    _native.check(lib.zk_voronoi_cells_dev(device, None, code, 0, pad, mode, dmax, threshold, byref(state), counts, c_void_p(ijs.data_ptr()),
                                           c_void_p(ridge.data_ptr()) if lengths else None, c_void_p(edge.data_ptr()) if lengths else None,
                                           stream), "zk_voronoi_cells_dev")
    return ijs, ridge, edge


def voronoi_neighbours_device(points, pad=0.05, stream=None):
    """:func:`mtflearn_amd.graph.voronoi_neighbours` of points resident on the GPU: ``points`` ``(N, 2)``, a torch tensor of
    any real type or a float64 / int32 :class:`~mtflearn_amd._native.DeviceArray`.  What :func:`local_max_device` returns --
    ``(N, 2)`` int32, column 0 is x, column 1 is y -- is taken as it is and widened on the device; the neighbours do not depend
    on which column is x.  Returns ``(ijs, ridge_lengths, edge_lengths)`` as device arrays of the same kind (int64 ``(M, 2)``,
    float64 ``(M)``, float64 ``(M)``).  Only the row count crosses to the host.  The values cannot be checked before the launch
    here: the device checks them, and a non-finite coordinate, two coincident points or a cell of more than 32 vertices (a point
    with more than 32 Voronoi neighbours, or nearly as many: cells are clipped in bin order) raise ``RuntimeError``
    (``ZK_E_BADARG``) with nothing computed.  Runs on ``stream`` (default: torch's current stream for tensors, the default
    stream for a DeviceArray), which is synchronised before the call returns."""
    return _voronoi_device(points, float(pad), _native.VORONOI_NEIGHBOURS, 0.0, 0.0, stream, "voronoi_neighbours_device")


def estimate_d_device(points, threshold='otsu', return_k=False):
    """:func:`mtflearn_amd.graph.estimate_d` of points resident on the GPU: ``points`` ``(N, 2)``, a torch tensor of any real
    type or a float64 / int32 :class:`~mtflearn_amd._native.DeviceArray` -- what :func:`local_max_device` or
    :func:`refine_points_device` return.  The points and their distance matrix stay on the device; a few hundred numbers per
    pass (ranges, histograms, side sums) cross to the host, where the scalar rules run.  ``N < 12`` raises ``ValueError``;
    a non-finite coordinate raises ``RuntimeError`` from the device.  Runs on torch's current stream."""
    from . import graph
    points, code = _resident_points(points, "estimate_d_device")
    n = int(points.shape[0])
    if n < graph.KNN:
        raise ValueError(f"Expected n_neighbors <= n_samples_fit, but n_neighbors = {graph.KNN}, n_samples_fit = {n}")
    device, stream = points.device.index, stream_ptr(points)
    dd = _empty_f64((n, graph.KNN), points)
    _native.check(_native.load().zk_knn_distances_dev(device, c_void_p(points.data_ptr()), code, n, graph.KNN, c_void_p(dd.data_ptr()),
                                                      c_void_p(stream)), "zk_knn_distances_dev")
    parts = graph._estimate_from_distances(device, dd.data_ptr(), n, stream, threshold)
    return (parts["t"], parts["k"]) if return_k else parts["t"]


def refine_points_device(image, points, size=3, mode=None):
    """:func:`mtflearn_amd.features.refine_points` of a frame and key points resident on the GPU: ``image`` ``(H, W)`` float32 /
    float64, ``points`` ``(N, 2)`` int32 ``(x, y)`` (what :func:`local_max_device` returns), both torch tensors or both
    :class:`~mtflearn_amd._native.DeviceArray`.  Returns the ``(N, 2)`` float64 ``(x, y)`` centroids on the device, of the same
    kind -- what :func:`vnn_graph_device`, :func:`estimate_d_device` and :func:`find_regions_device` accept; round them to
    int32 for :func:`points_moments_device`.  The numbers are those of the host ``center_of_mass_refine``, bit for bit.  A
    frame that is not float, ``N >= 2^24`` or a box that leaves the frame raise ``ValueError`` (the boxes are checked on the
    device: nothing is written for such a point, and only the flag crosses to the host).  Runs on torch's current stream."""
    image, code, points, _ = _device.resident_frame_points(image, points, "refine_points_device")
    size = int(size)
    if not 0 <= size <= 64:
        raise ValueError(f"size must be in [0, 64], not {size}")
    n = int(points.shape[0])
    h, w = (int(v) for v in image.shape)
    out = _empty_f64((n, 2), image)
    if n:
        lib = _native.load()
        rc = lib.zk_refine_points_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, c_void_p(points.data_ptr()), n, size,
                                      _native.REFINE_DISK if mode == 'disk' else _native.REFINE_BOX, c_void_p(out.data_ptr()),
                                      c_void_p(stream_ptr(image)))
        _device.check_refusal(rc, "zk_refine_points_dev")
    return out


def com_refine_device(image, points, size, threshold=None):
    """:func:`mtflearn_amd.features.com_refine_points` of a frame and key points resident on the GPU: ``image`` ``(H, W)``
    float32 / float64, ``points`` ``(N, 2)`` int32 or float64 ``(x, y)`` (what :func:`local_max_device` or
    :func:`refine_points_device` return), both torch tensors or both :class:`~mtflearn_amd._native.DeviceArray`.  Returns the
    ``(N, 2)`` float64 refined points on the device, of the same kind -- what :func:`vnn_graph_device`,
    :func:`estimate_d_device` and :func:`find_regions_device` accept.  Rounding the points to window corners and the two final
    additions are done on the device with the host function's own rounded operations: a point gives the same bits on either
    route.  As there, the thresholds (``threshold='otsu'``: Otsu, anything else: Li) are defined on the window widened to
    float64 and parity with scikit-image is unpinned.  There is NO border clearing here: every ``size x size`` window must lie
    inside the frame, or ``ValueError`` is raised (the windows are checked on the device: nothing is written for such a
    point, and only the flag crosses to the host) -- the contract of :func:`refine_points_device`.  A frame that is not float,
    ``size`` outside ``[2, 64]`` or ``N >= 2^24`` raise ``ValueError`` too.  Runs on torch's current stream."""
    image, code, points, points_code = _device.resident_frame_points(image, points, "com_refine_device", ("int32", "float64"))
    if int(size) != size or not 2 <= int(size) <= 64:
        raise ValueError(f"size must be an integer in [2, 64], not {size}")
    n = int(points.shape[0])
    h, w = (int(v) for v in image.shape)
    out = _empty_f64((n, 2), image)
    if n:
        rc = _native.load().zk_com_refine_points_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, c_void_p(points.data_ptr()),
                                                     points_code, n, int(size),
                                                     _native.THRESHOLD_OTSU if threshold == 'otsu' else _native.THRESHOLD_LI,
                                                     c_void_p(out.data_ptr()), c_void_p(stream_ptr(image)))
        _device.check_refusal(rc, "zk_com_refine_points_dev")
    return out


def vnn_graph_device(points, dmax=None, threshold=0.1, pad=0.05, stream=None, threshold_method=None):
    """:func:`mtflearn_amd.graph.vnn_graph` of points resident on the GPU (see :func:`voronoi_neighbours_device` for the
    operands, the errors and the stream): the int64 ``(E, 2)`` sorted, symmetrised bonds as a device array of the points'
    kind, ready for :func:`find_regions_device` -- key points go from :func:`local_max_device` to polygons without a host copy.
    Without ``dmax`` it is ``estimate_d_device(points, threshold=threshold_method)``, as in the reference."""
    if dmax is None:
        dmax = estimate_d_device(points, threshold=threshold_method)
    dmax, threshold = float(dmax), float(threshold)
    if not dmax > 0:
        raise ValueError(f"dmax must be positive, not {dmax}")
    if not threshold > 0:
        raise ValueError(f"threshold must be > 0, not {threshold}")
    return _voronoi_device(points, float(pad), _native.VORONOI_GRAPH, dmax, threshold, stream, "vnn_graph_device")[0]


def inverse_transform_device(zps, coeffs_dev, n_rows=None, method="lstsq", m_select=None, dtype=np.float64, out=None):
    """The resident twin of ``ZPs.inverse_transform``: ``coeffs_dev`` is an ``(N, P)`` float64 torch tensor or ``DeviceArray`` of
    real moments of ``zps``'s full set (k-means centres, class means, rows of ``points_moments_device``); the first ``n_rows``
    of them (default: all) come back as an ``(n_rows, size, size)`` array of ``dtype`` (float64 / float32) of the same kind on the
    same device, enqueued on torch's current stream (a ``DeviceArray``: the default stream) without synchronising.  The synthesis
    table is ``zps``'s cached one (``method``, ``m_select`` as there); everything is checked before any device call."""
    if not getattr(coeffs_dev, "is_cuda", False):
        raise ValueError("coeffs_dev must live on the GPU")
    if not coeffs_dev.is_contiguous():
        raise ValueError("coeffs_dev must be contiguous")
    if len(coeffs_dev.shape) != 2 or coeffs_dev.shape[1] != len(zps.n) or _device.np_dtype(coeffs_dev) != np.float64:
        raise ValueError(f"coeffs_dev must be an (N, {len(zps.n)}) float64 matrix of real Zernike moments")
    n_rows = int(coeffs_dev.shape[0] if n_rows is None else n_rows)
    if not 0 <= n_rows <= coeffs_dev.shape[0]:
        raise ValueError(f"n_rows must be between 0 and {coeffs_dev.shape[0]}")
    np_dtype = zps._inverse_dtype(dtype)
    entry = zps._synthesis_entry(method, m_select)
    if entry["cond"] is not None and entry["cond"] > zps._COND_LIMIT:
        warnings.warn(zps._cond_message(entry["cond"]), UserWarning, stacklevel=2)
    shape = (n_rows, zps.size, zps.size)
    if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or _device.np_dtype(out) != np_dtype
                            or out.device.index != coeffs_dev.device.index):
        raise ValueError(f"out must be a contiguous {shape} array of {np_dtype} on the device of coeffs_dev")
    if coeffs_dev.device.index != zps._pick_device():
        raise ValueError(f"coeffs_dev is on cuda:{coeffs_dev.device.index} but this ZPs computes on device {zps._pick_device()}: "
                         "bind it to the array's device (ZPs.to_device / MTFLEARN_AMD_DEVICE)")
    if out is None:
        out = _device.empty(shape, np_dtype, coeffs_dev)
    if n_rows == 0:
        return out
    synth = zps._synthesis_device(entry)
    synth.apply_dev(coeffs_dev.data_ptr(), n_rows, out.data_ptr(), _native.dtype_code(np_dtype), stream_ptr(coeffs_dev))
    return out


# align_device and rotate_rows_device are newer than the move out of mtflearn_amd.distributed: they are reached as
# resident.align_device / resident.rotate_rows_device and are not part of __all__, which lists exactly the names that module
# re-exports under their first address.
def _resident_rows(rows, n_cols, what):
    if not getattr(rows, "is_cuda", False):
        raise ValueError(f"{what} must live on the GPU")
    if not rows.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if len(rows.shape) != 2 or rows.shape[1] != n_cols or _device.np_dtype(rows) != np.float64:
        raise ValueError(f"{what} must be an (N, {n_cols}) float64 matrix of real Zernike moments")


def align_device(rows, n, m, templates, m_select=None, n_theta=360, symmetry=1, refine=True, key="distance"):
    """The resident twin of ``zmoments.align``: ``rows`` is an ``(N, P)`` float64 torch tensor or ``DeviceArray`` of real
    moments with labels ``n``, ``m`` (e.g. what :func:`points_moments_device` returns, with ``zps.n``, ``zps.m``);
    ``templates`` is a host ``(T, P)`` array (or a rank-2 real ``zmoments``) with the same labels -- small, and the library
    derives its operand tables from it on the host.  Returns ``AlignResult(angle (N, T), score (N, T), best (N) int32)`` as
    device arrays of ``rows``'s kind, enqueued on torch's current stream (a ``DeviceArray``: the default stream) without
    synchronising, except for the table upload of the first call with a new option set.  Everything is checked before any
    device call."""
    from .features.moments import AlignResult, zmoments
    n, m = np.asarray(n), np.asarray(m)
    _resident_rows(rows, len(n), "rows")
    tm = templates.to_real().data if isinstance(templates, zmoments) else np.asarray(templates)
    probe = zmoments._adopt(np.zeros((1, len(n))), n, m)
    if not np.array_equal(probe.n, n) or not np.array_equal(probe.m, m):
        raise ValueError("n, m must be in (n, m) lexicographic order, as ZPs.n / ZPs.m are")
    _, spec = probe._align_spec(tm, m_select, n_theta, symmetry, refine, key)
    rows_n, t = int(rows.shape[0]), spec.n_templates
    angle, score = _device.empty((rows_n, t), np.float64, rows), _device.empty((rows_n, t), np.float64, rows)
    best = _device.empty((rows_n,), np.int32, rows)
    if rows_n:
        _native.align_rows_dev(rows.device.index, rows.data_ptr(), rows_n, spec, angle.data_ptr(), score.data_ptr(), best.data_ptr(),
                               stream_ptr(rows))
    return AlignResult(angle, score, best)


def _resident_align_spec(n, m, templates, m_select, n_theta, symmetry, refine, key):
    """``(n, m, AlignSpec)`` of a resident alignment call: labels in (n, m) order, host templates, every refusal a ValueError."""
    from .features.moments import zmoments
    n, m = np.asarray(n), np.asarray(m)
    tm = templates.to_real().data if isinstance(templates, zmoments) else np.asarray(templates)
    probe = zmoments._adopt(np.zeros((1, len(n))), n, m)
    if not np.array_equal(probe.n, n) or not np.array_equal(probe.m, m):
        raise ValueError("n, m must be in (n, m) lexicographic order, as ZPs.n / ZPs.m are")
    return n, m, probe._align_spec(tm, m_select, n_theta, symmetry, refine, key)[1]


def _check_map(array, shape, dtype, like, name):
    if (not getattr(array, "is_cuda", False) or not array.is_contiguous() or tuple(array.shape) != tuple(shape)
            or _device.np_dtype(array) != dtype or is_native(array) != is_native(like) or array.device.index != like.device.index):
        raise ValueError(f"{name} must be a contiguous {tuple(shape)} {np.dtype(dtype).name} array of the operand's kind on its device")
    return array


def align_planes_device(planes, n, m, templates, m_select=None, n_theta=360, symmetry=1, refine=True, key="distance", out=None):
    """The resident twin of ``zmoments.align_map``: ``planes`` is a ``(P, ...)`` float64 torch tensor or ``DeviceArray`` of real
    moments, moment-major -- e.g. the ``(P, n_rows, W)`` that :func:`frame_moments_device` returns -- with labels ``n``, ``m``;
    ``templates`` is a host ``(T, P)`` array (or a rank-2 real ``zmoments``).  Returns ``AlignMaps(angle (T, ...), score (T, ...),
    best (...) int32, norm2 (...))`` as device arrays of ``planes``'s kind (``out``: four such arrays to write into), enqueued on
    torch's current stream without synchronising, except for the table upload of the first call with a new option set.
    Everything is checked before any device call.  Like :func:`align_device` it is newer than ``__all__``."""
    from .features.moments import AlignMaps
    n, m, spec = _resident_align_spec(n, m, templates, m_select, n_theta, symmetry, refine, key)
    if not getattr(planes, "is_cuda", False):
        raise ValueError("planes must live on the GPU")
    if not planes.is_contiguous():
        raise ValueError("planes must be contiguous")
    if len(planes.shape) < 2 or planes.shape[0] != len(n) or _device.np_dtype(planes) != np.float64:
        raise ValueError(f"planes must be a ({len(n)}, ...) float64 array of real Zernike moments, one plane per moment")
    rest = tuple(int(v) for v in planes.shape[1:])
    pixels, t = int(np.prod(rest, dtype=np.int64)), spec.n_templates
    shapes = ((t,) + rest, (t,) + rest, rest, rest)
    dtypes = (np.float64, np.float64, np.int32, np.float64)
    if out is None:
        out = tuple(_device.empty(s, d, planes) for s, d in zip(shapes, dtypes))
    else:
        out = tuple(_check_map(a, s, d, planes, name) for a, s, d, name in zip(out, shapes, dtypes, AlignMaps._fields))
    if pixels:
        _native.align_planes_dev(planes.device.index, planes.data_ptr(), pixels, pixels, spec, *(a.data_ptr() for a in out), pixels,
                                 stream_ptr(planes))
    return AlignMaps(*out)


def align_maps_device(plan: "_native.Plan", image, templates, m_select=None, n_theta=360, symmetry=1, refine=True, key="distance",
                      row0=0, n_rows=None, full=None):
    """The resident twin of ``ZPs.align_maps``, in the idiom of :func:`frame_maps_device`: the alignment maps of output rows
    ``[row0, row0 + n_rows)`` of a float32 / float64 frame ``(H, W)`` resident on the GPU.  Returns ``AlignMaps(angle (T, n_rows, W),
    score (T, n_rows, W), best (n_rows, W) int32, norm2 (n_rows, W))`` on the device; with ``full = (angle, score, best, norm2)``
    (whole-frame arrays ``(T, H, W)`` / ``(H, W)``, entries ``None`` where not wanted) the band is written in place into them and
    ``full`` is returned.  The moments pass through the plan's scratch matrix a band at a time and never exist as a whole.  Runs on
    torch's current stream without synchronising, except for the table upload of the first call with a new option set; calls on one
    plan share its scratch matrix and belong on one stream."""
    from .features.moments import AlignMaps
    _check_operand(plan, image, "image")
    code = _device.code(image, FLOATS)
    _, _, spec = _resident_align_spec(plan.n, plan.m, templates, m_select, n_theta, symmetry, refine, key)
    if len(image.shape) != 2:
        raise ValueError(f"align_maps_device needs a 2D image, not {len(image.shape)}-D")
    h, w = (int(v) for v in image.shape)
    n_rows = h - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row0 + n_rows > h:
        raise ValueError("row band outside the frame")
    t, stream = spec.n_templates, stream_ptr(image)
    dtypes = (np.float64, np.float64, np.int32, np.float64)
    if full is not None:
        shapes = ((t, h, w), (t, h, w), (h, w), (h, w))
        for a, s, d, name in zip(full, shapes, dtypes, AlignMaps._fields):
            if a is not None:
                _check_map(a, s, d, image, name)
        ptr = lambda a, size: a.data_ptr() + row0 * w * size if a is not None else 0
        _native.frame_align_dev(plan, image.data_ptr(), code, h, w, row0, n_rows, spec, ptr(full[0], 8), ptr(full[1], 8), ptr(full[2], 4),
                                ptr(full[3], 8), h * w, stream)
        return full
    out = tuple(_device.empty(s, d, image) for s, d in zip(((t, n_rows, w), (t, n_rows, w), (n_rows, w), (n_rows, w)), dtypes))
    _native.frame_align_dev(plan, image.data_ptr(), code, h, w, row0, n_rows, spec, *(a.data_ptr() for a in out), n_rows * w, stream)
    return AlignMaps(*out)


def rotate_rows_device(rows, n, m, angles, out=None):
    """The resident twin of ``zmoments.rotate_each``: every row of the ``(N, P)`` float64 device matrix rotated by its own
    angle (``angles``: ``(N)`` float64 degrees on the same device, e.g. a column of :func:`align_device`'s ``angle`` made
    contiguous).  ``out`` may be ``rows`` (in place).  Returns the rotated rows as a device array of ``rows``'s kind, enqueued
    on torch's current stream without synchronising."""
    n, m = np.asarray(n), np.asarray(m)
    _resident_rows(rows, len(n), "rows")
    rows_n = int(rows.shape[0])
    if (not getattr(angles, "is_cuda", False) or not angles.is_contiguous() or tuple(angles.shape) != (rows_n,)
            or _device.np_dtype(angles) != np.float64 or angles.device.index != rows.device.index):
        raise ValueError(f"angles must be a contiguous ({rows_n},) float64 array on the device of rows")
    if out is None:
        out = _device.empty((rows_n, len(n)), np.float64, rows)
    else:
        _resident_rows(out, len(n), "out")
        if int(out.shape[0]) != rows_n or out.device.index != rows.device.index:
            raise ValueError("out must have the shape and the device of rows")
    _native.check_paired(n, m)
    if rows_n:
        _native.rotate_rows_dev(rows.device.index, rows.data_ptr(), rows_n, n, m, angles.data_ptr(), out.data_ptr(), stream_ptr(rows))
    return out


def baseline_device(data, method="snip", axis=0, return_signal=False, return_info=False, **method_kw):
    """:mod:`mtflearn_amd.eels` on a spectrum cube resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray` of any rank >= 1, float32 / float64 / uint8 / uint16 / int16; ``axis`` is the energy
    axis).  ``method``: ``"snip"``, ``"als"``, ``"arpls"`` or ``"airpls"``, its parameters as keywords under the reference's names.
    Returns the float64 baseline as a device array of the cube's kind -- bit for bit the host function's -- or
    ``(signal, baseline)`` with ``return_signal``; with ``return_info`` the int32 solves per spectrum (``None`` for SNIP and a
    constant for ALS) are appended, on the device as well.  Cube and results never cross to the host; with ``return_info`` the
    counts are not read here, so no ``RuntimeWarning`` about ``itermax`` is raised.  Runs on torch's current stream, which is
    synchronised before the call returns.  Like :func:`align_device` it is newer than ``__all__`` and is reached as
    ``resident.baseline_device`` (or ``distributed.baseline_device``)."""
    from .eels import _call, _check_length, _layout, _method_spec
    spec = _method_spec(method, method_kw)
    shape = tuple(int(v) for v in data.shape)
    layout = _layout(shape, axis)
    _check_length(layout[1], spec["order"])
    data, code = _device.resident_frame(data, "baseline_device", ndim=None)
    baseline = _empty_f64(shape, data)
    signal = _empty_f64(shape, data) if return_signal else None
    ax = int(axis) % len(shape)
    iterations = None if spec.get("snip") or not return_info else _device.empty(shape[:ax] + shape[ax + 1:], np.int32, data)
    ptr = lambda a: c_void_p(a.data_ptr()) if a is not None else None
    _call(_native.load(), data.device.index, spec, ptr(data), code, layout, None, 0, ptr(baseline), ptr(signal), ptr(iterations),
          stream=stream_ptr(data))
    out = (signal, baseline) if return_signal else (baseline,)
    if return_info:
        out += (iterations,)
    return out if len(out) > 1 else out[0]


def scan_noise_device(images, dx, dy, order=1, mode="reflect", out=None):
    """The resampling of :func:`mtflearn_amd.denoise.apply_scan_noise` on a stack resident on the GPU: ``images`` ``(Z, H, W)``
    float32 or float64, ``dx`` ``(Z, H)`` and ``dy`` ``(Z, W)`` float64 shifts, all torch tensors or all
    :class:`~mtflearn_amd._native.DeviceArray` on one device.  Returns ``out[z, y, x] = S_z(y + dy[z, x], x + dx[z, y])`` in the
    stack's dtype as a device array of its kind (``out``: a contiguous array of that shape and dtype to write into) -- bit for
    bit the host function's numbers for the same shifts.  Runs on torch's current stream without a host copy; at order 3 the
    stream is synchronised before the call returns (the two float64 scratch planes per frame are released then).  Like
    :func:`baseline_device` it is newer than ``__all__`` and is reached as ``resident.scan_noise_device`` (or
    ``distributed.scan_noise_device``)."""
    from .denoise import _check_scan_order_mode, _check_scan_shape
    order, mode_code = _check_scan_order_mode(order, mode)
    z, h, w = shape = _check_scan_shape(tuple(images.shape))
    images, code = _device.resident_frame(images, "scan_noise_device", floats_only=True, ndim=3)

    def companion(array, name, want, dtype):
        if (not getattr(array, "is_cuda", False) or not array.is_contiguous() or tuple(array.shape) != want
                or _device.np_dtype(array) != dtype or is_native(array) != is_native(images) or array.device.index != images.device.index):
            raise ValueError(f"{name} must be a contiguous {want} {np.dtype(dtype).name} array of the stack's kind on its device")
        return array

    companion(dx, "dx", (z, h), np.float64)
    companion(dy, "dy", (z, w), np.float64)
    out = _device.empty(shape, _device.np_dtype(images), images) if out is None else companion(out, "out", shape, _device.np_dtype(images))
    ptr = lambda a: c_void_p(a.data_ptr())
    _native.check(_native.load().zk_scan_resample_dev(images.device.index, ptr(images), code, z, h, w, ptr(dx), ptr(dy), order, mode_code,
                                                      ptr(out), None, 0, c_void_p(stream_ptr(images))), "zk_scan_resample_dev")
    return out


def _resident_stack(stack, what, floats_only=False):
    """``(stack, ZK_* code, (B, H, W))`` of the stack operand of a registration entry point."""
    from .registration import _check_stack_shape
    shape = _check_stack_shape(stack.shape)
    stack, code = _device.resident_frame(stack, what, floats_only=floats_only, ndim=3)
    return stack, code, shape


def _estimate_shifts_resident(stack, code, shape, reference, options, planes=False):
    """``zk_register_shifts_dev`` on checked operands: ``Shifts`` on the device (and the two planes with ``planes``)."""
    from .registration import REF_PREVIOUS, Shifts, _accumulate, _check_reference, upsampled_size
    b, h, w = shape
    mode, index, frame = _check_reference(reference, shape)
    frame_code = 0
    if frame is not None:
        if not getattr(frame, "is_cuda", False) or is_native(frame) != is_native(stack) or frame.device.index != stack.device.index:
            raise ValueError("a reference frame must be an array of the stack's kind on its device")
        frame, frame_code = _device.resident_frame(frame, "the reference frame")
    upsample, lags, norm, win = options
    shift, peak = _empty_f64((b, 2), stack), _empty_f64((b,), stack)
    s = upsampled_size(upsample)
    corr = _empty_f64((b, h, w), stack) if planes else None
    up = _empty_f64((b, s, s), stack) if planes and upsample > 1 else None
    ptr = lambda a: c_void_p(a.data_ptr()) if a is not None else None
    _native.check(_native.load().zk_register_shifts_dev(stack.device.index, ptr(stack), code, b, h, w, mode, index, ptr(frame), frame_code,
                                                        upsample, lags, norm, win, ptr(shift), ptr(peak), ptr(corr), ptr(up),
                                                        c_void_p(stream_ptr(stack))), "zk_register_shifts_dev")
    if mode == REF_PREVIOUS:                       # the running sum is the host's np.cumsum, as in estimate_shifts: B x 2 numbers cross
        shift = _device.from_host(_accumulate(mode, _device.to_host(shift)), stack)
    shifts = Shifts(shift, peak)
    return (shifts, corr, up) if planes else shifts


def estimate_shifts_device(stack, reference=0, upsample=100, max_shift=None, normalization=None, window=None):
    """:func:`mtflearn_amd.registration.estimate_shifts` of a stack resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(B, H, W)`` of float32 / float64 / uint8 / uint16 / int16; an array
    ``reference`` is an ``(H, W)`` array of the same kind on the same device).  Returns ``Shifts(shift (B, 2), peak (B,))`` as
    float64 device arrays of the stack's kind, bit for bit the host function's numbers.  Runs on torch's current stream, which
    is synchronised before the call returns (the complex fields are released then); with ``reference="previous"`` the
    ``B x 2`` pairwise shifts cross to the host for the running sum.  Like :func:`scan_noise_device` it is newer than
    ``__all__`` and is reached as ``resident.estimate_shifts_device``."""
    from .registration import _check_options
    options = _check_options(upsample, max_shift, normalization, window)
    stack, code, shape = _resident_stack(stack, "estimate_shifts_device")
    return _estimate_shifts_resident(stack, code, shape, reference, options)


def _shift_rows_resident(stack, shifts):
    """The constant shift rows of :func:`shift_stack_device` on the stack's device; ``shifts`` from either side."""
    from .registration import _check_shifts, _shift_rows
    shifts = _check_shifts(_device.to_host(shifts) if getattr(shifts, "is_cuda", False) else shifts, int(stack.shape[0]))
    dx, dy = _shift_rows(shifts, int(stack.shape[1]), int(stack.shape[2]))
    return _device.from_host(dx, stack), _device.from_host(dy, stack)


def shift_stack_device(stack, shifts, order=3, mode="grid-wrap", out=None):
    """:func:`mtflearn_amd.registration.shift_stack` of a float32 / float64 stack resident on the GPU: ``out[b, y, x] = S_b(y -
    shifts[b, 0], x - shifts[b, 1])`` in the stack's dtype.  ``shifts`` is ``(B, 2)``, a host array or a device array (what
    :func:`estimate_shifts_device` returns; its ``B x 2`` numbers cross to the host, where the shift rows are laid out).  It is
    :func:`scan_noise_device` with the rows ``dx[b, :] = -shifts[b, 1]`` and ``dy[b, :] = -shifts[b, 0]``, bit for bit."""
    from .denoise import _check_scan_order_mode
    _check_scan_order_mode(order, mode)
    stack, _, _ = _resident_stack(stack, "shift_stack_device", floats_only=True)
    dx, dy = _shift_rows_resident(stack, shifts)
    return scan_noise_device(stack, dx, dy, order=order, mode=mode, out=out)


def stack_mean_device(stack):
    """The ``(H, W)`` float64 mean of a ``(B, H, W)`` stack resident on the GPU (``zk_stack_mean_dev``): per pixel the sum over
    ``b`` in ascending order, divided once by ``B``.  Enqueued on torch's current stream without synchronising."""
    stack, code = _device.resident_frame(stack, "stack_mean_device", ndim=3)
    b, h, w = (int(v) for v in stack.shape)
    if 0 in (b, h, w):
        raise ValueError(f"an empty stack has no mean: shape {(b, h, w)}")
    out = _empty_f64((h, w), stack)
    _native.check(_native.load().zk_stack_mean_dev(stack.device.index, c_void_p(stack.data_ptr()), code, b, h, w, c_void_p(out.data_ptr()),
                                                   c_void_p(stream_ptr(stack))), "zk_stack_mean_dev")
    return out


def register_stack_device(stack, reference=0, upsample=100, max_shift=None, normalization=None, window=None, order=3, mode="grid-wrap",
                          return_aligned=False):
    """:func:`mtflearn_amd.registration.register_stack` of a float32 / float64 stack resident on the GPU: ``Registered(mean (H, W)
    float64, shifts (B, 2), peak (B,), aligned)`` as device arrays of the stack's kind, bit for bit the host function's numbers.
    No frame crosses to the host (the ``B x 2`` shifts do, for the shift rows), so ``tmd_frames_device -> scan_noise_device ->
    register_stack_device -> denoise_svd_device`` runs on the device from end to end.  Runs on torch's current stream."""
    from .denoise import _check_scan_order_mode
    from .registration import Registered, _check_options
    options = _check_options(upsample, max_shift, normalization, window)
    _check_scan_order_mode(order, mode)
    stack, code, shape = _resident_stack(stack, "register_stack_device", floats_only=True)
    shifts = _estimate_shifts_resident(stack, code, shape, reference, options)
    dx, dy = _shift_rows_resident(stack, shifts.shift)
    aligned = scan_noise_device(stack, dx, dy, order=order, mode=mode)
    return Registered(stack_mean_device(aligned), shifts.shift, shifts.peak, aligned if return_aligned else None)


def _gpa_resident(frames, code, shape, options, return_phase, planes=False):
    """``zk_gpa_dev`` on checked operands: ``(maps (4, B, H, W), amp, G, phase or None)`` on the device (and ``H_k`` as
    ``(B, 2, H, W, 2)`` float64 with ``planes``)."""
    g, sigma, reference, window = options
    b, h, w = shape
    maps, amp, g_out = _empty_f64((4, b, h, w), frames), _empty_f64((b, 2, h, w), frames), _empty_f64((b, 2, 2), frames)
    phase = _empty_f64((b, 2, h, w), frames) if return_phase else None
    hk = _empty_f64((b, 2, h, w, 2), frames) if planes else None
    ptr = lambda a: c_void_p(a.data_ptr()) if a is not None else None
    host = lambda a: a.ctypes.data_as(c_void_p) if a is not None else None
    _native.check(_native.load().zk_gpa_dev(frames.device.index, ptr(frames), code, b, h, w, host(g), sigma, window, host(reference), ptr(maps),
                                            ptr(amp), ptr(g_out), ptr(phase), ptr(hk), c_void_p(stream_ptr(frames))), "zk_gpa_dev")
    return (maps, amp, g_out, phase, hk) if planes else (maps, amp, g_out, phase)


def gpa_device(image, g, sigma=None, reference=None, window=None, return_phase=False):
    """:func:`mtflearn_amd.strain.gpa` of a frame or stack resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` or ``(B, H, W)`` of float32 / float64 / uint8 / uint16 / int16; ``g``
    and ``reference`` are host values).  Returns ``GPAResult`` of float64 device arrays of the image's kind, bit for bit the host
    function's numbers, so ``register_stack_device -> gpa_device`` needs no host frame.  Runs on torch's current stream, which
    is synchronised before the call returns (the complex fields are released then).  Like :func:`estimate_shifts_device` it is
    reached as ``resident.gpa_device``."""
    from .strain import _check_image_shape, _check_options, _result
    shape, stack = _check_image_shape(image.shape)
    options = _check_options(g, sigma, reference, window, shape[1:])
    frames, code = _device.resident_frame(image, "gpa_device", ndim=None)
    return _result(*_gpa_resident(frames, code, shape, options, bool(return_phase)), stack)


def denoise_svd_device(image, patch_size, n_components, extraction_step=None, return_s=False):
    """:func:`mtflearn_amd.denoise_svd` of a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).  Returns the float64
    clean frame as a device array of the same kind (and the singular values, a host array, with ``return_s``): the frame and
    the result never cross to the host, only the thin factors of the randomized SVD do.  Runs on torch's current stream."""
    from ._denoise_svd import _check_components, _denoise_svd_device, _svd_arguments
    image = _device.resident_frame(image, "denoise_svd_device")[0]
    patch, _, ii, jj = _svd_arguments(tuple(int(v) for v in image.shape), patch_size, extraction_step)
    n_components = _check_components(n_components)
    clean, s = _denoise_svd_device(image, patch, ii, jj, n_components)
    return (clean, s) if return_s else clean


def denoise_svd_memory_view_device(image, patch_size, n_components=None, threshold=0.9):
    """:func:`mtflearn_amd.denoise.denoise_svd_memory_view` of a frame resident on the GPU (as :func:`denoise_svd_device`).
    Returns ``(recon, explained_variance_ratio, n_components)`` with ``recon`` a float64 device array of the image's kind; the
    ``(p^2, p^2)`` covariance and the eigenvectors are all that crosses to the host and back."""
    from .denoise import _memory_view_device, _memory_view_patch
    image = _device.resident_frame(image, "denoise_svd_memory_view_device")[0]
    p = _memory_view_patch(tuple(int(v) for v in image.shape), patch_size)
    return _memory_view_device(image, p, n_components, threshold)


def gaussian_fit_device(image, points, size, model="elliptical", mode=None, sigma=None, tol=1e-10, max_iter=100):
    """:func:`mtflearn_amd.features.gaussian_fit_points` of a frame and key points resident on the GPU: ``image`` ``(H, W)``
    float32 / float64, ``points`` ``(N, 2)`` int32 or float64 ``(x, y)`` (what :func:`local_max_device`,
    :func:`refine_points_device` or :func:`com_refine_device` return), both torch tensors or both
    :class:`~mtflearn_amd._native.DeviceArray`.  Returns ``(params, iterations, status)`` as device arrays of the same kind:
    ``params`` ``(N, 8)`` float64 with columns ``x, y, amplitude, sigma_major, sigma_minor, theta, background, rss``,
    ``iterations`` and ``status`` ``(N)`` int32 (the codes of the host function).  ``params[:, :2]`` is what
    :func:`vnn_graph_device` and :func:`estimate_d_device` accept (contiguous for a torch tensor after ``.contiguous()``).
    The corner ``rint(point) - size // 2`` is formed on the device and the fit depends on the window alone: a point gives the
    same bits here and through the host function.  There is NO border clearing: every ``size x size`` window must lie inside
    the frame, or ``ValueError`` is raised (the windows are checked on the device: nothing is written for such a point, and
    only the flag crosses to the host) -- the contract of :func:`com_refine_device`.  The options are the host function's and
    are checked before any device call.  Runs on torch's current stream.

    Newer than the move out of :mod:`mtflearn_amd.distributed`: this function is reached as ``resident.gaussian_fit_device``
    and is not part of ``__all__``."""
    from .features.keypoints import gaussian_fit_options
    image, code, points, points_code = _device.resident_frame_points(image, points, "gaussian_fit_device", ("int32", "float64"))
    size, model_code, mask_code, sigma, tol, max_iter = gaussian_fit_options(size, model, mode, sigma, tol, max_iter)
    n = int(points.shape[0])
    h, w = (int(v) for v in image.shape)
    params = _empty_f64((n, 8), image)
    steps, status = _device.empty((n,), np.int32, image), _device.empty((n,), np.int32, image)
    if n:
        rc = _native.load().zk_gauss_fit_points_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, c_void_p(points.data_ptr()),
                                                    points_code, n, size, model_code, mask_code, sigma, tol, max_iter,
                                                    c_void_p(params.data_ptr()), c_void_p(steps.data_ptr()), c_void_p(status.data_ptr()),
                                                    c_void_p(stream_ptr(image)))
        _device.check_refusal(rc, "zk_gauss_fit_points_dev")
    return params, steps, status
