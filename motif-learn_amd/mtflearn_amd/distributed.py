"""Multi-GPU sharding of the Zernike hot path: one process per GPU, one exchange step.

Every output vector depends on one K x K window only, so the path shards with no halo exchange and no
data-path collective: a batch of patches splits into contiguous equal blocks
(:func:`shard_bounds`), a frame into contiguous row bands (the frame itself is small and replicated), a batch
of frames into whole frames.  The only exchange is the all-gather that reassembles the result on every rank.

Layout is chosen so that the gather needs no copy on either side: every rank holds the FULL result array
(``(N, n_poly)``, ``(n_poly, H, W)``, ``(planes, H, W)`` maps or ``(F, n_poly, H, W)``), its kernels write
its own block straight into place (dense kernels through their plane stride), and the collective fills in the
other blocks in place (``zk_allgather_rows``).  The drivers below cut a rank's block into chunks and issue
kernel(c+1) while the transfer of chunk c runs on the communicator's own stream.

Two communicators share one interface:

* :class:`RcclComm` -- the product: ``zk_comm_*`` / ``zk_allgather_rows`` of ``libzernike_hip.so`` on RCCL
  (no ``torch.distributed`` involved; rendezvous through a file, a TCP port, or an id the caller moved).
* :class:`TorchComm` -- a test aid on ``torch.distributed`` (``gloo`` on CPU for the world-size-2 tests and
  for rehearsing the control flow with two ranks on one GPU).

torch is used for device memory and streams only; the arithmetic is ``libzernike_hip.so`` called on raw
device pointers.
"""
from __future__ import annotations

import struct
import warnings
from ctypes import byref, c_int64, c_void_p

import numpy as np

from . import _native

__all__ = ["shard_bounds", "one_gpu_rank_env", "RcclComm", "TorchComm", "DeviceCompute", "patch_moments_device",
           "frame_moments_device", "frame_maps_device", "normalize_image_device", "standardize_image_device",
           "percentile_clip_device", "local_max_device", "points_moments_device", "remove_background_device", "denoise_svd_device",
           "denoise_svd_memory_view_device", "find_regions_device", "voronoi_neighbours_device", "vnn_graph_device", "refine_points_device",
           "com_refine_device", "estimate_d_device", "inverse_transform_device", "sharded_patch_moments", "sharded_frame_moments",
           "sharded_frame_maps", "sharded_frames_moments"]


def shard_bounds(n_units: int, rank: int, world: int):
    """(start, count, padded): rank's contiguous block of ``n_units`` split into ``world`` blocks of
    ``padded = ceil(n_units / world)`` units; trailing ranks may own fewer (or zero) live units."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError("need 0 <= rank < world")
    padded = -(-n_units // world) if n_units > 0 else 0
    start = min(rank * padded, n_units)
    count = min(padded, n_units - start)
    return start, count, padded


def one_gpu_rank_env(rank, base=None):
    """Environment for rank ``rank`` of a REHEARSAL of several RCCL ranks on ONE GPU (a test aid: tests/
    test_gpu_multirank.py, ``bench.py --gpus N`` with ``ZK_BENCH_ONE_DEVICE=1``).  RCCL refuses two ranks of one
    communicator on the same device of the same host ("Duplicate GPU detected"); with a different ``NCCL_HOSTID`` per
    process it takes the ranks for different hosts and connects them through its socket transport on the loopback
    interface.  The data then moves over TCP instead of xGMI -- timings mean nothing -- but every call of the shipped
    collective (``ncclSend`` / ``ncclRecv`` groups, ``ncclAllGather``, ``ncclBroadcast`` as ``zk_allgather_rows``
    issues them) executes in librccl with more than one rank."""
    import os
    env = dict(os.environ if base is None else base)
    env.update(NCCL_HOSTID=f"zk-one-gpu-rank-{rank}", NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1",
               NCCL_SHM_DISABLE="1", NCCL_P2P_DISABLE="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def rccl_debug_env(rank, base=None, directory="/tmp"):
    """Environment additions that make RCCL write, per rank, which transport it connected every channel over
    (``NCCL_DEBUG=INFO`` restricted to the connection subsystems, into a file of this rank's own): what
    :func:`rccl_transport_summary` reads afterwards.  A level below INFO (unset, ``VERSION``, ``WARN`` -- the image exports
    ``VERSION``) is raised to INFO; a caller's ``INFO`` / ``TRACE`` run, its subsystem list and its log file are left alone."""
    import os
    env = {}
    have = os.environ if base is None else base
    if have.get("NCCL_DEBUG", "").upper() not in ("INFO", "TRACE"):
        env["NCCL_DEBUG"] = "INFO"
        if "NCCL_DEBUG_SUBSYS" not in have:
            env["NCCL_DEBUG_SUBSYS"] = "INIT,P2P,NET,SHM"
    if "NCCL_DEBUG_FILE" not in have:
        env["NCCL_DEBUG_FILE"] = os.path.join(directory, f"zk_rccl_{os.getpid()}_rank{rank}.log")
    return env


def rccl_transport_summary(log_text):
    """Channels per transport from an RCCL INFO log: the ``Channel NN : a[dev] -> b[dev] via P2P/IPC`` /
    ``... [send] via NET/Socket/0`` lines librccl prints when it connects a channel.  Returns ``{transport: count}``, e.g.
    ``{"P2P/IPC": 112}`` on an xGMI node or ``{"NET/Socket": 24}`` for ranks that met over sockets."""
    import re
    counts = {}
    for m in re.finditer(r"Channel \d+(?:/\d+)? *: *\d+\[[^\]]*\] *-> *\d+\[[^\]]*\](?: \[(?:send|receive)\])? via ([A-Za-z0-9]+(?:/[A-Za-z]+)?)",
                         log_text):
        counts[m.group(1)] = counts.get(m.group(1), 0) + 1
    return counts


def describe_transport(per_rank_counts, rehearsal=False):
    """One string for the bench line from every rank's ``rccl_transport_summary``: the transports seen, most used first --
    ``"P2P/IPC"`` when every channel of every rank is peer-to-peer (xGMI inside a node), ``"NET/Socket (rehearsal)"``
    for the one-GPU rehearsal, ``"unknown (no channel lines in the RCCL log)"`` when nothing could be parsed."""
    total = {}
    for c in per_rank_counts:
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    if not total:
        return "unknown (no channel lines in the RCCL log)"
    names = " + ".join(k for k, _ in sorted(total.items(), key=lambda kv: -kv[1]))
    return names + (" (rehearsal)" if rehearsal else "")


def _chunk_bounds(padded: int, n_chunks: int):
    """Cut ``[0, padded)`` into at most ``n_chunks`` consecutive non-empty windows (same on every rank)."""
    n_chunks = max(1, min(int(n_chunks), padded)) if padded > 0 else 1
    edges = [padded * c // n_chunks for c in range(n_chunks + 1)]
    return [(edges[c], edges[c + 1]) for c in range(n_chunks) if edges[c + 1] > edges[c]]


def _is_native(array):
    """A :class:`mtflearn_amd._native.DeviceArray` (device memory of the library's own, no torch involved)?"""
    return isinstance(array, _native.DeviceArray)


def _empty_like(shape, like):
    """Uninitialised float64 device array of ``shape`` on ``like``'s device, of ``like``'s kind."""
    if _is_native(like):
        return _native.DeviceArray(shape, np.float64, like.device.index)
    import torch
    return torch.empty(shape, dtype=torch.float64, device=like.device)


def _current_stream_ptr(tensor):
    if _is_native(tensor):
        return 0                                  # the device's default stream
    import torch
    return torch.cuda.current_stream(tensor.device).cuda_stream if tensor.is_cuda else 0


def _is_f64(array):
    if _is_native(array):
        return array.dtype == np.float64
    import torch
    return array.dtype == torch.float64


def _dtype_code(tensor):
    """ZK_F32 / ZK_F64 of a torch tensor or DeviceArray; anything else is an error (the kernels would read it as float64)."""
    if _is_native(tensor):
        if tensor.dtype == np.float32:
            return _native.ZK_F32
        if tensor.dtype == np.float64:
            return _native.ZK_F64
        raise TypeError(f"the device entry points take float32 or float64 arrays, not {tensor.dtype}; convert first "
                        "(ZPs.transform does that for NumPy input)")
    import torch
    if tensor.dtype == torch.float32:
        return _native.ZK_F32
    if tensor.dtype == torch.float64:
        return _native.ZK_F64
    raise TypeError(f"the device entry points take float32 or float64 tensors, not {tensor.dtype}; convert first "
                    "(ZPs.transform does that for NumPy input)")


def _check_operand(plan, tensor, what):
    if not tensor.is_cuda:
        raise ValueError(f"{what} must live on the GPU")
    if not tensor.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if tensor.device.index != plan.device:
        raise ValueError(f"{what} is on cuda:{tensor.device.index} but the plan was created on device {plan.device}: "
                         "create the plan on the tensor's device (MTFLEARN_AMD_DEVICE / ZPs.to_device)")


# ---------------------------------------------------------------------------------------------------------
# single-GPU device entry points on torch tensors
# ---------------------------------------------------------------------------------------------------------
def patch_moments_device(plan: "_native.Plan", patches, out=None):
    """Run the batch kernel on a CUDA/HIP torch tensor ``(N, K, K)`` (float32/float64) on torch's
    current stream; returns the ``(N, n_poly)`` float64 tensor (no host copies)."""
    _check_operand(plan, patches, "patches")
    code = _dtype_code(patches)
    n = patches.shape[0]
    if out is None:
        out = _empty_like((n, plan.n_poly), patches)
    else:
        _check_operand(plan, out, "out")
    plan.transform_patches_dev(patches.data_ptr(), code, n, out.data_ptr(), _current_stream_ptr(patches))
    return out


def frame_moments_device(plan: "_native.Plan", image, row0=0, n_rows=None, out=None, full=None):
    """Run the dense kernel for output rows ``[row0, row0+n_rows)`` of a CUDA/HIP torch frame ``(H, W)``.
    Returns ``(n_poly, n_rows, W)`` float64 -- or, with ``full`` (an ``(n_poly, H, W)`` tensor), writes the
    band in place into it and returns ``full``."""
    _check_operand(plan, image, "image")
    code = _dtype_code(image)
    h, w = image.shape
    n_rows = h - row0 if n_rows is None else n_rows
    stream = _current_stream_ptr(image)
    if full is not None:
        _check_operand(plan, full, "full")
        assert tuple(full.shape) == (plan.n_poly, h, w) and _is_f64(full)
        plan.transform_frame_dev(image.data_ptr(), code, h, w, row0, n_rows, full.data_ptr() + row0 * w * 8, stream,
                                 plane_stride=h * w)
        return full
    if out is None:
        out = _empty_like((plan.n_poly, n_rows, w), image)
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
    code = _dtype_code(image)
    h, w = image.shape
    n_rows = h - row0 if n_rows is None else n_rows
    stream = _current_stream_ptr(image)
    if full is not None:
        ptr = lambda t: t.data_ptr() + row0 * w * 8 if t is not None else 0
        plan.frame_maps_dev(image.data_ptr(), code, h, w, row0, n_rows, folds if full[0] is not None else None,
                            m_unselect, p, theta if full[2] is not None else None, ptr(full[0]), ptr(full[1]),
                            ptr(full[2]), stream, plane_stride=h * w)
        return full
    mk = lambda planes: _empty_like((planes, n_rows, w), image)
    rot = mk(len(folds)) if folds is not None and len(folds) else None
    ab = mk(n_complex) if want_abs else None
    mir = _empty_like((n_rows, w), image) if theta is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    plan.frame_maps_dev(image.data_ptr(), code, h, w, row0, n_rows, folds, m_unselect, p, theta,
                        ptr(rot), ptr(ab), ptr(mir), stream)
    return rot, ab, mir


def _image_code(image):
    """ZK_* code of a 2-D device image for ``zk_local_max_dev`` and ``zk_background_*_dev``: the two float types and the narrow detector formats."""
    if _is_native(image):
        code = _native.dtype_code(image.dtype)
        name = image.dtype
    else:
        import torch
        code = {torch.float32: _native.ZK_F32, torch.float64: _native.ZK_F64, torch.uint8: _native.ZK_U8,
                torch.int16: _native.ZK_I16, getattr(torch, "uint16", None): _native.ZK_U16}.get(image.dtype)
        name = image.dtype
    if code is None:
        raise TypeError(f"device images must be float32, float64, uint8, uint16 or int16, not {name}")
    return code


def _numpy_dtype(image):
    if _is_native(image):
        return image.dtype
    import torch
    return {torch.float32: np.float32, torch.float64: np.float64, torch.uint8: np.uint8, torch.int16: np.int16,
            getattr(torch, "uint16", None): np.uint16}[image.dtype]


def _empty_points(n, like):
    if _is_native(like):
        return _native.DeviceArray((n, 2), np.int32, like.device.index)
    import torch
    return torch.empty((n, 2), dtype=torch.int32, device=like.device)


def local_max_device(image, min_distance, threshold=None):
    """:func:`mtflearn_amd.features.local_max` of a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).  Returns the
    ``(N, 2)`` int32 ``(x, y)`` points as a device array of the same kind, in the layout :func:`points_moments_device`
    reads: the frame never crosses to the host, only the point count does.  Runs on torch's current stream."""
    from .features.peaks import _check_distance, _comparison_threshold
    if len(image.shape) != 2:
        raise ValueError(f"local_max_device needs a 2D image, not {len(image.shape)}-D")
    if not image.is_cuda:
        raise ValueError("image must live on the GPU")
    if not _is_native(image) and not image.is_contiguous():
        image = image.contiguous()
    code = _image_code(image)
    r = _check_distance(min_distance)
    has_t, t = (0, 0.0) if threshold is None else (1, _comparison_threshold(_numpy_dtype(image), threshold))
    h, w = (int(v) for v in image.shape)
    lib = _native.load()
    stream = c_void_p(_current_stream_ptr(image))
    capacity = max(1024, h * w // 8)                   # kept points of a real frame: a few % of its pixels
    out = _empty_points(capacity, image)
    n = c_int64()
    for _ in range(2):                                  # the second pass only when the first guess was short
        _native.check(lib.zk_local_max_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, r, has_t, t,
                                           c_void_p(out.data_ptr()), capacity, byref(n), stream), "zk_local_max_dev")
        if n.value <= capacity:
            break
        capacity = n.value
        out = _empty_points(capacity, image)
    n = n.value
    return out[:n]


def points_moments_device(plan: "_native.Plan", image, points, out=None):
    """Moments of the windows centred on device-resident key points (``zk_transform_points_dev``): ``image`` an
    ``(H, W)`` float32 / float64 frame, ``points`` ``(N, 2)`` int32 ``(x, y)`` (what :func:`local_max_device` returns),
    both torch tensors or both :class:`~mtflearn_amd._native.DeviceArray`.  Returns the ``(N, n_poly)`` float64 moments
    on the device -- ``ZPs.transform_at(frame, points)`` with neither the frame nor the points crossing PCIe."""
    _check_operand(plan, image, "image")
    _check_operand(plan, points, "points")
    code = _dtype_code(image)
    if len(points.shape) != 2 or points.shape[1] != 2 or points.element_size() != 4 or not (
            points.dtype == np.int32 if _is_native(points) else str(points.dtype) == "torch.int32"):
        raise TypeError("points must be an (N, 2) int32 array of (x, y)")
    h, w = image.shape
    n = int(points.shape[0])
    if out is None:
        out = _empty_like((n, plan.n_poly), image)
    else:
        _check_operand(plan, out, "out")
        assert tuple(out.shape) == (n, plan.n_poly) and _is_f64(out)
    if n:
        plan.transform_points_dev(image.data_ptr(), code, h, w, points.data_ptr(), n, out.data_ptr(), _current_stream_ptr(image))
    return out


def _empty_image(shape, dtype, like):
    """Uninitialised device array of ``shape`` and NumPy ``dtype`` on ``like``'s device, of ``like``'s kind."""
    if _is_native(like):
        return _native.DeviceArray(shape, dtype, like.device.index)
    import torch
    tdtype = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8,
              np.dtype(np.int16): torch.int16, np.dtype(np.uint16): getattr(torch, "uint16", None),
              np.dtype(np.int64): torch.int64}[np.dtype(dtype)]
    return torch.empty(shape, dtype=tdtype, device=like.device)


def remove_background_device(image, method, parameter, clip=True, **method_kw):
    """:mod:`mtflearn_amd.background` on a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).

    ``method``: ``"opening"`` (``parameter`` = size), ``"rolling_ball"`` (radius) or ``"baseline"`` (sigma; ``num_iters``
    as a keyword, default 10).  Returns ``(residual, background)`` as device arrays of the image's kind, in the image's dtype
    (float64 for the baseline), the same numbers as the host ``remove_background_*``.  Runs on torch's current stream and no
    pixel crosses to the host, so a frame goes to :func:`local_max_device` and :func:`points_moments_device` without PCIe."""
    from .background import _method_parameter
    if len(image.shape) != 2:
        raise ValueError("image must be a 2D array.")
    param = _method_parameter(method, parameter, method_kw)
    if not image.is_cuda:
        raise ValueError("image must live on the GPU")
    if not _is_native(image) and not image.is_contiguous():
        image = image.contiguous()
    code = _image_code(image)
    h, w = (int(v) for v in image.shape)
    out_dtype = np.float64 if method == "baseline" else _numpy_dtype(image)
    background = _empty_image((h, w), out_dtype, image)
    residual = _empty_image((h, w), out_dtype, image)
    lib = _native.load()
    args = (image.device.index, c_void_p(image.data_ptr()), code, h, w)
    outs = (int(bool(clip)), c_void_p(background.data_ptr()), c_void_p(residual.data_ptr()), c_void_p(_current_stream_ptr(image)))
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
    if not image.is_cuda:
        raise ValueError("image must live on the GPU")
    if not _is_native(image) and not image.is_contiguous():
        image = image.contiguous()
    return _Operand(image, _current_stream_ptr(image))


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
    _dtype_code(frame_dev)
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
    if like is None or _is_native(like):
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
        operand = _Operand(img, _current_stream_ptr(img))
        vmax = float(_stats(operand)[1])
        if vmax > 0.0:
            # x / vmax in float64 rounded once is the float32 quotient: 53 bits are more than 2 * 24 + 2
            img = _map(operand, _native.MAP_DIVIDE, [vmax])
    return img


def _as_dtype_device(array, np_dtype, what):
    """``array`` as a contiguous device array of ``np_dtype``: a torch tensor is converted on the device, a DeviceArray must
    already have the type."""
    if not array.is_cuda:
        raise ValueError(f"{what} must live on the GPU")
    if _is_native(array):
        if array.dtype != np_dtype:
            raise TypeError(f"{what} must be a {np.dtype(np_dtype).name} DeviceArray, not {array.dtype}")
        return array
    import torch
    return array.to({np.float64: torch.float64, np.int64: torch.int64}[np_dtype]).contiguous()


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
    if not _is_native(edges) and (edges.dtype.is_floating_point or edges.dtype.is_complex or str(edges.dtype) == "torch.bool"):
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
    device, stream = points.device.index, c_void_p(_current_stream_ptr(points))
    state, counts = c_void_p(), (c_int64 * 3)()
    _native.check(lib.zk_find_regions_dev(device, c_void_p(points.data_ptr()), n, c_void_p(edges.data_ptr()), e, byref(state), counts,
                                          None, None, None, None, None, stream), "zk_find_regions_dev")
    f, v, a = (int(c) for c in counts)
    offsets, vertices, ks = (_empty_image(shape, np.int64, points) for shape in ((f + 1,), (v,), (f,)))
    centers, adjacency = _empty_like((f, 2), points), _empty_image((a, 2), np.int64, points)
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
    if _is_native(points):
        if points.dtype not in (np.float64, np.int32):
            raise TypeError(f"points must be a float64 or int32 DeviceArray, not {points.dtype}")
        code = _native.ZK_F64 if points.dtype == np.float64 else _native.ZK_I32
    else:
        import torch
        if points.dtype.is_complex or points.dtype == torch.bool:
            raise ValueError(f"points must be real numbers, not {points.dtype}")
        if points.dtype not in (torch.float64, torch.int32):
            points = points.to(torch.float64)
        points = points.contiguous()
        code = _native.ZK_F64 if points.dtype == torch.float64 else _native.ZK_I32
    if int(points.shape[0]) + spare >= 2 ** 26:
        raise ValueError(f"{what} needs len(points) < 2^26" + (f" - {spare}" if spare else ""))
    return points, code


def _voronoi_device(points, pad, mode, dmax, threshold, stream, what):
    """Both phases of ``zk_voronoi_cells_dev`` on resident points; returns ``(ijs, ridge, edge)`` of the points' kind."""
    points, code = _resident_points(points, what, spare=4)
    if not (np.isfinite(pad) and pad > 0):
        raise ValueError(f"pad must be positive and finite, not {pad}")
    n = int(points.shape[0])
    lengths = mode == _native.VORONOI_NEIGHBOURS
    if n == 0:
        return _empty_image((0, 2), np.int64, points), _empty_like((0,), points), _empty_like((0,), points)
    lib = _native.load()
    device = points.device.index
    if stream is None:
        stream = _current_stream_ptr(points)
    stream = c_void_p(int(getattr(stream, "cuda_stream", stream)))
    state, counts = c_void_p(), (c_int64 * 1)()
    _native.check(lib.zk_voronoi_cells_dev(device, c_void_p(points.data_ptr()), code, n, pad, mode, dmax, threshold, byref(state), counts,
                                           None, None, None, stream), "zk_voronoi_cells_dev")
    m = int(counts[0])
    ijs = _empty_image((m, 2), np.int64, points)
    ridge, edge = (_empty_like((m,), points), _empty_like((m,), points)) if lengths else (None, None)
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
    device, stream = points.device.index, _current_stream_ptr(points)
    dd = _empty_like((n, graph.KNN), points)
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
    if len(image.shape) != 2:
        raise ValueError(f"refine_points_device needs a 2D image, not {len(image.shape)}-D")
    if not image.is_cuda or not points.is_cuda:
        raise ValueError("image and points must live on the GPU")
    if _is_native(image) != _is_native(points) or image.device.index != points.device.index:
        raise ValueError("image and points must be of one kind and on one device")
    try:
        code = _dtype_code(image)
    except TypeError as e:
        raise ValueError(f"refine_points_device needs a float frame: {e}") from None
    if len(points.shape) != 2 or points.shape[1] != 2 or not (
            points.dtype == np.int32 if _is_native(points) else str(points.dtype) == "torch.int32"):
        raise TypeError("points must be an (N, 2) int32 array of (x, y)")
    if not _is_native(image):
        image, points = image.contiguous(), points.contiguous()
    size = int(size)
    if not 0 <= size <= 64:
        raise ValueError(f"size must be in [0, 64], not {size}")
    n = int(points.shape[0])
    if n >= 2 ** 24:
        raise ValueError("refine_points_device needs len(points) < 2^24 (the reference's label image has the frame's type)")
    h, w = (int(v) for v in image.shape)
    out = _empty_like((n, 2), image)
    if n:
        lib = _native.load()
        rc = lib.zk_refine_points_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, c_void_p(points.data_ptr()), n, size,
                                      _native.REFINE_DISK if mode == 'disk' else _native.REFINE_BOX, c_void_p(out.data_ptr()),
                                      c_void_p(_current_stream_ptr(image)))
        if rc == _native.ZK_E_BADARG:
            raise ValueError(_native.last_error())
        _native.check(rc, "zk_refine_points_dev")
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
    if len(image.shape) != 2:
        raise ValueError(f"com_refine_device needs a 2D image, not {len(image.shape)}-D")
    if not image.is_cuda or not points.is_cuda:
        raise ValueError("image and points must live on the GPU")
    if _is_native(image) != _is_native(points) or image.device.index != points.device.index:
        raise ValueError("image and points must be of one kind and on one device")
    try:
        code = _dtype_code(image)
    except TypeError as e:
        raise ValueError(f"com_refine_device needs a float frame: {e}") from None
    kind = str(points.dtype).replace("torch.", "")
    if len(points.shape) != 2 or points.shape[1] != 2 or kind not in ("int32", "float64"):
        raise TypeError("points must be an (N, 2) int32 or float64 array of (x, y)")
    if not _is_native(image):
        image, points = image.contiguous(), points.contiguous()
    if int(size) != size or not 2 <= int(size) <= 64:
        raise ValueError(f"size must be an integer in [2, 64], not {size}")
    n = int(points.shape[0])
    if n >= 2 ** 24:
        raise ValueError("com_refine_device needs len(points) < 2^24")
    h, w = (int(v) for v in image.shape)
    out = _empty_like((n, 2), image)
    if n:
        rc = _native.load().zk_com_refine_points_dev(image.device.index, c_void_p(image.data_ptr()), code, h, w, c_void_p(points.data_ptr()),
                                                     _native.ZK_I32 if kind == "int32" else _native.ZK_F64, n, int(size),
                                                     _native.THRESHOLD_OTSU if threshold == 'otsu' else _native.THRESHOLD_LI,
                                                     c_void_p(out.data_ptr()), c_void_p(_current_stream_ptr(image)))
        if rc == _native.ZK_E_BADARG:
            raise ValueError(_native.last_error())
        _native.check(rc, "zk_com_refine_points_dev")
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
    if len(coeffs_dev.shape) != 2 or coeffs_dev.shape[1] != len(zps.n) or not _is_f64(coeffs_dev):
        raise ValueError(f"coeffs_dev must be an (N, {len(zps.n)}) float64 matrix of real Zernike moments")
    n_rows = int(coeffs_dev.shape[0] if n_rows is None else n_rows)
    if not 0 <= n_rows <= coeffs_dev.shape[0]:
        raise ValueError(f"n_rows must be between 0 and {coeffs_dev.shape[0]}")
    np_dtype = zps._inverse_dtype(dtype)
    entry = zps._synthesis_entry(method, m_select)
    if entry["cond"] is not None and entry["cond"] > zps._COND_LIMIT:
        warnings.warn(zps._cond_message(entry["cond"]), UserWarning, stacklevel=2)
    shape = (n_rows, zps.size, zps.size)
    if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or _numpy_dtype(out) != np_dtype
                            or out.device.index != coeffs_dev.device.index):
        raise ValueError(f"out must be a contiguous {shape} array of {np_dtype} on the device of coeffs_dev")
    if coeffs_dev.device.index != zps._pick_device():
        raise ValueError(f"coeffs_dev is on cuda:{coeffs_dev.device.index} but this ZPs computes on device {zps._pick_device()}: "
                         "bind it to the array's device (ZPs.to_device / MTFLEARN_AMD_DEVICE)")
    if out is None:
        out = _empty_image(shape, np_dtype, coeffs_dev)
    if n_rows == 0:
        return out
    synth = zps._synthesis_device(entry)
    synth.apply_dev(coeffs_dev.data_ptr(), n_rows, out.data_ptr(), _native.dtype_code(np_dtype), _current_stream_ptr(coeffs_dev))
    return out


def _device_frame(image, what):
    if len(image.shape) != 2:
        raise ValueError(f"{what} needs a 2D image, not {len(image.shape)}-D")
    if not image.is_cuda:
        raise ValueError("image must live on the GPU")
    if not _is_native(image) and not image.is_contiguous():
        image = image.contiguous()
    _image_code(image)
    return image


def denoise_svd_device(image, patch_size, n_components, extraction_step=None, return_s=False):
    """:func:`mtflearn_amd.denoise_svd` of a frame resident on the GPU (a torch tensor or a
    :class:`~mtflearn_amd._native.DeviceArray`, ``(H, W)`` of float32 / float64 / uint8 / uint16 / int16).  Returns the float64
    clean frame as a device array of the same kind (and the singular values, a host array, with ``return_s``): the frame and
    the result never cross to the host, only the thin factors of the randomized SVD do.  Runs on torch's current stream."""
    from ._denoise_svd import _check_components, _denoise_svd_device, _svd_arguments
    image = _device_frame(image, "denoise_svd_device")
    patch, _, ii, jj = _svd_arguments(tuple(int(v) for v in image.shape), patch_size, extraction_step)
    n_components = _check_components(n_components)
    clean, s = _denoise_svd_device(image, patch, ii, jj, n_components)
    return (clean, s) if return_s else clean


def denoise_svd_memory_view_device(image, patch_size, n_components=None, threshold=0.9):
    """:func:`mtflearn_amd.denoise.denoise_svd_memory_view` of a frame resident on the GPU (as :func:`denoise_svd_device`).
    Returns ``(recon, explained_variance_ratio, n_components)`` with ``recon`` a float64 device array of the image's kind; the
    ``(p^2, p^2)`` covariance and the eigenvectors are all that crosses to the host and back."""
    from .denoise import _memory_view_device, _memory_view_patch
    image = _device_frame(image, "denoise_svd_memory_view_device")
    p = _memory_view_patch(tuple(int(v) for v in image.shape), patch_size)
    return _memory_view_device(image, p, n_components, threshold)


# ---------------------------------------------------------------------------------------------------------
# communicators
# ---------------------------------------------------------------------------------------------------------
class RcclComm:
    """This process's endpoint of the RCCL communicator inside ``libzernike_hip.so`` (``zk_comm_*``).

    ``RcclComm(device, rank, world, path=...)`` (ranks of one node meet through a file), ``port=`` (TCP) or
    ``unique_id=``; see :class:`mtflearn_amd._native.Comm`."""

    def __init__(self, device, rank, world, **rendezvous):
        self._c = _native.Comm(device, rank, world, **rendezvous)
        self.rank, self.world, self.device = self._c.rank, self._c.world, self._c.device

    def allgather_rows(self, full, n_planes, height, width, rows_per_rank, row_off, n_rows, stream=0):
        if not full.is_cuda or full.device.index != self.device or not full.is_contiguous():
            raise ValueError("the gathered array must be a contiguous tensor on the communicator's device")
        if full.element_size() != 8 or full.numel() != n_planes * height * width:
            raise ValueError("the gathered array must hold n_planes * height * width float64 values")
        self._c.allgather_rows(full.data_ptr(), n_planes, height, width, rows_per_rank, row_off, n_rows, stream)

    def join(self, stream=0):
        self._c.join(stream)

    def ranks_seen(self):
        return self._c.ranks_seen()

    def allgather_host(self, payload: bytes):
        return self._c.allgather_host(payload)

    def max_over_ranks(self, value: float) -> float:
        return max(struct.unpack("d", b)[0] for b in self.allgather_host(struct.pack("d", float(value))))

    def barrier(self):
        self.allgather_host(b"\0")

    def close(self):
        self._c.close()


class TorchComm:
    """Same interface on ``torch.distributed`` -- a TEST AID (``gloo`` on CPU tensors for the world-size-2 / 3
    tests, ``gloo`` with GPU tensors staged through the host to rehearse several ranks on one GPU).  Blocking;
    ``stream`` is ignored.  ``allgather_rows`` executes the SAME schedule as the product: the list
    ``zk_allgather_rows_plan`` returns for this rank (the planner half of ``zk_allgather_rows``), entry by entry,
    with ``isend`` / ``irecv`` / ``broadcast`` / ``all_gather_into_tensor`` standing in for the RCCL calls and a
    wait at every group boundary -- so an error in the window arithmetic, in the pairing of sends and receives or
    in their order (gloo, like RCCL, matches point-to-point messages between two ranks in issue order) fails the
    gloo tests.  ``algo``: ``"p2p" | "allgather" | "bcast"`` as ``ZK_COMM_ALGO`` (default: the environment's)."""

    def __init__(self, group=None, algo=None):
        import os
        import torch.distributed as dist
        self._dist, self._group = dist, group
        self.rank, self.world = dist.get_rank(group), dist.get_world_size(group)
        self.algo = _native.COMM_ALGOS.get(os.environ.get("ZK_COMM_ALGO", "") if algo is None else algo, _native.COMM_AUTO)
        self.calls = 0          # RCCL-call stand-ins executed so far (tests read it)

    def _global(self, r):
        return r if self._group is None else self._dist.get_global_rank(self._group, r)

    def allgather_rows(self, full, n_planes, height, width, rows_per_rank, row_off, n_rows, stream=0):
        import torch
        dist = self._dist
        plan = _native.allgather_rows_plan(self.rank, self.world, n_planes, height, width, rows_per_rank, row_off,
                                           n_rows, self.algo)
        if not plan:
            return
        if full.numel() != n_planes * height * width or not full.is_contiguous():
            raise ValueError("the gathered array must be contiguous and hold n_planes * height * width values")
        on_gpu = full.is_cuda
        if on_gpu:
            torch.cuda.current_stream(full.device).synchronize()
        flat = full.view(-1)
        pending, landed = [], []       # requests of the open group; (host buffer, offset) pairs to copy back to the GPU

        def run(seg):                  # the tensor gloo works on: the run itself (CPU) or a host copy of it (GPU)
            return seg.cpu() if on_gpu else seg

        def flush():
            for req in pending:
                req.wait()
            pending.clear()
            for buf, off in landed:
                flat[off:off + buf.numel()].copy_(buf)
            landed.clear()

        group_now = plan[0][2]
        for op, peer, group, _plane, off, cnt in plan:
            if group != group_now:
                flush()
                group_now = group
            seg = flat[off:off + cnt]
            self.calls += 1
            if op == _native.XFER_SEND:
                pending.append(dist.isend(run(seg), self._global(peer), group=self._group))
            elif op == _native.XFER_RECV:
                buf = torch.empty(cnt, dtype=full.dtype) if on_gpu else seg
                pending.append(dist.irecv(buf, self._global(peer), group=self._group))
                if on_gpu:
                    landed.append((buf, off))
            elif op == _native.XFER_BCAST:
                flush()                # a collective does not overtake the point-to-point calls issued before it
                buf = run(seg)
                dist.broadcast(buf, src=self._global(peer), group=self._group)
                if on_gpu and peer != self.rank:
                    seg.copy_(buf)
            else:                      # XFER_ALLGATHER: send = own block, receive = the run of all blocks around it
                flush()
                base = off - self.rank * cnt
                out = torch.empty(cnt * self.world, dtype=full.dtype)
                dist.all_gather_into_tensor(out, run(seg).clone(), group=self._group)
                flat[base:base + cnt * self.world].copy_(out)
        flush()

    def join(self, stream=0):
        pass

    def allgather_host(self, payload: bytes):
        out = [None] * self.world
        self._dist.all_gather_object(out, payload, group=self._group)
        return out

    def max_over_ranks(self, value: float) -> float:
        return max(struct.unpack("d", b)[0] for b in self.allgather_host(struct.pack("d", float(value))))

    def barrier(self):
        self._dist.barrier(group=self._group)

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------------------
# what a driver asks of "the kernels": the product adapter calls libzernike_hip.so; the CPU tests plug in
# an oracle-backed stand-in with the same four methods (tests/test_distributed_cpu.py)
# ---------------------------------------------------------------------------------------------------------
class DeviceCompute:
    def __init__(self, plan: "_native.Plan"):
        self.plan, self.n_poly = plan, plan.n_poly

    def empty(self, shape, like):
        return _empty_like(shape, like)

    def stream(self, tensor):
        return _current_stream_ptr(tensor)

    def patches(self, patches, out_rows):
        patch_moments_device(self.plan, patches, out=out_rows)

    def frame_band(self, image, row0, n_rows, full):
        frame_moments_device(self.plan, image, row0=row0, n_rows=n_rows, full=full)

    def frame(self, image, out):
        frame_moments_device(self.plan, image, out=out)

    def maps_band(self, image, row0, n_rows, full, n_complex, folds, m_unselect, p, theta):
        frame_maps_device(self.plan, image, n_complex, folds=folds, m_unselect=m_unselect, p=p, theta=theta,
                          row0=row0, n_rows=n_rows, full=full)


def _as_compute(plan_or_compute):
    return plan_or_compute if hasattr(plan_or_compute, "frame_band") else DeviceCompute(plan_or_compute)


# ---------------------------------------------------------------------------------------------------------
# sharded drivers: kernel(chunk c+1) overlaps the transfer of chunk c; every rank ends with the full result
# ---------------------------------------------------------------------------------------------------------
def sharded_patch_moments(plan, comm, patches_local, n_total, out=None, n_chunks=4):
    """Batch of ``n_total`` patches split into the blocks of :func:`shard_bounds`; ``patches_local`` is this
    rank's block ``(count, K, K)``.  Returns the full ``(n_total, n_poly)`` float64 matrix on every rank."""
    compute = _as_compute(plan)
    start, count, padded = shard_bounds(n_total, comm.rank, comm.world)
    if patches_local.shape[0] != count:
        raise ValueError(f"rank {comm.rank} owns {count} of {n_total} patches, got {patches_local.shape[0]}")
    full = compute.empty((n_total, compute.n_poly), patches_local) if out is None else out
    stream = compute.stream(full)
    for c0, c1 in _chunk_bounds(padded, n_chunks):
        lo, hi = min(c0, count), min(c1, count)
        if hi > lo:
            compute.patches(patches_local[lo:hi], full[start + lo:start + hi])
        comm.allgather_rows(full, 1, n_total, compute.n_poly, padded, c0, c1 - c0, stream)
    comm.join(stream)
    return full


def sharded_frame_moments(plan, comm, image, out=None, n_chunks=4):
    """Dense transform of one frame (replicated on every rank -- it is small): rank r computes the row band
    ``shard_bounds(H, r, world)`` in place into the full ``(n_poly, H, W)`` array, sub-band by sub-band, each
    gathered while the next one is computed."""
    compute = _as_compute(plan)
    h, w = image.shape
    start, count, padded = shard_bounds(h, comm.rank, comm.world)
    full = compute.empty((compute.n_poly, h, w), image) if out is None else out
    stream = compute.stream(full)
    for c0, c1 in _chunk_bounds(padded, n_chunks):
        lo, hi = min(c0, count), min(c1, count)
        if hi > lo:
            compute.frame_band(image, start + lo, hi - lo, full)
        comm.allgather_rows(full, compute.n_poly, h, w, padded, c0, c1 - c0, stream)
    comm.join(stream)
    return full


def sharded_frame_maps(plan, comm, image, n_complex, folds=(2, 3, 4, 6), m_unselect=(0, 1), p=2, theta=None,
                       want_abs=True, n_chunks=4, out=None):
    """configs[4]: frame -> fused symmetry maps, row bands sharded, the maps (not the moments) gathered:
    ``len(folds) + n_complex + 1`` planes instead of ``n_poly``.  Returns ``(rot, abs, mirror)`` whole-frame
    tensors (``None`` where not requested) on every rank; ``out = (rot, abs, mirror)`` supplies them."""
    compute = _as_compute(plan)
    h, w = image.shape
    start, count, padded = shard_bounds(h, comm.rank, comm.world)
    n_folds = len(folds) if folds is not None else 0
    if out is not None:
        rot, ab, mir = out
    else:
        rot = compute.empty((n_folds, h, w), image) if n_folds else None
        ab = compute.empty((n_complex, h, w), image) if want_abs else None
        mir = compute.empty((h, w), image) if theta is not None else None
    full = (rot, ab, mir)
    stream = compute.stream(image)
    for c0, c1 in _chunk_bounds(padded, n_chunks):
        lo, hi = min(c0, count), min(c1, count)
        if hi > lo:
            compute.maps_band(image, start + lo, hi - lo, full, n_complex, folds, m_unselect, p, theta)
        for t in full:
            if t is not None:
                comm.allgather_rows(t, t.numel() // (h * w), h, w, padded, c0, c1 - c0, stream)
    comm.join(stream)
    return full


def sharded_frames_moments(plan, comm, frames_local, n_frames, out=None):
    """configs[3]: a batch of ``n_frames`` frames sharded by whole frames (``frames_local``: this rank's
    ``(count, H, W)`` block).  Frame i of every rank is transformed, then gathered while frame i+1 is
    computed; returns the full ``(n_frames, n_poly, H, W)`` array on every rank."""
    compute = _as_compute(plan)
    start, count, padded = shard_bounds(n_frames, comm.rank, comm.world)
    if frames_local.shape[0] != count:
        raise ValueError(f"rank {comm.rank} owns {count} of {n_frames} frames, got {frames_local.shape[0]}")
    h, w = frames_local.shape[1:]
    full = compute.empty((n_frames, compute.n_poly, h, w), frames_local) if out is None else out
    stream = compute.stream(full)
    for i in range(padded):
        if i < count:
            compute.frame(frames_local[i], full[start + i])
        comm.allgather_rows(full, 1, n_frames, compute.n_poly * h * w, padded, i, 1, stream)
    comm.join(stream)
    return full
