"""The one adapter over "a torch tensor or a :class:`~mtflearn_amd._native.DeviceArray`": what every resident entry point
(:mod:`mtflearn_amd.resident`) and every module that feeds one asks of a device operand -- its element type, a new array of
its kind on its device, its stream, a copy to or from the host -- and the operand checks those entry points share.

It imports :mod:`mtflearn_amd._native` and NumPy only (torch lazily, and only for a torch operand), so any module of the
package imports it at the top.  A type outside the table below is an error everywhere: no kernel may read it as float64.
"""
from __future__ import annotations

import numpy as np

from . import _native

# NumPy dtype, name of the torch dtype, ZK_* code (int64 is a result type only: no kernel takes it as an operand)
_TABLE = (
    (np.float32, "float32", _native.ZK_F32),
    (np.float64, "float64", _native.ZK_F64),
    (np.uint8, "uint8", _native.ZK_U8),
    (np.uint16, "uint16", _native.ZK_U16),
    (np.int16, "int16", _native.ZK_I16),
    (np.int32, "int32", _native.ZK_I32),
    (np.int64, "int64", None),
)
_NP_OF = {name: np.dtype(dtype) for dtype, name, _ in _TABLE}
_CODE_OF = {name: code for _, name, code in _TABLE}
_NAME_OF = {np.dtype(dtype): name for dtype, name, _ in _TABLE}

FLOATS = ("float32", "float64")                         # what the moment, refine and render kernels read
IMAGES = FLOATS + ("uint8", "uint16", "int16")          # ... and the narrow detector formats of the image kernels


def is_native(array):
    """A :class:`mtflearn_amd._native.DeviceArray` (device memory of the library's own, no torch involved)?"""
    return isinstance(array, _native.DeviceArray)


def _name(array):
    """The table's name of the array's element type, or None."""
    if is_native(array):
        return _NAME_OF.get(array.dtype)
    name = str(array.dtype)[6:]                         # "torch.float32"
    return name if name in _NP_OF else None


def np_dtype(array):
    """NumPy dtype of a device array of either kind; None for a type outside the table."""
    return _NP_OF.get(_name(array))


def code(array, allowed=IMAGES):
    """ZK_* code of a device array of either kind whose type is one of ``allowed`` (:data:`FLOATS`, :data:`IMAGES` or another
    tuple of the table's names); anything else is a ``TypeError`` -- the kernels would read it as float64."""
    name = _name(array)
    if name not in allowed:
        raise TypeError(f"device images must be {', '.join(allowed[:-1])} or {allowed[-1]}, not {array.dtype}; convert first "
                        "(ZPs.transform does that for NumPy input)")
    return _CODE_OF[name]


def empty(shape, dtype, like):
    """Uninitialised device array of ``shape`` and NumPy ``dtype`` on ``like``'s device, of ``like``'s kind."""
    name = _NAME_OF[np.dtype(dtype)]
    if is_native(like):
        return _native.DeviceArray(shape, _NP_OF[name], like.device.index)
    import torch
    return torch.empty(shape, dtype=getattr(torch, name), device=like.device)        # torch before 2.3 has no uint16


def stream_ptr(array):
    """The stream work on ``array`` is enqueued on: torch's current one of its device, the default one for a DeviceArray."""
    if is_native(array):
        return 0
    import torch
    return torch.cuda.current_stream(array.device).cuda_stream if array.is_cuda else 0


def to_host(array):
    """A host copy of a device array of either kind."""
    return array.numpy() if is_native(array) else array.cpu().numpy()


def from_host(array, like):
    """Host array -> float64 device array of ``like``'s kind on its device (torch: on the current stream)."""
    array = np.ascontiguousarray(array, dtype=np.float64)
    if is_native(like):
        return _native.DeviceArray.from_numpy(array, like.device.index)
    import torch
    return torch.from_numpy(array).to(like.device)


def resident_frame(image, what, floats_only=False, ndim=2):
    """``(image, ZK_* code)`` of the image operand of the entry point ``what``: ``ndim``-D (None: any rank), on the GPU, of one
    of :data:`IMAGES` (:data:`FLOATS` with ``floats_only``); a torch tensor is made contiguous on the device."""
    if ndim is not None and len(image.shape) != ndim:
        raise ValueError(f"{what} needs a {ndim}D image, not {len(image.shape)}-D")
    if not image.is_cuda:
        raise ValueError("image must live on the GPU")
    if not is_native(image) and not image.is_contiguous():
        image = image.contiguous()
    return image, code(image, FLOATS if floats_only else IMAGES)


def points_code(points, allowed=("int32",)):
    """ZK_* code of ``(N, 2)`` key points whose type is one of ``allowed`` (``("int32",)`` or ``("int32", "float64")``)."""
    name = _name(points)
    if len(points.shape) != 2 or points.shape[1] != 2 or name not in allowed:
        raise TypeError(f"points must be an (N, 2) {' or '.join(allowed)} array of (x, y), not {tuple(points.shape)} {points.dtype}")
    return _CODE_OF[name]


def resident_frame_points(image, points, what, allowed=("int32",)):
    """``(image, frame code, points, points code)`` of the operands of the refine entry point ``what``: a 2-D float frame and
    ``(N, 2)`` points of a type in ``allowed``, both on the GPU, of one kind and on one device, ``N < 2^24`` (the reference's
    label image has the frame's type).  A frame that is not float is a ``ValueError`` here; torch operands are made
    contiguous on the device."""
    if len(image.shape) != 2:
        raise ValueError(f"{what} needs a 2D image, not {len(image.shape)}-D")
    if not image.is_cuda or not points.is_cuda:
        raise ValueError("image and points must live on the GPU")
    if is_native(image) != is_native(points) or image.device.index != points.device.index:
        raise ValueError("image and points must be of one kind and on one device")
    try:
        frame_code = code(image, FLOATS)
    except TypeError as e:
        raise ValueError(f"{what} needs a float frame: {e}") from None
    pts_code = points_code(points, allowed)
    if int(points.shape[0]) >= 2 ** 24:
        raise ValueError(f"{what} needs len(points) < 2^24 (the reference's label image has the frame's type)")
    if not is_native(image):
        image, points = image.contiguous(), points.contiguous()
    return image, frame_code, points, pts_code


def check_refusal(rc, what):
    """``_native.check`` for the calls that test their operands' values on the device: a refused argument
    (``ZK_E_BADARG``, e.g. a window that leaves the frame) is a ``ValueError`` with the library's message."""
    if rc == _native.ZK_E_BADARG:
        raise ValueError(_native.last_error())
    _native.check(rc, what)
