"""ctypes binding of ``libzernike_hip.so`` (C ABI: ``include/zernike_hip.h``).

The library is built in-tree by ``__graft_entry__.build()`` / ``csrc/Makefile`` into
``mtflearn_amd/lib/``.  There is deliberately no CPU fallback here: if the shared object is
missing, or no HIP device is visible, every compute call raises ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import os
import sys
import threading
import weakref
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import numpy as np

ZK_F32, ZK_F64 = 0, 1
ZK_U8, ZK_U16, ZK_I16 = 2, 3, 4   # host-buffer entry points only: widened to float32 on the device (exact)
ZK_E_BADARG = -10001                # zernike_hip.h: a refused argument
ZK_I32 = 5                         # int32 key points (local_max): zk_voronoi_cells and zk_knn_distances only
VORONOI_NEIGHBOURS, VORONOI_GRAPH = 0, 1                           # zk_voronoi_cells modes
REFINE_BOX, REFINE_DISK = 0, 1                                     # zk_refine_points modes
THRESHOLD_LI, THRESHOLD_OTSU = 0, 1                                # zk_com_refine thresholds
GAUSS_CIRCULAR, GAUSS_ELLIPTICAL = 0, 1                            # zk_gauss_fit models
GAUSS_BOX, GAUSS_DISK = 0, 1                                       # zk_gauss_fit masks
GAUSS_CONVERGED, GAUSS_MAX_ITER, GAUSS_STALLED, GAUSS_NOT_FINITE = 0, 1, 2, 3   # zk_gauss_fit status codes
GAUSS_MODELS = {"circular": GAUSS_CIRCULAR, "elliptical": GAUSS_ELLIPTICAL}
ALIGN_DISTANCE, ALIGN_COSINE = 0, 1                                # zk_align_rows keys
ALIGN_KEYS = {"distance": ALIGN_DISTANCE, "cosine": ALIGN_COSINE}
EELS_WHITTAKER, EELS_ALS, EELS_ARPLS, EELS_AIRPLS = 0, 1, 2, 3      # zk_eels_pls modes
TMD_FFT, TMD_GAUSSIAN = 0, 1                                       # zk_tmd_render modes
RESAMPLE_MODES = {"reflect": 0, "mirror": 1, "nearest": 2, "grid-wrap": 3, "grid-constant": 4, "constant": 5}   # ZK_RESAMPLE_*
KNN_RANGES, KNN_HIST, KNN_SIDES, KNN_GAPS = 0, 1, 2, 3             # zk_knn_stats ops
PATH_AUTO, PATH_GENERIC, PATH_FOLDED, PATH_SEPARABLE, PATH_STREAM, PATH_DIRECT = 0, 1, 2, 3, 4, 5
OP_POINTS, OP_MAPS = 1, 2
STATS_CENTERED, STATS_WIDE = 1, 2                                  # zk_image_stats modes
ORDER_VALUES, ORDER_DEVIATIONS = 0, 1                              # zk_image_order_stats modes
MAP_RESCALE, MAP_DIVIDE, MAP_CLIP, MAP_STANDARDIZE = 0, 1, 2, 3    # zk_image_map operations
XFER_SEND, XFER_RECV, XFER_ALLGATHER, XFER_BCAST = 1, 2, 3, 4
COMM_AUTO, COMM_P2P, COMM_ALLGATHER, COMM_BCAST = 0, 1, 2, 3
COMM_ALGOS = {"": COMM_AUTO, "auto": COMM_AUTO, "p2p": COMM_P2P, "allgather": COMM_ALLGATHER, "bcast": COMM_BCAST}
PATH_NAMES = {PATH_GENERIC: "generic", PATH_FOLDED: "folded", PATH_SEPARABLE: "separable", PATH_STREAM: "stream",
              PATH_DIRECT: "direct"}



class Xfer(ctypes.Structure):
    """``zk_xfer``: one RCCL call of the all-gather schedule (include/zernike_hip.h)."""
    _fields_ = [("op", c_int32), ("peer", c_int32), ("group", c_int32), ("plane", c_int32),
                ("offset", c_int64), ("count", c_int64)]


# MTFLEARN_AMD_LIB: alternative build of the same ABI (e.g. a timing-only ablation variant)
LIB_PATH = os.environ.get("MTFLEARN_AMD_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "lib", "libzernike_hip.so")

# every symbol include/zernike_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "zk_abi_version": (c_int, []),
    "zk_device_count": (c_int, []),
    "zk_last_error_string": (c_char_p, []),
    "zk_plan_create": (c_int, [c_int, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_double),
                               c_int, POINTER(c_void_p)]),
    "zk_plan_destroy": (None, [c_void_p]),
    "zk_plan_has_path": (c_int, [c_void_p, c_int, c_int, c_int]),
    "zk_plan_resolved_path": (c_int, [c_void_p, c_int, c_int, c_int64]),
    "zk_plan_supports": (c_int, [c_void_p, c_int, c_int]),
    "zk_plan_disk_pixels": (c_int, [c_void_p]),
    "zk_plan_set_path": (c_int, [c_void_p, c_int]),
    "zk_transform_patches": (c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(c_double)]),
    "zk_transform_patches_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "zk_transform_frame": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, POINTER(c_double)]),
    "zk_transform_frame_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                                       c_void_p, c_void_p]),
    "zk_transform_points": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, POINTER(c_int32), c_int64,
                                    POINTER(c_double)]),
    "zk_transform_points_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                        c_void_p]),
    "zk_frame_maps": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, POINTER(c_int32), c_int,
                              POINTER(c_int32), c_int, c_int, POINTER(c_double), c_int, c_void_p, c_void_p,
                              c_void_p]),
    "zk_frame_maps_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, POINTER(c_int32),
                                  c_int, POINTER(c_int32), c_int, c_int, POINTER(c_double), c_int, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "zk_moment_maps": (c_int, [c_void_p, POINTER(c_double), c_int64, POINTER(c_int32), c_int, POINTER(c_int32), c_int, c_int,
                               POINTER(c_double), c_int, c_void_p, c_void_p, c_void_p]),
    "zk_moment_maps_dev": (c_int, [c_void_p, c_void_p, c_int64, POINTER(c_int32), c_int, POINTER(c_int32), c_int, c_int,
                                   POINTER(c_double), c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_points_maps": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, POINTER(c_int32), c_int64, POINTER(c_int32), c_int,
                               POINTER(c_int32), c_int, c_int, POINTER(c_double), c_int, c_void_p, c_void_p, c_void_p]),
    "zk_transform_frame_dev_strided": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                                               c_void_p, c_int64, c_void_p]),
    "zk_frame_maps_dev_strided": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64,
                                          POINTER(c_int32), c_int, POINTER(c_int32), c_int, c_int, POINTER(c_double),
                                          c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "zk_plan_set_host_chunk": (c_int, [c_void_p, c_int64]),
    "zk_plan_release_staging": (c_int, [c_void_p]),
    "zk_host_alloc": (c_int, [c_int64, POINTER(c_void_p)]),
    "zk_host_free": (c_int, [c_void_p]),
    "zk_comm_unique_id": (c_int, [c_void_p]),
    "zk_comm_init_rank": (c_int, [c_int, c_int, c_int, c_void_p, POINTER(c_void_p)]),
    "zk_comm_init_file": (c_int, [c_int, c_int, c_int, c_char_p, c_double, POINTER(c_void_p)]),
    "zk_comm_init_tcp": (c_int, [c_int, c_int, c_int, c_char_p, c_int, c_double, POINTER(c_void_p)]),
    "zk_comm_destroy": (c_int, [c_void_p]),
    "zk_comm_rank": (c_int, [c_void_p]),
    "zk_comm_world": (c_int, [c_void_p]),
    "zk_allgather_rows": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "zk_allgather_rows_plan": (c_int, [c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
                                       POINTER(Xfer), c_int64, POINTER(c_int64)]),
    "zk_comm_join": (c_int, [c_void_p, c_void_p]),
    "zk_comm_allgather_host": (c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    "zk_autocorr_mean": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, POINTER(c_int32), c_int, c_int,
                                 POINTER(c_double)]),
    "zk_polar_radii": (c_int64, [c_int64, c_int64]),
    "zk_polar_profile": (c_int, [c_int, POINTER(c_double), c_int64, c_int64, c_int64, c_int64, c_int64, c_int,
                                 POINTER(c_double)]),
    "zk_power_spectra": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, POINTER(c_int32), c_int,
                                 POINTER(c_double), POINTER(c_double)]),
    "zk_denoise_fft": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_double, POINTER(c_double)]),
    "zk_wavelet_sigma": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, POINTER(c_double)]),
    "zk_circular_autocorr": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p]),
    "zk_shifted_magnitude": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p]),
    "zk_char_length_fft": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p]),
    "zk_char_length": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "zk_angular_average": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "zk_local_max": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_double, c_int, c_double, c_void_p, c_int64,
                             POINTER(c_int64)]),
    "zk_local_max_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_double, c_int, c_double, c_void_p, c_int64,
                                 POINTER(c_int64), c_void_p]),
    "zk_local_max_last_launches": (c_int64, []),
    "zk_background_opening": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "zk_background_opening_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    "zk_background_rolling_ball": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_double, c_int, c_void_p, c_void_p]),
    "zk_background_rolling_ball_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_double, c_int, c_void_p, c_void_p,
                                               c_void_p]),
    "zk_background_baseline": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                       c_int, c_void_p, c_void_p]),
    "zk_background_baseline_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                           c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "zk_image_stats": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_double, c_void_p, POINTER(c_int64), c_void_p]),
    "zk_image_stats_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_double, c_void_p, POINTER(c_int64), c_void_p, c_void_p]),
    "zk_image_order_stats": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_float, c_void_p, c_int, c_void_p]),
    "zk_image_order_stats_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_float, c_void_p, c_int, c_void_p, c_void_p]),
    "zk_image_map": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_void_p]),
    "zk_image_map_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "zk_render_gaussians": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_double,
                                    c_double, c_int, c_int64]),
    "zk_render_gaussians_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                        c_double, c_double, c_int, c_int64, c_void_p]),
    "zk_find_regions": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_void_p), POINTER(c_int64), c_void_p, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "zk_find_regions_dev": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_void_p), POINTER(c_int64), c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_voronoi_cells": (c_int, [c_int, c_void_p, c_int, c_int64, c_double, c_int, c_double, c_double, POINTER(c_void_p), POINTER(c_int64),
                                 c_void_p, c_void_p, c_void_p]),
    "zk_voronoi_cells_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_double, c_int, c_double, c_double, POINTER(c_void_p),
                                     POINTER(c_int64), c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_refine_points": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "zk_refine_points_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "zk_com_refine": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "zk_com_refine_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "zk_com_refine_points_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_int64, c_int64, c_int, c_void_p,
                                         c_void_p]),
    "zk_gauss_fit": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_double, c_double, c_int64,
                             c_void_p, c_void_p, c_void_p]),
    "zk_gauss_fit_points_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_void_p, c_int, c_int64, c_int64, c_int, c_int, c_double,
                                        c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_knn_distances": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_void_p]),
    "zk_knn_distances_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p]),
    "zk_knn_stats": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "zk_knn_stats_dev": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_windows_apply": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                 c_void_p, c_int64, c_void_p, c_void_p]),
    "zk_windows_apply_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                     c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "zk_windows_apply_t": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                   c_void_p, c_int64, c_void_p]),
    "zk_windows_apply_t_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                       c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "zk_windows_moments": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "zk_windows_moments_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "zk_windows_reconstruct": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                       c_int64, c_void_p, c_void_p, c_void_p]),
    "zk_windows_reconstruct_dev": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                           c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_gram": (c_int, [c_int, POINTER(c_double), c_int64, c_int, POINTER(c_double), POINTER(c_void_p)]),
    "zk_project": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_double), POINTER(c_double), c_int, POINTER(c_double),
                           c_int]),
    "zk_gram_dev": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "zk_project_dev": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "zk_rows_create": (c_int, [c_int, POINTER(c_double), c_int64, c_int, POINTER(c_void_p)]),
    "zk_rows_adopt": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_void_p)]),
    "zk_rows_destroy": (c_int, [c_void_p]),
    "zk_rows_data": (c_void_p, [c_void_p]),
    "zk_rows_center": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "zk_rows_colsum": (c_int, [c_void_p, POINTER(c_double)]),
    "zk_rows_center_at": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "zk_rows_fetch": (c_int, [c_void_p, POINTER(c_int64), c_int, c_int, POINTER(c_double)]),
    "zk_rows_reset_labels": (c_int, [c_void_p]),
    "zk_rows_labels": (c_int, [c_void_p, POINTER(c_int32)]),
    "zk_rows_labels_dev": (c_void_p, [c_void_p]),
    "zk_kmeans_seed_step": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double), c_int, c_int, POINTER(c_double)]),
    "zk_kmeans_seed_pick": (c_int, [c_void_p, c_int, POINTER(c_double), c_int, POINTER(c_int64)]),
    "zk_kmeans_step": (c_int, [c_void_p, POINTER(c_double), c_int, c_int, POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "zk_rows_profile": (c_int, [c_void_p, c_int]),
    "zk_rows_last_kernel_ms": (c_double, [c_void_p]),
    "zk_kmeans_own_distance": (c_int, [c_void_p, POINTER(c_double), c_int, POINTER(c_double)]),
    "zk_gmm_estep": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int, c_int, POINTER(c_double)]),
    "zk_gmm_resp_from_labels": (c_int, [c_void_p, c_int]),
    "zk_gmm_moments": (c_int, [c_void_p, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    "zk_rows_gram": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double)]),
    "zk_rows_knn_correlation": (c_int, [c_void_p, c_int, c_int, c_double, POINTER(c_int64), POINTER(c_double), POINTER(c_double)]),
    "zk_uniform_choice_index": (c_int, [c_int64, c_double, POINTER(c_int64)]),
    "zk_uniform_choice_index_sequential": (c_int, [c_int64, c_double, POINTER(c_int64), POINTER(c_double)]),
    "zk_repeated_sum_f64": (c_double, [c_double, c_int64]),
    "zk_force_layout_stage": (c_int, [POINTER(c_double), c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_double), c_int64,
                                      POINTER(c_int64), c_int, c_int64, POINTER(c_double), c_int, c_double, POINTER(c_int64),
                                      POINTER(c_double)]),
    "zk_synth_create": (c_int, [c_int, c_int, c_int64, POINTER(c_double), POINTER(c_void_p)]),
    "zk_synth_destroy": (c_int, [c_void_p]),
    "zk_synth_set_host_chunk": (c_int, [c_void_p, c_int64]),
    "zk_synth_apply": (c_int, [c_void_p, POINTER(c_double), c_int64, c_int, c_void_p]),
    "zk_synth_apply_dev": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "zk_align_rows": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int,
                              POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                              c_void_p, c_void_p]),
    "zk_align_rows_dev": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int,
                                  POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "zk_align_set_host_chunk": (c_int, [c_int, c_int64]),
    "zk_align_planes": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int,
                                POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                                c_void_p, c_void_p, c_void_p, c_int64]),
    "zk_align_planes_dev": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int,
                                    POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "zk_frame_align": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, POINTER(c_double), c_int,
                               POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                               c_void_p, c_void_p, c_void_p, c_int64]),
    "zk_frame_align_dev": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, POINTER(c_double), c_int,
                                   POINTER(c_int32), c_int, c_int, c_int, c_int, POINTER(c_double), c_int, POINTER(c_double), c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "zk_align_set_band_bytes": (c_int, [c_int, c_int64]),
    "zk_rotate_rows": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), c_void_p, c_void_p]),
    "zk_rotate_rows_dev": (c_int, [c_int, c_void_p, c_int64, c_int, POINTER(c_int32), POINTER(c_int32), c_void_p, c_void_p, c_void_p]),
    "zk_eels_snip": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "zk_eels_snip_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "zk_eels_pls": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_double, c_double, c_int, c_void_p,
                            c_int, c_void_p, c_void_p, c_void_p]),
    "zk_eels_pls_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int, c_double, c_double, c_int, c_void_p,
                                c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_eels_set_chunk": (c_int, [c_int, c_int64]),
    "zk_scan_resample": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "zk_scan_resample_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "zk_scan_resample_set_chunk": (c_int, [c_int, c_int64]),
    "zk_register_shifts": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int64, c_void_p, c_int, c_int, c_int64, c_int,
                                   c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_register_shifts_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_int, c_int64, c_void_p, c_int, c_int, c_int64,
                                       c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_stack_mean": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p]),
    "zk_stack_mean_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "zk_gpa": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_void_p]),
    "zk_gpa_dev": (c_int, [c_int, c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_double, c_int, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_void_p]),
    "zk_gpa_set_run_bytes": (c_int, [c_int, c_int64]),
    "zk_tmd_render": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int]),
    "zk_tmd_render_dev": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "zk_device_malloc": (c_int, [c_int, c_int64, POINTER(c_void_p)]),
    "zk_device_free": (c_int, [c_int, c_void_p]),
    "zk_device_copy": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int]),
    "zk_device_synchronize": (c_int, [c_int]),
    "zk_hbm_probe": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int64, c_int, POINTER(c_double)]),
    "zk_debug_strip3_launches": (c_int64, []),
    "zk_clock_monitor_start": (c_int, [c_int, c_double, POINTER(c_void_p)]),
    "zk_clock_monitor_stop": (c_int, [c_void_p, POINTER(c_double), POINTER(c_double)]),
    "zk_plan_profile": (c_int, [c_void_p, c_int]),
    "zk_plan_profile_read": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_double)]),
    "zk_plan_profile_read_launches": (c_int, [c_void_p, POINTER(c_double), c_int64, POINTER(c_int64)]),
}

_lib = None


def _preload_torch_hip():
    """When PyTorch-ROCm is installed it ships its own ``libamdhip64.so`` (SONAME libamdhip64.so.7).
    Two HIP runtimes in one process do not coexist (the second one finds no device), so bind our
    library to torch's copy: loading it first satisfies our NEEDED libamdhip64.so.7 by SONAME, and a
    later ``import torch`` resolves to the same file.  Without torch the system ROCm runtime is used."""
    if os.environ.get("MTFLEARN_AMD_SYSTEM_HIP"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for base in (spec.submodule_search_locations or []) if spec else []:
            cand = os.path.join(base, "lib", "libamdhip64.so")
            if os.path.exists(cand):
                ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
                return
    except Exception:
        pass


def load():
    """Load the shared library once; raises RuntimeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C motif-learn_amd/csrc` (hipcc, --offload-arch=gfx950). "
            "mtflearn_amd has no CPU fallback.")
    _preload_torch_hip()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error():
    msg = load().zk_last_error_string()
    return msg.decode() if msg else ""


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}: {last_error()}")


def device_count():
    n = load().zk_device_count()
    if n < 0:
        raise RuntimeError(f"zk_device_count failed with code {n}: {last_error()}")
    return n


def require_device():
    if device_count() == 0:
        raise RuntimeError("no HIP device visible: mtflearn_amd computes on MI355X only (there is no CPU fallback)")


def default_device():
    """GPU of a call that names none: ``MTFLEARN_AMD_DEVICE``, else ``LOCAL_RANK``, else torch's current device when
    torch is already imported and has initialised HIP, else 0."""
    for var in ("MTFLEARN_AMD_DEVICE", "LOCAL_RANK"):
        if os.environ.get(var, "") != "":
            return int(os.environ[var])
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        return int(torch.cuda.current_device())
    return 0


class ClockMonitor:
    """``with ClockMonitor(device) as m: ...`` -- the mean shader clock (``m.ghz``) over the ``m.ms`` the block took, sampled by
    one resident wave (``zk_clock_monitor_start / _stop``).  Inside the block synchronise the STREAM the work runs on, not
    the device: a device-wide synchronisation waits for the monitor's own wave, i.e. for its whole time budget."""

    def __init__(self, device=0, max_ms=1500.0):
        self.device, self.max_ms, self.ghz, self.ms, self._h = device, max_ms, None, None, c_void_p()

    def __enter__(self):
        check(load().zk_clock_monitor_start(int(self.device), float(self.max_ms), byref(self._h)), "zk_clock_monitor_start")
        return self

    def __exit__(self, *exc):
        ghz, ms = c_double(), c_double()
        check(load().zk_clock_monitor_stop(self._h, byref(ghz), byref(ms)), "zk_clock_monitor_stop")
        self.ghz, self.ms = ghz.value, ms.value
        return False


def hbm_probe(device, src_ptr, nbytes, dst_ptr=None, store_per_group=0, reps=5):
    """Milliseconds per pass of a plain stream over device buffers (``zk_hbm_probe``): LDS-DMA read of ``nbytes`` at
    ``src_ptr`` (``dst_ptr`` None), a 16-B-per-lane copy, or the read stream plus ``store_per_group`` bytes written per
    256-KiB group."""
    ms = c_double()
    check(load().zk_hbm_probe(int(device), c_void_p(src_ptr), c_void_p(dst_ptr) if dst_ptr else None, int(nbytes),
                              int(store_per_group), int(reps), byref(ms)), "zk_hbm_probe")
    return ms.value


def dtype_code(dtype):
    """ZK_F32 / ZK_F64 for the two element types the kernels read natively, ZK_U8 / ZK_U16 / ZK_I16 for the narrow
    detector formats the host-buffer entry points widen on the device, else None."""
    if dtype == np.float32:
        return ZK_F32
    if dtype == np.float64:
        return ZK_F64
    return {np.dtype(np.uint8): ZK_U8, np.dtype(np.uint16): ZK_U16, np.dtype(np.int16): ZK_I16}.get(np.dtype(dtype))


class PinnedPool:
    """Page-locked host arrays for results, recycled.

    ``ZPs.transform`` returns arrays of hundreds of MB to GB; filling a fresh ``np.empty`` over PCIe pays a page
    fault per 4 KiB and the runtime's pageable staging.  Arrays from this pool are page-locked (``zk_host_alloc``
    = ``hipHostMalloc``): the device writes them by DMA at link speed.  A block returns to the pool when the last
    NumPy view of it is garbage-collected and is handed out again for the next result of a fitting size, so
    repeated calls neither allocate nor fault.  ``MTFLEARN_AMD_PINNED_MB`` caps the idle bytes the pool keeps
    (default 16384; 0 disables the pool: results are plain ``np.empty`` arrays)."""

    GRAIN = 2 << 20

    def __init__(self):
        self._free = []            # [(capacity, ptr)]
        self._lock = threading.Lock()
        self.max_idle = int(os.environ.get("MTFLEARN_AMD_PINNED_MB", "16384")) << 20
        self.min_bytes = 1 << 20   # smaller results are not worth a pinned block

    def empty(self, shape, dtype=np.float64):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if self.max_idle <= 0 or nbytes < self.min_bytes:
            return np.empty(shape, dtype=dtype)
        cap = -(-nbytes // self.GRAIN) * self.GRAIN
        ptr = None
        with self._lock:
            fits = [k for k, (c, _) in enumerate(self._free) if cap <= c <= 2 * cap]
            if fits:
                cap, ptr = self._free.pop(min(fits, key=lambda k: self._free[k][0]))
        if ptr is None:
            handle = c_void_p()
            if load().zk_host_alloc(cap, byref(handle)) != 0:     # no pinned memory to be had: pageable result
                return np.empty(shape, dtype=dtype)
            ptr = handle.value
        buf = (ctypes.c_char * cap).from_address(ptr)
        weakref.finalize(buf, self._release, cap, ptr)
        return np.ndarray(shape, dtype=dtype, buffer=buf)

    def _release(self, cap, ptr):
        with self._lock:
            if sum(c for c, _ in self._free) + cap <= self.max_idle:
                self._free.append((cap, ptr))
                return
        if _lib is not None:
            _lib.zk_host_free(c_void_p(ptr))

    def trim(self):
        """Give every idle block back to the system."""
        with self._lock:
            blocks, self._free = self._free, []
        for _, ptr in blocks:
            load().zk_host_free(c_void_p(ptr))


pinned = PinnedPool()


class Plan:
    """Owns one ``zk_plan`` (device tables for one basis on one GPU)."""

    def __init__(self, basis, n, m, device=0):
        lib = load()
        basis = np.ascontiguousarray(basis, dtype=np.float64)
        self.n_poly, self.size = int(basis.shape[0]), int(basis.shape[1])
        self.device = int(device)
        n32 = np.ascontiguousarray(n, dtype=np.int32)
        m32 = np.ascontiguousarray(m, dtype=np.int32)
        self.n, self.m = n32, m32          # the labels of the moment axis (what the alignment maps pair up)
        require_device()
        handle = c_void_p()
        check(lib.zk_plan_create(self.size, self.n_poly, n32.ctypes.data_as(POINTER(c_int32)),
                                 m32.ctypes.data_as(POINTER(c_int32)),
                                 basis.ctypes.data_as(POINTER(c_double)), self.device, byref(handle)),
              "zk_plan_create")
        self._h = handle
        self._lib = lib

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zk_plan_destroy(self._h)
            self._h = None

    __del__ = close

    # -- introspection / control -------------------------------------------------------
    def has_path(self, mode, dtype_code_, path):
        """True if kernel family ``path`` exists for mode (0 batch, 1 frame) and element type."""
        return bool(self._lib.zk_plan_has_path(self._h, mode, dtype_code_, path))

    def supports(self, op, dtype_code_):
        """True if the plan has the key-point (OP_POINTS) / fused-maps (OP_MAPS) kernel for the element type."""
        return bool(self._lib.zk_plan_supports(self._h, op, dtype_code_))

    def best_path(self, mode, dtype_code_, n_units=1 << 20):
        """The kernel family a transform runs on with the plan's current setting (what PATH_AUTO resolves to for a
        batch of ``n_units`` patches / a frame)."""
        return self._lib.zk_plan_resolved_path(self._h, mode, dtype_code_, n_units)

    @property
    def disk_pixels(self):
        return self._lib.zk_plan_disk_pixels(self._h)

    def set_path(self, path):
        check(self._lib.zk_plan_set_path(self._h, path), "zk_plan_set_path")

    def profile(self, enable=True):
        check(self._lib.zk_plan_profile(self._h, int(enable)), "zk_plan_profile")

    def profile_read(self):
        launches, ms = c_int64(), c_double()
        check(self._lib.zk_plan_profile_read(self._h, byref(launches), byref(ms)), "zk_plan_profile_read")
        return launches.value, ms.value

    def profile_read_launches(self, cap=65536):
        """Per-launch kernel times (ms) recorded since the last read, in launch order; raises if more than ``cap``
        launches were recorded (the library drops what does not fit -- a truncated list would skew every statistic)."""
        buf = (c_double * cap)()
        n = c_int64()
        check(self._lib.zk_plan_profile_read_launches(self._h, buf, cap, byref(n)), "zk_plan_profile_read_launches")
        if n.value > cap:
            raise RuntimeError(f"profile_read_launches: {n.value} launches recorded, room for {cap}")
        return list(buf[:n.value])

    # -- host-buffer entry points --------------------------------------------------------
    def transform_patches(self, patches):
        code = dtype_code(patches.dtype)
        out = pinned.empty((patches.shape[0], self.n_poly))
        check(self._lib.zk_transform_patches(self._h, patches.ctypes.data_as(c_void_p), code,
                                             patches.shape[0], out.ctypes.data_as(POINTER(c_double))),
              "zk_transform_patches")
        return out

    def transform_frame(self, image):
        code = dtype_code(image.dtype)
        h, w = image.shape
        out = pinned.empty((self.n_poly, h, w))
        check(self._lib.zk_transform_frame(self._h, image.ctypes.data_as(c_void_p), code, h, w,
                                           out.ctypes.data_as(POINTER(c_double))),
              "zk_transform_frame")
        return out

    def transform_points(self, image, points):
        """Moments of the windows at integer (x, y) points of a host frame -> (N, n_poly) float64."""
        code = dtype_code(image.dtype)
        h, w = image.shape
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
        out = pinned.empty((pts.shape[0], self.n_poly))
        check(self._lib.zk_transform_points(self._h, image.ctypes.data_as(c_void_p), code, h, w,
                                            pts.ctypes.data_as(POINTER(c_int32)), pts.shape[0],
                                            out.ctypes.data_as(POINTER(c_double))), "zk_transform_points")
        return out

    def transform_points_dev(self, image_ptr, code, height, width, points_ptr, n_points, out_ptr, stream=0):
        """``zk_transform_points_dev``: (n_points, 2) int32 (x, y) on the device -> (n_points, n_poly) float64 on the device."""
        check(self._lib.zk_transform_points_dev(self._h, c_void_p(image_ptr), code, height, width, c_void_p(points_ptr),
                                                n_points, c_void_p(out_ptr), c_void_p(stream)), "zk_transform_points_dev")

    def frame_maps(self, image, n_complex, folds=None, m_unselect=(0, 1), p=2, theta=None, want_abs=True):
        """Fused frame -> (rot_maps, |Z^c|, mirror_map); any of them None when not requested."""
        code = dtype_code(image.dtype)
        h, w = image.shape
        folds32 = np.ascontiguousarray(folds if folds is not None else [], dtype=np.int32)
        unsel32 = np.ascontiguousarray(m_unselect, dtype=np.int32)
        rot = pinned.empty((len(folds32), h, w)) if len(folds32) else None
        ab = pinned.empty((n_complex, h, w)) if want_abs else None
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        mir = pinned.empty((h, w)) if th is not None else None
        ptr = lambda a: a.ctypes.data_as(c_void_p) if a is not None else None
        check(self._lib.zk_frame_maps(
            self._h, image.ctypes.data_as(c_void_p), code, h, w,
            folds32.ctypes.data_as(POINTER(c_int32)), len(folds32),
            unsel32.ctypes.data_as(POINTER(c_int32)), len(unsel32), 2 if p == 2 else 0,
            th.ctypes.data_as(POINTER(c_double)) if th is not None else None, 0 if th is None else len(th),
            ptr(rot), ptr(ab), ptr(mir)), "zk_frame_maps")
        return rot, ab, mir

    def _rows_maps(self, n_rows, n_complex, folds, m_unselect, p, theta, want_abs, call):
        folds32 = np.ascontiguousarray(folds if folds is not None else [], dtype=np.int32)
        unsel32 = np.ascontiguousarray(m_unselect, dtype=np.int32)
        rot = pinned.empty((n_rows, len(folds32))) if len(folds32) else None
        ab = pinned.empty((n_rows, n_complex)) if want_abs else None
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        mir = pinned.empty((n_rows,)) if th is not None else None
        ptr = lambda a: a.ctypes.data_as(c_void_p) if a is not None else None
        call(folds32.ctypes.data_as(POINTER(c_int32)), len(folds32),
             unsel32.ctypes.data_as(POINTER(c_int32)), len(unsel32), 2 if p == 2 else 0,
             th.ctypes.data_as(POINTER(c_double)) if th is not None else None, 0 if th is None else len(th),
             ptr(rot), ptr(ab), ptr(mir))
        return rot, ab, mir

    def moment_maps(self, moments, n_complex, folds=None, m_unselect=(0, 1), p=2, theta=None, want_abs=True):
        """(N, n_poly) host moments -> (rot (N, n_folds), |Z^c| (N, N_c), mirror (N)); None when not requested."""
        mom = np.ascontiguousarray(moments, dtype=np.float64)
        return self._rows_maps(mom.shape[0], n_complex, folds, m_unselect, p, theta, want_abs,
                               lambda *tail: check(self._lib.zk_moment_maps(
                                   self._h, mom.ctypes.data_as(POINTER(c_double)), mom.shape[0], *tail), "zk_moment_maps"))

    def points_maps(self, image, points, n_complex, folds=None, m_unselect=(0, 1), p=2, theta=None, want_abs=True):
        """Windows at integer (x, y) points of a host frame -> the same three outputs; the moments stay on the device."""
        code = dtype_code(image.dtype)
        h, w = image.shape
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 2)
        return self._rows_maps(pts.shape[0], n_complex, folds, m_unselect, p, theta, want_abs,
                               lambda *tail: check(self._lib.zk_points_maps(
                                   self._h, image.ctypes.data_as(c_void_p), code, h, w,
                                   pts.ctypes.data_as(POINTER(c_int32)), pts.shape[0], *tail), "zk_points_maps"))

    def frame_maps_dev(self, image_ptr, code, height, width, row0, n_rows, folds, m_unselect, p, theta,
                       rot_ptr, abs_ptr, mirror_ptr, stream=0, plane_stride=None):
        folds32 = np.ascontiguousarray(folds if folds is not None else [], dtype=np.int32)
        unsel32 = np.ascontiguousarray(m_unselect, dtype=np.int32)
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        head = (self._h, c_void_p(image_ptr), code, height, width, row0, n_rows,
                folds32.ctypes.data_as(POINTER(c_int32)), len(folds32),
                unsel32.ctypes.data_as(POINTER(c_int32)), len(unsel32), 2 if p == 2 else 0,
                th.ctypes.data_as(POINTER(c_double)) if th is not None else None, 0 if th is None else len(th),
                c_void_p(rot_ptr), c_void_p(abs_ptr), c_void_p(mirror_ptr))
        if plane_stride is None:
            check(self._lib.zk_frame_maps_dev(*head, c_void_p(stream)), "zk_frame_maps_dev")
        else:
            check(self._lib.zk_frame_maps_dev_strided(*head, plane_stride, c_void_p(stream)),
                  "zk_frame_maps_dev_strided")

    # -- device-pointer entry points (bench / multi-GPU harness) ------------------------------
    def transform_patches_dev(self, patches_ptr, code, n_patches, out_ptr, stream=0):
        check(self._lib.zk_transform_patches_dev(self._h, c_void_p(patches_ptr), code, n_patches,
                                                 c_void_p(out_ptr), c_void_p(stream)),
              "zk_transform_patches_dev")

    def transform_frame_dev(self, image_ptr, code, height, width, row0, n_rows, out_ptr, stream=0, plane_stride=None):
        """Row band -> (n_poly, n_rows, W) at ``out_ptr``; with ``plane_stride`` (doubles) the planes are that far
        apart, i.e. the band is written in place into a larger (n_poly, H, W) array."""
        if plane_stride is None:
            check(self._lib.zk_transform_frame_dev(self._h, c_void_p(image_ptr), code, height, width, row0,
                                                   n_rows, c_void_p(out_ptr), c_void_p(stream)),
                  "zk_transform_frame_dev")
        else:
            check(self._lib.zk_transform_frame_dev_strided(self._h, c_void_p(image_ptr), code, height, width, row0,
                                                           n_rows, c_void_p(out_ptr), plane_stride, c_void_p(stream)),
                  "zk_transform_frame_dev_strided")

    def set_host_chunk(self, chunk_bytes):
        check(self._lib.zk_plan_set_host_chunk(self._h, int(chunk_bytes)), "zk_plan_set_host_chunk")

    def release_staging(self):
        """Free the staging buffers the host-buffer entry points have grown (re-created on demand)."""
        check(self._lib.zk_plan_release_staging(self._h), "zk_plan_release_staging")


class Synthesis:
    """Owns one ``zk_synth``: a ``(n_funcs, n_pixels)`` float64 table resident on one GPU and the product ``out = C . table``
    on its matrix cores (csrc/zk_synth.hip) -- the device side of ``ZPs.inverse_transform``, usable with any table."""

    def __init__(self, table, device=0):
        lib = load()
        table = np.ascontiguousarray(table, dtype=np.float64)
        if table.ndim != 2 or table.size == 0:
            raise ValueError("the synthesis table must be a non-empty (n_funcs, n_pixels) matrix")
        self.n_funcs, self.n_pixels = int(table.shape[0]), int(table.shape[1])
        self.device = int(device)
        require_device()
        handle = c_void_p()
        check(lib.zk_synth_create(self.device, self.n_funcs, self.n_pixels, table.ctypes.data_as(POINTER(c_double)), byref(handle)),
              "zk_synth_create")
        self._h = handle
        self._lib = lib

    @classmethod
    def create(cls, table, device=0):
        return cls(table, device=device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zk_synth_destroy(self._h)
            self._h = None

    __del__ = close

    def set_host_chunk(self, chunk_bytes):
        """Bytes of coefficients + output per chunk of :meth:`apply` (0: the default of 256 MiB)."""
        check(self._lib.zk_synth_set_host_chunk(self._h, int(chunk_bytes)), "zk_synth_set_host_chunk")

    def apply(self, coeffs, dtype=np.float64):
        """``(N, n_funcs)`` host coefficients -> ``(N, n_pixels)`` host array of ``dtype`` (float64 / float32)."""
        code = dtype_code(np.dtype(dtype))
        if code not in (ZK_F32, ZK_F64):
            raise ValueError("dtype must be float64 or float32")
        coeffs = np.ascontiguousarray(coeffs, dtype=np.float64)
        if coeffs.ndim != 2 or coeffs.shape[1] != self.n_funcs:
            raise ValueError(f"coefficients must be (N, {self.n_funcs})")
        out = pinned.empty((coeffs.shape[0], self.n_pixels), dtype=dtype)
        check(self._lib.zk_synth_apply(self._h, coeffs.ctypes.data_as(POINTER(c_double)), coeffs.shape[0], code,
                                       out.ctypes.data_as(c_void_p)), "zk_synth_apply")
        return out

    def apply_dev(self, coeffs_ptr, n_rows, out_ptr, code=ZK_F64, stream=0):
        """``zk_synth_apply_dev``: ``(n_rows, n_funcs)`` float64 on the device -> ``(n_rows, n_pixels)`` of ``code`` on the
        device, enqueued on ``stream`` (no synchronisation)."""
        check(self._lib.zk_synth_apply_dev(self._h, c_void_p(coeffs_ptr), int(n_rows), int(code), c_void_p(out_ptr), c_void_p(stream)),
              "zk_synth_apply_dev")


class AlignSpec:
    """The host-side operands of one ``zk_align_rows`` option set, checked and laid out once: labels, templates ``(T, P)``, the
    0 / 1 selection, the grid's cos / sin table (NumPy's, so that a NumPy statement of the search shares its bits) and the
    ``T`` key values (``|t|^2`` or ``1 / |t|`` over the selection, NumPy's sums).  Everything the library would refuse is
    a ``ValueError`` here, before any device call."""

    def __init__(self, n, m, templates, select=None, n_theta=360, symmetry=1, newton_iters=3, key="distance"):
        self.n = np.ascontiguousarray(n, dtype=np.int32).ravel()
        self.m = np.ascontiguousarray(m, dtype=np.int32).ravel()
        check_paired(self.n, self.m)
        self.templates = np.ascontiguousarray(templates, dtype=np.float64)
        if self.templates.ndim != 2 or self.templates.shape[1] != len(self.n):
            raise ValueError(f"templates must be a (T, {len(self.n)}) matrix of real moments with the rows' labels")
        if not 1 <= self.templates.shape[0] <= 64:
            raise ValueError(f"align takes between 1 and 64 templates, not {self.templates.shape[0]}")
        if int(n_theta) != n_theta or not 1 <= n_theta <= 4096:
            raise ValueError(f"n_theta must be an integer between 1 and 4096, not {n_theta!r}")
        if int(symmetry) != symmetry or not 1 <= symmetry <= 360:
            raise ValueError(f"symmetry must be an integer between 1 and 360, not {symmetry!r}")
        if int(newton_iters) != newton_iters or not 0 <= newton_iters <= 16:
            raise ValueError(f"newton_iters must be an integer between 0 and 16, not {newton_iters!r}")
        if key not in ALIGN_KEYS:
            raise ValueError(f"key must be 'distance' or 'cosine', not {key!r}")
        self.select = np.ones(len(self.n), dtype=np.int32) if select is None else np.ascontiguousarray(select, dtype=np.int32).ravel()
        if self.select.shape != self.n.shape:
            raise ValueError("the selection must have one entry per moment")
        self.n_theta, self.symmetry, self.newton_iters, self.key = int(n_theta), int(symmetry), int(newton_iters), key
        kept = self.select != 0
        self.trig_m = int(np.abs(self.m[kept]).max()) if kept.any() else 0
        self.theta = np.linspace(0, 360 / self.symmetry, self.n_theta, endpoint=False)
        angles = np.multiply.outer(np.deg2rad(self.theta), np.arange(1, self.trig_m + 1))
        self.trig = np.ascontiguousarray(np.hstack([np.cos(angles), np.sin(angles)]))       # (n_theta, 2 trig_m)
        sq = (self.templates[:, kept] ** 2).sum(axis=1)
        self.key_values = np.ascontiguousarray(sq if key == "distance" else 1.0 / np.sqrt(sq))

    @property
    def n_templates(self):
        return self.templates.shape[0]

    def _tail(self):
        pi, pd = POINTER(c_int32), POINTER(c_double)
        return (len(self.n), self.n.ctypes.data_as(pi), self.m.ctypes.data_as(pi), self.templates.ctypes.data_as(pd), self.n_templates,
                self.select.ctypes.data_as(pi), self.n_theta, self.symmetry, self.newton_iters, ALIGN_KEYS[self.key],
                self.trig.ctypes.data_as(pd) if self.trig_m else None, self.trig_m, self.key_values.ctypes.data_as(pd))


def check_paired(n, m):
    """The label set of the alignment kernels: ``0 <= |m| <= n <= 40``, no label twice, every ``(n, m)`` with its ``(n, -m)``."""
    n, m = np.asarray(n), np.asarray(m)
    if n.shape != m.shape or n.ndim != 1 or n.size == 0:
        raise ValueError("`n` and `m` must be 1-D and of one length")
    if (n < 0).any() or (n > 40).any() or (np.abs(m) > n).any():
        raise ValueError("the alignment kernels take labels with 0 <= |m| <= n <= 40")
    have = set(zip(n.tolist(), m.tolist()))
    if len(have) != n.size:
        raise ValueError("a label (n, m) occurs twice")
    for nn, mm in have:
        if (nn, -mm) not in have:
            raise ValueError(f"the label set is not paired: (n, m) = ({nn}, {mm}) has no (n, -m) beside it "
                             "(full ZPs sets and select()ed sets qualify)")


def align_rows(rows, spec, device=None):
    """``zk_align_rows``: host rows ``(N, P)`` float64 against ``spec`` (:class:`AlignSpec`) -> ``(angle (N, T), score (N, T),
    best (N) int32)`` host arrays."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[1] != len(spec.n):
        raise ValueError(f"rows must be (N, {len(spec.n)})")
    n, t = rows.shape[0], spec.n_templates
    angle, score, best = np.empty((n, t)), np.empty((n, t)), np.empty(n, dtype=np.int32)
    if n == 0:
        return angle, score, best
    require_device()
    dev = default_device() if device is None else int(device)
    check(load().zk_align_rows(dev, rows.ctypes.data_as(c_void_p), n, *spec._tail(), angle.ctypes.data_as(c_void_p),
                               score.ctypes.data_as(c_void_p), best.ctypes.data_as(c_void_p)), "zk_align_rows")
    return angle, score, best


def align_rows_dev(device, rows_ptr, n_rows, spec, angle_ptr, score_ptr, best_ptr, stream=0):
    """``zk_align_rows_dev``: rows and outputs on the device (an output pointer may be 0), enqueued on ``stream``."""
    check(load().zk_align_rows_dev(int(device), c_void_p(rows_ptr), int(n_rows), *spec._tail(), c_void_p(angle_ptr), c_void_p(score_ptr),
                                   c_void_p(best_ptr), c_void_p(stream)), "zk_align_rows_dev")


def align_set_host_chunk(chunk_bytes, device=None):
    """Bytes of input + output per chunk of :func:`align_rows` and :func:`rotate_rows` (0: the default of 256 MiB)."""
    check(load().zk_align_set_host_chunk(default_device() if device is None else int(device), int(chunk_bytes)),
          "zk_align_set_host_chunk")


def _out_ptr(array):
    return c_void_p(array.ctypes.data) if array is not None else None


def align_planes(planes, spec, n_pixels=None, out=None, device=None):
    """``zk_align_planes``: host planes ``(P, S)`` float64 -- moment ``j`` of pixel ``i`` at ``planes[j, i]``, the first
    ``n_pixels`` (default ``S``) of every plane count, so ``S`` is the plane stride -- against ``spec`` (:class:`AlignSpec`) ->
    ``(angle (T, n_pixels), score (T, n_pixels), best (n_pixels) int32, norm2 (n_pixels))`` host arrays.  ``out``: the four
    arrays to write into instead, ``angle`` and ``score`` C-contiguous ``(T, S_out)`` with one ``S_out >= n_pixels`` (the output
    plane stride; columns past ``n_pixels`` are left alone), ``best`` / ``norm2`` of at least ``n_pixels`` entries; an entry may be
    ``None`` (that output is not computed).  Everything is checked here, before any device call."""
    planes = np.asarray(planes)
    if planes.ndim != 2 or planes.shape[0] != len(spec.n) or planes.dtype != np.float64 or not planes.flags.c_contiguous:
        raise ValueError(f"planes must be a C-contiguous ({len(spec.n)}, S) float64 matrix, one plane per moment")
    stride = planes.shape[1]
    n = stride if n_pixels is None else int(n_pixels)
    if n < 0:
        raise ValueError("n_pixels must not be negative")
    if stride < n:
        raise ValueError(f"plane_stride ({stride}) is smaller than n_pixels ({n})")
    t = spec.n_templates
    if out is None:
        out = (np.empty((t, n)), np.empty((t, n)), np.empty(n, dtype=np.int32), np.empty(n))
    angle, score, best, norm2 = out
    out_stride = _check_plane_outputs(angle, score, best, norm2, t, n)
    if n == 0:
        return angle, score, best, norm2
    require_device()
    dev = default_device() if device is None else int(device)
    check(load().zk_align_planes(dev, planes.ctypes.data_as(c_void_p), n, stride, *spec._tail(), _out_ptr(angle), _out_ptr(score),
                                 _out_ptr(best), _out_ptr(norm2), out_stride), "zk_align_planes")
    return angle, score, best, norm2


def _check_plane_outputs(angle, score, best, norm2, t, n):
    """The output plane stride of host outputs of :func:`align_planes` (``n`` when neither map is wanted)."""
    stride = None
    for name, a in (("angle", angle), ("score", score)):
        if a is None:
            continue
        if a.ndim != 2 or a.shape[0] != t or a.dtype != np.float64 or not a.flags.c_contiguous:
            raise ValueError(f"{name} must be a C-contiguous ({t}, S_out) float64 array")
        if stride is not None and a.shape[1] != stride:
            raise ValueError("angle and score must share one plane stride")
        stride = a.shape[1]
    stride = n if stride is None else stride
    if stride < n:
        raise ValueError(f"out_plane_stride ({stride}) is smaller than n_pixels ({n})")
    for name, a, dt in (("best", best, np.int32), ("norm2", norm2, np.float64)):
        if a is not None and (a.ndim != 1 or a.shape[0] < n or a.dtype != dt or not a.flags.c_contiguous):
            raise ValueError(f"{name} must be a C-contiguous {np.dtype(dt).name} vector of at least {n} entries")
    return stride


def align_planes_dev(device, planes_ptr, n_pixels, plane_stride, spec, angle_ptr, score_ptr, best_ptr, norm2_ptr, out_plane_stride,
                     stream=0):
    """``zk_align_planes_dev``: planes and outputs on the device (an output pointer may be 0), enqueued on ``stream``."""
    if plane_stride < n_pixels:
        raise ValueError(f"plane_stride ({plane_stride}) is smaller than n_pixels ({n_pixels})")
    if out_plane_stride < n_pixels:
        raise ValueError(f"out_plane_stride ({out_plane_stride}) is smaller than n_pixels ({n_pixels})")
    check(load().zk_align_planes_dev(int(device), c_void_p(planes_ptr), int(n_pixels), int(plane_stride), *spec._tail(), c_void_p(angle_ptr),
                                     c_void_p(score_ptr), c_void_p(best_ptr), c_void_p(norm2_ptr), int(out_plane_stride),
                                     c_void_p(stream)), "zk_align_planes_dev")


def _check_plan_labels(plan, spec):
    if len(spec.n) != plan.n_poly:
        raise ValueError(f"the templates carry {len(spec.n)} moments but the plan has {plan.n_poly}")


def frame_align(plan, image, spec, row0=0, n_rows=None):
    """``zk_frame_align``: host frame ``(H, W)`` (one of the element types of ``ZPs.transform``) -> the maps of its output rows
    ``[row0, row0 + n_rows)``: ``(angle (T, n_rows, W), score (T, n_rows, W), best (n_rows, W) int32, norm2 (n_rows, W))`` host
    arrays.  ``plan``: the :class:`Plan` whose dense transform feeds the search; ``spec`` carries the plan's labels."""
    _check_plan_labels(plan, spec)
    h, w = image.shape
    n_rows = h - row0 if n_rows is None else int(n_rows)
    if row0 < 0 or n_rows < 0 or row0 + n_rows > h:
        raise ValueError("row band outside the frame")
    t = spec.n_templates
    angle, score = pinned.empty((t, n_rows, w)), pinned.empty((t, n_rows, w))
    best, norm2 = np.empty((n_rows, w), dtype=np.int32), pinned.empty((n_rows, w))
    if n_rows * w:
        check(plan._lib.zk_frame_align(plan._h, image.ctypes.data_as(c_void_p), dtype_code(image.dtype), h, w, int(row0), n_rows,
                                       *spec._tail()[3:], _out_ptr(angle), _out_ptr(score), _out_ptr(best), _out_ptr(norm2), n_rows * w),
              "zk_frame_align")
    return angle, score, best, norm2


def frame_align_dev(plan, image_ptr, code, height, width, row0, n_rows, spec, angle_ptr, score_ptr, best_ptr, norm2_ptr,
                    out_plane_stride, stream=0):
    """``zk_frame_align_dev``: frame and outputs on the device (an output pointer may be 0), enqueued on ``stream``."""
    _check_plan_labels(plan, spec)
    check(plan._lib.zk_frame_align_dev(plan._h, c_void_p(image_ptr), int(code), int(height), int(width), int(row0), int(n_rows),
                                       *spec._tail()[3:], c_void_p(angle_ptr), c_void_p(score_ptr), c_void_p(best_ptr), c_void_p(norm2_ptr),
                                       int(out_plane_stride), c_void_p(stream)), "zk_frame_align_dev")


def align_set_band_bytes(band_bytes, device=None):
    """Bytes of moments per row band of :func:`frame_align` / :func:`frame_align_dev` (0: the default of 1 GiB; never less than
    one row)."""
    check(load().zk_align_set_band_bytes(default_device() if device is None else int(device), int(band_bytes)),
          "zk_align_set_band_bytes")


def gpa_set_run_bytes(run_bytes, device=None):
    """Bytes of complex fields per run of frames of ``zk_gpa`` / ``zk_gpa_dev`` (0: the default of 1 GiB; never less than one
    frame)."""
    check(load().zk_gpa_set_run_bytes(default_device() if device is None else int(device), int(run_bytes)), "zk_gpa_set_run_bytes")


def _labels32(n, m):
    n32, m32 = np.ascontiguousarray(n, dtype=np.int32).ravel(), np.ascontiguousarray(m, dtype=np.int32).ravel()
    check_paired(n32, m32)
    return n32, m32


def rotate_rows(rows, n, m, angles, out=None, device=None):
    """``zk_rotate_rows``: host rows ``(N, P)`` float64, each rotated by its own angle (degrees) -> ``(N, P)``; ``out`` may be
    ``rows`` itself (in place)."""
    n32, m32 = _labels32(n, m)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    angles = np.ascontiguousarray(angles, dtype=np.float64).ravel()
    if rows.ndim != 2 or rows.shape[1] != len(n32) or angles.shape[0] != rows.shape[0]:
        raise ValueError(f"rows must be (N, {len(n32)}) and angles (N)")
    if out is None:
        out = np.empty_like(rows)
    elif out.shape != rows.shape or out.dtype != np.float64 or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float64 array of the rows' shape")
    if rows.shape[0] == 0:
        return out
    require_device()
    dev = default_device() if device is None else int(device)
    pi = POINTER(c_int32)
    check(load().zk_rotate_rows(dev, rows.ctypes.data_as(c_void_p), rows.shape[0], len(n32), n32.ctypes.data_as(pi), m32.ctypes.data_as(pi),
                                angles.ctypes.data_as(c_void_p), out.ctypes.data_as(c_void_p)), "zk_rotate_rows")
    return out


def rotate_rows_dev(device, rows_ptr, n_rows, n, m, angles_ptr, out_ptr, stream=0):
    """``zk_rotate_rows_dev``: everything on the device, enqueued on ``stream``; ``out_ptr`` may equal ``rows_ptr``."""
    n32, m32 = _labels32(n, m)
    pi = POINTER(c_int32)
    check(load().zk_rotate_rows_dev(int(device), c_void_p(rows_ptr), int(n_rows), len(n32), n32.ctypes.data_as(pi), m32.ctypes.data_as(pi),
                                    c_void_p(angles_ptr), c_void_p(out_ptr), c_void_p(stream)), "zk_rotate_rows_dev")


def allgather_rows_plan(rank, world, n_planes, height, width, rows_per_rank, row_off, n_rows, algo=COMM_AUTO):
    """The schedule ``zk_allgather_rows`` executes on rank ``rank`` of ``world``, as a list of
    ``(op, peer, group, plane, offset, count)`` tuples in issue order (``zk_allgather_rows_plan``; pure host code)."""
    lib = load()
    if isinstance(algo, str):
        algo = COMM_ALGOS[algo]
    need = c_int64()
    args = (int(rank), int(world), int(n_planes), int(height), int(width), int(rows_per_rank), int(row_off), int(n_rows),
            int(algo))
    check(lib.zk_allgather_rows_plan(*args, None, 0, byref(need)), "zk_allgather_rows_plan")
    buf = (Xfer * max(1, need.value))()
    check(lib.zk_allgather_rows_plan(*args, buf, need.value, byref(need)), "zk_allgather_rows_plan")
    return [(x.op, x.peer, x.group, x.plane, x.offset, x.count) for x in buf[:need.value]]


class Comm:
    """Owns one ``zk_comm``: this process's endpoint of the RCCL communicator (one process per GPU).

    Rendezvous: ``Comm(device, rank, world, path=...)`` -- ranks of one node meet through a file rank 0
    writes; ``host=/port=`` -- rank 0 listens on a TCP port; ``unique_id=`` -- the caller moved the
    128-byte id from rank 0 (``Comm.unique_id()``) to the others by its own means."""

    ID_BYTES = 128

    def __init__(self, device, rank, world, path=None, host=None, port=None, unique_id=None, timeout=120.0):
        lib = load()
        handle = c_void_p()
        self.device, self.rank, self.world = int(device), int(rank), int(world)
        if unique_id is not None:
            buf = ctypes.create_string_buffer(bytes(unique_id), self.ID_BYTES)
            check(lib.zk_comm_init_rank(self.device, self.rank, self.world, buf, byref(handle)), "zk_comm_init_rank")
        elif path is not None:
            check(lib.zk_comm_init_file(self.device, self.rank, self.world, os.fsencode(path), float(timeout),
                                        byref(handle)), "zk_comm_init_file")
        elif port is not None:
            check(lib.zk_comm_init_tcp(self.device, self.rank, self.world, (host or "127.0.0.1").encode(), int(port),
                                       float(timeout), byref(handle)), "zk_comm_init_tcp")
        else:
            raise ValueError("Comm needs one of path=, port= or unique_id=")
        self._h, self._lib = handle, lib

    def ranks_seen(self):
        """World size as the communicator inside the library holds it (``zk_comm_world``)."""
        return int(self._lib.zk_comm_world(self._h))

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(Comm.ID_BYTES)
        check(load().zk_comm_unique_id(buf), "zk_comm_unique_id")
        return buf.raw

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zk_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def allgather_rows(self, full_ptr, n_planes, height, width, rows_per_rank, row_off, n_rows, stream=0):
        """In-place all-gather of the row window ``[row_off, row_off+n_rows)`` of every rank's block of the
        ``(n_planes, height, width)`` float64 array at ``full_ptr`` (see ``zk_allgather_rows``)."""
        check(self._lib.zk_allgather_rows(self._h, c_void_p(full_ptr), n_planes, height, width, rows_per_rank,
                                          row_off, n_rows, c_void_p(stream)), "zk_allgather_rows")

    def join(self, stream=0):
        check(self._lib.zk_comm_join(self._h, c_void_p(stream)), "zk_comm_join")

    def allgather_host(self, payload: bytes):
        """Blocking all-gather of the same number of host bytes from every rank; returns the list of every rank's bytes."""
        n = len(payload)
        send = ctypes.create_string_buffer(payload, n)
        recv = ctypes.create_string_buffer(n * self.world)
        check(self._lib.zk_comm_allgather_host(self._h, send, recv, n), "zk_comm_allgather_host")
        return [recv.raw[r * n:(r + 1) * n] for r in range(self.world)]


class _DeviceRef:
    """What ``array.device`` answers for a :class:`DeviceArray` (``.index``, ``.type``: the attributes the drivers read)."""
    type = "cuda"

    def __init__(self, index):
        self.index = int(index)

    def __repr__(self):
        return f"device(index={self.index})"


class DeviceArray:
    """A C-contiguous array in device memory, allocated through the library (``zk_device_malloc``) -- what the device entry
    points and the sharded drivers of :mod:`mtflearn_amd.distributed` run on when torch is not used at all.  It offers the few
    attributes those functions read from an operand (``shape``, ``dtype``, ``device.index``, ``data_ptr()``, ``numel()``,
    ``element_size()``, ``is_cuda``, ``is_contiguous()``) and views of whole leading-axis items (``a[i]``, ``a[lo:hi]``).
    Work on it runs on the device's default stream (stream 0)."""
    is_cuda = True

    def __init__(self, shape, dtype=np.float64, device=0, _base=None, _ptr=0):
        self.shape = tuple(int(v) for v in (shape if hasattr(shape, "__len__") else (shape,)))
        self.dtype = np.dtype(dtype)
        self.device = _DeviceRef(device)
        self._base = _base                       # the owning array of a view
        if _base is None:
            ptr = c_void_p()
            check(load().zk_device_malloc(self.device.index, max(self.nbytes, 16), byref(ptr)), "zk_device_malloc")
            self._ptr = int(ptr.value)
        else:
            self._ptr = int(_ptr)

    # ---- the tensor-like surface ----
    @property
    def nbytes(self):
        return self.numel() * self.dtype.itemsize

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64)) if self.shape else 1

    def element_size(self):
        return self.dtype.itemsize

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return True

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        if not self.shape:
            raise IndexError("a 0-d DeviceArray has no items")
        n = self.shape[0]
        item = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        owner = self if self._base is None else self._base
        if isinstance(key, (int, np.integer)):
            i = int(key) + (n if key < 0 else 0)
            if not 0 <= i < n:
                raise IndexError(f"index {key} out of range for axis 0 with size {n}")
            return DeviceArray(self.shape[1:], self.dtype, self.device.index, _base=owner, _ptr=self._ptr + i * item)
        if isinstance(key, slice):
            lo, hi, step = key.indices(n)
            if step != 1:
                raise IndexError("only contiguous slices of the leading axis are views")
            hi = max(hi, lo)
            return DeviceArray((hi - lo,) + self.shape[1:], self.dtype, self.device.index, _base=owner, _ptr=self._ptr + lo * item)
        raise IndexError("DeviceArray views take an integer or a contiguous slice of the leading axis")

    # ---- host <-> device ----
    @classmethod
    def from_numpy(cls, array, device=0):
        array = np.ascontiguousarray(array)
        out = cls(array.shape, array.dtype, device)
        if array.nbytes:
            check(load().zk_device_copy(out.device.index, c_void_p(out._ptr), array.ctypes.data_as(c_void_p), array.nbytes, 1), "zk_device_copy")
        return out

    def numpy(self):
        """A host copy (the device is synchronised first: pending work on any stream of it has written its results)."""
        check(load().zk_device_synchronize(self.device.index), "zk_device_synchronize")
        out = np.empty(self.shape, dtype=self.dtype)
        if out.nbytes:
            check(load().zk_device_copy(self.device.index, out.ctypes.data_as(c_void_p), c_void_p(self._ptr), out.nbytes, 2), "zk_device_copy")
        return out

    def fill_(self, value):
        """Fill with a constant (through a host array: a test / set-up helper, not a fast path)."""
        host = np.full(self.shape, value, dtype=self.dtype)
        if host.nbytes:
            check(load().zk_device_copy(self.device.index, c_void_p(self._ptr), host.ctypes.data_as(c_void_p), host.nbytes, 1), "zk_device_copy")
        return self

    def close(self):
        if self._base is None and getattr(self, "_ptr", 0):
            load().zk_device_free(self.device.index, c_void_p(self._ptr))
            self._ptr = 0

    __del__ = close
