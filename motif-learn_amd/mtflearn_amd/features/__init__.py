"""Hot-path subset of ``mtflearn.features`` (reference ``mtflearn/features/__init__.py:1-4,11-16``): the transformer,
the moment container and index algebra, the two routines that pick its parameters, the key-point
detector and caller, and the Fourier window-size estimators of ``features/_window_size.py`` / ``_fft_related.py``
(``compute_autocorrelation``, ``get_characteristic_length``, ``get_characteristic_length_fft``, ``fft_power_spectrum``,
``angular_average``: :mod:`.window_size`), which also take whole stacks of frames."""
from .zernike_polys import ZPs
from .moments import (zmoments, construct_rot_maps_matrix, construct_complex_matrix,
                      construct_real_matrix, nm2j, nm2j_complex, check_array1d)
from .pickers import (estimate_patch_size, radial_profile, autocorrelation, estimate_n_max, estimate_n_max_from_patch,
                      _get_cumulative_energy)
from .consumers import pca
from .keypoints import GaussianFit, KeyPoints, com_refine_points, gaussian_fit_points, refine_points
from .peaks import local_max
from .window_size import (compute_autocorrelation, get_characteristic_length, get_characteristic_length_fft,
                          fft_power_spectrum, angular_average)


def baseline_correction(y, niter=10):
    """The reference's ``features/_window_size.py`` holds a second copy of SNIP under this name: an alias of
    :func:`mtflearn_amd.eels.baseline_snip`."""
    from ..eels import baseline_snip
    return baseline_snip(y, niter=niter)


__all__ = ["ZPs", "zmoments", "construct_rot_maps_matrix", "construct_complex_matrix",
           "construct_real_matrix", "nm2j", "nm2j_complex", "check_array1d",
           "estimate_patch_size", "radial_profile", "autocorrelation", "estimate_n_max", "estimate_n_max_from_patch", "pca",
           "KeyPoints", "refine_points", "com_refine_points", "gaussian_fit_points", "GaussianFit", "local_max", "baseline_correction",
           "compute_autocorrelation", "get_characteristic_length", "get_characteristic_length_fft", "fft_power_spectrum",
           "angular_average"]
