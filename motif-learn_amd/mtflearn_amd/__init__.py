"""mtflearn_amd -- MI355X-native drop-in for motif-learn's ``ZPs`` / ``zmoments`` hot path.

``from mtflearn_amd import ZPs, zmoments`` mirrors ``from mtflearn import ZPs, zmoments``
(reference ``mtflearn/__init__.py:37-38``).  Only this path and the rows SURVEY 8(f) names around it are provided
(``mtflearn_amd.features``: parameter pickers, ``pca``, the Fourier window-size estimators
``get_characteristic_length`` / ``get_characteristic_length_fft`` / ``compute_autocorrelation`` with ``fft_power_spectrum`` /
``angular_average``; ``mtflearn_amd.clustering``: ``kmeans_lbs`` / ``gmm_lbs`` /
``sort_lbs``; ``mtflearn_amd.manifold``: ``ForceGraph8``; ``mtflearn_amd.background``: ``estimate_background_*`` /
``remove_background_*`` and their parameter picker; ``mtflearn_amd.denoise``: ``denoise_svd`` / ``DenoiseSVD`` /
``denoise_svd_memory_view``, the reference's other two top-level names; ``mtflearn_amd.utils``: ``normalize_image`` /
``normalize_image_robust`` / ``standardize_image`` / ``percentile_clip`` / ``value_clip``; ``mtflearn_amd.datasets``:
``HoneyCombLattice`` / ``add_tapered_gaussian`` / ``get_zps_test_image`` / ``get_zps_test_patches``, the noise models and
``TMDImageSimulator``, the labelled defect frames;
``mtflearn_amd.graph``: ``find_regions`` / ``LatticeGraph`` / ``MotifsGraph``, the polygons of a lattice graph;
``mtflearn_amd.eels``: ``baseline_als`` / ``baseline_snip`` / ``baseline_arpls`` / ``baseline_airpls`` / ``WhittakerSmooth`` /
``remove_baseline`` over whole spectrum cubes; ``mtflearn_amd.registration``: ``estimate_shifts`` / ``shift_stack`` /
``register_stack``, sub-pixel drift of a frame stack and its average, and ``mtflearn_amd.strain``: ``gpa`` / ``pick_g``, strain and
rotation maps by geometric phase analysis, both beyond the reference); see DESIGN.md.
"""
__version__ = "0.1.0"

from .features import ZPs, zmoments
from . import features
from ._denoise_svd import DenoiseSVD, denoise_svd

__all__ = ["ZPs", "zmoments", "features", "denoise_svd", "DenoiseSVD"]
