"""MI355X-native Chebyshev graph convolution behind the deepsphere layer API.

Only the hot path of deepsphere/deepsphere-cosmo-tf2 lives here: ``gnn_layers.Chebyshev``,
``healpy_layers.HealpyChebyshev``, the Laplacian preparation in ``utils`` and a HEALPix graph
producer in ``healpix``.  The arithmetic runs in ``_lib/libdsphere_hip.so`` (hand-written HIP
for gfx950, C ABI in ``include/dsphere.h``).
"""

__version__ = "0.1.0"

from . import healpix, sht, utils  # noqa: F401
from .gnn_layers import Bernstein, Chebyshev, GCNN_ResidualLayer, Monomial  # noqa: F401
from .gnn_transformers import Graph_Transformer, Graph_ViT  # noqa: F401
from .healpy_layers import (HealpyBernstein, HealpyChebyshev, HealpyMonomial, HealpyPool, HealpyPowerSpectrum,  # noqa: F401
                            HealpyPseudoConv, HealpyPseudoConv_Transpose, HealpyReorder, HealpyRotate, HealpySmoothing, Healpy_ResidualLayer,
                            Healpy_Transformer, Healpy_ViT)
from .healpy_networks import HealpyGCNN  # noqa: F401
