"""
fastbox_amd -- MI355X-native density-field hot path of philbull/FastBox.

    from fastbox_amd import CosmoBox, default_cosmo      # as fastbox.box

Importing the package does not need a GPU; constructing a ``CosmoBox`` does
(the HIP library is loaded and a plan is created on the device; there is no
CPU fallback).
"""
from .box import CosmoBox, default_cosmo          # noqa: F401
from .transfer import BeamHighpass, Wedge         # noqa: F401
from .device import DeviceArray                   # noqa: F401
from .sky import ForegroundModel, NoiseModel      # noqa: F401
from . import filters                             # noqa: F401
from . import inpaint                             # noqa: F401
from . import losfit                              # noqa: F401
from .losfit import GPRKernel, LSQfitting         # noqa: F401
from . import analysis                            # noqa: F401
from .analysis import interpolate_onto_grid, grid_catalogue   # noqa: F401
from . import utils                               # noqa: F401
from .utils import comoving_dimensions_from_survey            # noqa: F401
from . import montecarlo                          # noqa: F401
from .beams import BeamModel                      # noqa: F401
from .halos import HaloDistribution, HaloCatalogue, ColaParticles   # noqa: F401
from . import recon                               # noqa: F401
from .recon import Reconstruction                 # noqa: F401
from . import minkowski                           # noqa: F401
from .minkowski import MinkowskiFunctionals, minkowski_functionals   # noqa: F401
from . import web                                 # noqa: F401
from .web import CosmicWeb, TensorField           # noqa: F401
from . import interferometer                      # noqa: F401
from .interferometer import Interferometer, UVCoverage, Observation   # noqa: F401

__version__ = "0.1.0"
