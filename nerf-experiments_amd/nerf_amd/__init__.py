"""nerf_amd — MI355X (gfx950) NeRF ray-marching hot path behind the
sarphiv/nerf-experiments module API (positional_encodings, NerfModel,
NerfInterpolation).  See DESIGN.md at the repository root."""
from . import _lib, kernels  # noqa: F401
from .positional_encodings import (BarfPositionalEncoding, FourierFeatures, IdentityPositionalEncoding,  # noqa: F401
                                   IntegratedBarfFourierFeatures, IntegratedFourierFeatures, PositionalEncoding)
from .model_interpolation_architecture import NerfBaseModel, NerfModel  # noqa: F401
from .model_interpolation import MAGIC_NUMBER, NerfInterpolation, SchedulerLeNice  # noqa: F401
from .model_garf import GaussAct, ProposalNetwork, RadianceNetwork  # noqa: F401
# the GaborF / SARF networks share the GARF class names: import them from their modules
from .model_gaborf import GaborAct  # noqa: F401
from .model_sarf import SarfAct  # noqa: F401
from .model_ingp import INGPEncoding, INGPTable, NaiveINGP, NerfModelINGP  # noqa: F401
# the SIREN field network stays nerf_amd.model_siren.NerfModel (NerfModel above is the interpolation one)
from .model_siren import LinearSine, NerfSiren  # noqa: F401
from .model_2d import FourierFeatures2d, Nerf2d  # noqa: F401
from .model_ingp2d import Gigapixel  # noqa: F401  (its INGPTable / INGPEncoding stay in model_ingp2d)
from .optim import FusedAdam  # noqa: F401
from .pose import compute_pose_error, kabsch_algorithm, validation_transform_rays  # noqa: F401
from .prop_sampler import PropNetEstimator, render_weight_from_density, rendering  # noqa: F401
from .occ_grid import CascadedOccGridEstimator, OccGridEstimator  # noqa: F401
from .occ_render import OccGridRenderer, distortion, packed_points  # noqa: F401
from .model_ngp import (NGPRadianceField, SHEncoding, contract_to_unisphere, normalize_to_aabb,  # noqa: F401
                        trunc_exp)

__version__ = "0.1.0"
