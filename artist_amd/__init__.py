"""artist_amd - MI355X-native (gfx950) implementation of ARTIST's heliostat ray-tracing hot path.

Scope: NURBS surface points + normals, ray-mirror reflection, sun-shape
scattering, receiver-plane intersection and the bilinear scatter-add flux bitmap, forward and
backward, behind ARTIST's own call surface:

    artist_amd.HeliostatRayTracer   <-> artist.raytracing.heliostat_ray_tracer.HeliostatRayTracer
    artist_amd.NURBSSurfaces        <-> artist.nurbs.NURBSSurfaces
    artist_amd.crop_flux_distributions_around_center, get_center_of_mass, PixelLoss, KLDivergenceLoss, FocalSpotLoss
                                    <-> artist.flux.bitmap / artist.optim.loss (the per-epoch flux epilogue)
    artist_amd.JensenShannonLoss, ShapePixelLoss, TotalVariationLoss, CosineFluxLoss
                                    (no counterpart) flux losses that do not depend on the gain of either bitmap
    artist_amd.RigidBody            <-> artist.field.kinematics_rigid_body.RigidBody (ideal + linear actuators)
    artist_amd.Scenario             <-> artist.scenario.scenario.Scenario (load_scenario_from_hdf5, index_mapping)
    artist_amd.optim.Adam           <-> torch.optim.Adam as the reconstructors use it (the epoch's optimiser step)
    artist_amd.optim.AimPointOptimizer, artist_amd.training, artist_amd.flux.trapezoid_distribution
                                    <-> artist.optim.AimPointOptimizer, artist.optim.training, artist.flux.bitmap.trapezoid_distribution
    artist_amd.optim.SurfaceReconstructor <-> artist.optim.SurfaceReconstructor (CalibrationSamples: its data parser, in memory;
                                              parameters=(...): facet canting and translations learn too, beyond the reference)
    artist_amd.optim.KinematicsReconstructor, VectorLoss, AngleLoss, CosineSimilarityLoss
                                    <-> artist.optim.KinematicsReconstructor ("raytracing" and "alignment"), artist.optim.loss
    artist_amd.SmoothnessRegularizer, IdealSurfaceRegularizer
                                    <-> artist.optim.SmoothnessRegularizer, IdealSurfaceRegularizer (the epoch's regularisers)
    artist_amd.SurfaceGenerator     <-> artist.scenario.surface_generator.SurfaceGenerator (+ fit_nurbs_batch: all facets at once)
    artist_amd.optics               (no counterpart) per-heliostat reflectivity, attenuation by slant range and optical error
    artist_amd.blur_flux, optics.sun_image_covariance, Sun.integration = "convolved"
                                    (no counterpart) the convolved sun: one chief ray per point and a Gaussian window per bitmap
    artist_amd.radial_blur_flux, optics.radial_window_kept_fraction, Sun.window = "shape"
                                    (no counterpart) the convolved sun for pillbox, Buie and tabulated shapes: a radial window
    artist_amd.differentiable_blur_flux, Sun.window_gradient
                                    (no counterpart) the convolved sun's window learns: optical errors from flux images
    artist_amd.EpochGraph           (no counterpart) an epoch captured into a HIP graph and replayed: same bits, one host call

All arithmetic runs in hand-written HIP kernels (``artist_amd/csrc``) reached through the C ABI in
``include/artist_hip.h``; there is no CPU fallback.
"""
from ._lib import ArtistHipError, build, lib  # noqa: F401
from .nurbs import NURBSSurfaces, create_nurbs_evaluation_grid, create_planar_nurbs_control_points  # noqa: F401
from .flux import (CosineFluxLoss, FocalSpotLoss, JensenShannonLoss, KLDivergenceLoss, PixelLoss, ShapePixelLoss,  # noqa: F401
                   TotalVariationLoss, bitmap_coordinates_to_target_coordinates, blur_flux, crop_and_kl_loss, crop_and_pixel_loss,
                   crop_flux_distributions_around_center, differentiable_blur_flux, get_center_of_mass, radial_blur_flux, trapezoid_distribution)
from .kinematics import Actuators, RigidBody  # noqa: F401
from .ops import align_surfaces, nurbs_surface_points_and_normals, per_target_sum, perform_canting, trace_rays  # noqa: F401
from . import optics, optim, training  # noqa: F401
from .aim_point_optimizer import AimPointOptimizer  # noqa: F401
from .surface_reconstructor import CalibrationSamples, SurfaceReconstructor, flux_integral_constraint  # noqa: F401
from .kinematics_reconstructor import KinematicsReconstructor  # noqa: F401
from .regularizers import IdealSurfaceRegularizer, SmoothnessRegularizer, surface_regularization_terms  # noqa: F401
from .raytracing import HeliostatRayTracer  # noqa: F401
from .scenario import Scenario, open_scenario_file  # noqa: F401
from .sampling import DistortionsDataset, RestrictedDistributedSampler  # noqa: F401
from .surface_generator import FittedFacet, SurfaceGenerator  # noqa: F401
from .graphs import EpochGraph  # noqa: F401

__version__ = "0.1.0"
