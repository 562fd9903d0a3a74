"""Drop-in for ``artist.raytracing.heliostat_ray_tracer.HeliostatRayTracer`` on MI355X.

Same constructor arguments, method names, return values and error behaviour as
``artist/raytracing/heliostat_ray_tracer.py:19-778``; the per-batch Python loop of eager ATen
ops inside ``trace_rays`` (:316-506) is ONE fused HIP kernel launch (``art_trace_fwd``), and its
autograd is ``art_trace_bwd``.  ``scenario`` / ``heliostat_group`` are duck-typed: ARTIST's own
``Scenario`` / ``HeliostatGroup`` objects work unchanged, and so do the light stand-ins in
``artist_amd.scene`` used by the tests and the benchmark.

Multi-rank contract (the reference's is broken for world_size > 1): a rank
returns rows for the heliostat samples it OWNS only, in ``get_sampler_indices()`` order, so that
``get_bitmaps_per_target(flux_local, target_area_indices[sampler_indices])`` is well defined and
the sum over ranks equals the single-rank result.
"""
from __future__ import annotations

import os

import logging

import torch

from . import _lib, ops, optics
from ._memo import Memo
from .blocking import create_blocking_primitives_rectangles_by_index, create_shading_primitives
from .flux import blur_flux, differentiable_blur_flux, radial_blur_flux
from .sampling import DistortionsDataset, RestrictedDistributedSampler

log = logging.getLogger(__name__)

_DEFAULT_RESOLUTION = torch.tensor([256, 256])   # artist/util/indices.py:307


def reflect(incident_ray_directions: torch.Tensor, reflection_surface_normals: torch.Tensor) -> torch.Tensor:
    """``i - 2 (i.n) n`` (artist/raytracing/geometry.py:11-41); only used to publish
    ``heliostat_group.preferred_reflection_directions`` - the kernel reflects in registers.  ``[H,1,4]`` directions and
    ``[H,P,4]`` normals on the GPU go through ``art_reflect`` (one pass, the reference's operation order) instead of
    five elementwise torch kernels (0.41 -> 0.07 ms per call at the metric size)."""
    i, nrm = incident_ray_directions, reflection_surface_normals
    if (nrm.is_cuda and nrm.dim() == 3 and nrm.shape[-1] == 4 and i.dim() == 3 and i.shape == (nrm.shape[0], 1, 4)
            and nrm.dtype == torch.float32 and i.dtype == torch.float32 and not torch.is_grad_enabled()):
        return ops.reflect_directions(i[:, 0], nrm)
    return i - 2 * torch.sum(i * nrm, dim=-1, keepdim=True) * nrm


def target_area_counts(tower) -> tuple[int, int]:
    """(planar, cylindrical) target areas of a tower, from the HOST side of its tables (``number_of_target_areas`` is
    ``len(names)``, artist/field/tower_target_areas.py:62): ``solar_tower.number_of_target_areas_per_type``
    is a device tensor, and reading it costs a host-device synchronisation in every call."""
    counts = []
    for k in range(2):
        if k >= len(tower.target_areas):
            counts.append(0)
            continue
        area = tower.target_areas[k]
        n = getattr(area, "number_of_target_areas", None)
        if not isinstance(n, int):
            table = getattr(area, "centers", None)
            n = int(table.shape[0]) if table is not None else 0
        counts.append(n)
    return counts[0], counts[1]


def _planar_tables(tower, device):
    """(centers [T,4], normals [T,4], dimensions [T,2]) of ``solar_tower.target_areas[planar]``; empty tables when
    the tower has cylindrical receivers only."""
    planar = tower.target_areas[0]
    if target_area_counts(tower)[0] == 0 or not hasattr(planar, "centers"):
        z = torch.zeros((0, 4), device=device)
        return z, z, torch.zeros((0, 2), device=device)
    return planar.centers, planar.normals, planar.dimensions


def _cylinder_tables(tower):
    """The six ``TowerTargetAreasCylindrical`` tensors (artist/field/tower_target_areas_cylindrical.py:52-102) or
    None when the tower has none."""
    if target_area_counts(tower)[1] == 0:
        return None
    c = tower.target_areas[1]
    return (c.centers, c.normals, c.axes, c.radii, c.heights, c.opening_angles)


class _ChiefRayDataset:
    """The distortions of a convolved sun (``Sun.integration == "convolved"``): one ray per point and no tilt, ``[rows,1,P]``
    views of one interleaved buffer like a sample's.  Nothing is drawn."""

    def __init__(self, number_of_rows: int, number_of_points: int, device) -> None:
        both = torch.zeros((int(number_of_rows), 1, int(number_of_points), 2), dtype=torch.float32, device=device)
        self.distortions_u, self.distortions_e = both[..., 0], both[..., 1]


class HeliostatRayTracer:
    """See ``artist/raytracing/heliostat_ray_tracer.py:19-69`` for the attribute documentation.

    ``shading_active`` (an extension; the reference has no shading): the sun ray to a mirror point can be stopped by a
    neighbouring heliostat before it arrives, evaluated with the blocking mask against per-heliostat sheared copies of the
    neighbours' rectangles.  The third factor returned by ``trace_rays``, ``blocking_factor``, then counts the
    rays that are neither blocked nor shaded.  ``shading_active=True`` with ``blocking_active=False`` traces with shading
    only: the rectangles are built, the blocking filter is skipped.

    A light source with ``integration == "convolved"`` (``artist_amd.scene.Sun``; read here, when the tracer is built;
    DESIGN.md 4.16) is not sampled: every mirror point sends its one undistorted chief ray, carrying the power of the
    ``number_of_rays`` rays it stands for, and each heliostat's bitmap is convolved with the Gaussian image of the sun on its
    target (``optics.sun_image_covariance``, ``flux.blur_flux``) - the expectation of the sampled bitmap to first order,
    without sampling noise, differentiable like it.  The sun's angular covariance is ``scale_tril scale_tril^T`` plus
    ``sigma_h^2 I`` for a heliostat with an optical error (exact: both are Gaussian).  For a Gaussian sun centred on 0, planar
    targets and constant optical errors (``ValueError`` otherwise), on the GPU.  Known limits: a chief ray that misses the target
    contributes nothing, though part of its image would land on it; blocking and shading act on the chief rays; the window does
    not depend on the learned surface and is not differentiated.  The three factors returned by the trace calls are those of
    the chief rays.

    A radial sun (pillbox, Buie, tabulated) is convolved when its ``window == "shape"`` (read with ``integration``; DESIGN.md
    4.17): the window is then the sun's quantile table on the ellipses of the metric ``M = J J^T``
    (``sun_image_covariance`` of the unit covariance, ``flux.radial_blur_flux``), and a heliostat's optical error is a Gaussian
    blur of covariance ``sigma_h^2 M`` on top of it.  Annuli whose ellipse is wider than 64 pixels are dropped, not deposited
    (``optics.radial_window_kept_fraction``); the other conditions and limits are those above.

    Optical errors that learn (the sun's ``window_gradient = True``, read with ``integration``): the tracer of a
    convolved sun then accepts ``active_optical_errors`` that require grad.  ``C_h = C + sigma_h^2 I`` and ``S_h = J_h C_h J_h^T``
    are formed in the autograd graph (``sun_image_covariance(..., differentiable=True)``) and the blur is
    ``flux.differentiable_blur_flux``, whose backward pass returns the gradient with respect to the window - so a loss on the
    flux images reaches ``sigma_h`` without sampling noise (under ``window = "shape"`` through the Gaussian blur of
    ``sigma_h^2 M`` on top of the radial window, which itself does not learn).  The flux is the flux of the same constants, bit
    for bit; with constant optical errors, or with none, the launches are those of ``window_gradient = False``.  ``sigma_h = 0``
    has zero gradient (``dS/dsigma = 2 sigma M``): start from a positive sigma.  The gradient reaches ``group.optical_errors``
    through ``activate_heliostats``; for a fixed-order sum over a heliostat's activations rebind
    ``group.active_optical_errors = optics.expand_over_samples(group.optical_errors, counts)``."""

    #: publish ``heliostat_group.preferred_reflection_directions`` like the reference does (:285-290)
    publish_reflection_directions = True

    def __init__(self, scenario, heliostat_group, blocking_active: bool = True, world_size: int = 1, rank: int = 0,
                 batch_size: int = 100, random_seed: int = 7, bitmap_resolution: torch.Tensor = _DEFAULT_RESOLUTION,
                 dni: float | None = None, shading_active: bool = False) -> None:
        self.scenario = scenario
        self.heliostat_group = heliostat_group
        self.blocking_active = blocking_active
        self.shading_active = shading_active
        self.world_size = world_size
        self.rank = rank
        self.batch_size = batch_size   # accepted for API parity; the fused kernel has no per-ray intermediates

        self.light_source = scenario.light_sources.light_source_list[0]
        number_of_samples = int(self.heliostat_group.number_of_active_heliostats)
        self.distortions_sampler = RestrictedDistributedSampler(
            number_of_samples=number_of_samples,
            number_of_active_heliostats=int((self.heliostat_group.active_heliostats_mask > 0).sum()),
            world_size=self.world_size,
            rank=self.rank,
        )
        # A rank keeps the distortions of the heliostat samples it owns only (the reference samples all [H,R,P] on every
        # rank, sampling.py:49-53): 8 B per ray of this rank instead of 8 B per ray of the field.
        self.integration = getattr(self.light_source, "integration", "sampled")
        self._radial_window = False     # (set by the checks of a convolved sun)
        self._window_gradient = False   # (the sun's window_gradient, read with its integration)
        self.distortions_dataset = self._chief_rays(number_of_samples) if self.integration == "convolved" else DistortionsDataset(
            light_source=self.light_source,
            number_of_points_per_heliostat=self.heliostat_group.active_surface_points.shape[1],
            number_of_active_heliostats=number_of_samples,
            random_seed=random_seed,
            rows=self.distortions_sampler.rank_indices if self.world_size > 1 else None,
            # sigma of each heliostat's optical error (an extension; None in the reference's groups): the tensor itself on one
            # rank, so that the sun's sample cache recognises it
            optical_errors=getattr(self.heliostat_group, "active_optical_errors", None),
        )
        self.bitmap_resolution = bitmap_resolution
        self._resolution_host = (int(bitmap_resolution[0]), int(bitmap_resolution[1]))

        if self.blocking_active or self.shading_active:
            # heliostat_ray_tracer.py:159-183: every heliostat of every group can block; aligned surfaces where a
            # group has been aligned, horizontal ones at their positions otherwise
            surfaces = []
            for group in self.scenario.heliostat_field.heliostat_groups:
                points = group.surface_points + group.positions.unsqueeze(1)
                mask = group.active_heliostats_mask.bool()
                if mask.any():
                    points = points.index_put((torch.nonzero(mask, as_tuple=True)[0],), group.active_surface_points)
                else:
                    log.warning("Not all heliostat groups have been aligned yet. "
                                "Using horizontal heliostats as blocking planes.")
                surfaces.append(points)
            self.blocking_heliostat_surfaces = torch.cat(
                [group.surface_points for group in self.scenario.heliostat_field.heliostat_groups])
            self.blocking_heliostat_surfaces_active = torch.cat(surfaces)
        #: reproduce which rectangles the reference's LBVH can reach (see artist_amd/blocking.py); False = every
        #: rectangle whose box is hit, as ``lbvh_filter_blocking_planes`` documents
        self.lbvh_compat = True
        #: indices of the rectangles the last ``trace_rays`` call filtered (blocking only)
        self._filter_flags = self._filtered = None
        #: ``(shader_idx [H,S], shade_count [H])`` of the last ``trace_rays`` call (shading only), on the device
        self._shading = None

        if dni is not None:
            # heliostat_ray_tracer.py:185-201
            canting_norm = (torch.norm(self.heliostat_group.canting[0], dim=1)[0])[:2]
            dimensions = (canting_norm * 4) + 0.02
            heliostat_surface_area = dimensions[0] * dimensions[1]
            power_single_heliostat = dni * heliostat_surface_area
            rays_per_heliostat = self.heliostat_group.surface_points.shape[1] * self.light_source.number_of_rays
            self.ray_magnitude = power_single_heliostat / rays_per_heliostat
        else:
            self.ray_magnitude = 1.0
        # a chief ray carries what the rays of its point carry together: the bitmap is the expectation of the sampled one
        self._rays_per_traced_ray = int(self.light_source.number_of_rays) if self.integration == "convolved" else 1
        self._local_cache = None
        # what a trace call learns from its arguments by a host read: once per tensor object and version (artist_amd/_memo.py),
        # so index tensors and masks are changed with tracked in-place ops, or replaced
        self._checked_targets = Memo("the host check of target_area_indices")
        self._checked_factors = Memo("the host check of a per-heliostat intensity factor", capacity=4)
        self._owner = Memo("the rectangle index of each active heliostat (nonzero)")
        self._scatter_angle = Memo("the largest scatter angle of the distortions")

    # ------------------------------------------------------------------------------------------
    def _chief_rays(self, number_of_samples: int) -> _ChiefRayDataset:
        """The checks of a convolved sun, and its zero distortions for the rows this rank owns."""
        from .scene import RadialSunShape
        sun = self.light_source
        dist = getattr(sun, "distribution", None)
        # the window of a radial sun: its own image (Sun.window = "shape"); a normal sun's is the Gaussian either way
        self._radial_window = isinstance(dist, RadialSunShape) and getattr(sun, "window", "gaussian") == "shape"
        self._window_gradient = bool(getattr(sun, "window_gradient", False))
        if not self._radial_window and not isinstance(dist, torch.distributions.MultivariateNormal):
            raise ValueError("integration='convolved' needs a Gaussian sun (distribution_type 'normal'): the image of a radial sun "
                             "shape (pillbox, Buie, tabulated) is not a Gaussian window; set the sun's window = 'shape' to convolve "
                             "with the shape's own image")
        loc, _ = sun._host_law()
        if loc[0] != 0.0 or loc[1] != 0.0:
            raise ValueError(f"integration='convolved' needs a sun centred on 0 (the chief ray is the undistorted one), got loc {loc}")
        errors = getattr(self.heliostat_group, "active_optical_errors", None)
        if errors is not None:
            if not isinstance(errors, torch.Tensor) or tuple(errors.shape) != (number_of_samples,):
                raise ValueError(f"optical_errors must be a tensor with one sigma per active heliostat, shape [{number_of_samples}]; "
                                 f"got {tuple(getattr(errors, 'shape', ()))}")
            if errors.requires_grad and not self._window_gradient:
                raise ValueError("integration='convolved' takes the optical errors as constants (the window is not differentiated): "
                                 "optical_errors.requires_grad must be False")
        if dist.loc.device.type != "cuda":
            raise _lib.ArtistHipError(f"integration='convolved' runs on the GPU only (the light source is on {dist.loc.device}); "
                                      "there is no CPU fallback")
        with torch.no_grad():
            if self._radial_window:     # the unit covariance, whose image is the metric M = J J^T
                self._sun_covariance = torch.tensor([1.0, 0.0, 1.0], device=dist.loc.device)
            else:                     # C = L L^T of the sun's scale_tril, element by element: (C_uu, C_ue, C_ee)
                tril = dist.scale_tril.float()
                self._sun_covariance = torch.stack((tril[0, 0] * tril[0, 0], tril[0, 0] * tril[1, 0],
                                                    tril[1, 0] * tril[1, 0] + tril[1, 1] * tril[1, 1]))
        rows = len(self.distortions_sampler.rank_indices) if self.world_size > 1 else number_of_samples
        return _ChiefRayDataset(rows, self.heliostat_group.active_surface_points.shape[1], dist.loc.device)

    def _angular_covariance(self, idx) -> torch.Tensor:
        """``(C_uu, C_ue, C_ee)`` of the sun (formed when the tracer was built), ``[3]``, or ``[rows,3]`` with the optical errors
        of this rank's rows as the group holds them now: device ops, in the autograd graph of optical errors that learn."""
        C = self._sun_covariance
        variance = self._optical_error_variance(idx)
        if variance is None:
            return C
        return torch.stack((C[0] + variance, C[1].expand_as(variance), C[2] + variance), dim=1)

    def _optical_error_variance(self, idx):
        """``sigma_h^2 [rows]`` of this rank's rows as the group holds the optical errors now (None: the group has none): device
        ops; part of the autograd graph when the errors learn (the sun's ``window_gradient``) and gradients are recorded."""
        errors = getattr(self.heliostat_group, "active_optical_errors", None)
        if errors is None:
            return None
        if errors.requires_grad and not self._window_gradient:
            # (every activation rebinds the group's tensor: what was checked at construction is gone)
            raise ValueError("integration='convolved' takes the optical errors as constants: optical_errors.requires_grad "
                             "must be False")
        if not (errors.requires_grad and torch.is_grad_enabled()):
            errors = errors.detach()
        errors = errors.float().to(self._sun_covariance.device)
        if idx is not None:
            errors = errors.index_select(0, idx)
        return errors * errors           # (no host constant: this runs inside a captured epoch)

    def get_sampler_indices(self) -> torch.Tensor:
        """Indices of the heliostat samples assigned to this rank (:205-218)."""
        return torch.tensor(self.distortions_sampler.rank_indices, device=self.distortions_dataset.distortions_u.device)

    def _local_rows(self, device):
        """(index tensor of the owned heliostat samples or None when this rank owns all, dist_u, dist_e of those rows)."""
        if self._local_cache is not None and self._local_cache[0] == device:
            _lib.keep_alive(*self._local_cache[1:])
            return self._local_cache[1:]
        if _lib.capturing():                           # (index tensors built from host lists: not while the stream is captured)
            raise _lib.first_use_under_capture("the rank's rows of the distortions")
        ds = self.distortions_dataset
        du, de = ds.distortions_u, ds.distortions_e
        idx_list = self.distortions_sampler.rank_indices
        n_total = int(self.heliostat_group.number_of_active_heliostats)
        owns_all = len(idx_list) == n_total and idx_list == list(range(n_total))
        if len(idx_list) != du.shape[0]:            # a dataset someone swapped in: select the owned rows here
            sel = torch.tensor(idx_list, dtype=torch.long, device=du.device)
            du, de = du.index_select(0, sel), de.index_select(0, sel)
        if du.device != device:
            both = torch.stack((du, de), dim=-1).to(device)          # one interleaved buffer on the device
            du, de = both[..., 0], both[..., 1]
        idx = None if owns_all else torch.tensor(idx_list, dtype=torch.long, device=device)
        self._local_cache = (device, idx, du, de)
        return idx, du, de

    def _trace(self, incident_ray_directions, active_heliostats_mask, target_area_indices, ray_extinction_factor,
               mirror_reflectivity, device, per_target: bool):
        """The one place that assembles a trace call: alignment check, the rank's rows of every per-heliostat tensor, the
        tower's tables, the blocking rectangles.  ``per_target``: splat into the targets' bitmaps instead of the heliostats'."""
        group = self.heliostat_group
        # (the same tensor object needs no device comparison: one host-device synchronisation less per epoch)
        assert group.active_heliostats_mask is active_heliostats_mask or \
            torch.equal(group.active_heliostats_mask, active_heliostats_mask), \
            "Some heliostats were not aligned and cannot be raytraced."

        points, normals = group.active_surface_points, group.active_surface_normals
        device = points.device if device is None else torch.device(device)
        if self.publish_reflection_directions and not per_target:
            with torch.no_grad():
                group.preferred_reflection_directions = reflect(incident_ray_directions.unsqueeze(1), normals)

        tower = self.scenario.solar_tower
        self._validate_targets(target_area_indices, tower)
        convolved = self.integration == "convolved"
        # a float goes to the kernel as before; a tensor [H] is applied to the traced bitmaps (ops.scale_heliostat_rows)
        ray_extinction_factor, mirror_reflectivity, extinction_rows, reflectivity_rows = ops.split_intensity_factors(
            ray_extinction_factor, mirror_reflectivity, int(group.number_of_active_heliostats), points.device, self._checked_factors)
        scaled = extinction_rows is not None or reflectivity_rows is not None
        idx, dist_u, dist_e = self._local_rows(device)
        if idx is not None:
            points, normals = points.index_select(0, idx), normals.index_select(0, idx)
            extinction_rows = None if extinction_rows is None else extinction_rows.index_select(0, idx)
            reflectivity_rows = None if reflectivity_rows is None else reflectivity_rows.index_select(0, idx)
            incident_ray_directions = incident_ray_directions.index_select(0, idx)
            target_area_indices = target_area_indices.index_select(0, idx)

        width, height = self._resolution_host
        rectangles = self._blocking_arguments(idx, active_heliostats_mask)
        shading = ()
        if self.shading_active:
            corners, _, _, owner, max_scatter, _ = rectangles
            tabs = create_shading_primitives(corners, owner, incident_ray_directions, max_scatter)
            self._shading = (tabs["shader_idx"], tabs["shade_count"])     # (diagnostics: the last call's lists, on the device)
            shading = (tabs["corners"], tabs["spans"], tabs["normals"], tabs["shader_idx"], tabs["shade_count"],
                       bool(self.blocking_active))
        flux, factors, flags = ops.TraceRays.apply(
            points, normals, incident_ray_directions, dist_u, dist_e, target_area_indices, *_planar_tables(tower, points.device),
            float(self.ray_magnitude) * self._rays_per_traced_ray, float(ray_extinction_factor), float(mirror_reflectivity),
            width, height, bool(per_target) and not scaled and not convolved,
            _cylinder_tables(tower), *(rectangles or (None, None, None, None, -1.0, True)),
            self._points_per_facet(points), *shading)
        if self.blocking_active:
            self._filter_flags, self._filtered = flags, None       # (indices on demand: nonzero() waits for the device)
        if convolved and self._radial_window:
            # a radial sun's own image: its table on the ellipses of M = J J^T; a heliostat's optical error, a Gaussian of
            # covariance sigma_h^2 M in pixels, is convolved on top (sigma_h = 0 is the blur's identity)
            metric = optics.sun_image_covariance(
                points, normals, incident_ray_directions, target_area_indices, *_planar_tables(tower, points.device),
                self._sun_covariance, (width, height))
            flux = radial_blur_flux(flux, metric, self.light_source.distribution.quantile_table)
            variance = self._optical_error_variance(idx)
            if variance is not None:
                covariance = metric * variance.unsqueeze(1)
                flux = (differentiable_blur_flux if covariance.requires_grad else blur_flux)(flux, covariance)
        elif convolved:         # the sun's image on each heliostat's target (a new tensor: ops.bitmap_moments has nothing for it)
            angular = self._angular_covariance(idx)
            learns = angular.requires_grad       # optical errors that learn: S in the graph, the blur differentiable in it
            covariance = optics.sun_image_covariance(
                points, normals, incident_ray_directions, target_area_indices, *_planar_tables(tower, points.device),
                angular, (width, height), **(dict(differentiable=True) if learns else {}))
            flux = (differentiable_blur_flux if learns else blur_flux)(flux, covariance)
        if scaled:
            flux, factors = ops.scale_heliostat_rows(flux, factors, extinction_rows, reflectivity_rows)
        if per_target and (scaled or convolved):
            # (the fused per-target mode sums inside the kernel: trace per heliostat, scale or blur, then sum)
            flux = ops.per_target_sum(flux, target_area_indices, sum(target_area_counts(tower)))
        return flux, factors[0], factors[1], factors[2]

    def trace_rays(self, incident_ray_directions: torch.Tensor, active_heliostats_mask: torch.Tensor,
                   target_area_indices: torch.Tensor, ray_extinction_factor: float = 0.0,
                   mirror_reflectivity: float = 0.935, device: torch.device | None = None
                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Heliostat ray tracing (:220-508).  Returns ``(flux [H,res_u,res_e], intercept_factor [H],
        on_target_factor [H], blocking_factor [H])`` for the heliostat samples owned by this rank.  With ``shading_active``
        the blocking factor is the fraction of rays that are neither blocked nor shaded.

        ``ray_extinction_factor`` and ``mirror_reflectivity`` are, independently, a float for the whole field (the reference's
        form; a 0-d or one-element tensor counts as one) or a tensor ``[H]``: one value per active heliostat in activation
        order, field-wide, on the tracer's device - a rank takes its own rows, as it does for the other arguments.  A tensor
        is not handed to the kernel (which then runs with extinction 0 / reflectivity 1 for that factor): bitmap row ``h`` is
        multiplied by ``(1 - eps_h) * rho_h`` afterwards, one differentiable op, so a factor tensor that requires grad
        receives its gradient; the intercept factor of a row with weight 0 is 0.  Such bitmaps are not untouched trace
        outputs: ``ops.bitmap_moments`` has nothing for them and the fused crop forms its own sums (the same bits)."""
        return self._trace(incident_ray_directions, active_heliostats_mask, target_area_indices, ray_extinction_factor,
                           mirror_reflectivity, device, per_target=False)

    @property
    def filtered_blocking_primitive_indices(self):
        """Indices of the blocking rectangles the last ``trace_rays`` call kept (heliostat_ray_tracer.py:445-461) or None.
        The call leaves one flag per rectangle on the device; the index list is made when somebody reads it, so an epoch
        that never looks at it has no host-device synchronisation in its ray tracing."""
        if self._filtered is None and self._filter_flags is not None:
            self._filtered = torch.nonzero(self._filter_flags, as_tuple=True)[0]
            # this read waited for the device anyway: the moment to learn that the filter met more candidate rectangles
            # than the kernels hold (the device-side report of the asynchronous call, ops.check_async_errors)
            ops.check_async_errors(self._filter_flags.device, clear=False)
        return self._filtered

    def finish(self, device: torch.device | None = None) -> None:
        """Wait for the ray tracing queued so far and raise what only the device could find out (a target index outside
        the tables, more blocking rectangles inside one heliostat's ray cone than the kernels hold) -
        ``ops.check_async_errors``.  ``trace_rays`` itself never waits; call this after a single prediction or the last
        epoch (an overflowed heliostat's bitmap and factors are NaN either way)."""
        points = self.heliostat_group.active_surface_points
        ops.check_async_errors(points.device if device is None else device)

    @filtered_blocking_primitive_indices.setter
    def filtered_blocking_primitive_indices(self, value) -> None:
        self._filter_flags, self._filtered = None, value

    def _points_per_facet(self, points) -> int:
        """The group's surface tensors are facet-major ``[H, F * M, 4]`` (heliostat_group.py:26-63): tell the kernels M, so
        that a block of points never holds two facets' images (a layout hint - results do not depend on it)."""
        if os.environ.get("ARTIST_HIP_DEBUG") == "1" and os.environ.get("ARTIST_AMD_FACET_HINT", "1") == "0":      # A/B switch (debug only)
            return 0
        facets = int(getattr(self.heliostat_group, "number_of_facets_per_heliostat", 0) or 0)
        n_points = int(points.shape[1])
        return n_points // facets if facets > 1 and n_points % facets == 0 else 0

    def _validate_targets(self, target_area_indices, tower) -> None:
        """The kernels index the target tables with these: validated on the host, once per tensor object and version
        (one host-device synchronisation, not one per epoch).  The C ABI checks them again on the device and reports
        ``ART_ETARGET`` instead of reading out of bounds (include/artist_hip.h)."""
        def check() -> bool:
            lo, hi = int(target_area_indices.min()), int(target_area_indices.max())
            if lo < 0 or hi >= sum(target_area_counts(tower)):
                raise IndexError("target_area_indices out of range")
            if self.integration == "convolved" and hi >= target_area_counts(tower)[0]:
                raise ValueError("integration='convolved' traces planar target areas only (the sun's image on a cylinder is not "
                                 "one Gaussian window per bitmap); target_area_indices name a cylindrical area")
            return True
        if target_area_indices.numel() > 0:
            self._checked_targets.lookup(target_area_indices, check)

    def _blocking_arguments(self, idx, active_heliostats_mask):
        """Rectangles of all heliostats (:291-301) + the rectangle index of each traced heliostat (:445-448)."""
        if not (self.blocking_active or self.shading_active):
            return ()
        corners, spans, normals = create_blocking_primitives_rectangles_by_index(self.blocking_heliostat_surfaces_active)
        # rectangle index of each active heliostat: once per mask tensor object and version (nonzero() waits for the device)
        def find() -> torch.Tensor:
            owner = torch.nonzero(active_heliostats_mask, as_tuple=True)[0]
            return owner if idx is None else owner.index_select(0, idx.to(owner.device))
        owner = self._owner.lookup((active_heliostats_mask, idx), find)
        return corners, spans, normals, owner, self._max_scatter_angle(), self.lbvh_compat

    def _max_scatter_angle(self) -> float:
        """Largest scatter angle of the distortion dataset: bounds every heliostat's ray cone for the blocking cull.
        Computed once per dataset (one reduction + host read), again if a caller swaps or writes the dataset's tensors: a
        bound that is too small would change results."""
        ds = self.distortions_dataset
        u, e = ds.distortions_u, ds.distortions_e
        return self._scatter_angle.lookup((u, e), lambda: float(torch.maximum(u.abs().max(), e.abs().max())))

    def trace_rays_per_target(self, incident_ray_directions, active_heliostats_mask, target_area_indices,
                              ray_extinction_factor: float = 0.0, mirror_reflectivity: float = 0.935,
                              device: torch.device | None = None):
        """``trace_rays`` + ``get_bitmaps_per_target`` without materialising ``[H,res,res]``: every
        heliostat's rays are splatted straight into its target's bitmap (``[T,res_u,res_e]``, planar areas
        first, cylindrical second).  Extension of the reference API for field-scale flux prediction
        (configs 3 and 5).

        With a tensor ``[H]`` for either intensity factor (see ``trace_rays``) the fused mode cannot be used - it sums
        inside the kernel: the heliostats' bitmaps are traced, scaled and then summed (``art_per_target_sum``), so
        ``[H,res_u,res_e]`` IS materialised; the result equals ``get_bitmaps_per_target(trace_rays(...))`` bit for bit."""
        return self._trace(incident_ray_directions, active_heliostats_mask, target_area_indices, ray_extinction_factor,
                           mirror_reflectivity, device, per_target=True)

    def get_bitmaps_per_target(self, bitmaps_per_heliostat: torch.Tensor, target_area_indices: torch.Tensor,
                               device: torch.device | None = None) -> torch.Tensor:
        """Bitmaps per heliostat -> bitmaps per target area ``[T,res_u,res_e]`` (:563-608)."""
        n_targets = sum(target_area_counts(self.scenario.solar_tower))
        return ops.per_target_sum(bitmaps_per_heliostat, target_area_indices, n_targets)
