"""Surface reconstruction: learn every heliostat's NURBS control points from measured flux bitmaps of its calibration samples.
Drop-in for ``artist.optim.SurfaceReconstructor`` (artist/optim/surface_reconstructor.py:50-1224): same constructor, same
nested configuration, same ``reconstruct_surfaces()`` and return values, same histories, same loop.

An epoch is assembled from what the package already has, all of it hand-written HIP on the hot path: NURBS
evaluation (``art_nurbs_fwd/_bwd``), orientations from the rigid-body kinematics (``art_rigid_body_fwd``, no gradient),
alignment (``art_align_fwd/_bwd``), the trace without blocking (``art_trace_fwd/_bwd``), the crop around the centre of mass
(``art_flux_crop_fwd/_bwd``), the caller's loss on the cropped bitmaps (``art_flux_loss`` for ``PixelLoss`` /
``KLDivergenceLoss``), the regularisers (``art_surface_regularizers_fwd/_bwd``) and the step (``art_adam_step``).  What is left
on top are vectors per sample and per heliostat: the flux-integral constraint (:func:`flux_integral_constraint`, torch ops on
whichever device its arguments live), the dynamic balancing and the mean.

The samples of one heliostat share one control net.  Each active heliostat's surface is evaluated ONCE per epoch; its points
and normals are repeated over the sample axis and aligned per sample.  Backwards, the per-sample gradients of the points are
summed over that axis as ``[heliostats, samples, ...].sum(1)`` - a fixed order - before the one NURBS adjoint per heliostat:
two runs give the same bits, and the NURBS work does not grow with the number of samples.

Host reads: the loop reads the device ONCE per epoch - the epoch's six scalars, stacked (the stop test, early stopping and
``ReduceLROnPlateau`` need the loss on the host); the multiplier and the reference integrals stay device tensors.  The group is
activated for the training samples once and again after every validation, and one ray tracer per group serves all training
epochs, another all validations: a tracer's distortions depend on the seed and the shapes only.

``epoch_graph=True`` ("The epoch as a graph"): per group the training step - ``predict_flux``, ``epoch_loss``,
``backward()`` - is captured once into an ``artist_amd.EpochGraph`` and replayed every epoch; the multiplier update, the nested
all-reduce, the edge lock, ``Adam.step()``, the one host transfer, the scheduler, early stopping, the history and every
validation stay eager, in the same order.  The replayed epoch gives the eager epoch's bits.

``parameters=(...)`` ("Rigid facet parameters"; beyond the reference's class): the facets' canting vectors and
translations learn beside or instead of the control points.  Their active rows are selected inside the step, the evaluation
takes the staged route (``art_nurbs_fwd`` without canting, ``art_cant_facets_fwd``; backwards ``art_cant_facets_bwd`` and, if
the control points learn, ``art_nurbs_bwd``) - still once per heliostat and epoch, with the same fixed-order sum over the
samples - and the gradient of the homogeneous w components is set to zero before the step.

Slope errors: a group with ``slope_errors`` has every evaluated normal tilted by ``sigma_h * zeta`` (torch ops,
``artist_amd.optics.tilt_normals``) once per heliostat and epoch, between the evaluation and the expansion over the samples;
with ``"slope_errors"`` among the parameters sigma learns, its gradient arriving through the trace's gradient of the normals.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from functools import partial
from typing import Any

import torch

from . import reconstruction
from .flux import KLDivergenceLoss, PixelLoss, crop_flux_distributions_around_center
from .nurbs import NURBSSurfaces, create_nurbs_evaluation_grid
from .raytracing import HeliostatRayTracer
from .reconstruction import LearnsParameters, ReconstructionGroupState, Reconstructor, _TakesParameters, tensors_held_by  # noqa: F401
from .regularizers import surface_regularization_terms
from .training import reduce_loss_per_sample

log = logging.getLogger(__name__)

__all__ = ["SurfaceReconstructor", "CalibrationSamples", "GroupState", "EpochLoss", "flux_integral_constraint", "HISTORY_KEYS",
           "PARAMETER_NAMES", "GEOMETRY_PARAMETER_NAMES", "LEARNING_RATE_KEYS", "canonical_parameters", "learning_rates", "tensors_held_by", "LearnsParameters"]

#: the per-epoch lists of a group's history, in the order the epoch's scalars are stacked; ``"test_loss"`` comes on top
HISTORY_KEYS = ("total_loss", "flux_loss", "smoothness_regularizer", "ideal_regularizer", "flux_integral",
                "flux_integral_constraint")

#: what a reconstruction can learn, in the canonical order: the order of the optimiser's parameter groups, of the reduces in
#: nested mode and of the broadcasts after the run.  The names are the group's attributes.
PARAMETER_NAMES = ("nurbs_control_points", "canting", "facet_translations", "slope_errors")

#: the names whose rates :func:`learning_rates` reports when it is asked for none in particular: the tensors that shape the
#: surface.  ``"slope_errors"`` (sigma per heliostat) has a rate when it is named.
GEOMETRY_PARAMETER_NAMES = PARAMETER_NAMES[:3]

_mean_over_samples = partial(torch.mean, dim=-1)


#: the configuration key of every name's initial learning rate; the first is required and the default of the others
LEARNING_RATE_KEYS = {"nurbs_control_points": "initial_learning_rate", "canting": "initial_learning_rate_canting",
                      "facet_translations": "initial_learning_rate_facet_translations",
                      "slope_errors": "initial_learning_rate_slope_errors"}


def canonical_parameters(parameters, names=PARAMETER_NAMES) -> tuple:
    """``reconstruction.canonical_parameters`` with the surface reconstructor's names as the default."""
    return reconstruction.canonical_parameters(parameters, names)


def learning_rates(optimizer_dict: dict, parameters=None, keys=LEARNING_RATE_KEYS) -> dict:
    """``reconstruction.learning_rates`` with the surface reconstructor's keys as the default: ``"initial_learning_rate"`` for
    the control points, ``"initial_learning_rate_canting"`` and ``"initial_learning_rate_facet_translations"`` for the two
    rigid tensors, ``"initial_learning_rate_slope_errors"`` for sigma.  Asked for no names in particular, these keys report
    the three ``GEOMETRY_PARAMETER_NAMES``."""
    if parameters is None and keys is LEARNING_RATE_KEYS:
        parameters = GEOMETRY_PARAMETER_NAMES
    return reconstruction.learning_rates(optimizer_dict, parameters, keys)


def flux_integral_constraint(cropped_sums: torch.Tensor, reference: torch.Tensor, multiplier, rho: float, energy_tolerance: float,
                             samples_per_heliostat: int, epsilon: float = 1e-12):
    """The augmented-Lagrangian term that keeps a reconstruction from losing power (surface_reconstructor.py:593-654).

    ``cropped_sums`` are the sums of the cropped predictions per sample, ``reference`` those of the first epoch.  A sample
    violates by ``v = max(-energy_tolerance - (sum - reference) / (reference + eps), 0)``: by how much its relative loss of flux
    exceeds the tolerance.  The violation of a heliostat is the mean over its samples, its term ``lambda v + rho / 2 v^2`` with
    the heliostat's ``multiplier`` (a number or ``[heliostats]``).  Returns ``(term [heliostats], relative differences
    [samples], violation [heliostats])``.  After the backward pass the multiplier moves to ``clamp(lambda + rho v, min=0)``.
    Torch ops only, on the device of the arguments."""
    relative = (cropped_sums - reference) / (reference + torch.tensor(epsilon))
    violation = reduce_loss_per_sample(torch.clamp(-energy_tolerance - relative, min=0.0), samples_per_heliostat, _mean_over_samples)
    return multiplier * violation + 0.5 * rho * violation ** 2, relative, violation


class CalibrationSamples:
    """Calibration samples held in memory, for callers without PAINT files: stands where the reference's
    ``CalibrationDataParser`` stands, ``data = {"data_parser": CalibrationSamples(...), "heliostat_data_mapping": []}``.

    ``samples`` are the six tensors of one heliostat group - measured flux ``[N, res_u, res_e]``, focal spots ``[N, 4]``,
    incident ray directions ``[N, 4]``, motor positions ``[N, 2]``, the mask ``[heliostats]`` (samples per heliostat, the same
    for all that have any; a heliostat's samples follow one another) and target area indices ``[N]`` - or a list of such
    six-tuples, one per group in the field's order.  ``parse_data_for_reconstruction`` hands back the group's six, on ``device``."""

    def __init__(self, samples) -> None:
        self.samples = [tuple(samples)] if isinstance(samples[0], torch.Tensor) else [tuple(s) for s in samples]
        for six in self.samples:
            if len(six) != 6:
                raise ValueError("a group's calibration samples are six tensors: measured flux, focal spots, incident ray "
                                 "directions, motor positions, active heliostats mask, target area indices")

    def parse_data_for_reconstruction(self, heliostat_data_mapping, heliostat_group, scenario, bitmap_resolution=None,
                                      device: torch.device | None = None):
        groups = scenario.heliostat_field.heliostat_groups
        index = next(i for i, group in enumerate(groups) if group is heliostat_group)
        return tuple(t.to(device) for t in self.samples[index])


@dataclass
class EpochLoss:
    """One epoch's loss and its parts: ``total`` (the mean of ``total_per_heliostat``), the flux loss per sample and per
    heliostat, the constraint's term, relative differences and violation, the balancing factors and the regularisers."""
    total: torch.Tensor
    total_per_heliostat: torch.Tensor
    flux_loss_per_sample: torch.Tensor
    flux_loss_per_heliostat: torch.Tensor
    constraint: torch.Tensor
    relative_differences: torch.Tensor
    violation: torch.Tensor
    alpha: torch.Tensor
    smoothness: torch.Tensor
    beta: torch.Tensor
    ideal: torch.Tensor

    def scalars(self) -> torch.Tensor:
        """The six history values of the epoch (``HISTORY_KEYS``) as one ``[6]`` tensor on the device."""
        with torch.no_grad():
            return torch.stack([s.detach().reshape(()) for s in (
                self.total, self.flux_loss_per_heliostat.mean(), (self.alpha * self.smoothness).mean(),
                (self.beta * self.ideal).mean(), self.relative_differences.mean(), self.constraint.mean())])


@dataclass(kw_only=True)
class GroupState(ReconstructionGroupState):
    """What the epochs of one heliostat group share (``SurfaceReconstructor.prepare``), beside the fields every reconstruction
    has."""
    original_control_points: torch.Tensor       # the active heliostats' nets before the first step (frozen), [active, F, U, V, 3]
    evaluation_points: torch.Tensor             # [active, F, M, 2] (expanded)
    canting: torch.Tensor
    facet_translations: torch.Tensor
    multiplier: torch.Tensor                    # lambda of the flux-integral constraint, [this rank's heliostats]
    reference_integrals: torch.Tensor | None = None
    aim_points: dict = field(default_factory=dict)
    # epoch_graph: whether the state a captured step reads must stay where it is, and the ideal mount's orientations per kind
    # (constants; their geometry copies from the host in every call)
    static: bool = False
    orientations: dict = field(default_factory=dict)
    # the learnables (in the order of PARAMETER_NAMES) that did not require grad before ``prepare`` marked them
    marked: list = field(default_factory=list)
    # a group with slope errors: zeta of the heliostats that have samples, [active, F, M, 2] (a constant of the run)
    slope_sample: torch.Tensor | None = None


class SurfaceReconstructor(Reconstructor):
    """``artist.optim.SurfaceReconstructor``: see the module docstring; attributes as in the reference (:58-84).

    ``prepare`` / ``predict_flux`` / ``epoch_loss`` / ``validate`` are the pieces ``reconstruct_surfaces`` runs per group, for
    callers that step themselves.

    ``epoch_graph`` (a public attribute, read when a group's loop starts): replay each group's training step from an
    ``artist_amd.EpochGraph`` (:meth:`build_epoch_graph`) instead of running it eagerly; the same bits, less host time per
    epoch.  ``loss_definition`` must then not read the device (``.item()``, ``nonzero``, a host comparison): torch's capture
    error propagates as it is, and there is no fall-back to the eager loop.  After a replay ``heliostat_group.active_surface_points``
    / ``active_surface_normals`` are whatever the last eager call - the capture or a validation - left: a replay does not
    look at the group's ``active_*`` attributes.

    ``parameters`` (an addition, a keyword of the class call after ``epoch_graph``; the reference's class learns the control
    points only).  It is NOT a parameter of ``__init__`` and does not show in its signature: the metaclass ``_TakesParameters``
    takes it from the call, checks it before ``__init__`` runs and sets the attribute after it, so inside ``__init__`` - also
    a subclass's - the attribute still is the default, and ``inspect.signature(SurfaceReconstructor)`` shows ``(*args,
    parameters=..., **kwargs)``.  What learns: a non-empty tuple or list
    of ``"nurbs_control_points"``, ``"canting"`` ``[N, F, 2, 4]`` and ``"facet_translations"`` ``[N, F, 4]`` - the group's
    attributes of these names, in any order; anything else is a ``ValueError``.  Kept as ``self.parameters``, a tuple in
    this order (assigning the attribute checks and orders it the same way), and read in :meth:`prepare`.  A facet that sits
    tilted or shifted on its mounts is then learnt as two vectors and an offset, not by bending its 300 control points against the
    ideal-surface regulariser.  One ``artist_amd.optim.Adam`` steps them, one parameter group each, at
    ``optimization["initial_learning_rate"]``, ``["initial_learning_rate_canting"]`` and
    ``["initial_learning_rate_facet_translations"]`` (the latter two optional, defaulting to the first).  The schedulers scale
    every group; ``cyclic``'s ``lr_min`` / ``lr_max`` are one pair for ALL groups, whatever their initial rates.  The w
    components of both rigid tensors are homogeneous zeros and no parameters: their gradient is set to zero before the step
    (the alignment's adjoint leaves one on a translation's w), so they keep their bits.  Regularisers, constraint, histories,
    validation and the stop logic are the same for every choice; without the control points the two regulariser terms are
    constants of the run.  After the run the rigid tensors that ``prepare`` marked no longer require grad.

    ``"slope_errors"`` ``[N]`` is the fourth name: the group's sigma of the mirrors' slope error, which must be
    set before :meth:`prepare` (``ValueError`` otherwise), at ``optimization["initial_learning_rate_slope_errors"]``.  Alone or
    beside the others; the evaluation keeps the route the other names choose.  A sigma that learns is not checked for its sign
    and is left as its magnitude, detached, on ``group.slope_errors``."""

    def __init__(self, ddp_setup: dict, scenario, data: dict, optimization_configuration: dict[str, Any],
                 dni: float | None = None, number_of_surface_points: torch.Tensor = torch.tensor([50, 50]),
                 bitmap_resolution: torch.Tensor = torch.tensor([256, 256]), epsilon: float | None = 1e-12,
                 plot_results: bool = False, device: torch.device | None = None, epoch_graph: bool = False) -> None:
        if plot_results:
            raise NotImplementedError("plot_results=True: plotting stays ARTIST's (artist/optim/surface_reconstructor.py)")
        self._device(device)
        if ddp_setup["rank"] == 0:
            log.info("Create a surface reconstructor.")
        self.ddp_setup = ddp_setup
        self.scenario = scenario
        self.data = data
        self.optimizer_dict = optimization_configuration["optimization"]
        self.scheduler_dict = optimization_configuration["scheduler"]
        self.constraint_dict = optimization_configuration["constraints"]
        # (host copies: the evaluation grid and every tracer want the sizes on the host)
        self.number_of_surface_points = torch.tensor([int(number_of_surface_points[0]), int(number_of_surface_points[1])])
        self.dni = dni
        self.bitmap_resolution = torch.tensor([int(bitmap_resolution[0]), int(bitmap_resolution[1])])
        self.epsilon = epsilon
        self.plot_results = False
        self.epoch_graph = bool(epoch_graph)
        self.validation_loss_pixel = PixelLoss()
        self.validation_loss_kl_div = KLDivergenceLoss()

    PARAMETER_NAMES = PARAMETER_NAMES           # (the control points alone, unless chosen otherwise)
    HISTORY_KEYS = HISTORY_KEYS
    RECONSTRUCTS = "surface"

    # ------------------------------------------------------------------------------------------
    def prepare(self, heliostat_group_index: int, device: torch.device | None = None) -> GroupState | None:
        """Everything before a group's first epoch (:343-474, 898-966): its calibration samples from
        ``data["data_parser"].parse_data_for_reconstruction``, the train/test split, the evaluation grid, a frozen copy of the
        nets of the heliostats that have samples, ``artist_amd.optim.Adam`` with one parameter group per tensor of
        ``self.parameters`` (``requires_grad_()`` on those, and on no other), the configured scheduler, early stopping and a
        zero multiplier.  None for a group without samples."""
        group = self.scenario.heliostat_field.heliostat_groups[heliostat_group_index]
        if "slope_errors" in self.parameters and getattr(group, "slope_errors", None) is None:
            raise ValueError(f"parameters={self.parameters!r}: heliostat group {heliostat_group_index} has no slope_errors to start "
                             "from; set group.slope_errors to a tensor with one sigma per heliostat before the reconstruction")
        device = self._device(device)
        parsed = self._parse_and_split(heliostat_group_index, device)
        if parsed is None:
            return None
        (_, _, _, _, mask, _), split, active_rows = parsed
        active = int(active_rows.numel())
        grid = create_nurbs_evaluation_grid(self.number_of_surface_points, device=device)
        with torch.no_grad():
            original = group.nurbs_control_points.index_select(0, active_rows).clone()
        # a tensor that is not chosen is left as it is
        learnables = {name: getattr(group, name) for name in self.parameters}
        marked = [tensor for name, tensor in learnables.items() if name != "nurbs_control_points" and not tensor.requires_grad]
        optimizer, scheduler, stopper = self._optimizer_for(learnables, LEARNING_RATE_KEYS)
        state = GroupState(index=heliostat_group_index, group=group, mask=mask, split=split, active_rows=active_rows,
                           original_control_points=original,
                           evaluation_points=grid[None, None].expand(active, int(group.number_of_facets_per_heliostat), -1, -1),
                           canting=group.canting.detach().index_select(0, active_rows),        # (constants unless they learn)
                           facet_translations=group.facet_translations.detach().index_select(0, active_rows),
                           optimizer=optimizer, scheduler=scheduler, early_stopper=stopper, multiplier=torch.zeros((), device=device),
                           learnables=learnables, marked=marked)
        if getattr(group, "slope_errors", None) is not None:
            group.checked_slope_errors()        # (the marked leaf: shape, dtype and device; a constant sigma: its values too)
            facets = int(group.number_of_facets_per_heliostat)
            state.slope_sample = group.slope_sample.index_select(0, active_rows).reshape(active, facets, -1, 2)
        _, heliostat_rows = self._rank_rows(state, "train", device)
        state.multiplier = torch.zeros(active if heliostat_rows is None else int(heliostat_rows.numel()), device=device)
        return state

    def _cropped_flux(self, state: GroupState, kind: str, device) -> torch.Tensor:
        """Control points -> cropped flux of this rank's samples of ``kind`` (:476-591 and :197-262): evaluate each active
        heliostat once, repeat over its samples, align per sample, trace without blocking, crop around the centre of mass."""
        group, split, tower = state.group, state.split, self.scenario.solar_tower
        train = kind == "train"
        mask = split.active_heliostats_mask_train if train else split.active_heliostats_mask_test
        incident = split.incident_ray_directions_train if train else split.incident_ray_directions_test
        targets = split.target_area_indices_train if train else split.target_area_indices_test
        samples = split.number_of_train_samples if train else split.number_of_test_samples
        if state.activated != kind:
            with torch.no_grad():           # (the per-sample copies of the nets it makes are not what the gradient goes through)
                group.activate_heliostats(active_heliostats_mask=mask, device=device)
            state.activated = kind

        nets = group.nurbs_control_points.index_select(0, state.active_rows)
        # a rigid tensor that learns: its active rows selected inside the step, so that the gradient lands on the group's own
        # tensor (exact zeros on the rows without samples) and the evaluation takes the staged route (ops.nurbs_eval); under
        # no_grad, and for constants, the one fused launch
        canting = group.canting.index_select(0, state.active_rows) if "canting" in state.learnables else state.canting
        translations = group.facet_translations.index_select(0, state.active_rows) if "facet_translations" in state.learnables \
            else state.facet_translations
        points, normals = NURBSSurfaces(group.nurbs_degrees, nets, device=device).calculate_surface_points_and_normals(
            state.evaluation_points, canting, translations)
        if state.slope_sample is not None:
            # slope errors: tilted here, once per distinct heliostat and before the samples' expansion - the gradient lands on
            # the group's own sigma, summed over the samples in the same fixed order - and not again in the alignment
            normals = group.tilted_normals(normals, group.slope_errors.index_select(0, state.active_rows).reshape(-1, 1),
                                           state.slope_sample)
        active, per_heliostat = points.shape[0], points.shape[1] * points.shape[2]
        repeat = lambda t: t.reshape(active, 1, per_heliostat, 4).expand(-1, samples, -1, -1).reshape(  # noqa: E731
            active * samples, per_heliostat, 4)              # backward: .sum(1) over the samples, a fixed order
        group.active_surface_points, group.active_surface_normals = repeat(points), repeat(normals)
        if kind not in state.aim_points:      # (the samples' targets do not change: a few small launches less per epoch)
            state.aim_points[kind] = tower.get_centers_of_target_areas(target_area_indices=targets, device=device)
        aim_points = state.aim_points[kind]
        with torch.no_grad():               # nothing of the kinematics learns here
            if getattr(group, "kinematics", None) is not None:
                orientations = group.kinematics.incident_ray_directions_to_orientations(
                    incident_ray_directions=incident, aim_points=aim_points, device=device)
            elif state.static and kind in state.orientations:
                orientations = state.orientations[kind]
            else:
                from .scene import ideal_orientations
                orientations = ideal_orientations(group.active_positions, aim_points, incident)
                if state.static:            # (one of its constants comes from a host list: a copy that cannot be captured)
                    state.orientations[kind] = orientations
        if state.slope_sample is not None:
            group._align(orientations, tilt=False)
        else:
            group._align(orientations)

        tracer = state.tracers.get(kind)
        if tracer is None:
            ddp = self.ddp_setup
            tracer = state.tracers[kind] = HeliostatRayTracer(
                scenario=self.scenario, heliostat_group=group, blocking_active=False, world_size=ddp["heliostat_group_world_size"],
                rank=ddp["heliostat_group_rank"], batch_size=self.optimizer_dict["batch_size"],
                random_seed=ddp["heliostat_group_rank"], bitmap_resolution=self.bitmap_resolution, dni=self.dni)
        flux, _, _, _ = tracer.trace_rays(incident_ray_directions=incident, active_heliostats_mask=mask,
                                          target_area_indices=targets, device=device)
        return crop_flux_distributions_around_center(flux_distributions=flux, solar_tower=tower,
                                                     target_area_indices=self._own(state, kind, targets, device), device=device)

    def predict_flux(self, state: GroupState, device: torch.device | None = None) -> torch.Tensor:
        """The cropped flux of this rank's training samples from the group's current control points,
        ``[samples, res_u, res_e]``, inside the autograd graph (:476-591)."""
        return self._cropped_flux(state, "train", self._device(device))

    def epoch_loss(self, state: GroupState, cropped_flux: torch.Tensor, loss_definition,
                   device: torch.device | None = None) -> EpochLoss:
        """An epoch's loss from its cropped flux (:984-1052): ``loss_definition`` against the measured bitmaps per sample,
        the mean per heliostat, :func:`flux_integral_constraint` - the first call's cropped sums become the reference
        integrals (``state.reference_integrals`` is None before) - and ``alpha S + beta I`` with the dynamic balancing of
        ``artist_amd.surface_regularization_terms``.  The multiplier is left as it is: :meth:`update_multiplier`."""
        device = self._device(device)
        split = state.split
        samples = split.number_of_train_samples
        per_sample = loss_definition(prediction=cropped_flux, ground_truth=self._own(state, "train", split.flux_measured_train, device),
                                     target_area_indices=self._own(state, "train", split.target_area_indices_train, device),
                                     reduction_dimensions=(1, 2), device=device)
        per_heliostat = reduce_loss_per_sample(per_sample, samples, _mean_over_samples)
        sums = cropped_flux.sum(dim=(1, 2))
        if state.reference_integrals is None:
            state.reference_integrals = sums.detach()
        constraint, relative, violation = flux_integral_constraint(
            sums, state.reference_integrals, state.multiplier, self.constraint_dict["rho_flux_integral"],
            self.constraint_dict["energy_tolerance"], samples, self.epsilon)
        _, heliostat_rows = self._rank_rows(state, "train", device)
        rows = state.active_rows if heliostat_rows is None else state.active_rows.index_select(0, heliostat_rows)
        original = state.original_control_points if heliostat_rows is None else \
            state.original_control_points.index_select(0, heliostat_rows)
        alpha, smoothness, beta, ideal = surface_regularization_terms(
            state.group.nurbs_control_points.index_select(0, rows), original, per_heliostat,
            self.constraint_dict["weight_smoothness"], self.constraint_dict["weight_ideal_surface"], epsilon=self.epsilon)
        total_per_heliostat = per_heliostat + constraint + alpha * smoothness + beta * ideal
        return EpochLoss(total=total_per_heliostat.mean(), total_per_heliostat=total_per_heliostat, flux_loss_per_sample=per_sample,
                         flux_loss_per_heliostat=per_heliostat, constraint=constraint, relative_differences=relative,
                         violation=violation, alpha=alpha, smoothness=smoothness, beta=beta, ideal=ideal)

    def update_multiplier(self, state: GroupState, violation: torch.Tensor) -> None:
        """``lambda <- clamp(lambda + rho * violation, min=0)`` per heliostat, after the backward pass (:1056-1062).  While a
        captured step reads the multiplier (``state.static``) the same values are written into the same tensor."""
        with torch.no_grad():
            multiplier = torch.clamp(state.multiplier + self.constraint_dict["rho_flux_integral"] * violation.detach(), min=0.0)
            if state.static:
                state.multiplier.copy_(multiplier)
            else:
                state.multiplier = multiplier

    def validate(self, state: GroupState, device: torch.device | None = None) -> dict[str, torch.Tensor]:
        """The group's test samples under the current control points (:157-303), without gradient: ``{"pixel_loss", "kl_div"}``,
        each the mean over a heliostat's test samples, ``[this rank's heliostats]`` on the device.  Leaves the group activated
        for the test samples; the next ``predict_flux`` activates it for training again."""
        device = self._device(device)
        split = state.split
        with torch.no_grad():
            cropped = self._cropped_flux(state, "test", device)
            measured = self._own(state, "test", split.flux_measured_test, device)
            losses = {}
            for key, loss in (("pixel_loss", self.validation_loss_pixel), ("kl_div", self.validation_loss_kl_div)):
                losses[key] = reduce_loss_per_sample(loss(prediction=cropped, ground_truth=measured, reduction_dimensions=(1, 2)),
                                                     split.number_of_test_samples, _mean_over_samples)
        if log.isEnabledFor(logging.INFO):          # (two more reads of the device, only for a reader of the log)
            log.info("pixel mean: %.5f, kl-div mean: %.5f", float(losses["pixel_loss"].mean()), float(losses["kl_div"].mean()))
        return losses

    # ------------------------------------------------------------------------------------------
    def build_epoch_graph(self, state: GroupState, loss_definition, device: torch.device | None = None):
        """The group's training step - :meth:`predict_flux`, :meth:`epoch_loss`, ``backward()`` - as an
        ``artist_amd.EpochGraph`` (``state.graph``), built after :meth:`prepare` and before the control points' first use.
        ``replay()`` leaves the gradient on every learnable tensor (``state.learnables``) and returns ``(the six history
        scalars [6], total loss per heliostat, flux loss per sample, violation)``, detached, the bits of the eager step.

        The warm-up runs make what an eager first epoch makes - the activation for the training samples, the training
        tracer, ``state.reference_integrals`` - and nothing else: no step of the optimiser, the multiplier, the scheduler or
        the early stopper.  From here on (``state.static``) :meth:`update_multiplier` writes in place, and the state keeps
        every tensor that the captured step reads and that was made outside the capture (``state.kept``: the activation's
        tables, which ``activate_heliostats`` rebinds and never writes, the reference integrals, the aim points, the rank's
        rows), so that a validation is not handed their memory.  The step is not activated for training again after a
        validation.  :meth:`close_epoch_graph` ends it."""
        device = self._device(device)
        state.static = True
        return self._capture(state, loss_definition, device)

    def _step(self, state: GroupState, loss_definition, device) -> tuple:
        """``(the six history scalars [6], total loss per heliostat, flux loss per sample, violation)``, detached."""
        loss = self.epoch_loss(state, self.predict_flux(state, device), loss_definition, device)
        loss.total.backward()
        return loss.scalars(), loss.total_per_heliostat.detach(), loss.flux_loss_per_sample.detach(), loss.violation.detach()

    def close_epoch_graph(self, state: GroupState) -> None:
        """Close ``state.graph`` and let go of what was kept for it.  No autograd graph that was built on the graph's stream
        outlives it: the surfaces the capture left on the group are detached."""
        state.static = False
        self._release(state)

    def _synchronize_and_lock_gradients(self, parameter: torch.Tensor, device: torch.device | None = None) -> None:
        """In nested mode the ranks that share a group average the gradient: SUM over ``process_subgroup``, divided by the
        sub-world size.  Then the outer edges are locked (:749-788)."""
        if parameter.grad is None:
            return
        self._nested_mean(parameter.grad)
        parameter.grad = self.lock_control_points_on_outer_edges(gradients=parameter.grad, device=device)

    def _synchronize_and_zero_w_gradients(self, parameter: torch.Tensor, device: torch.device | None = None) -> None:
        """What :meth:`_synchronize_and_lock_gradients` is to the control points, for ``canting`` ``[N, F, 2, 4]`` and
        ``facet_translations`` ``[N, F, 4]``: the nested average, then the gradient of every w component is set to zero, in
        place.  The w components are homogeneous zeros, not parameters; ``art_align_bwd`` returns a w component for points
        (``g @ orientation`` picks up the translation column), which reaches a translation's w and would let Adam move the
        points' w away from 1."""
        if parameter.grad is None:
            return
        self._nested_mean(parameter.grad)
        with torch.no_grad():
            parameter.grad[..., 3] = 0

    def _synchronize_gradients(self, parameter: torch.Tensor) -> None:
        """The nested average alone, for ``slope_errors`` ``[N]``: every component is a parameter."""
        self._nested_mean(parameter.grad)

    def _synchronize_and_lock_learnables(self, state: GroupState, device: torch.device | None = None) -> None:
        """Before the step: one reduce per learnable tensor in the canonical order (the same on every rank), the edge lock on
        the control points, the w rule on the rigid tensors."""
        for name, tensor in state.learnables.items():
            if name == "nurbs_control_points":
                self._synchronize_and_lock_gradients(tensor, device)
            elif name == "slope_errors":
                self._synchronize_gradients(tensor)
            else:
                self._synchronize_and_zero_w_gradients(tensor, device)

    def _synchronize_reconstruction_across_ranks(self, final_loss_per_heliostat: torch.Tensor, loss_history: list) -> list:
        """Every group's learnable tensors (the control points by default) from the first rank that owns the group, the
        final losses MIN-reduced (a heliostat another rank reconstructed is ``inf`` here), the histories of all ranks
        gathered (:790-840).  Returns the histories per rank; ``[loss_history]`` in a single process."""
        return self._gather(final_loss_per_heliostat, loss_history, lambda group: [getattr(group, name) for name in self.parameters])

    # ------------------------------------------------------------------------------------------ the loop's four places
    def _before_optimizer_step(self, state: GroupState, outcome: tuple, device) -> None:
        self.update_multiplier(state, outcome[3])   # (the violation)
        self._synchronize_and_lock_learnables(state, device)

    def _host_values(self, scalars: torch.Tensor) -> list:
        return scalars.tolist()                     # the epoch's six scalars in ONE transfer

    def _finish_group(self, state: GroupState) -> None:
        for tensor in state.marked:                 # the rigid tensors are constants again for whoever evaluates next
            tensor.requires_grad_(False)
        if "slope_errors" in state.learnables:      # zeta is symmetric: a learnt sigma is reported as its magnitude
            with torch.no_grad():
                state.learnables["slope_errors"].abs_()

    def reconstruct_surfaces(self, loss_definition, device: torch.device | None = None):
        """Reconstruct the surfaces of the groups this rank owns (:842-1160).  Returns ``(final loss per heliostat of the
        scenario on the CPU, +inf where a heliostat was not reconstructed; the histories: one list per rank, one entry per
        group)``; an entry has the per-epoch float lists ``HISTORY_KEYS`` and ``"test_loss"``, the last validation's
        ``{"pixel_loss", "kl_div"}`` per heliostat.  A group runs while its loss is above ``tolerance`` and
        ``epoch <= max_epoch``, or until early stopping, which ends the group before that epoch's history entry
        (``Reconstructor._reconstruct``).  Afterwards the ranks are synchronised and the field's surface points follow the new
        control points, canting and translations (``update_surfaces``)."""
        device = self._device(device)
        if self.ddp_setup["rank"] == 0:
            log.info("Beginning surface reconstruction.")
        final_loss_per_heliostat, loss_history = self._reconstruct(loss_definition, device)
        histories = self._synchronize_reconstruction_across_ranks(final_loss_per_heliostat, loss_history)
        self.scenario.heliostat_field.update_surfaces(device=device)
        return final_loss_per_heliostat.detach().cpu(), histories

    @staticmethod
    def lock_control_points_on_outer_edges(gradients: torch.Tensor, device: torch.device | None = None) -> torch.Tensor:
        """A copy of ``gradients`` ``[heliostats, facets, U, V, 3]`` with the u and v components of every net's first and last
        row and column set to zero (:1163-1224): the clamped knots make a surface end in its outer control points, so a
        facet keeps its rectangular outline when those stay where they are; z stays free."""
        with torch.no_grad():
            locked = gradients.clone()
            for edge in (locked[:, :, 0], locked[:, :, -1], locked[:, :, :, 0], locked[:, :, :, -1]):
                edge[..., :2] = 0
            return locked
