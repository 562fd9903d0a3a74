"""Kinematics reconstruction: learn every heliostat's four rotation deviations from its calibration samples.
Drop-in for ``artist.optim.KinematicsReconstructor`` (artist/optim/kinematics_reconstructor.py:29-1063): same constructor, same
configuration, same two reconstruction methods, same ``reconstruct_kinematics()`` and return values, same loop.

An epoch is assembled from what the package already has, all of it hand-written HIP on the hot path.  In the
flux-driven mode (``"raytracing"``, :535-622): the rigid-body kinematics from the samples' motor positions
(``art_rigid_body_fwd/_bwd``, mode 0), alignment (``art_align_fwd/_bwd``), the trace without blocking (``art_trace_fwd/_bwd``),
the caller's loss on the bitmaps (``FocalSpotLoss``: ``art_flux_center_of_mass(_bwd)``), the median over a heliostat's samples,
the mean over the heliostats and the step (``art_adam_step``).  In the alignment-driven mode (``"alignment"``, :421-533) nothing
is traced: the predicted normal of a sample is the third column of its orientation, the measured one follows once from its focal
spot, the heliostat's position and the incident ray direction, and the caller's loss (``artist_amd.losses``) compares the two -
the mean over the samples, then over the heliostats.

The samples of one heliostat share one row of deviations.  ``HeliostatGroup.activate_heliostats`` repeats the rows with
``repeat_interleave``, whose backward is a scatter-add over a heliostat's samples.  Here the rows of the heliostats that have
samples are taken once (``index_select``, unique rows) and expanded over the sample axis with a view, so the backward is
``[heliostats, samples, 4].sum(1)`` - a fixed order: two runs give the same bits.

Host reads: the loop reads the device ONCE per epoch - the loss, after the step has been queued (the stop test, early stopping
and ``ReduceLROnPlateau`` need it on the host).  The group is activated for the training samples once and again after every
validation; one ray tracer per group serves all training epochs, another - made the reference's way, seed 7 and a world of
one - all validations.

``epoch_graph=True`` ("The epoch as a graph"): per group the training step - ``epoch_loss`` and ``backward()`` -
is captured once into an ``artist_amd.EpochGraph`` and replayed every epoch, in both modes; ``nan_to_num_`` on the gradient, the
nested all-reduce, ``Adam.step()``, the one host read, the scheduler, early stopping, the history and every validation stay eager,
in the same order.  The replayed epoch gives the eager epoch's bits.

``parameters=(...)`` ("More kinematic parameters"; beyond the reference's class): the translation deviations
``[H, 9]`` and the optimisable actuator parameters ``[H, 2, 2]`` learn beside or instead of the rotation deviations.
``art_rigid_body_bwd`` writes all three gradients in its one launch anyway; a tensor that learns is bound to the kinematics'
per-sample table the way the rotation deviations are - unique rows, expanded with a view, the same fixed-order sum backwards -
and one ``artist_amd.optim.Adam`` steps one parameter group per tensor.  An epoch calls the library as before, but for one
``art_adam_step`` per further tensor.

More than one rank has not run on a GPU: the collectives (``_synchronize_gradients_nested_ddp``,
``_synchronize_reconstruction_across_ranks``) are tested with two gloo processes on CPU tensors.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from functools import partial
from typing import Any

import torch

from .flux import FocalSpotLoss, KLDivergenceLoss, PixelLoss
from .raytracing import HeliostatRayTracer
from .reconstruction import ReconstructionGroupState, Reconstructor
from .training import reduce_loss_per_sample

log = logging.getLogger(__name__)

__all__ = ["KinematicsReconstructor", "KinematicsGroupState", "KinematicsEpochLoss", "KINEMATICS_RECONSTRUCTION_RAYTRACING",
           "KINEMATICS_RECONSTRUCTION_ALIGNMENT", "KINEMATICS_PARAMETER_NAMES", "KINEMATICS_LEARNING_RATE_KEYS"]

#: the two reconstruction methods (artist/util/constants.py)
KINEMATICS_RECONSTRUCTION_RAYTRACING = "raytracing"
KINEMATICS_RECONSTRUCTION_ALIGNMENT = "alignment"

#: what a reconstruction can learn, in the canonical order: the order of the optimiser's parameter groups and of the reduces
#: in nested mode.  ``kinematics.rotation_deviation_parameters`` ``[H, 4]``, ``kinematics.translation_deviation_parameters``
#: ``[H, 9]`` and ``kinematics.actuators.optimizable_parameters`` ``[H, 2, 2]``.
KINEMATICS_PARAMETER_NAMES = ("rotation_deviations", "translation_deviations", "actuator_parameters")

#: the configuration key of every name's initial learning rate; the first is required and the default of the others
KINEMATICS_LEARNING_RATE_KEYS = {"rotation_deviations": "initial_learning_rate_rotation_deviation",
                                 "translation_deviations": "initial_learning_rate_translation_deviation",
                                 "actuator_parameters": "initial_learning_rate_actuator_parameters"}

_mean_over_samples = partial(torch.mean, dim=-1)
_median_over_samples = partial(torch.median, dim=1)


@dataclass
class KinematicsEpochLoss:
    """One epoch's loss: ``total`` (the mean of ``per_heliostat``), the loss per sample and per heliostat of this rank, and
    what the loss was taken of - the predicted flux ``[samples, res_u, res_e]`` or the predicted normals ``[samples, 4]``."""
    total: torch.Tensor
    per_heliostat: torch.Tensor
    per_sample: torch.Tensor
    prediction: torch.Tensor


@dataclass
class KinematicsGroupState(ReconstructionGroupState):
    """What the epochs of one heliostat group share (``KinematicsReconstructor.prepare``), beside the fields every
    reconstruction has; ``learnables`` are the kinematics' own tensors."""
    normals_measured: torch.Tensor | None = None    # alignment mode: of all samples, [samples, 4]
    normals_measured_train: torch.Tensor | None = None
    surfaces: tuple | None = None               # the activated samples' surface points and normals before alignment


def _slot(kinematics, name: str) -> tuple:
    """Where the tensor ``name`` lives: ``(holder, its attribute, the attribute of its per-sample table)``."""
    if name == "actuator_parameters":
        return kinematics.actuators, "optimizable_parameters", "active_optimizable_parameters"
    stem = {"rotation_deviations": "rotation_deviation_parameters", "translation_deviations": "translation_deviation_parameters"}[name]
    return kinematics, stem, "active_" + stem


class KinematicsReconstructor(Reconstructor):
    """``artist.optim.KinematicsReconstructor``: see the module docstring; attributes as in the reference (:38-60).

    ``prepare`` / ``epoch_loss`` / ``validate`` are the pieces ``reconstruct_kinematics`` runs per group, for callers that step
    themselves.

    ``epoch_graph`` (a public attribute, read when a group's loop starts): replay each group's training step from an
    ``artist_amd.EpochGraph`` (:meth:`build_epoch_graph`) instead of running it eagerly, in both modes; the same bits, less host
    time per epoch.  ``loss_definition`` must then not read the device (``.item()``, ``nonzero``, a host comparison): torch's
    capture error propagates as it is, and there is no fall-back to the eager loop.  After a replay
    ``heliostat_group.active_surface_points`` / ``active_surface_normals`` and the kinematics' ``active_*`` tables are whatever
    the last eager call - the capture or a validation - left: a replay does not look at them.

    ``parameters`` (an addition, a keyword of the class call after ``epoch_graph``, taken the way ``SurfaceReconstructor``
    takes its own - ``__init__`` keeps the reference's signature; the reference's class learns the rotation deviations only).
    What learns: a non-empty tuple or list of ``KINEMATICS_PARAMETER_NAMES`` - ``"rotation_deviations"``
    (``kinematics.rotation_deviation_parameters``), ``"translation_deviations"`` (``kinematics.translation_deviation_parameters``)
    and ``"actuator_parameters"`` (``kinematics.actuators.optimizable_parameters``: the linear actuators' initial angles and
    stroke lengths) - in any order; anything else is a ``ValueError``.  Kept as ``self.parameters``, a tuple in this order, and
    read in :meth:`prepare`, which refuses (``ValueError``) the translations in the alignment-driven mode - they do not enter
    the predicted normal, their gradient is identically zero - and the actuator parameters of a group with ideal actuators.
    One ``artist_amd.optim.Adam`` steps them, one parameter group each, at
    ``optimization["initial_learning_rate_rotation_deviation"]``, ``["initial_learning_rate_translation_deviation"]`` and
    ``["initial_learning_rate_actuator_parameters"]`` (the latter two optional, defaulting to the first); the schedulers
    scale every group.  Loss, validation, histories and the stop logic are the same for every choice.  Every learned tensor
    is detached at the end of :meth:`reconstruct_kinematics`; a tensor that is not chosen is never marked and never written."""

    def __init__(self, ddp_setup: dict, scenario, data: dict, optimization_configuration: dict[str, Any],
                 dni: float | None = None, reconstruction_method: str = KINEMATICS_RECONSTRUCTION_RAYTRACING,
                 bitmap_resolution: torch.Tensor = torch.tensor([256, 256]), device: torch.device | None = None,
                 epoch_graph: bool = False) -> None:
        self._device(device)
        if ddp_setup["rank"] == 0:
            log.info("Create a kinematics reconstructor.")
        self.ddp_setup = ddp_setup
        self.scenario = scenario
        self.data = data
        self.optimizer_dict = optimization_configuration["optimization"]
        self.scheduler_dict = optimization_configuration["scheduler"]
        self.dni = dni
        self.bitmap_resolution = torch.tensor([int(bitmap_resolution[0]), int(bitmap_resolution[1])])   # (a host copy)
        self.validation_loss_focal_spot = FocalSpotLoss(scenario=scenario)
        self.validation_loss_pixel = PixelLoss()
        self.validation_loss_kl_div = KLDivergenceLoss()
        if reconstruction_method not in (KINEMATICS_RECONSTRUCTION_RAYTRACING, KINEMATICS_RECONSTRUCTION_ALIGNMENT):
            raise ValueError(f"The kinematics reconstruction method '{reconstruction_method}' is unknown. "
                             f"Please select another reconstruction method and try again!")
        self.reconstruction_method = reconstruction_method
        self.epoch_graph = bool(epoch_graph)

    PARAMETER_NAMES = KINEMATICS_PARAMETER_NAMES        # (the rotation deviations alone, unless chosen otherwise)
    HISTORY_KEYS = ("total_loss",)
    RECONSTRUCTS = "kinematics"

    @property
    def _flux_driven(self) -> bool:
        return self.reconstruction_method == KINEMATICS_RECONSTRUCTION_RAYTRACING

    # ------------------------------------------------------------------------------------------
    def prepare(self, heliostat_group_index: int, device: torch.device | None = None) -> KinematicsGroupState | None:
        """Everything before a group's first epoch (:332-419, 758-794, 937-964): its calibration samples from
        ``data["data_parser"].parse_data_for_reconstruction``, the train/test split, in alignment mode the measured normals,
        ``artist_amd.optim.Adam`` with one parameter group per tensor of ``self.parameters`` (``requires_grad_()`` on those, and on
        no other; ``state.learnables``), the configured scheduler and early stopping.  A ``ValueError`` for a choice that cannot
        be learned (the class docstring).  None for a group without samples."""
        device = self._device(device)
        if "translation_deviations" in self.parameters and not self._flux_driven:
            raise ValueError("'translation_deviations' cannot be learned with reconstruction_method='alignment': the predicted "
                             "normal is the third column of the orientation, translations do not enter it, and their gradient "
                             "is identically zero; use the flux-driven method ('raytracing') or leave them out")
        group = self.scenario.heliostat_field.heliostat_groups[heliostat_group_index]
        if "actuator_parameters" in self.parameters and group.kinematics.actuators.optimizable_parameters.numel() == 0:
            raise ValueError(f"'actuator_parameters' cannot be learned on heliostat group {heliostat_group_index}: its actuators "
                             f"are ideal, actuators.optimizable_parameters is empty")
        parsed = self._parse_and_split(heliostat_group_index, device)
        if parsed is None:
            return None
        (_, focal_spots, incident, _, mask, _), split, active_rows = parsed
        learnables = {}
        for name in self.parameters:
            holder, attribute, _ = _slot(group.kinematics, name)
            learnables[name] = getattr(holder, attribute)
        optimizer, scheduler, stopper = self._optimizer_for(learnables, KINEMATICS_LEARNING_RATE_KEYS)
        state = KinematicsGroupState(index=heliostat_group_index, group=group, mask=mask, split=split, active_rows=active_rows,
                                     optimizer=optimizer, scheduler=scheduler, early_stopper=stopper, learnables=learnables)
        if not self._flux_driven:
            state.normals_measured = self._compute_measured_normals(group, focal_spots, incident, mask, device)
            state.normals_measured_train = state.normals_measured[split.train_indices.to(device)]
        return state

    @staticmethod
    def _compute_measured_normals(heliostat_group, focal_spots_measured: torch.Tensor, incident_ray_directions: torch.Tensor,
                                  active_heliostats_mask: torch.Tensor, device: torch.device | None = None) -> torch.Tensor:
        """The normals the samples were measured under, ``[samples, 4]`` (:421-470): a mirror that sends the incident ray to
        the measured focal spot has the normalised difference of the direction to the spot and the incident direction as its
        normal.  On the device of the arguments."""
        positions = heliostat_group.positions.repeat_interleave(active_heliostats_mask, dim=0)
        to_focal_spot = torch.nn.functional.normalize(focal_spots_measured[:, :3] - positions[:, :3], p=2, dim=1)
        normals = torch.nn.functional.normalize(to_focal_spot - incident_ray_directions[:, :3], dim=-1)
        return torch.cat((normals, torch.zeros_like(normals[:, :1])), dim=1)

    def _rank_rows(self, state: KinematicsGroupState, kind: str, device):
        """As the base's; in alignment mode every rank owns all rows."""
        return super()._rank_rows(state, kind, device) if self._flux_driven else (None, None)

    def _orientations(self, state: KinematicsGroupState, kind: str, device) -> torch.Tensor:
        """The learned tensors -> the orientations of the samples of ``kind``, ``[samples, 4, 4]`` (:506-514, 568-577).  The
        group is activated for ``kind`` when it is not; of every learned tensor the rows of the heliostats that have samples
        are taken once and expanded over the sample axis with a view."""
        group, split = state.group, state.split
        train = kind == "train"
        mask = split.active_heliostats_mask_train if train else split.active_heliostats_mask_test
        samples = split.number_of_train_samples if train else split.number_of_test_samples
        if state.activated != kind:
            with torch.no_grad():           # (the per-sample copies of the deviations it makes are not what the gradient goes through)
                group.activate_heliostats(active_heliostats_mask=mask, device=device)
            state.surfaces = (group.active_surface_points, group.active_surface_normals)
            state.activated = kind
        kinematics = group.kinematics
        for name, tensor in state.learnables.items():            # (a tensor that does not learn keeps the activation's copy)
            holder, _, active_attribute = _slot(kinematics, name)
            rows = tensor.index_select(0, state.active_rows)
            active, shape = rows.shape[0], rows.shape[1:]
            setattr(holder, active_attribute, rows.reshape(active, 1, *shape).expand(active, samples, *shape).reshape(
                active * samples, *shape))                       # backward: .sum(1) over the samples, a fixed order
        return kinematics.motor_positions_to_orientations(
            motor_positions=split.motor_positions_train if train else split.motor_positions_test, device=device)

    def _flux(self, state: KinematicsGroupState, kind: str, device) -> torch.Tensor:
        """Rotation deviations -> the flux of the samples of ``kind`` (:568-597 and :214-239): orientations from the motor
        positions, alignment, the trace without blocking.  Training: this rank's samples, the tracer seeded with the rank in
        the group's sub-world; validation: all test samples on every rank, seed 7."""
        group, split = state.group, state.split
        train = kind == "train"
        orientations = self._orientations(state, kind, device)
        group.active_surface_points, group.active_surface_normals = state.surfaces      # (the last epoch left them aligned)
        group._align(orientations)
        tracer = state.tracers.get(kind)
        if tracer is None:
            ddp = self.ddp_setup
            where = dict(world_size=ddp["heliostat_group_world_size"], rank=ddp["heliostat_group_rank"],
                         random_seed=ddp["heliostat_group_rank"]) if train else {}
            tracer = state.tracers[kind] = HeliostatRayTracer(
                scenario=self.scenario, heliostat_group=group, blocking_active=False, batch_size=self.optimizer_dict["batch_size"],
                bitmap_resolution=self.bitmap_resolution, dni=self.dni, **where)
        flux, _, _, _ = tracer.trace_rays(
            incident_ray_directions=split.incident_ray_directions_train if train else split.incident_ray_directions_test,
            active_heliostats_mask=split.active_heliostats_mask_train if train else split.active_heliostats_mask_test,
            target_area_indices=split.target_area_indices_train if train else split.target_area_indices_test, device=device)
        return flux

    def epoch_loss(self, state: KinematicsGroupState, loss_definition, device: torch.device | None = None) -> KinematicsEpochLoss:
        """An epoch's loss from the group's current rotation deviations, inside the autograd graph.  Flux-driven (:535-622):
        ``loss_definition`` on the predicted and the measured flux of this rank's training samples, the median over a
        heliostat's samples.  Alignment-driven (:472-533): ``loss_definition(prediction, ground_truth)`` on the predicted and
        the measured normals, the mean over a heliostat's samples.  The total is the mean over the heliostats."""
        device = self._device(device)
        split = state.split
        if self._flux_driven:
            prediction = self._flux(state, "train", device)
            per_sample = loss_definition(prediction=prediction, ground_truth=self._own(state, "train", split.flux_measured_train, device),
                                         target_area_indices=self._own(state, "train", split.target_area_indices_train, device),
                                         reduction_dimensions=(1, 2), device=device)
            reduction = _median_over_samples
        else:
            # orientations @ (0, 0, 1, 0): the third column, as it stands
            prediction = self._orientations(state, "train", device)[:, :, 2]
            per_sample = loss_definition(prediction=prediction, ground_truth=state.normals_measured_train)
            reduction = _mean_over_samples
        per_heliostat = reduce_loss_per_sample(per_sample, split.number_of_train_samples, reduction)
        return KinematicsEpochLoss(total=per_heliostat.mean(), per_heliostat=per_heliostat, per_sample=per_sample, prediction=prediction)

    def validate(self, state: KinematicsGroupState, device: torch.device | None = None) -> dict[str, torch.Tensor]:
        """The group's test samples under the current rotation deviations (:184-295), traced in both modes, without gradient:
        ``{"pixel_loss", "kl_div", "focal_spot_loss"}``, each reduced over a heliostat's test samples - by the median in the
        flux-driven mode, by the mean in the alignment-driven one - ``[active heliostats]`` on the device.  Leaves the group
        activated for the test samples; the next ``epoch_loss`` activates it for training again."""
        device = self._device(device)
        split = state.split
        reduction = _median_over_samples if self._flux_driven else _mean_over_samples
        with torch.no_grad():
            flux = self._flux(state, "test", device)
            measured = split.flux_measured_test
            per_sample = {
                "pixel_loss": self.validation_loss_pixel(prediction=flux, ground_truth=measured, reduction_dimensions=(1, 2)),
                "kl_div": self.validation_loss_kl_div(prediction=flux, ground_truth=measured, reduction_dimensions=(1, 2)),
                "focal_spot_loss": self.validation_loss_focal_spot(prediction=flux, ground_truth=measured,
                                                                   target_area_indices=split.target_area_indices_test, device=device)}
            losses = {key: reduce_loss_per_sample(value, split.number_of_test_samples, reduction) for key, value in per_sample.items()}
        if log.isEnabledFor(logging.INFO):          # (three more reads of the device, only for a reader of the log)
            log.info("test loss focal spot: %.5f, pixel: %.5f, kl-div: %.5f", float(losses["focal_spot_loss"].mean()),
                     float(losses["pixel_loss"].mean()), float(losses["kl_div"].mean()))
        return losses

    # ------------------------------------------------------------------------------------------
    def build_epoch_graph(self, state: KinematicsGroupState, loss_definition, device: torch.device | None = None):
        """The group's training step - :meth:`epoch_loss` and ``backward()`` - as an ``artist_amd.EpochGraph`` (``state.graph``),
        built after :meth:`prepare` and before the deviations' first use.  ``replay()`` leaves the gradient on
        every learned tensor (``state.learnables``) and returns ``(total loss, loss per heliostat, loss per sample)``, detached, the bits
        of the eager step.

        The warm-up runs make what an eager first epoch makes - the activation for the training samples and, flux-driven, the
        training tracer - and nothing else: no step of the optimiser, the scheduler or the early stopper.  The state keeps
        every tensor that the captured step reads and that was made outside the capture (``state.kept``: the activation's
        tables and the unaligned ``state.surfaces``, which ``activate_heliostats`` and a validation rebind and never write,
        the measured normals, the rank's rows), so that a validation is not handed their memory.  The step is not activated
        for training again after a validation.  :meth:`close_epoch_graph` ends it."""
        device = self._device(device)
        return self._capture(state, loss_definition, device)

    def _step(self, state: KinematicsGroupState, loss_definition, device) -> tuple:
        """``(total loss, loss per heliostat, loss per sample)``, detached."""
        loss = self.epoch_loss(state, loss_definition, device)
        loss.total.backward()
        return loss.total.detach(), loss.per_heliostat.detach(), loss.per_sample.detach()

    def close_epoch_graph(self, state: KinematicsGroupState) -> None:
        """Close ``state.graph`` and let go of what was kept for it.  No autograd graph that was built on the graph's stream
        outlives it: what the capture left on the group and its kinematics is detached."""
        self._release(state)
        for name in state.learnables:
            holder, _, active_attribute = _slot(state.group.kinematics, name)
            setattr(holder, active_attribute, getattr(holder, active_attribute).detach())

    def _synchronize_gradients_nested_ddp(self, optimizer: torch.optim.Optimizer) -> None:
        """In nested mode the ranks that share a group average the gradient: SUM over ``process_subgroup``, divided by the
        sub-world size (:624-648).  Flux-driven mode only."""
        for param_group in optimizer.param_groups:
            for parameter in param_group["params"]:
                self._nested_mean(parameter.grad)

    def _synchronize_reconstruction_across_ranks(self, final_loss_per_heliostat: torch.Tensor, loss_history: list) -> list:
        """Every group's rotation deviations and optimisable actuator parameters - and its translation deviations when they
        are learned - from the first rank that owns the group, the final losses MIN-reduced (a heliostat another rank
        reconstructed is ``inf`` here), the histories of all ranks gathered (:650-705).  Returns the histories per rank;
        ``[loss_history]`` in a single process."""
        def tensors(group):
            kinematics = group.kinematics
            learned = [kinematics.translation_deviation_parameters] if "translation_deviations" in self.parameters else []
            return [kinematics.rotation_deviation_parameters, *learned, kinematics.actuators.optimizable_parameters]
        return self._gather(final_loss_per_heliostat, loss_history, tensors)

    # ------------------------------------------------------------------------------------------ the loop's four places
    def _before_optimizer_step(self, state: KinematicsGroupState, outcome: tuple, device) -> None:
        if self._flux_driven:
            self._synchronize_gradients_nested_ddp(state.optimizer)
        else:
            # a sample whose normals are parallel has a non-finite gradient: it does not take part in the epoch
            for parameter in state.learnables.values():
                parameter.grad.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)

    def _host_values(self, total: torch.Tensor) -> list:
        return [total.item()]                       # the epoch's one read

    def reconstruct_kinematics(self, loss_definition, device: torch.device | None = None):
        """Reconstruct the rotation deviations (or what ``self.parameters`` names) of the groups this rank owns (:707-884
        alignment-driven, :886-1063 flux-driven).  Returns ``(final loss per heliostat of the scenario on the CPU, +inf where a
        heliostat was not reconstructed; the histories: one list per rank, one entry per group)``; an entry is ``{"total_loss":
        a float per epoch, "test_loss": the last validation's {"pixel_loss", "kl_div", "focal_spot_loss"} per heliostat}``.  A
        group runs while its loss is above ``tolerance`` and ``epoch <= max_epoch``, or until early stopping, which ends the
        group before that epoch's history entry (``Reconstructor._reconstruct``).  The flux-driven mode averages the gradients
        over a group's sub-world and synchronises the ranks afterwards; the alignment-driven mode issues no collective, as in
        the reference, and returns this rank's histories alone.  The learned tensors are detached at the end."""
        device = self._device(device)
        if self.ddp_setup["rank"] == 0:
            log.info("Beginning kinematics reconstruction with %s.", "ray tracing" if self._flux_driven else "alignment")
        final_loss_per_heliostat, loss_history = self._reconstruct(loss_definition, device)
        histories = self._synchronize_reconstruction_across_ranks(final_loss_per_heliostat, loss_history) if self._flux_driven \
            else [loss_history]
        for group in self.scenario.heliostat_field.heliostat_groups:
            for name in self.parameters:
                holder, attribute, _ = _slot(group.kinematics, name)
                setattr(holder, attribute, getattr(holder, attribute).detach())
        return final_loss_per_heliostat.detach().cpu(), histories
