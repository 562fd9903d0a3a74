"""Aim-point optimisation: learn every heliostat's motor positions so that the field's flux on one target area takes a wanted
shape.  Drop-in for ``artist.optim.AimPointOptimizer`` (artist/optim/aim_point_optimizer.py:19-972): same constructor, same
nested configuration, same ``optimize()`` and return values, same histories.

An epoch is assembled from what the package already has, all of it hand-written HIP on the hot path:
motor positions -> orientations (``art_rigid_body_fwd/_bwd`` mode 0, the gradient w.r.t. the motor positions), alignment
(``art_align_fwd/_bwd``), the blocking filter and the fused per-target trace with the soft blocking mask
(``art_blocking_filter``, ``art_trace_fwd/_bwd``), the KL divergence against the wanted distribution (``art_flux_loss``) and the
step (``art_adam_step``).  The objective on top - the KL term plus three augmented-Lagrangian terms on ONE bitmap and one
``[number of heliostats]`` vector - is :func:`aim_point_objective`: a dozen element-wise and reduction ops in torch, on
whichever device its arguments live.

Host reads: the loop reads the device ONCE per epoch - the epoch's six scalars, stacked (the stop test needs the loss on the
host); the multipliers and references stay device tensors.  Building a new ray tracer every epoch (its blocking rectangles are
the surfaces as aligned in this epoch) keeps the reads ``HeliostatGroup.activate_heliostats`` and ``HeliostatRayTracer`` make.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from functools import partial
from typing import Any

import torch

from . import distributed, optics, training
from .flux import JensenShannonLoss, KLDivergenceLoss
from .raytracing import HeliostatRayTracer
from .reconstruction import gpu_device, scheduler_and_stopper

log = logging.getLogger(__name__)

__all__ = ["AimPointOptimizer", "ConstraintState", "aim_point_objective"]

ACTUATOR_MIN_MOTOR_POSITION, ACTUATOR_MAX_MOTOR_POSITION = 2, 3     # rows of the actuator table (artist/util/indices.py)
HISTORY_KEYS = ("total_loss", "flux_loss", "local_flux_constraint", "intercept_constraint", "flux_integral_constraint",
                "flux_integral")


@dataclass
class ConstraintState:
    """What the augmented-Lagrangian terms carry from epoch to epoch: the penalty weights ``rho_*``, the allowed flux per
    pixel, the multipliers ``lambda_*`` (0-d tensors) and the references of the first epoch (None until then)."""
    rho_flux_integral: float
    rho_intercept: float
    rho_local_flux: float
    max_flux_density_per_pixel: torch.Tensor
    lambda_flux_integral: torch.Tensor
    lambda_intercept: torch.Tensor
    lambda_local_flux: torch.Tensor
    flux_integral_reference: torch.Tensor | None = None
    intercept_factors_reference: torch.Tensor | None = None
    epsilon: float = 1e-12

    @classmethod
    def fresh(cls, constraints: dict, max_flux_density_per_pixel: torch.Tensor, epsilon: float = 1e-12) -> "ConstraintState":
        """Multipliers at zero and no references yet; ``constraints`` is the configuration's ``"constraints"`` dict."""
        zero = lambda: torch.zeros((), dtype=max_flux_density_per_pixel.dtype, device=max_flux_density_per_pixel.device)  # noqa: E731
        return cls(rho_flux_integral=float(constraints["rho_flux_integral"]), rho_intercept=float(constraints["rho_intercept"]),
                   rho_local_flux=float(constraints["rho_local_flux"]), max_flux_density_per_pixel=max_flux_density_per_pixel,
                   lambda_flux_integral=zero(), lambda_intercept=zero(), lambda_local_flux=zero(), epsilon=epsilon)


def _augmented_lagrangian(multiplier, rho: float, violation: torch.Tensor) -> torch.Tensor:
    return multiplier * violation + 0.5 * rho * violation ** 2


def aim_point_objective(flux_loss: torch.Tensor, total_flux: torch.Tensor, intercept_factors: torch.Tensor,
                        state: ConstraintState):
    """The total loss of an aim-point epoch (aim_point_optimizer.py:606-667): ``flux_loss`` plus three augmented-Lagrangian
    terms ``lambda v + rho/2 v^2`` on clamped violations ``v >= 0``.  Returns ``(total loss, flux-integral term, intercept term,
    local-flux term)`` and updates ``state``.

    * flux integral: the field must not lose power - ``v = (reference - sum) / (reference + eps)``;
    * intercept: no heliostat may spill more - the same per heliostat on the intercept factors, then the mean of the terms;
    * local flux: no pixel above ``state.max_flux_density_per_pixel`` - ``v = (flux - max) / (max + eps)`` per pixel, the term is
      the LARGEST pixel's.

    The references are the first call's flux integral and intercept factors (detached; ``state`` holds None before).  After the
    terms, without gradient, every multiplier moves by ``rho`` times its UNCLAMPED violation (the largest pixel's, the mean
    over heliostats, the integral's) and is clamped at zero.  Nothing here leaves the device of the arguments, and nothing is
    specific to one: torch ops only."""
    integral = total_flux.sum()
    if state.flux_integral_reference is None:
        state.flux_integral_reference = integral.detach()
        state.intercept_factors_reference = intercept_factors.detach()
    eps = state.epsilon

    integral_violation = (state.flux_integral_reference - integral) / (state.flux_integral_reference + eps)
    flux_integral_term = _augmented_lagrangian(state.lambda_flux_integral, state.rho_flux_integral,
                                               torch.clamp(integral_violation, min=0.0))

    intercept_violation = (state.intercept_factors_reference - intercept_factors) / (state.intercept_factors_reference + eps)
    intercept_term = _augmented_lagrangian(state.lambda_intercept, state.rho_intercept,
                                           torch.clamp(intercept_violation, min=0.0)).mean()

    allowed = state.max_flux_density_per_pixel.detach()
    local_violation = (total_flux - allowed) / (allowed + eps)
    local_flux_term = torch.max(_augmented_lagrangian(state.lambda_local_flux, state.rho_local_flux,
                                                      torch.clamp(local_violation, min=0.0)))

    total = flux_loss + flux_integral_term + intercept_term + local_flux_term
    with torch.no_grad():
        state.lambda_local_flux = torch.clamp(state.lambda_local_flux + state.rho_local_flux * local_violation.max(), min=0.0)
        state.lambda_intercept = torch.clamp(state.lambda_intercept + state.rho_intercept * intercept_violation.mean(), min=0.0)
        state.lambda_flux_integral = torch.clamp(state.lambda_flux_integral + state.rho_flux_integral * integral_violation,
                                                 min=0.0)
    return total, flux_integral_term, intercept_term, local_flux_term


def _require_kl(loss_definition) -> None:
    # (... or its bounded relative, the Jensen-Shannon divergence: the same kind of loss on the same normalised bitmaps)
    if not isinstance(loss_definition, (KLDivergenceLoss, JensenShannonLoss)):
        raise TypeError("AimPointOptimizer defines its total loss (flux loss + flux-integral, intercept and local-flux "
                        f"constraints) for artist_amd.KLDivergenceLoss only, got {type(loss_definition).__name__}: with any "
                        "other loss definition there is no loss to differentiate")


_gpu_device = partial(gpu_device, who="AimPointOptimizer")


class AimPointOptimizer:
    """``artist.optim.AimPointOptimizer``: see the module docstring; attributes as in the reference (:28-61).

    ``attenuation`` (keyword only, an extension): a model of ``artist_amd.optics`` - ``("exponential", beta_per_km)``,
    ``("polynomial", coefficients)`` or a callable.  ``prepare`` then computes every heliostat's extinction over its slant range to
    the optimised target's centre once, and every epoch traces with it and with the group's ``active_reflectivities`` when the
    group has them (the per-target bitmaps are then summed from scaled per-heliostat bitmaps,
    ``HeliostatRayTracer.trace_rays_per_target``).  Without either, an epoch is what it was.

    ``blocking_active`` (True, as the reference always traces) may be cleared on an instance to see an epoch without
    blocking; ``prepare`` / ``trace_epoch`` / ``epoch_loss`` are the pieces ``optimize`` runs, for callers that step
    themselves."""

    def __init__(self, ddp_setup: dict, scenario, optimization_configuration: dict[str, Any], incident_ray_direction: torch.Tensor,
                 target_area_index: int, ground_truth: torch.Tensor, dni: float,
                 bitmap_resolution: torch.Tensor = torch.tensor([256, 256]), epsilon: float = 1e-12,
                 device: torch.device | None = None, *, attenuation=None) -> None:
        _gpu_device(device)
        if ddp_setup["rank"] == 0:
            log.info("Create an aim points optimizer.")
        #: atmospheric attenuation by slant range (an extension): None, or a model of ``artist_amd.optics``
        self.attenuation = attenuation
        self.ddp_setup = ddp_setup
        self.scenario = scenario
        self.optimizer_dict = optimization_configuration["optimization"]
        self.scheduler_dict = optimization_configuration["scheduler"]
        self.constraint_dict = optimization_configuration["constraints"]
        self.incident_ray_direction = incident_ray_direction
        self.target_area_index = int(target_area_index)
        self.ground_truth = ground_truth
        self.dni = dni
        self.bitmap_resolution = bitmap_resolution
        # (read once: every epoch's new tracer and the pixel count want it on the host)
        self._resolution_host = (int(bitmap_resolution[0]), int(bitmap_resolution[1]))
        self._resolution_cpu = torch.tensor(self._resolution_host)
        self.epsilon = epsilon
        self.blocking_active = True
        self.groups: list[dict] = []
        self.optimizer = self.scheduler = self.early_stopper = self.state = None

    # ------------------------------------------------------------------------------------------
    def _target_plane_dimensions(self) -> torch.Tensor:
        """(width, height) in metres of the optimised target area: a planar area's dimensions, or arc length of the opening
        sector and height of a cylinder (:305-348)."""
        areas, row = self.scenario.solar_tower.index_to_target_area[self.target_area_index]
        if hasattr(areas, "dimensions"):
            return areas.dimensions[row]
        return torch.stack((areas.radii.reshape(-1)[row] * areas.opening_angles.reshape(-1)[row], areas.heights.reshape(-1)[row]))

    def prepare(self, device: torch.device | None = None) -> None:
        """Everything before the first epoch (:167-303, 808-821).  Per heliostat group: all heliostats active, all on the one
        target, all under the one sun; one alignment to the target's centre gives the initial motor positions, the distance
        to the nearer actuator limit (at least 1) the scale, and the learnable parameter starts at zero.  Then one
        ``artist_amd.optim.Adam`` over all groups' parameters, the configured scheduler, early stopping and the constraints'
        state."""
        from .optim import Adam
        device = _gpu_device(device)
        field, tower = self.scenario.heliostat_field, self.scenario.solar_tower
        self.groups = []
        offset = 0
        incident = self.incident_ray_direction.to(device)
        for group in field.heliostat_groups:
            n = int(group.number_of_heliostats)
            mask = torch.ones(n, dtype=torch.int32, device=device)
            targets = torch.full((n,), self.target_area_index, dtype=torch.int32, device=device)
            directions = incident.repeat(n, 1)
            group.activate_heliostats(active_heliostats_mask=mask, device=device)
            group.align_surfaces_with_incident_ray_directions(
                aim_points=tower.get_centers_of_target_areas(target_area_indices=targets, device=device),
                incident_ray_directions=directions, active_heliostats_mask=mask, device=device)
            initial = group.kinematics.active_motor_positions.detach().clone()
            limits = group.kinematics.actuators.non_optimizable_parameters
            scale = torch.minimum(initial - limits[:, ACTUATOR_MIN_MOTOR_POSITION],
                                  limits[:, ACTUATOR_MAX_MOTOR_POSITION] - initial).clamp(min=1.0)
            extinction = None
            if self.attenuation is not None:        # once: positions and the target's centre do not move with the motors
                with torch.no_grad():
                    extinction, _ = optics.heliostat_intensity_factors(group, tower, targets, self.attenuation)
            self.groups.append(dict(group=group, mask=mask, targets=targets, incident=directions, initial=initial, scale=scale,
                                    parameter=torch.nn.Parameter(torch.zeros_like(initial)), offset=offset, extinction=extinction))
            offset += n
        self.number_of_heliostats = offset

        self.optimizer = Adam([g["parameter"] for g in self.groups], lr=float(self.optimizer_dict["initial_learning_rate"]))
        self.scheduler, self.early_stopper = scheduler_and_stopper(self.optimizer, self.optimizer_dict, self.scheduler_dict)
        pixels = self._resolution_host[0] * self._resolution_host[1]
        allowed = torch.prod(self._target_plane_dimensions().to(device)) / pixels * float(self.constraint_dict["max_flux_density"])
        self.state = ConstraintState.fresh(self.constraint_dict, allowed, self.epsilon)
        self._ground_truth = self.ground_truth.to(device).unsqueeze(0)
        self._target_index = torch.tensor([self.target_area_index], device=device)

    def trace_epoch(self, device: torch.device | None = None):
        """The groups this rank owns, from the current parameters to the field's flux on the target (:350-521): motor positions
        ``initial + tanh(parameter) * scale``, alignment with them, a new ray tracer (its blocking rectangles are the surfaces
        as they are aligned now) and the fused per-target trace, of which the target's bitmap is taken.  Returns
        ``(total_flux [res_u, res_e], intercept_factors, on_target_factors, blocking_factors)``, the factors field-wide
        ``[number of heliostats]`` with this rank's heliostats filled in."""
        device = _gpu_device(device)
        ddp = self.ddp_setup
        total_flux = None
        factors = torch.zeros((3, self.number_of_heliostats), device=device)
        for index in ddp["groups_to_ranks_mapping"][ddp["rank"]]:
            g = self.groups[index]
            group = g["group"]
            group.kinematics.motor_positions = g["initial"] + torch.tanh(g["parameter"]) * g["scale"]
            group.activate_heliostats(active_heliostats_mask=g["mask"], device=device)
            group.align_surfaces_with_motor_positions(motor_positions=group.kinematics.active_motor_positions,
                                                      active_heliostats_mask=g["mask"], device=device)
            tracer = HeliostatRayTracer(scenario=self.scenario, heliostat_group=group, blocking_active=self.blocking_active,
                                        world_size=ddp["heliostat_group_world_size"], rank=ddp["heliostat_group_rank"],
                                        batch_size=self.optimizer_dict["batch_size"], random_seed=ddp["heliostat_group_rank"],
                                        bitmap_resolution=self._resolution_cpu, dni=self.dni)
            # per-heliostat optics (an extension): the extinction over each slant range and the group's reflectivities, when
            # there are any - without them the call is the one it was
            optics_arguments = {}
            if g["extinction"] is not None:
                optics_arguments["ray_extinction_factor"] = g["extinction"]
            if getattr(group, "active_reflectivities", None) is not None:
                optics_arguments["mirror_reflectivity"] = group.active_reflectivities
            per_target, intercept, on_target, blocking = tracer.trace_rays_per_target(
                incident_ray_directions=g["incident"], active_heliostats_mask=g["mask"], target_area_indices=g["targets"],
                device=device, **optics_arguments)
            flux = per_target[self.target_area_index]
            total_flux = flux if total_flux is None else total_flux + flux
            rows = g["offset"] + tracer.get_sampler_indices().to(device)
            factors[:, rows] = torch.stack((intercept, on_target, blocking))
        if total_flux is None:                                       # a rank without a group of its own
            total_flux = torch.zeros((self._resolution_host[1], self._resolution_host[0]), device=device)
        if ddp["is_distributed"]:
            total_flux = distributed.all_reduce_sum_autograd(total_flux)
        return total_flux, factors[0], factors[1], factors[2]

    def epoch_loss(self, loss_definition, device: torch.device | None = None):
        """One epoch's forward pass: ``trace_epoch``, the flux loss against the ground truth, :func:`aim_point_objective`.
        Returns ``(total loss, flux loss, (flux-integral, intercept, local-flux term), total_flux, (three factors))``."""
        _require_kl(loss_definition)
        device = _gpu_device(device)
        total_flux, intercept, on_target, blocking = self.trace_epoch(device)
        flux_loss = loss_definition(prediction=total_flux.unsqueeze(0), ground_truth=self._ground_truth,
                                    target_area_indices=self._target_index, reduction_dimensions=(1, 2), device=device)
        total, *terms = aim_point_objective(flux_loss, total_flux, intercept, self.state)
        return total, flux_loss, tuple(terms), total_flux, (intercept, on_target, blocking)

    def _synchronize_gradients(self) -> None:
        """SUM over all ranks, divided by the world size (:681-702).  A group that another rank traced has no gradient here:
        it enters as zeros, so that every rank takes part in every group's reduce, in the same order (the reference skips a
        parameter without gradient, and its ranks would then pair up reduces of different groups)."""
        if self.ddp_setup["is_distributed"]:
            for g in self.groups:
                parameter = g["parameter"]
                if parameter.grad is None:
                    parameter.grad = torch.zeros_like(parameter)
                distributed.all_reduce_sum(parameter.grad)
                parameter.grad /= self.ddp_setup["world_size"]

    def _broadcast_motor_positions(self) -> None:
        """Every group's final motor positions from the first rank that owns the group (:704-722)."""
        if self.ddp_setup["is_distributed"]:
            for index, g in enumerate(self.groups):
                source = self.ddp_setup["ranks_to_groups_mapping"][index][0]
                torch.distributed.broadcast(g["group"].kinematics.motor_positions.detach(), src=source)
            log.info(f"Rank: {self.ddp_setup['rank']}, synchronized after aim point optimization.")

    def optimize(self, loss_definition, device: torch.device | None = None):
        """Optimise the motor positions (:724-972).  Returns ``(final loss on the CPU, loss history, intercept factors,
        on-target factors, blocking factors)``; the history has the keys ``HISTORY_KEYS``, one float per epoch.  Runs while
        the loss is above ``tolerance`` and ``epoch <= max_epoch`` - ``max_epoch + 1`` epochs at most - or until early stopping.
        The scenario's ``kinematics.motor_positions`` are left as the last epoch traced them."""
        _require_kl(loss_definition)                # (the reference would trace an epoch and then fail inside autograd)
        device = _gpu_device(device)
        rank = self.ddp_setup["rank"]
        if rank == 0:
            log.info("Start the aim point optimization.")
        self.prepare(device)
        optimizer, scheduler = self.optimizer, self.scheduler
        tolerance, max_epoch = float(self.optimizer_dict["tolerance"]), int(self.optimizer_dict["max_epoch"])
        log_step = max_epoch if self.optimizer_dict["log_step"] == 0 else self.optimizer_dict["log_step"]
        history = {key: [] for key in HISTORY_KEYS}
        factors = tuple(torch.zeros(self.number_of_heliostats, device=device) for _ in range(3))
        loss_host = float("inf")
        epoch = 0
        while loss_host > tolerance and epoch <= max_epoch:
            optimizer.zero_grad()
            loss, flux_loss, (integral_term, intercept_term, local_term), total_flux, factors = self.epoch_loss(loss_definition, device)
            loss.backward()
            self._synchronize_gradients()
            optimizer.step()
            # the epoch's scalars in ONE transfer (the stop test below needs the loss on the host, and so does ReduceLROnPlateau)
            with torch.no_grad():
                reference = self.state.flux_integral_reference
                scalars = torch.stack([s.detach().reshape(()) for s in (
                    loss, flux_loss, local_term, intercept_term, integral_term,
                    100 / reference * (total_flux.sum() - reference + 1e-8))]).tolist()
            loss_host = scalars[0]
            training.step_scheduler(scheduler, loss_host)
            if log_step and epoch % log_step == 0 and rank == 0:
                log.info(f"Epoch: {epoch}, Loss: {loss_host}, LR: {optimizer.param_groups[0]['lr']}")
            for key, value in zip(HISTORY_KEYS, scalars):
                history[key].append(value)
            if self.early_stopper.step(loss_host):
                log.info(f"Early stopping at epoch {epoch}.")
                break
            epoch += 1
        log.info(f"Rank: {rank}, aim points optimized.")
        self._broadcast_motor_positions()
        return torch.tensor([loss_host]), history, factors[0], factors[1], factors[2]
