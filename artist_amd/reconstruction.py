"""What ``SurfaceReconstructor`` and ``KinematicsReconstructor`` share, and nothing that is specific to either: the
``parameters=(...)`` keyword, the learning rates by name, the device check, the fields of a group's state, the rows a rank owns,
the nested mean, the capture of a training step (``epoch_graph``), the synchronisation after the run - and the loop over the
groups, :meth:`Reconstructor._reconstruct`, which is the reference's loop (artist/optim/surface_reconstructor.py:842-1160,
kinematics_reconstructor.py:707-1063) written once.  What an epoch computes is each class's own.
"""
from __future__ import annotations

import logging
from dataclasses import dataclass, field
from functools import partial
from typing import Any

import torch

from . import _lib, distributed, graphs, training
from ._memo import Memo
from .sampling import RestrictedDistributedSampler

log = logging.getLogger(__name__)

__all__ = ["Reconstructor", "ReconstructionGroupState", "LearnsParameters", "canonical_parameters", "learning_rates",
           "tensors_held_by", "gpu_device", "scheduler_and_stopper"]


def canonical_parameters(parameters, names) -> tuple:
    """``parameters`` - a non-empty tuple or list of ``names`` (a reconstructor's parameter names in their canonical order),
    in any order, duplicates allowed - as a tuple in the canonical order.  Anything else is a ``ValueError`` that lists the
    names."""
    allowed = ", ".join(repr(name) for name in names)
    if not isinstance(parameters, (tuple, list)) or len(parameters) == 0:
        raise ValueError(f"parameters must be a non-empty tuple or list drawn from {allowed}; got {parameters!r}")
    unknown = [name for name in parameters if name not in names]
    if unknown:
        raise ValueError(f"unknown parameter(s) {unknown!r}: parameters must be drawn from {allowed}")
    return tuple(name for name in names if name in parameters)


def learning_rates(optimizer_dict: dict, parameters, keys: dict) -> dict:
    """The initial learning rate of every name in ``parameters`` (None: all of ``keys``), in the canonical order, from the
    configuration's ``"optimization"`` table.  ``keys`` maps a reconstructor's parameter names, in their canonical order, to
    their configuration keys; the first key is required, the others are optional and default to it."""
    names = tuple(keys)
    default = float(optimizer_dict[keys[names[0]]])
    return {name: float(optimizer_dict.get(keys[name], default))
            for name in canonical_parameters(names if parameters is None else parameters, names)}


def tensors_held_by(*holders, depth: int = 3) -> list:
    """Every tensor that ``holders`` - tensors, lists, tuples, dicts, objects with attributes - hold, ``depth`` levels down: what
    a reconstructor keeps for as long as a captured step reads it (``torch.cuda.graph`` does not keep a capture's inputs)."""
    found = []
    for holder in holders:
        if isinstance(holder, torch.Tensor):
            found.append(holder)
        elif depth > 0 and holder is not None:
            inner = holder.values() if isinstance(holder, dict) else holder if isinstance(holder, (list, tuple)) else \
                vars(holder).values() if hasattr(holder, "__dict__") else ()
            found += tensors_held_by(*inner, depth=depth - 1)
    return found


def gpu_device(device, who: str) -> torch.device:
    """``device`` (None: the current GPU) as a ``torch.device``; ``who`` refuses anything that is no GPU."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else device
    device = torch.device("cpu") if device is None else torch.device(device)
    if device.type != "cuda":
        raise _lib.ArtistHipError(f"{who} runs on the GPU only (device {device}); there is no CPU fallback")
    return device


def scheduler_and_stopper(optimizer: torch.optim.Optimizer, optimizer_dict: dict, scheduler_dict: dict) -> tuple:
    """The scheduler that ``scheduler_dict["scheduler_type"]`` names (``artist_amd.training``) and early stopping from the
    three ``early_stopping_*`` keys of ``optimizer_dict``."""
    scheduler = getattr(training, scheduler_dict["scheduler_type"])(optimizer=optimizer, parameters=scheduler_dict)
    stopper = training.EarlyStopping(window_size=optimizer_dict["early_stopping_window"],
                                     patience=optimizer_dict["early_stopping_patience"],
                                     min_improvement=optimizer_dict["early_stopping_delta"], relative=True)
    return scheduler, stopper


class _TakesParameters(type):
    """``SurfaceReconstructor(..., epoch_graph=False, parameters=(...))``: the class call takes the one keyword that the
    reference's constructor has no place for, checks it before ``__init__`` runs - so before any device work - and sets the
    attribute.  ``__init__`` itself keeps the signature both reconstructors share, the reference's arguments and then
    ``epoch_graph`` (tests/test_reconstructor_graphs_host.py holds it to that).  ``KinematicsReconstructor`` takes its
    keyword the same way: the class's ``PARAMETER_NAMES`` are the names it draws from, the first of them the default."""

    _first = object()       # (the keyword left out; None is a wrong value like any other)

    def __call__(cls, *args, parameters=_first, **kwargs):
        names = cls.PARAMETER_NAMES
        chosen = canonical_parameters(names[:1] if parameters is _TakesParameters._first else parameters, names)
        reconstructor = super().__call__(*args, **kwargs)
        reconstructor.parameters = chosen
        return reconstructor


class LearnsParameters(metaclass=_TakesParameters):
    """What the reconstructors share of the keyword: the attribute ``parameters``, checked and ordered on assignment against
    the class's ``PARAMETER_NAMES``; the first name alone unless chosen otherwise."""
    PARAMETER_NAMES: tuple = ()
    _parameters = None

    @property
    def parameters(self) -> tuple:
        """What learns, in the canonical order (``PARAMETER_NAMES``)."""
        return type(self).PARAMETER_NAMES[:1] if self._parameters is None else self._parameters

    @parameters.setter
    def parameters(self, parameters) -> None:
        self._parameters = canonical_parameters(parameters, type(self).PARAMETER_NAMES)


@dataclass
class ReconstructionGroupState:
    """What the epochs of one heliostat group share, whatever is reconstructed (a reconstructor's ``prepare``)."""
    index: int
    group: Any
    mask: torch.Tensor
    split: training.TrainTestSplit
    active_rows: torch.Tensor                   # group-local rows of the heliostats that have samples, [active] on the device
    optimizer: torch.optim.Optimizer
    scheduler: Any
    early_stopper: training.EarlyStopping
    activated: str | None = None                # "train" / "test": which samples the group is activated for
    tracers: dict = field(default_factory=dict)
    rows: dict = field(default_factory=dict)    # per kind: (sample rows, heliostat rows) of this rank, None = all
    # this rank's rows of the per-sample tensors (_own): flux and targets, train and test - four, so eight are never reached
    own: Memo = field(default_factory=lambda: Memo("this rank's rows of a per-sample tensor", capacity=8, under_capture="serve"))
    # epoch_graph: the captured training step and what is kept alive for it
    graph: Any = None
    kept: list = field(default_factory=list)
    # what learns: name -> the tensor itself, in the canonical order (the class's PARAMETER_NAMES)
    learnables: dict = field(default_factory=dict)


class Reconstructor(LearnsParameters):
    """The base of both reconstructors.  A subclass has the attributes ``ddp_setup``, ``scenario``, ``data``,
    ``optimizer_dict``, ``scheduler_dict``, ``bitmap_resolution`` and ``epoch_graph``, the methods ``prepare``, ``validate``,
    ``build_epoch_graph`` and ``close_epoch_graph``, ``HISTORY_KEYS`` - the per-epoch lists of a group's history, the loss
    first - and what :meth:`_reconstruct` calls per epoch: :meth:`_step`, :meth:`_before_optimizer_step`,
    :meth:`_host_values` and, per group, :meth:`_finish_group`."""
    HISTORY_KEYS: tuple = ()
    RECONSTRUCTS = ""           # what the log lines say is reconstructed: "surface", "kinematics"

    def _device(self, device) -> torch.device:
        return gpu_device(device, type(self).__name__)

    # -------------------------------------------------------------------------------- before a group's first epoch
    def _parse_and_split(self, heliostat_group_index: int, device):
        """The group's calibration samples from ``data["data_parser"].parse_data_for_reconstruction`` - ``(the six tensors,
        the train/test split, the group-local rows of the heliostats that have samples)`` - or None for a group without
        samples."""
        group = self.scenario.heliostat_field.heliostat_groups[heliostat_group_index]
        six = self.data["data_parser"].parse_data_for_reconstruction(
            heliostat_data_mapping=self.data["heliostat_data_mapping"], heliostat_group=group, scenario=self.scenario,
            bitmap_resolution=self.bitmap_resolution, device=device)
        flux_measured, focal_spots, incident, motor_positions, mask, targets = six
        active_rows = torch.nonzero(mask > 0, as_tuple=True)[0]
        if active_rows.numel() == 0:
            return None
        split = training.train_test_split(active_heliostats_mask=mask, flux_measured=flux_measured, focal_spots_measured=focal_spots,
                                          incident_ray_directions=incident, motor_positions=motor_positions,
                                          target_area_indices=targets, device=device)
        return six, split, active_rows

    def _optimizer_for(self, learnables: dict, rate_keys: dict) -> tuple:
        """``(artist_amd.optim.Adam, scheduler, early stopper)`` for ``learnables`` (name -> tensor, in the canonical order):
        one parameter group per tensor at the rate ``rate_keys`` names for it (:func:`learning_rates`), ``requires_grad_()`` on
        each.  The leaves are only marked here: nothing builds an autograd graph through them before the first step
        (graphs.py, "Fresh leaves")."""
        from .optim import Adam
        rates = learning_rates(self.optimizer_dict, tuple(learnables), rate_keys)
        optimizer = Adam([dict(params=[tensor.requires_grad_()], lr=rates[name]) for name, tensor in learnables.items()],
                         lr=float(self.optimizer_dict[next(iter(rate_keys.values()))]))
        return (optimizer, *scheduler_and_stopper(optimizer, self.optimizer_dict, self.scheduler_dict))

    # -------------------------------------------------------------------------------- this rank's share of a group
    def _rank_rows(self, state, kind: str, device):
        """``(sample rows, heliostat rows)`` that this rank owns among the group's samples of ``kind`` and among its active
        heliostats - index tensors on the device, or ``(None, None)`` when it owns all.  From the sampler's host list
        (artist/raytracing/sampling.py:107-157): a heliostat's samples stay together."""
        if kind not in state.rows:
            split = state.split
            samples = split.number_of_train_samples if kind == "train" else split.number_of_test_samples
            active = int(state.active_rows.numel())
            owned = RestrictedDistributedSampler(active * samples, active, self.ddp_setup["heliostat_group_world_size"],
                                                 self.ddp_setup["heliostat_group_rank"]).rank_indices
            if owned == list(range(active * samples)):
                state.rows[kind] = (None, None)
            else:
                state.rows[kind] = (torch.tensor(owned, dtype=torch.long, device=device),
                                    torch.tensor([i // samples for i in owned[::samples]], dtype=torch.long, device=device))
        return state.rows[kind]

    def _own(self, state, kind: str, per_sample: torch.Tensor, device) -> torch.Tensor:
        """This rank's rows of a per-sample tensor of ``kind``; the tensor itself when the rank owns all (kept per tensor object
        and version, so that callers which remember a tensor object they have checked meet the same object every epoch)."""
        sample_rows, _ = self._rank_rows(state, kind, device)
        if sample_rows is None:
            return per_sample
        return state.own.lookup(per_sample, lambda: per_sample.index_select(0, sample_rows), key=kind)

    def _nested_mean(self, gradient: torch.Tensor | None) -> None:
        """In nested mode the ranks that share a group average ``gradient``, in place: SUM over ``process_subgroup``, divided
        by the sub-world size.  None, or a run that is not nested: nothing."""
        ddp = self.ddp_setup
        if gradient is not None and ddp["is_nested"]:
            distributed.all_reduce_sum(gradient, group=ddp["process_subgroup"])
            gradient /= ddp["heliostat_group_world_size"]

    # -------------------------------------------------------------------------------- epoch_graph
    def _capture(self, state, loss_definition, device):
        """:meth:`_step` as an ``artist_amd.EpochGraph`` on ``state.graph``, after two warm-up runs, and on ``state.kept`` every
        tensor that the state, the group, its kinematics and actuators hold now.  A capture that fails closes what it began
        (``close_epoch_graph``) and raises as it is."""
        try:
            state.graph = graphs.EpochGraph(partial(self._step, state, loss_definition, device), warmup=2,
                                            parameters=list(state.learnables.values()), device=device)
        except BaseException:
            self.close_epoch_graph(state)
            raise
        kinematics = getattr(state.group, "kinematics", None)
        state.kept = tensors_held_by(state, state.group, kinematics, getattr(kinematics, "actuators", None))
        return state.graph

    def _release(self, state) -> None:
        """Close ``state.graph``, let go of what was kept for it and detach the surfaces the capture left on the group."""
        if state.graph is not None:
            state.graph.close()
        state.graph, state.kept = None, []
        group = state.group
        group.active_surface_points, group.active_surface_normals = group.active_surface_points.detach(), group.active_surface_normals.detach()

    # -------------------------------------------------------------------------------- after the run
    def _gather(self, final_loss_per_heliostat: torch.Tensor, loss_history: list, tensors_to_broadcast) -> list:
        """The end of a run on several ranks: per group, in the field's order, every tensor of ``tensors_to_broadcast(group)``
        from the first rank that owns the group; the final losses MIN-reduced (a heliostat another rank reconstructed is
        ``inf`` here); the histories of all ranks gathered.  Returns the histories per rank; ``[loss_history]``, and no
        collective, in a single process."""
        ddp = self.ddp_setup
        if not ddp["is_distributed"]:
            return [loss_history]
        with torch.no_grad():
            for index, group in enumerate(self.scenario.heliostat_field.heliostat_groups):
                for tensor in tensors_to_broadcast(group):
                    torch.distributed.broadcast(tensor.detach(), src=ddp["ranks_to_groups_mapping"][index][0])
        torch.distributed.all_reduce(final_loss_per_heliostat, op=torch.distributed.ReduceOp.MIN)
        histories: list = [[] for _ in range(ddp["world_size"])]
        torch.distributed.all_gather_object(histories, loss_history)
        log.info(f"Rank: {ddp['rank']}, synchronized after {self.RECONSTRUCTS} reconstruction.")
        return histories

    # -------------------------------------------------------------------------------- the loop
    def _step(self, state, loss_definition, device) -> tuple:
        """The training step up to and including ``backward()``: what an eager epoch runs, what :meth:`_capture` captures and
        so what ``state.graph.replay()`` returns.  A tuple of detached tensors: the epoch's scalars, the loss per heliostat of
        this rank, and whatever else the class wants of an epoch."""
        raise NotImplementedError

    def _before_optimizer_step(self, state, outcome: tuple, device) -> None:
        """Between ``backward()`` and ``optimizer.step()``, with the step's ``outcome``: what is done to the gradients, and in
        which order."""
        raise NotImplementedError

    def _host_values(self, scalars: torch.Tensor) -> list:
        """The epoch's ONE read of the device: ``scalars`` as floats in the order of ``HISTORY_KEYS`` - what the epoch's
        history entry holds, the loss first."""
        raise NotImplementedError

    def _finish_group(self, state) -> None:
        """A group's ``finally``, after its graph has been closed; it also runs when the loop raises."""

    def _reconstruct(self, loss_definition, device) -> tuple:
        """The groups this rank owns, one after the other.  Returns ``(final loss per heliostat of the scenario on the device,
        +inf where a heliostat was not reconstructed; this rank's histories, one entry per group)``; an entry has a list of
        floats per name of ``HISTORY_KEYS`` and ``"test_loss"``, the last validation's result.

        A group runs while its loss is above ``tolerance`` and ``epoch <= max_epoch``, or until early stopping, which ends
        the group before that epoch's history entry.  An epoch: ``zero_grad``, :meth:`_step` or its replay,
        :meth:`_before_optimizer_step`, ``optimizer.step()``, :meth:`_host_values` - the one read, after the step has been
        queued - the scheduler, the early stopper, a validation when one is due, the history entry."""
        rank = self.ddp_setup["rank"]
        sizes = [int(group.number_of_heliostats) for group in self.scenario.heliostat_field.heliostat_groups]
        final_loss_per_heliostat = torch.full((sum(sizes),), torch.inf, device=device)
        tolerance, max_epoch = float(self.optimizer_dict["tolerance"]), int(self.optimizer_dict["max_epoch"])
        log_step = max_epoch if self.optimizer_dict["log_step"] == 0 else int(self.optimizer_dict["log_step"])
        loss_history: list[dict] = []

        for group_index in self.ddp_setup["groups_to_ranks_mapping"][rank]:
            state = self.prepare(group_index, device)
            if state is None:                                        # a group without samples
                continue
            optimizer, scheduler = state.optimizer, state.scheduler
            history: dict = {key: [] for key in self.HISTORY_KEYS}
            test_loss = None
            loss_host = float("inf")
            epoch = 0
            if self.epoch_graph:
                self.build_epoch_graph(state, loss_definition, device)
            try:
                while loss_host > tolerance and epoch <= max_epoch:
                    optimizer.zero_grad()
                    outcome = self._step(state, loss_definition, device) if state.graph is None else state.graph.replay()
                    self._before_optimizer_step(state, outcome, device)
                    optimizer.step()
                    values = self._host_values(outcome[0])
                    loss_host = values[0]
                    training.step_scheduler(scheduler, loss_host)
                    stop = state.early_stopper.step(loss_host)
                    if not log_step or epoch % log_step == 0 or epoch == max_epoch - 1 or stop:
                        log.info(f"Rank: {rank}, Epoch: {epoch}, Loss: {loss_host}")
                        test_loss = self.validate(state, device)
                    if stop:
                        log.info(f"Early stopping at epoch {epoch}.")
                        break
                    for key, value in zip(self.HISTORY_KEYS, values):
                        history[key].append(value)
                    epoch += 1
                history["test_loss"] = test_loss
                loss_history.append(history)

                _, heliostat_rows = self._rank_rows(state, "train", device)
                rows = state.active_rows if heliostat_rows is None else state.active_rows.index_select(0, heliostat_rows)
                final_loss_per_heliostat[rows + sum(sizes[:group_index])] = outcome[1]                  # (the last epoch's)
            finally:
                if state.graph is not None:
                    self.close_epoch_graph(state)
                self._finish_group(state)
            log.info(f"Rank: {rank}, {self.RECONSTRUCTS} of group {group_index} reconstructed.")
        return final_loss_per_heliostat, loss_history
