"""What ARTIST's optimisers share around the epoch: learning-rate schedulers by name, early stopping.

Drop-ins for ``artist.optim.training`` (artist/optim/training.py:13-367): the same function names - an optimiser's
configuration names one of them under ``"scheduler_type"`` - the same configuration keys, the same stopping rule, the same
train/test split of the calibration samples; ``reduce_loss_per_sample`` is ``artist.optim.loss``'s (loss.py:509-549).  Host-side
bookkeeping only; the schedulers are torch's own and work with ``artist_amd.optim.Adam``, which is a ``torch.optim.Optimizer``.
"""
from __future__ import annotations

from collections import deque
from dataclasses import dataclass
from typing import Any, Callable

import torch

__all__ = ["exponential", "cyclic", "reduce_on_plateau", "step_scheduler", "EarlyStopping", "TrainTestSplit", "train_test_split",
           "reduce_loss_per_sample"]


def exponential(optimizer: torch.optim.Optimizer, parameters: dict) -> torch.optim.lr_scheduler.LRScheduler:
    """``ExponentialLR`` with ``parameters["gamma"]``."""
    return torch.optim.lr_scheduler.ExponentialLR(optimizer, gamma=float(parameters["gamma"]))


def cyclic(optimizer: torch.optim.Optimizer, parameters: dict) -> torch.optim.lr_scheduler.LRScheduler:
    """``CyclicLR`` between ``parameters["lr_min"]`` and ``["lr_max"]``, ``["step_size_up"]`` steps up."""
    return torch.optim.lr_scheduler.CyclicLR(optimizer, base_lr=float(parameters["lr_min"]), max_lr=float(parameters["lr_max"]),
                                             step_size_up=int(parameters["step_size_up"]))


def reduce_on_plateau(optimizer: torch.optim.Optimizer, parameters: dict) -> torch.optim.lr_scheduler.ReduceLROnPlateau:
    """``ReduceLROnPlateau`` with ``parameters["reduce_factor"]``, ``["patience"]``, ``["threshold"]``, ``["cooldown"]`` and
    ``["lr_min"]`` as the floor."""
    return torch.optim.lr_scheduler.ReduceLROnPlateau(
        optimizer, factor=float(parameters["reduce_factor"]), patience=int(parameters["patience"]),
        threshold=float(parameters["threshold"]), cooldown=int(parameters["cooldown"]), min_lr=float(parameters["lr_min"]))


def step_scheduler(scheduler, loss: float) -> None:
    """One epoch's step of ``scheduler``: ``ReduceLROnPlateau`` wants the epoch's loss, the others take nothing."""
    if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
        scheduler.step(loss)
    else:
        scheduler.step()


class EarlyStopping:
    """Stop when the loss has stopped improving over a sliding window (artist/optim/training.py:93-185).

    ``step(loss)`` keeps the last ``window_size`` losses.  Once the window is full, the improvement is the oldest loss minus
    the newest - divided by ``max(|oldest|, eps)`` when ``relative`` - and a call whose improvement does not exceed
    ``min_improvement`` counts; one that does resets the count.  ``step`` returns True when ``patience`` calls in a row have
    counted.  Before the window is full nothing is decided."""

    def __init__(self, window_size: int = 10, patience: int = 20, min_improvement: float = 1e-4, relative: bool = True,
                 eps: float = 1e-8) -> None:
        self.window_size = window_size
        self.patience = patience
        self.min_improvement = min_improvement
        self.relative = relative
        self.eps = eps
        self.loss_history: deque = deque(maxlen=window_size)
        self.counter = 0

    def step(self, loss: float) -> bool:
        window = self.loss_history
        window.append(loss)
        if len(window) < self.window_size:
            return False
        oldest, newest = window[0], window[-1]
        improvement = oldest - newest
        if self.relative:
            improvement /= max(abs(oldest), self.eps)
        self.counter = 0 if improvement > self.min_improvement else self.counter + 1
        return self.counter >= self.patience


@dataclass
class TrainTestSplit:
    """The calibration samples of one heliostat group, split (artist/optim/training.py:188-265): the five per-sample tensors of
    the training and of the test samples, the masks after the split (samples per heliostat), the positions of both kinds in the
    unsplit tensors (host tensors) and the three counts per heliostat."""
    flux_measured_train: torch.Tensor
    focal_spots_measured_train: torch.Tensor
    incident_ray_directions_train: torch.Tensor
    motor_positions_train: torch.Tensor
    target_area_indices_train: torch.Tensor

    flux_measured_test: torch.Tensor
    focal_spots_measured_test: torch.Tensor
    incident_ray_directions_test: torch.Tensor
    motor_positions_test: torch.Tensor
    target_area_indices_test: torch.Tensor

    active_heliostats_mask_train: torch.Tensor
    active_heliostats_mask_test: torch.Tensor

    train_indices: torch.Tensor
    test_indices: torch.Tensor

    number_of_train_samples: int
    number_of_test_samples: int
    number_of_samples_per_heliostat: int


def train_test_split(active_heliostats_mask: torch.Tensor, flux_measured: torch.Tensor, focal_spots_measured: torch.Tensor,
                     incident_ray_directions: torch.Tensor, motor_positions: torch.Tensor, target_area_indices: torch.Tensor,
                     test_fraction: float = 0.25, device: torch.device | None = None) -> TrainTestSplit:
    """Split every heliostat's samples in their order (artist/optim/training.py:268-367).  The mask holds the number of samples
    per heliostat - the same for every heliostat that has any - and the per-sample tensors hold the heliostats' blocks one
    after the other.  ``max(1, int(samples * test_fraction))`` samples from the END of each block are the test samples, the ones
    before them the training samples.  The index tensors live on the host; the masks stay where ``active_heliostats_mask`` is.
    Reads the mask once (two counts in one transfer)."""
    total, active = (int(v) for v in torch.stack((active_heliostats_mask.sum(), (active_heliostats_mask > 0).sum())).tolist())
    per_heliostat = int(total / active)
    n_test = max(1, int(per_heliostat * test_fraction))
    n_train = per_heliostat - n_test
    starts = torch.arange(active) * per_heliostat
    train_indices = (starts[:, None] + torch.arange(n_train)).reshape(-1)
    test_indices = (starts[:, None] + torch.arange(n_train, per_heliostat)).reshape(-1)
    take = lambda t, index: t[index.to(t.device)]  # noqa: E731
    per_sample = (flux_measured, focal_spots_measured, incident_ray_directions, motor_positions, target_area_indices)
    return TrainTestSplit(*(take(t, train_indices) for t in per_sample), *(take(t, test_indices) for t in per_sample),
                          active_heliostats_mask_train=torch.clamp(active_heliostats_mask - n_test, min=0),
                          active_heliostats_mask_test=torch.clamp(active_heliostats_mask - n_train, min=0),
                          train_indices=train_indices, test_indices=test_indices, number_of_train_samples=n_train,
                          number_of_test_samples=n_test, number_of_samples_per_heliostat=per_heliostat)


def reduce_loss_per_sample(loss_per_sample: torch.Tensor, number_of_samples_per_heliostat: int,
                           reduction: Callable[..., Any]) -> torch.Tensor:
    """A loss per sample ``[heliostats * samples]`` -> a loss per heliostat (artist/optim/loss.py:509-549): ``reduction`` is
    applied to the ``[heliostats, samples]`` view - ``partial(torch.mean, dim=-1)``, ``partial(torch.median, dim=-1)``, whose
    ``values`` are taken.  Samples beyond the last whole heliostat are dropped."""
    heliostats = int(loss_per_sample.numel() // number_of_samples_per_heliostat)
    whole = loss_per_sample[:heliostats * number_of_samples_per_heliostat]
    reduced = reduction(whole.view(heliostats, number_of_samples_per_heliostat))
    return reduced if isinstance(reduced, torch.Tensor) else reduced.values
