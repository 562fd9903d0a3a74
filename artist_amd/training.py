"""What ARTIST's optimisers share around the epoch: learning-rate schedulers by name, early stopping.

Drop-ins for ``artist.optim.training`` (artist/optim/training.py:13-186): the same function names - an optimiser's
configuration names one of them under ``"scheduler_type"`` - the same configuration keys, the same stopping rule.  Host-side
bookkeeping only; the schedulers are torch's own and work with ``artist_amd.optim.Adam``, which is a ``torch.optim.Optimizer``.
"""
from __future__ import annotations

from collections import deque

import torch

__all__ = ["exponential", "cyclic", "reduce_on_plateau", "EarlyStopping"]


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
