"""The losses on vectors that ARTIST's alignment-driven kinematics reconstruction compares normals with.

Drop-ins for ``artist.optim.loss.VectorLoss``, ``AngleLoss`` and ``CosineSimilarityLoss`` (artist/optim/loss.py:61-121, 413-506):
called as ``loss(prediction, ground_truth, **kwargs)`` on ``[samples, 4]`` tensors, one value per sample.  A handful of torch ops
on a few floats per sample, on whichever device the arguments live (like ``artist_amd.flux_integral_constraint``); the flux
losses, which read whole bitmaps, are the fused ones of ``artist_amd.flux``; its four gain-invariant ones are exported here too.
"""
from __future__ import annotations

from typing import Any

import torch

from .flux import CosineFluxLoss, JensenShannonLoss, ShapePixelLoss, TotalVariationLoss  # noqa: F401  (the gain-invariant flux losses)

__all__ = ["VectorLoss", "AngleLoss", "CosineSimilarityLoss", "JensenShannonLoss", "ShapePixelLoss", "TotalVariationLoss",
           "CosineFluxLoss"]


class VectorLoss:
    """The squared distance between prediction and ground truth, summed over ``reduction_dimensions`` (a keyword the
    reference insists on, loss.py:111-121)."""

    def __init__(self) -> None:
        self.loss_function = torch.nn.MSELoss(reduction="none")

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        if "reduction_dimensions" not in kwargs:          # same message as artist/optim/loss.py:111-117
            raise ValueError("The vector loss expects 'reduction_dimensions' as keyword argument. Please add this argument.")
        return self.loss_function(prediction, ground_truth).sum(dim=kwargs["reduction_dimensions"])


class AngleLoss:
    """The angle in radians between the first three components of prediction and ground truth (loss.py:457-459).  Its
    derivative is unbounded where the two are parallel: the reconstructor zeroes non-finite gradients before it steps."""

    def __init__(self) -> None:
        self.loss_function = None

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        prediction = torch.nn.functional.normalize(prediction[:, :3])
        ground_truth = torch.nn.functional.normalize(ground_truth[:, :3])
        return torch.acos((prediction * ground_truth).sum(dim=-1).clamp(-1.0, 1.0))


class CosineSimilarityLoss:
    """One minus the cosine similarity of prediction and ground truth over the last dimension (loss.py:478, 506)."""

    def __init__(self) -> None:
        self.loss_function = torch.nn.CosineSimilarity(dim=-1)

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        return 1.0 - self.loss_function(prediction, ground_truth)
