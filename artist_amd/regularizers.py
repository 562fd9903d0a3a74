"""The surface regularisers of ARTIST's surface reconstruction on the gfx950 kernels ``art_surface_regularizers_fwd / _bwd``.

``SmoothnessRegularizer`` and ``IdealSurfaceRegularizer`` take the reference's constructor (``reduction_dimensions``) and call
signature (artist/optim/regularizers.py:60-186) and return what it returns: the per-(heliostat, facet) term summed over
``reduction_dimensions``.  ``surface_regularization_terms`` is ``SurfaceReconstructor._compute_regularization_terms``
(artist/optim/surface_reconstructor.py:656-749) with both terms from one launch.  The C ABI is declared in
``include/artist_hip_regularizers.h``; there is no CPU fallback.
"""
from __future__ import annotations

from typing import Any

import torch

from .ops import _f32c, _require_cuda, _timed_call

__all__ = ["Regularizer", "SmoothnessRegularizer", "IdealSurfaceRegularizer", "SurfaceRegularizers", "surface_regularizers",
           "surface_regularization_terms"]


def _check_nets(current: torch.Tensor, original: torch.Tensor) -> None:
    if not isinstance(current, torch.Tensor) or not isinstance(original, torch.Tensor):
        raise TypeError("the control points must be tensors")
    if current.dim() != 5 or current.shape[-1] != 3 or current.shape[2] < 1 or current.shape[3] < 1:
        raise ValueError(f"control points must be [H, F, U, V, 3] with U, V >= 1, got {tuple(current.shape)}")
    if original.shape != current.shape:
        raise ValueError(f"original control points {tuple(original.shape)} differ in shape from the current ones {tuple(current.shape)}")
    for x in (current, original):
        if not x.is_floating_point():
            raise TypeError(f"control points must be floating point, got {x.dtype}")


class SurfaceRegularizers(torch.autograd.Function):
    """Per-net smoothness and ideal-surface terms ``[H, F]`` of ``current`` against ``original`` (both ``[H, F, U, V, 3]``), one
    launch forward and one backward.  ``smoothness`` / ``ideal`` (bools) select the terms; an unselected one comes back as an empty
    tensor and costs nothing."""

    @staticmethod
    def forward(ctx, current, original, smoothness: bool, ideal: bool):
        _check_nets(current, original)
        dev = _require_cuda(current, original)
        current, original = _f32c(current), _f32c(original)
        H, F, U, V, _ = current.shape
        N = H * F
        out_s = current.new_empty((H, F) if smoothness else (0,))
        out_i = current.new_empty((H, F) if ideal else (0,))
        if N > 0 and (smoothness or ideal):
            _timed_call("art_surface_regularizers_fwd", dev, current.data_ptr(), original.data_ptr(), N, U, V,
                        out_s.data_ptr() if smoothness else None, out_i.data_ptr() if ideal else None)
        ctx.save_for_backward(current, original)
        ctx.set_materialize_grads(False)
        if not smoothness:
            ctx.mark_non_differentiable(out_s)
        if not ideal:
            ctx.mark_non_differentiable(out_i)
        return out_s, out_i

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_s, grad_i):
        current, original = ctx.saved_tensors
        need_cur, need_org = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_cur or need_org):
            return None, None, None, None
        dev = current.device
        H, F, U, V, _ = current.shape
        N = H * F
        gs = None if grad_s is None or grad_s.numel() == 0 else _f32c(grad_s)
        gi = None if grad_i is None or grad_i.numel() == 0 else _f32c(grad_i)
        g = torch.empty_like(current)
        if N > 0:
            _timed_call("art_surface_regularizers_bwd", dev, current.data_ptr(), original.data_ptr(), N, U, V,
                        None if gs is None else gs.data_ptr(), None if gi is None else gi.data_ptr(), g.data_ptr())
        return (g if need_cur else None), (-g if need_org else None), None, None


def surface_regularizers(current: torch.Tensor, original: torch.Tensor, smoothness: bool = True, ideal: bool = True):
    """``(smoothness [H, F], ideal [H, F])`` per net before any reduction; an unselected term is ``None``."""
    s, i = SurfaceRegularizers.apply(current, original, bool(smoothness), bool(ideal))
    return (s if smoothness else None), (i if ideal else None)


class Regularizer:
    """Base class of the regularisers (artist/optim/regularizers.py:6-57)."""

    def __init__(self, reduction_dimensions: tuple[int, ...]) -> None:
        self.reduction_dimensions = reduction_dimensions

    def __call__(self, current_control_points: torch.Tensor, original_control_points: torch.Tensor,
                 device: torch.device | None = None, **kwargs: Any) -> torch.Tensor:
        raise NotImplementedError("Must be overridden!")


class SmoothnessRegularizer(Regularizer):
    """Mean squared clamped Laplacian of the control-point displacement per surface (artist/optim/regularizers.py:60-131),
    summed over ``reduction_dimensions``."""

    def __call__(self, current_control_points: torch.Tensor, original_control_points: torch.Tensor,
                 device: torch.device | None = None, **kwargs: Any) -> torch.Tensor:
        s, _ = surface_regularizers(current_control_points, original_control_points, smoothness=True, ideal=False)
        return s.sum(dim=self.reduction_dimensions)


class IdealSurfaceRegularizer(Regularizer):
    """Mean squared control-point displacement per surface (artist/optim/regularizers.py:134-186), summed over
    ``reduction_dimensions``."""

    def __call__(self, current_control_points: torch.Tensor, original_control_points: torch.Tensor,
                 device: torch.device | None = None, **kwargs: Any) -> torch.Tensor:
        _, i = surface_regularizers(current_control_points, original_control_points, smoothness=False, ideal=True)
        return i.sum(dim=self.reduction_dimensions)


def surface_regularization_terms(current: torch.Tensor, original: torch.Tensor, flux_loss_per_heliostat: torch.Tensor,
                                 weight_smoothness: float, weight_ideal_surface: float, epsilon: float = 1e-12):
    """``(alpha, smoothness_per_heliostat, beta, ideal_per_heliostat)`` as ``SurfaceReconstructor._compute_regularization_terms``
    builds them (surface_reconstructor.py:656-749, regularisers reduced over the facets as at :940-945): ``current`` and
    ``original`` are the already selected ``[H, F, U, V, 3]`` nets.  Both terms come from one launch when both weights are > 0; a
    term with weight 0 is a zeros tensor outside the graph.  The balancing factors are the reference's, NOT detached:
    ``alpha = w_s * mean(flux loss) / (mean(S) + eps)`` with ``eps`` an fp32 tensor, and ``beta`` the same with ``I``
    (their gradient cancels most of the terms' own)."""
    smoothness = torch.zeros_like(flux_loss_per_heliostat)
    ideal = torch.zeros_like(flux_loss_per_heliostat)
    if weight_smoothness > 0 or weight_ideal_surface > 0:
        s, i = surface_regularizers(current, original, smoothness=weight_smoothness > 0, ideal=weight_ideal_surface > 0)
        if s is not None:
            smoothness = s.sum(dim=1)
        if i is not None:
            ideal = i.sum(dim=1)
    alpha = weight_smoothness * flux_loss_per_heliostat.mean() / (smoothness.mean() + torch.tensor(epsilon, dtype=torch.float32))
    beta = weight_ideal_surface * flux_loss_per_heliostat.mean() / (ideal.mean() + torch.tensor(epsilon, dtype=torch.float32))
    return alpha, smoothness, beta, ideal
