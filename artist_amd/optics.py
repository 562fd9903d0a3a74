"""Per-heliostat optics: atmospheric attenuation by slant range, and the intensity factors of a heliostat group.

The reference takes one ``ray_extinction_factor`` and one ``mirror_reflectivity`` for the whole field; here
``HeliostatRayTracer.trace_rays`` takes either as a tensor with one value per active heliostat, and this
module makes such tensors: torch ops only, O(number of heliostats), on whichever device the arguments live, differentiable.

An attenuation ``model`` is one of

* ``("exponential", beta_per_km)``: transmittance ``exp(-beta d)``, ``d`` the slant range in km;
* ``("polynomial", coefficients)``: the LOSS fraction is ``sum_k c_k d^k`` (``d`` in km, ``c_0`` first), clamped to [0, 1] - the
  form of the DELSOL / Leary-Hankins fits.  No coefficients are shipped: take them from the source you trust;
* a callable ``slant range in metres [H] -> transmittance [H]``.
"""
from __future__ import annotations

import torch

__all__ = ["slant_ranges", "atmospheric_transmittance", "heliostat_intensity_factors"]


def slant_ranges(active_positions: torch.Tensor, target_centres: torch.Tensor) -> torch.Tensor:
    """Distance in metres from each active heliostat to its aim point: ``[H,4]`` (or ``[H,3]``) positions and centres -> ``[H]``."""
    if active_positions.dim() != 2 or active_positions.shape != target_centres.shape or active_positions.shape[1] not in (3, 4):
        raise ValueError(f"active_positions and target_centres must both be [H,4], got {tuple(active_positions.shape)} and "
                         f"{tuple(target_centres.shape)}")
    return torch.linalg.vector_norm(target_centres[:, :3] - active_positions[:, :3], dim=1)


def atmospheric_transmittance(slant_range: torch.Tensor, model) -> torch.Tensor:
    """Fraction of a ray's power that arrives after ``slant_range`` metres of atmosphere, in [0, 1]; ``model`` as in the
    module docstring."""
    if callable(model):
        return model(slant_range)
    try:
        kind, parameter = model
    except (TypeError, ValueError):
        raise ValueError(f"an attenuation model is ('exponential', beta_per_km), ('polynomial', coefficients) or a callable, "
                         f"got {model!r}") from None
    km = slant_range / 1000.0
    if kind == "exponential":
        beta = float(parameter)
        if not beta >= 0.0:
            raise ValueError(f"beta_per_km must be >= 0, got {beta}")
        return torch.exp(-beta * km)
    if kind == "polynomial":
        coefficients = [float(c) for c in parameter]
        if not coefficients:
            raise ValueError("a polynomial attenuation model needs at least one coefficient")
        loss = torch.full_like(km, coefficients[-1])
        for c in reversed(coefficients[:-1]):                   # Horner
            loss = loss * km + c
        return 1.0 - loss.clamp(0.0, 1.0)
    raise ValueError(f"unknown attenuation model {kind!r}; expected 'exponential', 'polynomial' or a callable")


def heliostat_intensity_factors(heliostat_group, solar_tower, target_area_indices: torch.Tensor, model):
    """``(ray_extinction_factor [H], mirror_reflectivity)`` for ``HeliostatRayTracer.trace_rays``: the extinction
    ``1 - transmittance`` over each active heliostat's slant range to the centre of its target area
    (``solar_tower.get_centers_of_target_areas``, the point the alignment aims at), and the group's
    ``active_reflectivities [H]`` - or the reference's default 0.935 as a float when the group has none."""
    positions = heliostat_group.active_positions
    centres = solar_tower.get_centers_of_target_areas(target_area_indices=target_area_indices, device=positions.device)
    transmittance = atmospheric_transmittance(slant_ranges(positions, centres.to(positions.dtype)), model)
    reflectivity = getattr(heliostat_group, "active_reflectivities", None)
    return (1.0 - transmittance).clamp(0.0, 1.0), (0.935 if reflectivity is None else reflectivity)
