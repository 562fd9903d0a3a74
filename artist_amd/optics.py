"""Per-heliostat optics: atmospheric attenuation by slant range, and the intensity factors of a heliostat group.

The reference takes one ``ray_extinction_factor`` and one ``mirror_reflectivity`` for the whole field; here
``HeliostatRayTracer.trace_rays`` takes either as a tensor with one value per active heliostat, and this
module makes such tensors: torch ops only, O(number of heliostats), on whichever device the arguments live, differentiable.

An attenuation ``model`` is one of

* ``("exponential", beta_per_km)``: transmittance ``exp(-beta d)``, ``d`` the slant range in km;
* ``("polynomial", coefficients)``: the LOSS fraction is ``sum_k c_k d^k`` (``d`` in km, ``c_0`` first), clamped to [0, 1] - the
  form of the DELSOL / Leary-Hankins fits.  No coefficients are shipped: take them from the source you trust;
* a callable ``slant range in metres [H] -> transmittance [H]``.

Mirror slope errors: :func:`tilt_normals` tilts surface normals by slope pairs before alignment,
:func:`slope_sample` draws the standard-normal pairs of a group's heliostats, :func:`expand_over_samples` repeats per-heliostat
rows over their activations with a fixed-order backward.

The convolved sun: :func:`sun_image_covariance` is the covariance, in pixels^2, of the image that a Gaussian
sun leaves on a planar target around each heliostat's chief ray - the window of ``artist_amd.flux.blur_flux``.  With the unit
angular covariance ``(1, 0, 1)`` it is the metric ``M = J J^T`` of a radial sun's image, the window of
``artist_amd.flux.radial_blur_flux``; :func:`radial_window_kept_fraction` says how much of such a sun its 64-pixel stencil keeps.
"""
from __future__ import annotations

import contextlib

import torch

__all__ = ["slant_ranges", "atmospheric_transmittance", "heliostat_intensity_factors", "tilt_normals", "slope_sample",
           "expand_over_samples", "SLOPE_ERROR_STREAM", "sun_image_covariance", "radial_window_kept_fraction",
           "RADIAL_WINDOW_RADIUS"]

#: The stream of a mirror's slope-error sample is the sampler's with the seed XOR this: the 64-bit constant of
#: the splitmix64 finaliser, non-zero and different from ``artist_amd.scene.OPTICAL_ERROR_STREAM``, so that the Philox keys
#: (seed, row) of the sun, of the optical error and of the slope error all differ.
SLOPE_ERROR_STREAM = 0xBF58476D1CE4E5B9
_NO_CPU_SLOPES = ("slope errors are not drawn on the CPU: their sample comes from the HIP sampler's Philox streams, which have no "
                  "CPU fallback; put the group on the GPU (or hand the group a sample of your own, HeliostatGroup.slope_sample)")


def tilt_normals(normals: torch.Tensor, slopes: torch.Tensor) -> torch.Tensor:
    """Surface normals ``[..., 4]`` in the heliostat's canonical frame (before alignment), each tilted by its slope pair
    ``slopes [..., 2]``: with ``x = (1, 0, 0)``, ``t1 = normalize(x - (x.n) n)``, ``t2 = n x t1`` and
    ``n' = normalize(n + a t1 + b t2)`` on the xyz part; w passes through.  ``(a, b)`` are slopes - the tangents of the tilt
    angles about ``-t2`` and ``t1`` - the quantity deflectometry reports; any tensor will do, a measured residual map or
    ``sigma * zeta`` with :func:`slope_sample`.  Torch ops, differentiable in both arguments, on whichever device they live;
    zero slopes give ``normalize(n)`` bit for bit.  A normal along x has no ``t1`` and comes back as ``normalize(n)``."""
    if normals.shape[-1] != 4 or slopes.shape[-1] != 2 or normals.shape[:-1] != slopes.shape[:-1]:
        raise ValueError(f"normals must be [...,4] and slopes [...,2] with the same leading shape, got {tuple(normals.shape)} and "
                         f"{tuple(slopes.shape)}")
    normalize = torch.nn.functional.normalize
    n = normals[..., :3]
    x = torch.zeros_like(n)
    x[..., 0] = 1.0
    t1 = normalize(x - n[..., :1] * n, dim=-1)
    t2 = torch.linalg.cross(n, t1, dim=-1)
    tilted = normalize(n + slopes[..., :1] * t1 + slopes[..., 1:] * t2, dim=-1)
    return torch.cat((tilted, normals[..., 3:]), dim=-1)


def slope_sample(rows, number_of_points: int, seed: int, device) -> torch.Tensor:
    """The standard-normal slope pairs ``zeta [len(rows), P, 2]`` of heliostats ``rows`` - their indices IN THE GROUP, not
    active rows: a mirror keeps its roughness across samples, sun positions and ranks, so every activation of a heliostat shares
    its realisation, and a rank's rows are the rows of the full draw.  One ``art_sample_distortions`` launch with one ray per
    point, ``loc = 0``, ``scale_tril = I`` and the seed XOR ``SLOPE_ERROR_STREAM``.  On the GPU only (``ValueError`` otherwise)."""
    from . import ops
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(_NO_CPU_SLOPES)
    key = (int(seed) & 0xFFFFFFFFFFFFFFFF) ^ SLOPE_ERROR_STREAM
    rows = [int(r) for r in rows]
    return ops.sample_distortions(rows, 1, int(number_of_points), key, (0.0, 0.0), ((1.0, 0.0), (0.0, 1.0)), device).reshape(
        len(rows), int(number_of_points), 2)


def expand_over_samples(tensor: torch.Tensor, counts, rows: torch.Tensor | None = None) -> torch.Tensor:
    """Row ``i`` of ``tensor [N, ...]`` ``counts[i]`` times, rows in order: the values of ``repeat_interleave(counts)``, whose
    backward is an ``index_add`` with float atomics on the device.  Here the gradient of a row that is repeated is summed in a
    fixed order: with one count for all rows that have any (the usual activation) the rows are taken once - ``rows``, their
    indices on the tensor's device, or all of them for None - and expanded over the sample axis with a view, backwards
    ``[rows, samples, ...].sum(1)``, as the kinematics reconstructor expands its deviations; with mixed counts, a
    concatenation of per-row expansions."""
    counts = [int(c) for c in counts]
    taken = [i for i, c in enumerate(counts) if c]
    shape = tuple(tensor.shape[1:])
    if len({counts[i] for i in taken}) <= 1:
        samples = counts[taken[0]] if taken else 0
        if len(taken) != len(counts):
            tensor = tensor.index_select(0, torch.tensor(taken, dtype=torch.long, device=tensor.device) if rows is None else rows)
        return tensor.reshape(len(taken), 1, *shape).expand(len(taken), samples, *shape).reshape(len(taken) * samples, *shape)
    return torch.cat([tensor[i:i + 1].expand(counts[i], *shape) for i in taken])


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


def sun_image_covariance(points: torch.Tensor, normals: torch.Tensor, incident: torch.Tensor, target_area_indices: torch.Tensor,
                         centers: torch.Tensor, plane_normals: torch.Tensor, dimensions: torch.Tensor,
                         angular_covariance: torch.Tensor, resolution, differentiable: bool = False) -> torch.Tensor:
    """``[H,3]`` = ``(S_rr, S_rc, S_cc)`` in pixels^2 (r the bitmap's row, c its column): the covariance of the spot that a
    Gaussian sun of ``angular_covariance`` - ``(C_uu, C_ue, C_ee)`` in rad^2, ``[3]`` or one row per heliostat ``[H,3]``, in the
    ``(u, e)`` order of the distortions - leaves on the planar target of each heliostat, to first order in the tilt of the
    reflected ray.

    ``points``, ``normals [H,P,4]`` the aligned surfaces, ``incident [H,4]``, ``target_area_indices [H]`` into the PLANAR tables
    ``centers``, ``plane_normals [T,4]`` and ``dimensions [T,2]`` (width, height), ``resolution`` = (columns, rows) of the bitmap,
    the tracer's ``bitmap_resolution``.  Per heliostat: ``o`` the mean point, ``n`` the normalised mean normal,
    ``d = i - 2 (i.n) n`` the chief ray, ``t = ((c - o).m) / (d.m)`` its range to the plane of normal ``m``.  A tilt ``(u, e)``
    turns ``d`` by ``u a_u + e a_e`` with ``a_u = (-d_n, d_e, 0)`` and ``a_e = (0, -d_u, d_n)`` (the first-order term of the
    reference's ``rotate_distortions``), which moves the hit point by ``t (a - d (a.m) / (d.m))``; with the bitmap's two flips
    (row = top - U, column = right - E) that is ``J [2,2]`` and ``S = J C J^T``.

    One ``J`` per heliostat: slant range and incidence vary by about a percent across a mirror.  Torch ops in fp64 on a few
    values per heliostat, under ``no_grad``, on the arguments' device, no synchronisation; the result is fp32 and a constant
    (to first order the image does not depend on the learned surface).

    ``differentiable=True``: ``J`` is a constant as before, and ``S = J C J^T`` is formed by the same fp64 ops
    inside the autograd graph of ``angular_covariance`` - the same values, bit for bit, and a gradient for a covariance that
    learns (a heliostat's optical error through ``C + sigma_h^2 I``)."""
    with torch.no_grad():
        f64 = torch.float64
        # (the sums run in fp64 inside the reduction: no fp64 copy of the surfaces)
        o = points[..., :3].mean(dim=1, dtype=f64)
        n = torch.nn.functional.normalize(normals[..., :3].mean(dim=1, dtype=f64), dim=-1)
        i = incident[..., :3].to(f64)
        d = i - 2.0 * (i * n).sum(-1, keepdim=True) * n
        index = target_area_indices.long()
        c = centers.index_select(0, index)[:, :3].to(f64)
        m = plane_normals.index_select(0, index)[:, :3].to(f64)
        size = dimensions.index_select(0, index).to(f64)
        dm = (d * m).sum(-1, keepdim=True)
        t = ((c - o) * m).sum(-1, keepdim=True) / dm
        # the two tilt axes at once: a_u = z x d = (-d_n, d_e, 0) and a_e = x x d = (0, -d_u, d_n), as [H,2,3]
        eye = torch.eye(3, dtype=f64, device=d.device)
        axes = torch.stack((eye[2], eye[0])).unsqueeze(0).expand(d.shape[0], 2, 3)
        d2, m2 = d.unsqueeze(1), m.unsqueeze(1)
        a = torch.linalg.cross(axes, d2.expand(-1, 2, -1), dim=-1)
        shift = t.unsqueeze(1) * (a - d2 * ((a * m2).sum(-1, keepdim=True) / dm.unsqueeze(1)))       # [H, (u, e), (E, N, U)]
        per_metre = torch.stack(((float(resolution[1]) - 1.0) / size[:, 1], (float(resolution[0]) - 1.0) / size[:, 0]), dim=-1)
        # J [H, (row, column), (u, e)]: row = top - U, column = right - E
        J = -torch.stack((shift[..., 2], shift[..., 0]), dim=1) * per_metre.unsqueeze(-1)
    with contextlib.nullcontext() if differentiable else torch.no_grad():
        C = angular_covariance.to(device=d.device, dtype=f64)
        if C.shape not in ((3,), (d.shape[0], 3)):
            raise ValueError(f"angular_covariance must be [3] or [{d.shape[0]},3] = (C_uu, C_ue, C_ee), got {tuple(C.shape)}")
        C = torch.stack((C[..., 0], C[..., 1], C[..., 1], C[..., 2]), dim=-1).reshape(-1, 2, 2)      # [H or 1, (u, e), (u, e)]
        JC = (J.unsqueeze(-1) * C.unsqueeze(1)).sum(dim=2)                                           # element-wise: no batched GEMM
        S = (JC.unsqueeze(2) * J.unsqueeze(1)).sum(dim=-1)                                           # [H, (r, c), (r, c)]
        return torch.stack((S[:, 0, 0], S[:, 0, 1], S[:, 1, 1]), dim=-1).to(torch.float32)


#: the radial window's stencil reaches 64 pixels from its centre, in rows and in columns (the Gaussian blur's own limit)
RADIAL_WINDOW_RADIUS = 64


def radial_window_kept_fraction(metric: torch.Tensor, quantile_table: torch.Tensor) -> torch.Tensor:
    """``[B]`` (fp64): the share ``k* / K`` of a radial sun's energy that ``flux.radial_blur_flux`` deposits for each ``metric
    [B,3]`` = ``(M_rr, M_rc, M_cc)`` in pixels^2/rad^2 and the sun's ``quantile_table [K+1]`` in rad^2.  Node
    ``k`` of the table is the ellipse of half extents ``sqrt(t2[k] M_rr)`` rows and ``sqrt(t2[k] M_cc)`` columns; ``k*`` is the
    largest node whose two half extents are both at most 64 pixels, and the annuli beyond it are dropped.  NaN where the kernel
    writes NaN: a metric that is not finite, has ``M_rr <= 0`` or ``M_cc <= 0`` or ``det <= 1e-6 M_rr M_cc``, ``k* = 0`` (not even
    the first annulus fits), and everywhere for a table that is not finite, starts below 0 or decreases.  The rule of the
    kernel in torch ops: fp64 from the arguments' fp32 values (so ``t2[k] M`` is exact), on the metric's device, no host read."""
    if metric.dim() != 2 or metric.shape[1] != 3 or quantile_table.dim() != 1 or quantile_table.shape[0] < 2:
        raise ValueError(f"the metric must be [B,3] and the quantile table [K+1] with K >= 1, got {tuple(metric.shape)} and "
                         f"{tuple(quantile_table.shape)}")
    with torch.no_grad():
        f64 = torch.float64
        M = metric.to(f64)
        t2 = quantile_table.to(device=M.device, dtype=f64)
        K = t2.shape[0] - 1
        m_rr, m_rc, m_cc = M[:, 0], M[:, 1], M[:, 2]
        det = m_rr * m_cc - m_rc * m_rc
        metric_ok = torch.isfinite(M).all(dim=1) & (m_rr > 0) & (m_cc > 0) & (det > 1e-6 * (m_rr * m_cc))
        table_ok = torch.isfinite(t2).all() & (t2[0] >= 0) & (t2[1:] >= t2[:-1]).all()
        limit = float(RADIAL_WINDOW_RADIUS * RADIAL_WINDOW_RADIUS)
        fits = (t2.unsqueeze(0) * m_rr.unsqueeze(1) <= limit) & (t2.unsqueeze(0) * m_cc.unsqueeze(1) <= limit)
        k_star = fits.sum(dim=1) - 1                    # (the table does not decrease: the nodes that fit are a prefix)
        kept = k_star.to(f64) / K
        return torch.where(metric_ok & table_ok & (k_star >= 1), kept, torch.full_like(kept, float("nan")))
