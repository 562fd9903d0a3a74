"""Blocking primitives - the host-side half of ``artist/raytracing/blocking.py``.

A heliostat blocks as the rectangle spanned by four of its aligned surface points.  Building those
rectangles is a gather of ``4 N`` points plus one cross product per heliostat: it stays in torch so that
the corner points remain in the autograd graph (the reference differentiates through them as well), and
the per-ray work - which primitives matter, the soft blocking mask, its adjoint - runs inside the HIP
trace kernels (``artist_amd/csrc/trace_kernels.hip``), which receive the tables built here.

The reference narrows the primitives with an LBVH (``lbvh_filter_blocking_planes``, blocking.py:832-995)
because its mask is a dense ``[rays x primitives]`` tensor; a leaf of that tree is reached exactly when the
ray passes the leaf's own box test, so the set it returns is the set of primitives whose box is hit by at
least one foreign ray.  The HIP path computes that same set directly (per-heliostat beam cull + per-ray box
test, ``art_blocking_filter``), no tree needed.

Shading - the sun ray to a mirror point stopped by a neighbour - is blocking by per-heliostat sheared copies of the
rectangles (``create_shading_primitives``): which neighbours can shade whom and the sheared tables with
their adjoint are HIP kernels (``artist_amd/csrc/shading_kernels.hip``), the per-ray work is the trace kernels' as it is.
"""
from __future__ import annotations

import math

import torch

from . import _lib, ops
from ._memo import Memo


def _spans_and_normals(corners: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """spans = (corner1 - corner0, corner3 - corner0); normal = normalize(span_u x span_v)  (blocking.py:190-207)."""
    spans = torch.stack((corners[:, 1] - corners[:, 0], corners[:, 3] - corners[:, 0]), dim=1)
    cross = torch.linalg.cross(spans[:, 0, :3], spans[:, 1, :3], dim=-1)
    normals = torch.cat((torch.nn.functional.normalize(cross, dim=-1), torch.zeros_like(cross[:, :1])), dim=-1)
    return spans, normals


# (one entry per number of surface points and device: no field here has sixteen)
_CORNER_INDEX = Memo("the corner indices of the blocking rectangles", capacity=16)


def create_blocking_primitives_rectangles_by_index(blocking_heliostats_active_surface_points: torch.Tensor,
                                                   device: torch.device | None = None
                                                   ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rectangles from the known indices of the corner points (blocking.py:123-209).

    Four facets in two rows and two columns, each with ``sqrt(P/4)`` x ``sqrt(P/4)`` row-major points.
    Corner order ``1 | 2 / 0 | 3`` (0 = lower left).  Returns ``corners [N,4,4]``, ``spans [N,2,4]``,
    ``normals [N,4]``.
    """
    pts = blocking_heliostats_active_surface_points
    P = pts.shape[1]
    side = math.sqrt(P / 4)
    # (a host list -> device tensor copy waits for the stream: once per shape, not once per trace call)
    index = _CORNER_INDEX.lookup((), lambda: torch.tensor([int(P / 2), int(side - 1), int((P / 2) - 1), int(P - side)],
                                                          device=pts.device), key=(P, pts.device))
    corners = pts.index_select(1, index)
    spans, normals = _spans_and_normals(corners)
    return corners, spans, normals


def create_blocking_primitives_rectangle(blocking_heliostats_surface_points: torch.Tensor,
                                         blocking_heliostats_active_surface_points: torch.Tensor,
                                         device: torch.device | None = None
                                         ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Rectangles from the surface points closest to the east/north bounding box of the UNALIGNED surface
    (blocking.py:13-120); positions are then read from the aligned surface."""
    unaligned, aligned = blocking_heliostats_surface_points, blocking_heliostats_active_surface_points
    e, n = unaligned[:, :, 0], unaligned[:, :, 1]
    lo_e, hi_e, lo_n, hi_n = e.amin(1), e.amax(1), n.amin(1), n.amax(1)
    wanted = torch.stack((torch.stack((lo_e, lo_n), 1), torch.stack((lo_e, hi_n), 1), torch.stack((hi_e, hi_n), 1),
                          torch.stack((hi_e, lo_n), 1)), dim=1)                                  # [N,4,2]
    distance = torch.linalg.vector_norm(unaligned[:, :, None, :2] - wanted[:, None], dim=-1)     # [N,P,4]
    index = distance.argmin(dim=1)                                                               # [N,4]
    corners = torch.gather(aligned, 1, index[:, :, None].expand(-1, -1, 4))
    spans, normals = _spans_and_normals(corners)
    return corners, spans, normals


class ShadingTables(torch.autograd.Function):
    """The sheared tables ``(corners [H*S,4,4], spans [H*S,2,4], normals [H*S,4])`` of the rectangles listed in ``shader_idx``
    ``[H,S]`` (``art_shading_prims_fwd`` / ``_bwd``, include/artist_hip_shading.h), differentiable w.r.t.
    ``prim_corners`` through the shader's corners and through the shaded heliostat's own plane; ``incident`` is a constant."""

    @staticmethod
    def forward(ctx, prim_corners, owner, incident, shader_idx):
        dev = ops._require_cuda(prim_corners, owner, incident, shader_idx)
        corners, incident = ops._f32c(prim_corners), ops._f32c(incident)
        H, S = int(shader_idx.shape[0]), int(shader_idx.shape[1])
        N = int(corners.shape[0])
        if corners.shape != (N, 4, 4) or incident.shape != (H, 4) or owner.shape != (H,):
            raise ValueError("prim_corners must be [N,4,4], incident [H,4], owner [H] and shader_idx [H,S]")
        if owner.dtype != torch.int32 or shader_idx.dtype != torch.int32 or not (owner.is_contiguous() and shader_idx.is_contiguous()):
            raise ValueError("owner and shader_idx must be contiguous int32 tensors")
        out_c = torch.empty((H * S, 4, 4), dtype=torch.float32, device=dev)
        out_s = torch.empty((H * S, 2, 4), dtype=torch.float32, device=dev)
        out_n = torch.empty((H * S, 4), dtype=torch.float32, device=dev)
        _lib.call("art_shading_prims_fwd", dev, corners.data_ptr(), owner.data_ptr(), incident.data_ptr(), shader_idx.data_ptr(),
                  H, N, S, out_c.data_ptr(), out_s.data_ptr(), out_n.data_ptr())
        ctx.save_for_backward(corners, owner, incident, shader_idx)
        ctx.set_materialize_grads(False)
        return out_c, out_s, out_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_c, g_s, g_n):
        corners, owner, incident, shader_idx = ctx.saved_tensors
        if (g_c is None and g_s is None and g_n is None) or not ctx.needs_input_grad[0]:
            return None, None, None, None
        dev = corners.device
        H, S = int(shader_idx.shape[0]), int(shader_idx.shape[1])
        N = int(corners.shape[0])
        g_c = torch.zeros((H * S, 4, 4), dtype=torch.float32, device=dev) if g_c is None else ops._f32c(g_c)
        g_s = torch.zeros((H * S, 2, 4), dtype=torch.float32, device=dev) if g_s is None else ops._f32c(g_s)
        g_n = torch.zeros((H * S, 4), dtype=torch.float32, device=dev) if g_n is None else ops._f32c(g_n)
        scratch = torch.empty((H * S * 24,), dtype=torch.float32, device=dev)
        grad = torch.empty_like(corners)
        _lib.call("art_shading_prims_bwd", dev, corners.data_ptr(), owner.data_ptr(), incident.data_ptr(), shader_idx.data_ptr(),
                  g_c.data_ptr(), g_s.data_ptr(), g_n.data_ptr(), H, N, S, scratch.data_ptr(), grad.data_ptr())
        return grad, None, None, None


def shading_cull(prim_corners: torch.Tensor, owner: torch.Tensor, incident: torch.Tensor, max_scatter_angle: float,
                 slots: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(shader_idx [H,S] int32, shade_count [H] int32)``: per traced heliostat the rectangles that can shade it, ascending,
    ``-1`` in the empty slots, and the number found, which may exceed ``S`` (``art_shading_cull``: the rule is stated in
    artist_amd/csrc/shading_kernels.hip).  No gradient, nothing read back.  ``slots`` = None: ``ops.SHADING_SLOTS``."""
    dev = ops._require_cuda(prim_corners, owner, incident)
    S = int(ops.SHADING_SLOTS if slots is None else slots)
    corners, incident = ops._f32c(prim_corners.detach()), ops._f32c(incident.detach())
    H, N = int(incident.shape[0]), int(corners.shape[0])
    if corners.shape != (N, 4, 4) or incident.shape != (H, 4) or owner.shape != (H,):
        raise ValueError("prim_corners must be [N,4,4], incident [H,4] and owner [H]")
    if not max_scatter_angle >= 0.0:
        raise ValueError("max_scatter_angle must be the largest |distortion angle| of the trace (>= 0)")
    owner = ops._int32c(owner)
    shader_idx = torch.empty((H, S), dtype=torch.int32, device=dev)
    shade_count = torch.empty((H,), dtype=torch.int32, device=dev)
    _lib.call("art_shading_cull", dev, corners.data_ptr(), owner.data_ptr(), incident.data_ptr(), H, N, float(max_scatter_angle), S,
              shader_idx.data_ptr(), shade_count.data_ptr())
    return shader_idx, shade_count


def create_shading_primitives(prim_corners: torch.Tensor, owner: torch.Tensor, incident: torch.Tensor, max_scatter_angle: float,
                              slots: int | None = None) -> dict:
    """The shading tables of a trace: for each traced heliostat ``h`` (own rectangle ``owner[h]``, sun rays along
    ``incident[h]``) the rectangles that can shade it, sheared by ``A_h`` so that blocking of the REFLECTED ray by the sheared
    copy is shading of the sunward ray by the rectangle.  Returns ``corners [H*S,4,4]``, ``spans [H*S,2,4]``,
    ``normals [H*S,4]`` (in the autograd graph of ``prim_corners``), ``shader_idx [H,S]`` and ``shade_count [H]``; row
    ``h*S + k`` belongs to heliostat ``h`` alone."""
    shader_idx, shade_count = shading_cull(prim_corners, owner, incident, max_scatter_angle, slots)
    corners, spans, normals = ShadingTables.apply(prim_corners, ops._int32c(owner), incident.detach(), shader_idx)
    return dict(corners=corners, spans=spans, normals=normals, shader_idx=shader_idx, shade_count=shade_count)
