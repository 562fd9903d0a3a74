"""``torch.autograd.Function`` wrappers around the C ABI of ``libartist_hip.so``.

PyTorch is plumbing here (device memory, streams, autograd tape); every number is produced by
the hand-written gfx950 kernels in ``artist_amd/csrc``.  No CPU path exists: non-CUDA inputs
raise.
"""
from __future__ import annotations

import math

import torch

from . import _lib, _memo

__all__ = ["trace_rays", "nurbs_surface_points_and_normals", "per_target_sum", "align_surfaces", "TraceRays",
           "NurbsEval", "AlignSurfaces", "check_async_errors", "record_launch_events",
           "sample_distortions", "CantFacets", "perform_canting", "nurbs_eval"]


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


# Measurement hook (bench.py's roofline leg, tools/): when switched on, the calls made through _timed_call (the trace calls, the
# sampler, the regularisers, the surface fit) are bracketed by a pair of HIP events on the stream they are launched on, so a
# caller can read the launch durations of a region it times WITHOUT changing that region (no synchronisation; two event records
# per call).  Off by default: None.
_LAUNCH_EVENTS = None


def record_launch_events(on: bool = True):
    """Start (``True``: returns the dict that fills up, ``{"art_trace_fwd": [(start, end), ...], "art_trace_bwd": [...]}``
    of ``torch.cuda.Event`` pairs) or stop (``False``: returns the dict collected so far) recording.  Read the pairs with
    ``start.elapsed_time(end)`` after a synchronisation."""
    global _LAUNCH_EVENTS
    if on:
        _LAUNCH_EVENTS = {}
        return _LAUNCH_EVENTS
    out, _LAUNCH_EVENTS = _LAUNCH_EVENTS, None
    return out


def _timed_call(name: str, device: torch.device, *args, on_error=_lib.check) -> None:
    """``_lib.call`` for the entry points that ``record_launch_events`` times."""
    rec = _LAUNCH_EVENTS
    if rec is None:
        return _lib.call(name, device, *args, on_error=on_error)
    stream = torch.cuda.current_stream(device)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.device(device):
        start.record(stream)
        try:
            _lib.call(name, device, *args, on_error=on_error)
        finally:                                   # (a call that reports an error is recorded like any other)
            end.record(stream)
            rec.setdefault(name, []).append((start, end))


def _require_cuda(*tensors: torch.Tensor) -> torch.device:
    dev = tensors[0].device
    if dev.type != "cuda":
        raise _lib.ArtistHipError(
            f"artist_amd ops run on the GPU only (got a tensor on {dev}); there is no CPU fallback")
    for t in tensors:
        if t is not None and t.device != dev:
            raise ValueError(f"all tensors must be on {dev}, found one on {t.device}")
    return dev


def _f32c(t: torch.Tensor) -> torch.Tensor:
    """float32 + contiguous (no copy when already so)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _f32c16(t: torch.Tensor) -> torch.Tensor:
    """``_f32c`` whose first element is 16-byte aligned as well: the align and reflect kernels move [4] rows as float4 and their
    entry points refuse a pointer that is not (a contiguous view at a storage offset of one float); such a view is copied."""
    t = _f32c(t)
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


# Small per-call conversions that an optimisation loop repeats with the SAME tensors every epoch - the int32 copy of the
# target indices, the [H,F,K] materialisation of an expanded knot vector - are kept (sixteen entries of a few KB).  Each is a
# 5 us kernel that a 1 ms epoch of a rank's share of a field would pay several times over.
_CONVERTED = _memo.Memo("a converted copy of an index or knot tensor", capacity=16, under_capture="serve", pin=True)


def _converted(t: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """``t`` as a contiguous ``dtype`` tensor: ``t`` itself when it is one already (nothing to keep when no copy is made)."""
    if t.dtype == dtype and t.is_contiguous():
        return t
    make = lambda: t.to(dtype).contiguous()         # noqa: E731
    return _CONVERTED.lookup(t, make, key=dtype) if t.numel() <= (1 << 20) else make()


def _int32c(t: torch.Tensor) -> torch.Tensor:
    return _converted(t, torch.int32)


def _dist_views(dist_u: torch.Tensor, dist_e: torch.Tensor, shape):
    """Validate the two [H,R,P] distortion views and return (u, e, element strides).

    ``Sun.get_distortions`` (artist/scene/sun.py:227-234) returns stride-(2RP,2P,2) views of one
    interleaved buffer; they are passed through as-is (the kernel does one 8-byte load per ray)."""
    if dist_u.shape != dist_e.shape:
        # same condition / message as transforms.rotate_distortions (artist/geometry/transforms.py:47-50)
        raise ValueError("The two tensors containing angles for the east and up rotation must have the same shape.")
    if tuple(dist_u.shape) != tuple(shape):
        raise ValueError(f"distortions must have shape {tuple(shape)}, got {tuple(dist_u.shape)}")
    if dist_u.dtype != torch.float32 or dist_e.dtype != torch.float32:
        dist_u, dist_e = dist_u.float(), dist_e.float()
    if dist_u.stride() != dist_e.stride():
        dist_u, dist_e = dist_u.contiguous(), dist_e.contiguous()
    return dist_u, dist_e, dist_u.stride()


def _cyl_tables(cyl, dev):
    """(centers[Tc,4], normals[Tc,4], axes[Tc,4], radii[Tc], heights[Tc], opening[Tc]) -> fp32 contiguous
    tensors on ``dev`` + their data pointers (NULL x 6 when there are no cylindrical target areas)."""
    if cyl is None or cyl[0].shape[0] == 0:
        return (), (None,) * 6, 0
    if len(cyl) != 6:
        raise ValueError("cylindrical target areas: (centers, normals, axes, radii, heights, opening_angles)")
    tabs = tuple(_f32c(t.to(dev)) for t in cyl)
    Tc = tabs[0].shape[0]
    for t, shape in zip(tabs, ((Tc, 4), (Tc, 4), (Tc, 4), (Tc,), (Tc,), (Tc,))):
        if tuple(t.shape) != shape:
            raise ValueError(f"cylindrical target table has shape {tuple(t.shape)}, expected {shape}")
    return tabs, tuple(t.data_ptr() for t in tabs), Tc


def _planar_ptrs(centers, plane_normals, dims):
    if centers.shape[0] == 0:
        return (None, None, None)
    return (centers.data_ptr(), plane_normals.data_ptr(), dims.data_ptr())


#: Row width of a heliostat's list of candidate blocking rectangles (``Cmax`` of art_blocking_filter) - workspace, not a limit of
#: the kernels: they keep the first 32 rectangles of a list in LDS and read any others from the list itself (slower, never
#: refused).  A list that does not fit its ROW is reported (ART_ECANDIDATES: workspace exhausted - raise this number; ``None`` =
#: the number of rectangles, which no list can exceed; 4 B per heliostat and entry, 96 B more in the backward scratch).
BLOCKING_CANDIDATES = 256
#: Slots per heliostat for the rectangles that can shade it (``S`` of art_shading_cull): the candidate row of a trace with shading is
#: this much wider.  A heliostat with more shaders than slots is reported like a row that is too narrow: NaN bitmap and factors.
SHADING_SLOTS = 8
_LAST_BLOCKING = None

# Pixel accumulators of art_trace_fwd ([n_maps,Hh,W] uint64, zero on entry and zero again afterwards): one buffer per
# (device, stream), grown on demand, so that calls on different streams never share one.
_ACCUM: dict = {}


def _accumulators(dev: torch.device, n: int) -> torch.Tensor:
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), _stream(dev))
    buf = _ACCUM.get(key)
    if buf is None or buf.numel() < n:
        if _lib.capturing():     # a captured torch.zeros is a memset node: not zero until a replay, and zero is the kernels' invariant
            raise _lib.first_use_under_capture("pixel accumulators of art_trace_fwd")
        buf = torch.zeros((n,), dtype=torch.int64, device=dev)
        _ACCUM[key] = buf
    _lib.keep_alive(buf)                            # (_raise_status drops the table; a captured step keeps its buffer)
    return buf


def reflect_directions(incident: torch.Tensor, normals: torch.Tensor) -> torch.Tensor:
    """``incident[h] - 2 (incident[h] . normals[h,p]) normals[h,p]`` for ``incident [H,4]``, ``normals [H,P,4]``
    (``art_reflect``; artist/raytracing/geometry.py:11-41).  Not differentiable."""
    dev = _require_cuda(incident, normals)
    incident, normals = _f32c16(incident.detach()), _f32c16(normals.detach())
    H, P = int(normals.shape[0]), int(normals.shape[1])
    if incident.shape != (H, 4) or normals.shape != (H, P, 4):
        raise ValueError("incident must be [H,4] and normals [H,P,4]")
    out = torch.empty_like(normals)
    _lib.call("art_reflect", dev, incident.data_ptr(), normals.data_ptr(), H, P, out.data_ptr())
    return out


def _sampler_call(rows, number_of_rays: int, number_of_points: int, seed: int, device):
    """What both samplers do before their launch: ``(device, seed as int64, rows on the device, n, R, P, out)``."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.ArtistHipError(
            f"artist_amd ops run on the GPU only (sampler asked for {dev}); there is no CPU fallback")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    R, P = int(number_of_rays), int(number_of_points)
    if R < 0 or P < 0:
        raise ValueError(f"number_of_rays and number_of_points must be >= 0, got {R}, {P}")
    if isinstance(rows, torch.Tensor):
        if rows.dtype.is_floating_point or rows.dim() != 1:
            raise ValueError("rows must be a 1-D integer tensor or a list of ints")
        rows_t = rows.to(dev, torch.int64).contiguous() if rows.device == dev else \
            rows.to(torch.int64).contiguous().pin_memory().to(dev, non_blocking=True)
    else:
        rows_t = torch.tensor([int(r) for r in rows], dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
    n = int(rows_t.shape[0])
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF                      # the seed as a 64-bit two's-complement value
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed
    out = torch.empty((n, R, P, 2), dtype=torch.float32, device=dev)
    return dev, int(seed), rows_t, n, R, P, out


def sample_distortions(rows, number_of_rays: int, number_of_points: int, seed: int, loc, scale_tril, device) -> torch.Tensor:
    """Rows ``rows`` of the Gaussian sun-shape sample, ``[len(rows), R, P, 2]`` fp32 with ``(u, e)`` interleaved, drawn in one
    launch on the current stream of ``device`` (``art_sample_distortions``, include/artist_hip_sampler.h).  Row ``rows[k]``
    comes from a Philox stream keyed by ``(seed, rows[k])``: the same bits whatever the other rows of the call.

    ``loc`` (2 values) and ``scale_tril`` (2x2, lower triangular) are HOST values: the call reads nothing back from the device.
    ``rows`` is a list of ints or an integer tensor (a list travels through pinned memory, without a synchronisation)."""
    dev, seed, rows_t, n, R, P, out = _sampler_call(rows, number_of_rays, number_of_points, seed, device)
    (lu, le), ((l00, _), (l10, l11)) = [float(v) for v in loc], [[float(v) for v in r] for r in scale_tril]
    _timed_call("art_sample_distortions", dev, seed, rows_t.data_ptr(), n, R, P, lu, le, l00, l10, l11, out.data_ptr())
    return out


def sample_radial_distortions(rows, number_of_rays: int, number_of_points: int, seed: int, loc, table, device) -> torch.Tensor:
    """``sample_distortions`` for a radially symmetric sun shape (``art_sample_radial_distortions``,
    include/artist_hip_sampler.h): same rows, layout and
    streams, the radius of a ray drawn from ``table``, the fp32 ``[K+1]`` quantile table of squared radii that
    ``artist_amd.scene.radial_quantile_table`` builds, ``1 <= K <= 4096``.

    ``loc`` (2 values) is a HOST value; ``table`` is a tensor on ``device`` and stays there: nothing is read back."""
    dev, seed, rows_t, n, R, P, out = _sampler_call(rows, number_of_rays, number_of_points, seed, device)
    if not isinstance(table, torch.Tensor) or table.dim() != 1 or table.dtype != torch.float32 or table.device != dev \
            or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous 1-D float32 tensor on {dev}")
    K = int(table.shape[0]) - 1
    if not 1 <= K <= 4096:
        raise ValueError(f"table must hold K+1 nodes with 1 <= K <= 4096, got {K + 1} values")
    lu, le = (float(v) for v in loc)
    _timed_call("art_sample_radial_distortions", dev, seed, rows_t.data_ptr(), n, R, P, lu, le, table.data_ptr(), K,
                out.data_ptr())
    return out


def check_async_errors(device=None, clear: bool = True) -> None:
    """Synchronise ``device`` and raise if a kernel met a target index outside the target tables or the blocking filter
    found more candidate rectangles for a heliostat than the kernels hold (``art_async_status``): the entry points are
    asynchronous, so the device-side checks report here - or at the next trace call, which refuses to start while the
    status is set.  The status is ONE sticky word per GPU, shared by every stream and tracer of the process: whoever
    calls this clears it for all of them (``clear=False`` only looks).  A heliostat that was skipped or traced with an
    incomplete rectangle list is also marked in the results themselves: zero bitmap and factors for a bad target index,
    NaN bitmap and factors for a candidate overflow."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if _lib.capturing():
        raise _lib.ArtistHipError("check_async_errors waits for the device, which a stream under graph capture cannot do: "
                                  "call it before the capture or after a replay")
    with torch.cuda.device(dev):
        # the status word is one per GPU (include/artist_hip.h): a kernel on ANY stream of this process may have set it,
        # so wait for the whole device, not only for the current stream
        torch.cuda.synchronize(dev)
        rc = _lib.lib().art_async_status(_stream(dev), 1 if clear else 0)
    if rc != _lib.ART_OK:
        _raise_status(rc, "art_async_status")


def _raise_status(code: int, what: str) -> None:
    """The exception for a non-zero ``code`` of ``what`` = art_trace_fwd, art_trace_bwd or art_async_status: the sticky status
    of the device (include/artist_hip.h), which the trace calls return at once for as long as it is set, or the call's own
    error."""
    # The pixel accumulators must be all zero when a trace starts.  A skipped heliostat leaves nothing behind, but take no
    # chances with the invariant; a launch that ended abnormally (ART_EQUEUE) may have left some.  A forward call that
    # refused or failed drops them whatever the code; the backward call does not use them.
    if what == "art_trace_fwd" or (what == "art_async_status" and code in (_lib.ART_ETARGET, _lib.ART_EQUEUE)):
        _ACCUM.clear()
    if code == _lib.ART_ETARGET:
        raise IndexError(f"target_area_indices out of range (found by the kernels, reported by {what}; "
                         "artist_amd.ops.check_async_errors() clears the status)")
    if code == _lib.ART_ECANDIDATES:
        raise _lib.ArtistHipError(
            f"a heliostat has more blocking rectangles inside its ray cone than its candidate row holds "
            f"(artist_amd.ops.BLOCKING_CANDIDATES = {BLOCKING_CANDIDATES}: raise it, or set it to None for no bound; found by "
            f"art_blocking_filter, reported by {what}): its blocking is incomplete, and its bitmaps and factors are NaN; "
            "artist_amd.ops.check_async_errors() clears the status")
    _lib.check(code, what)


# Centre-of-mass sums that came with a traced bitmap tensor.  An entry serves exactly the tensor OBJECT the trace returned, at
# the version it returned it with (an in-place edit, a copy or a slice of the bitmaps is another tensor or another version: the
# crop then forms the sums itself - the same bits).  64: more traced bitmap tensors than any caller here keeps alive at once.
_MOMENTS = _memo.Memo("the centre-of-mass sums of traced bitmaps", capacity=64)


def bitmap_moments(flux: torch.Tensor):
    """The sums ``art_trace_fwd`` left for ``flux`` (``[n_maps,4,3]`` float64) if ``flux`` is an untouched output of
    :func:`trace_rays` / ``HeliostatRayTracer.trace_rays``, else None.

    "Untouched" is judged by the tensor's version counter, so a write that bypasses it - through ``.data``, by a raw kernel,
    by ``torch.distributed`` called directly - is invisible and leaves stale sums behind.  The package's own in-place
    helpers (``distributed.all_reduce_sum``, ``all_reduce_sum_async``, ``reduce_flux_per_target``) forget the sums of the
    tensor they write; a caller that writes in such a way hands the crop a view (``flux[:]``: another object, no sums)."""
    return _MOMENTS.get(flux)


class TraceRays(torch.autograd.Function):
    """reflect -> scatter -> plane / cylinder intersection -> (blocking mask) -> bilinear splat (+ factors), fused.

    Replaces the body of ``HeliostatRayTracer.trace_rays``
    (artist/raytracing/heliostat_ray_tracer.py:285-506).  Target index ``t < T`` is planar area ``t``; ``t >= T``
    is cylindrical area ``t - T`` of the ``cyl`` tables.  With ``prim_corners/spans/normals`` (the rectangles of
    ``create_blocking_primitives_rectangles_by_index``) blocking is on: ``art_blocking_filter`` picks the
    rectangles (``lbvh_filter_blocking_planes``) and the kernels evaluate ``soft_ray_blocking_mask`` per ray.
    Differentiable w.r.t. ``origins``, ``normals`` and the three rectangle tables exactly like the eager chain
    (indices, masks and the filter are constants).  Returns ``(flux, factors, filter_flags)``.

    With ``shade_corners/spans/normals [H*S,...]``, ``shader_idx [H,S]`` and ``shade_count [H]`` (the tables of
    ``artist_amd.blocking.create_shading_primitives``) shading is on as well: the filter sees the ``N`` real rectangles only,
    ``art_shading_append`` enters the virtual rows ``N + h*S + k`` into the candidate row of heliostat ``h`` alone (the row is
    ``S`` entries wider), and the kernels trace against the concatenated tables of ``N + H*S`` rows; the three shading tables
    receive gradients like the real ones.  ``filter_active=False`` (shading without blocking): the filter is skipped and the
    rows hold the virtual rectangles only.  A call without these arguments runs exactly what it ran before they existed.
    """

    @staticmethod
    def forward(ctx, origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                ray_magnitude, extinction, reflectivity, width, height, per_target, cyl=None,
                prim_corners=None, prim_spans=None, prim_normals=None, owner=None, max_scatter_angle=-1.0,
                lbvh_compat=True, points_per_facet=0, shade_corners=None, shade_spans=None, shade_normals=None,
                shader_idx=None, shade_count=None, filter_active=True):
        dev = _require_cuda(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims)
        origins, normals, incident = _f32c(origins), _f32c(normals), _f32c(incident)
        H, P = origins.shape[0], origins.shape[1]
        if origins.shape != (H, P, 4) or normals.shape != (H, P, 4) or incident.shape != (H, 4):
            raise ValueError("origins/normals must be [H,P,4] and incident [H,4]")
        # a performance hint, never a semantic one: the kernels cut a heliostat's points into blocks that share an LDS
        # window, and blocks that do not straddle two facets (two separate images) fit their windows better
        points_per_facet = int(points_per_facet or 0)
        if points_per_facet < 0 or (points_per_facet and P % points_per_facet):
            raise ValueError("points_per_facet must divide the number of surface points per heliostat")
        R = dist_u.shape[1] if dist_u.dim() == 3 else -1
        dist_u, dist_e, (sh, sr, sp) = _dist_views(dist_u, dist_e, (H, R, P))
        target_idx = _int32c(target_idx)
        centers, plane_normals, dims = _f32c(centers), _f32c(plane_normals), _f32c(dims)
        T = centers.shape[0]
        cyl_tabs, cyl_ptrs, Tc = _cyl_tables(cyl, dev)
        n_maps = T + Tc if per_target else H
        geometry = (origins.data_ptr(), normals.data_ptr(), incident.data_ptr(), dist_u.data_ptr(), dist_e.data_ptr(),
                    sh, sr, sp, target_idx.data_ptr(), *_planar_ptrs(centers, plane_normals, dims), *cyl_ptrs)

        blocking = prim_corners is not None
        shading = shade_corners is not None
        if blocking and _lib.capturing():
            raise _lib.ArtistHipError("blocking / shading under graph capture is not supported (the library refuses it with "
                                      "ART_EUNSUPPORTED): trace with blocking eagerly, or capture the step with blocking_active=False")
        if (shading or not filter_active) and not blocking:
            raise ValueError("shading needs the blocking rectangles (prim_corners, prim_spans, prim_normals, owner)")
        if not shading and not filter_active:
            raise ValueError("filter_active=False is for shading without blocking: the shading tables are missing")
        block_tabs, block_ptrs, Cmax, N, S = (), (None,) * 5, 0, 0, 0
        flags = torch.empty((0,), dtype=torch.int32, device=dev)
        if blocking and H > 0:
            _require_cuda(prim_corners, prim_spans, prim_normals, owner)
            if max_scatter_angle < 0:    # the kernels cull per surface point with this bound: measure it once
                max_scatter_angle = float(torch.maximum(dist_u.abs().max(), dist_e.abs().max()))
            prim_corners, prim_spans, prim_normals = _f32c(prim_corners), _f32c(prim_spans), _f32c(prim_normals)
            N = prim_corners.shape[0]
            if prim_corners.shape != (N, 4, 4) or prim_spans.shape != (N, 2, 4) or prim_normals.shape != (N, 4):
                raise ValueError("blocking primitives must be corners [N,4,4], spans [N,2,4], normals [N,4]")
            owner = owner.to(torch.int32).contiguous()
            if owner.shape != (H,):
                raise ValueError("owner must hold one primitive index per traced heliostat")
            Cmax = N if BLOCKING_CANDIDATES is None else max(1, min(N, int(BLOCKING_CANDIDATES)))
            if shading:
                _require_cuda(shade_corners, shade_spans, shade_normals, shader_idx, shade_count)
                S = int(shader_idx.shape[1]) if shader_idx.dim() == 2 else 0
                if S < 1 or shader_idx.shape != (H, S) or shade_count.shape != (H,) or shader_idx.dtype != torch.int32 or \
                        shade_count.dtype != torch.int32 or not (shader_idx.is_contiguous() and shade_count.is_contiguous()):
                    raise ValueError("shader_idx must be [H,S] and shade_count [H], contiguous int32 (artist_amd.blocking.shading_cull)")
                if shade_corners.shape != (H * S, 4, 4) or shade_spans.shape != (H * S, 2, 4) or shade_normals.shape != (H * S, 4):
                    raise ValueError("shading tables must be corners [H*S,4,4], spans [H*S,2,4], normals [H*S,4]")
                # the blocking width plus the slots.  The filter's one `Cmax` is both its limit and the row stride, so it may
                # list up to S more real rectangles than without shading; a list that fits the blocking width - every list
                # that traces without shading - always leaves the S entries the append needs, so shading never turns a row
                # that traced into an overflow
                Cmax = Cmax + S if filter_active else S
            cand = torch.empty((H, Cmax), dtype=torch.int32, device=dev)
            if filter_active:
                flags = torch.empty((N,), dtype=torch.int32, device=dev)
                cand_count = torch.empty((H,), dtype=torch.int32, device=dev)
                workspace = torch.empty((int(_lib.lib().art_blocking_workspace_bytes(H, N)),), dtype=torch.uint8, device=dev)
                _lib.call("art_blocking_filter", dev, *geometry, float(ray_magnitude), H, R, P, T, Tc, width, height,
                          prim_corners.data_ptr(), owner.data_ptr(), N, float(max_scatter_angle), 1 if lbvh_compat else 0, Cmax,
                          flags.data_ptr(), cand.data_ptr(), cand_count.data_ptr(), workspace.data_ptr())
                # (more than Cmax rectangles inside a heliostat's ray cone: the device reports it - ART_ECANDIDATES from
                #  check_async_errors() or from the next trace call - instead of a host read of the counts in every call)
            else:
                flags = torch.zeros((N,), dtype=torch.int32, device=dev)
                cand_count = torch.zeros((H,), dtype=torch.int32, device=dev)
            if shading:
                # the virtual rectangles of heliostat h enter row h only, behind the real ones (they never pass the filter: a
                # sheared copy lies in real space and could sit in another heliostat's beam); a row without room for them, or a
                # heliostat with more shaders than slots, is marked overflowed and comes back NaN - nothing is read back here
                _lib.call("art_shading_append", dev, shader_idx.data_ptr(), shade_count.data_ptr(), H, N, S, Cmax,
                          cand.data_ptr(), cand_count.data_ptr())
                prim_corners = torch.cat((prim_corners, _f32c(shade_corners)))
                prim_spans = torch.cat((prim_spans, _f32c(shade_spans)))
                prim_normals = torch.cat((prim_normals, _f32c(shade_normals)))
            block_tabs = (prim_corners, prim_spans, prim_normals, cand, cand_count)
            global _LAST_BLOCKING
            _LAST_BLOCKING = (cand, cand_count)            # (diagnostics and tests: the last call's candidate lists, still on the device; never a captured call's)
            block_ptrs = tuple(t.data_ptr() for t in block_tabs)

        flux = torch.empty((n_maps, height, width), dtype=torch.float32, device=dev)
        factors = torch.empty((3, H), dtype=torch.float32, device=dev)
        accum = _accumulators(dev, n_maps * height * width)
        # the bitmaps' centre-of-mass sums, left behind by the pass that converts the accumulators (include/artist_hip.h): the
        # crop + loss op that follows in a reconstruction epoch starts from them (artist_amd.flux: bitmap_moments)
        moments = None
        if height >= 4 and (height * width) % 2 == 0 and 0 < n_maps <= 65535:
            moments = torch.empty((n_maps, 4, 3), dtype=torch.float64, device=dev)
        _timed_call("art_trace_fwd", dev, *geometry, *block_ptrs, Cmax, float(max_scatter_angle), float(ray_magnitude),
                    float(extinction), float(reflectivity), H, R, P, points_per_facet, T, Tc, width, height, 1 if per_target else 0,
                    flux.data_ptr(), factors.data_ptr(), accum.data_ptr(), None if moments is None else moments.data_ptr(),
                    on_error=_raise_status)
        ctx.save_for_backward(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                              *cyl_tabs, *block_tabs)
        ctx.n_cyl = len(cyl_tabs)
        ctx.scalars = (float(ray_magnitude), float(extinction), float(reflectivity), width, height, bool(per_target),
                       Cmax, N + H * S, float(max_scatter_angle), points_per_facet)
        ctx.n_real = N
        ctx.mark_non_differentiable(factors, flags)
        ctx.set_materialize_grads(False)            # no zero tensors (one fill kernel each) for outputs nobody differentiates
        if moments is not None:
            # (kept under graph capture too: the entry serves this tensor object alone, sums and bitmaps are written by the same
            #  captured launch, and the crop captured behind it must take the path it takes eagerly)
            _MOMENTS.put(flux, moments)
        return flux, factors, flags

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_flux, _grad_factors, _grad_flags):
        origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims = ctx.saved_tensors[:9]
        cyl_tabs = ctx.saved_tensors[9:9 + ctx.n_cyl]
        block_tabs = ctx.saved_tensors[9 + ctx.n_cyl:]
        cyl_ptrs = tuple(t.data_ptr() for t in cyl_tabs) if cyl_tabs else (None,) * 6
        block_ptrs = tuple(t.data_ptr() for t in block_tabs) if block_tabs else (None,) * 5
        Tc = cyl_tabs[0].shape[0] if cyl_tabs else 0
        mag, ext, refl, width, height, per_target, Cmax, N, max_scatter, points_per_facet = ctx.scalars
        dev = origins.device
        if grad_flux is None:                       # the bitmaps were not used downstream
            return (None,) * 29
        H, P = origins.shape[0], origins.shape[1]
        R = dist_u.shape[1]
        sh, sr, sp = dist_u.stride()
        grad_flux = _f32c(grad_flux)
        g_o = torch.empty_like(origins)
        g_n = torch.empty_like(normals)
        g_pc = g_ps = g_pn = None
        if block_tabs:
            g_pc, g_ps, g_pn = (torch.empty_like(t) for t in block_tabs[:3])
        n_scratch = int(_lib.lib().art_trace_bwd_scratch_floats(H, R, P, points_per_facet, Cmax if block_tabs else 0))
        scratch = torch.empty((n_scratch,), dtype=torch.float32, device=dev) if n_scratch else None
        _timed_call("art_trace_bwd", dev,
                    origins.data_ptr(), normals.data_ptr(), incident.data_ptr(), dist_u.data_ptr(), dist_e.data_ptr(),
                    sh, sr, sp, target_idx.data_ptr(), *_planar_ptrs(centers, plane_normals, dims), *cyl_ptrs,
                    *block_ptrs, Cmax, N, max_scatter, mag, ext, refl, H, R, P, points_per_facet, centers.shape[0], Tc, width, height,
                    1 if per_target else 0, grad_flux.data_ptr(), g_o.data_ptr(), g_n.data_ptr(),
                    *(t.data_ptr() if t is not None else None for t in (g_pc, g_ps, g_pn)),
                    None if scratch is None else scratch.data_ptr(), n_scratch, on_error=_raise_status)
        g_sc = g_ss = g_sn = None
        if block_tabs and N > ctx.n_real:            # rows N_real ... of the concatenated tables are the shading tables'
            n = ctx.n_real
            (g_pc, g_sc), (g_ps, g_ss), (g_pn, g_sn) = ((g[:n], g[n:]) for g in (g_pc, g_ps, g_pn))
        # (a call that passed today's 23 arguments is handed 23 values: autograd drops trailing Nones)
        return (g_o, g_n) + (None,) * 14 + (g_pc, g_ps, g_pn, None, None, None, None) + (g_sc, g_ss, g_sn, None, None, None)


_FACTOR_CHECKS = _memo.Memo("the host check of a per-heliostat intensity factor", capacity=8)


def split_intensity_factors(extinction, reflectivity, n_heliostats: int, device, checked: "_memo.Memo" = _FACTOR_CHECKS):
    """``(extinction for the kernel, reflectivity for the kernel, extinction [H] or None, reflectivity [H] or None)``.

    A Python number, a 0-d tensor or a one-element tensor is a float for the kernel (what every call did before tensors were
    accepted: same launches, same bits).  A tensor with more elements is one value per heliostat: the kernel then runs with
    extinction 0 / reflectivity 1 for that factor and :func:`scale_heliostat_rows` applies it to the results.  Such a tensor is
    ``[n_heliostats]``, floating point, on ``device``, finite, ``0 <= extinction <= 1``, ``reflectivity >= 0``: checked with one
    fused reduction and one host read per tensor object and version (``checked``, artist_amd/_memo.py), not per call."""
    out = []
    for name, value, neutral in (("ray_extinction_factor", extinction, 0.0), ("mirror_reflectivity", reflectivity, 1.0)):
        if not isinstance(value, torch.Tensor) or value.numel() <= 1:
            out.append((float(value), None))
            continue
        if value.dim() != 1 or value.shape[0] != int(n_heliostats):
            raise ValueError(f"{name} must be a float or one value per active heliostat, shape [{int(n_heliostats)}]; "
                             f"got shape {tuple(value.shape)}")
        if not value.dtype.is_floating_point:
            raise ValueError(f"{name} must be a floating-point tensor, got {value.dtype}")
        if value.device != torch.device(device):
            raise ValueError(f"{name} must be on the device that traces, {torch.device(device)}; it is on {value.device}")

        def check(name=name, value=value) -> bool:
            lo, hi = torch.stack(torch.aminmax(value.detach().float())).tolist()      # (NaN propagates through both)
            if not (math.isfinite(lo) and math.isfinite(hi)):
                raise ValueError(f"{name} must be finite, got values in [{lo}, {hi}]")
            if name == "ray_extinction_factor" and not (0.0 <= lo and hi <= 1.0):
                raise ValueError(f"ray_extinction_factor must lie in [0, 1], got values in [{lo}, {hi}]")
            if name == "mirror_reflectivity" and lo < 0.0:
                raise ValueError(f"mirror_reflectivity must be >= 0, got values in [{lo}, {hi}]")
            return True
        checked.lookup(value, check, key=name)
        out.append((neutral, value))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def scale_heliostat_rows(flux: torch.Tensor, factors: torch.Tensor, extinction, reflectivity):
    """Per-heliostat intensity factors on the results of a trace that ran without them: bitmap row ``h`` times
    ``w_h = (1 - extinction_h) * reflectivity_h`` in fp32 - ONE differentiable element-wise op on ``[H,Hh,W]`` (gradients reach
    the surfaces through ``TraceRays.backward`` and a factor tensor that requires them) - and the intercept factor, which
    counts rays with intensity > 0, set to 0 where ``w_h == 0``.  Either factor may be None (already in the kernel).

    The result is not an untouched trace output: it has no ``bitmap_moments`` (the fused crop forms its own sums - the same
    bits with or without them)."""
    w = None if extinction is None else 1.0 - extinction.float()
    if reflectivity is not None:
        w = reflectivity.float() if w is None else w * reflectivity.float()
    flux = flux * w.view(-1, 1, 1)
    intercept = factors[0].masked_fill(w.detach() == 0, 0.0)
    return flux, torch.cat((intercept.unsqueeze(0), factors[1:]))


def trace_rays(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
               ray_magnitude=1.0, extinction=0.0, reflectivity=0.935, resolution=(256, 256), per_target=False,
               cyl=None, blocking=None, points_per_facet=0, shading=None):
    """Functional form; see :func:`_trace_rays` for the arguments.  ``extinction`` and ``reflectivity`` are each a float or a
    tensor ``[H]``, one value per heliostat: a tensor is applied to the traced bitmaps
    (:func:`scale_heliostat_rows`), and with ``per_target`` the scaled ``[H,Hh,W]`` bitmaps are then summed per target
    (``art_per_target_sum``) - the fused per-target mode sums inside the kernel and cannot take them."""
    extinction, reflectivity, ext_rows, refl_rows = split_intensity_factors(extinction, reflectivity, origins.shape[0],
                                                                            origins.device)
    if ext_rows is None and refl_rows is None:
        return _trace_rays(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims, ray_magnitude,
                           extinction, reflectivity, resolution, per_target, cyl, blocking, points_per_facet, shading)
    flux, factors, *flags = _trace_rays(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                                        ray_magnitude, extinction, reflectivity, resolution, False, cyl, blocking,
                                        points_per_facet, shading)
    flux, factors = scale_heliostat_rows(flux, factors, ext_rows, refl_rows)
    if per_target:
        flux = per_target_sum(flux, target_idx, int(centers.shape[0]) + (0 if cyl is None else int(cyl[0].shape[0])))
    return (flux, factors, *flags)


def _trace_rays(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                ray_magnitude=1.0, extinction=0.0, reflectivity=0.935, resolution=(256, 256), per_target=False,
                cyl=None, blocking=None, points_per_facet=0, shading=None):
    """Returns ``(flux, factors)`` with ``flux`` ``[H,Hh,W]`` (or ``[T+Tc,Hh,W]`` when
    ``per_target``) and ``factors`` ``[3,H]`` = intercept, on-target, blocking fractions.  ``cyl`` = the six
    ``TowerTargetAreasCylindrical`` tensors (centers, normals, axes, radii, heights, opening_angles) or None.
    ``blocking`` = None or a dict with ``corners [N,4,4]``, ``spans [N,2,4]``, ``normals [N,4]``, ``owner [H]`` and
    optionally ``max_scatter_angle`` / ``lbvh_compat``; the filtered set is then returned as a third value.
    ``points_per_facet`` (optional, performance only): the surface points of a heliostat are F runs of that many points,
    one run per facet (ARTIST's ``[H, F * M, 4]`` layout) - results do not depend on it.
    ``shading`` = None or the dict of ``artist_amd.blocking.create_shading_primitives`` (needs ``blocking``; with
    ``blocking["filter"] = False`` the trace is shaded only)."""
    if shading is not None:
        if blocking is None:
            raise ValueError("shading needs the blocking rectangles")
        return TraceRays.apply(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                               ray_magnitude, extinction, reflectivity, int(resolution[0]), int(resolution[1]),
                               bool(per_target), cyl, blocking["corners"], blocking["spans"], blocking["normals"],
                               blocking["owner"], float(blocking.get("max_scatter_angle", -1.0)),
                               bool(blocking.get("lbvh_compat", True)), points_per_facet, shading["corners"], shading["spans"],
                               shading["normals"], shading["shader_idx"], shading["shade_count"], bool(blocking.get("filter", True)))
    if blocking is None:
        flux, factors, _ = TraceRays.apply(origins, normals, incident, dist_u, dist_e, target_idx, centers,
                                           plane_normals, dims, ray_magnitude, extinction, reflectivity,
                                           int(resolution[0]), int(resolution[1]), bool(per_target), cyl,
                                           None, None, None, None, -1.0, True, points_per_facet)
        return flux, factors
    return TraceRays.apply(origins, normals, incident, dist_u, dist_e, target_idx, centers, plane_normals, dims,
                           ray_magnitude, extinction, reflectivity, int(resolution[0]), int(resolution[1]),
                           bool(per_target), cyl, blocking["corners"], blocking["spans"], blocking["normals"],
                           blocking["owner"], float(blocking.get("max_scatter_angle", -1.0)),
                           bool(blocking.get("lbvh_compat", True)), points_per_facet)


def per_target_sum(bitmaps: torch.Tensor, target_idx: torch.Tensor, n_targets: int) -> torch.Tensor:
    """``get_bitmaps_per_target`` (heliostat_ray_tracer.py:563-608) as one kernel; differentiable
    through a gather in torch (the backward of a masked sum is an index_select)."""
    _require_cuda(bitmaps, target_idx)
    return _PerTargetSum.apply(bitmaps, _int32c(target_idx), int(n_targets))


class _PerTargetSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bitmaps, target_idx, n_targets):
        dev = bitmaps.device
        b = _f32c(bitmaps)
        H = b.shape[0]
        npix = int(math.prod(b.shape[1:]))
        out = torch.empty((n_targets,) + tuple(b.shape[1:]), dtype=torch.float32, device=dev)
        _lib.call("art_per_target_sum", dev, b.data_ptr(), target_idx.data_ptr(), H, n_targets, npix, out.data_ptr())
        ctx.save_for_backward(target_idx)
        ctx.n_targets = n_targets
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (target_idx,) = ctx.saved_tensors
        idx = target_idx.long()
        ok = (idx >= 0) & (idx < ctx.n_targets)
        g = grad_out.index_select(0, idx.clamp(0, ctx.n_targets - 1))
        return g * ok.view(-1, *([1] * (g.dim() - 1))), None, None


class NurbsEval(torch.autograd.Function):
    """``NURBSSurfaces.calculate_surface_points_and_normals`` (artist/nurbs/surfaces.py:475-689),
    differentiable w.r.t. the control points.  Canting and translations are constants of this fused launch: tensors that
    require grad take :func:`nurbs_eval`, which routes them through :class:`CantFacets`."""

    @staticmethod
    def forward(ctx, control_points, eval_points, knots_u, knots_v, canting, translations, p, q, uniform,
                n_unique_u, n_unique_v, orientation=None):
        dev = _require_cuda(control_points, eval_points, knots_u, knots_v)
        cp = _f32c(control_points)
        H, F, nu, nv, three = cp.shape
        if three != 3:
            raise ValueError("control_points must be [H,F,nu,nv,3]")
        uv = eval_points if eval_points.dtype == torch.float32 else eval_points.float()
        if uv.dim() != 4 or uv.shape[0] != H or uv.shape[1] != F or uv.shape[3] != 2:
            raise ValueError("evaluation_points must be [H,F,M,2]")
        M = uv.shape[2]
        if uv.stride(3) != 1 or uv.stride(2) != 2 or (uv.data_ptr() % 8) != 0:
            uv = uv.contiguous()   # expanded (stride-0) heliostat/facet dims are passed through
        ku = _converted(knots_u.expand(H, F, nu + p + 1), torch.float32)
        kv = _converted(knots_v.expand(H, F, nv + q + 1), torch.float32)
        cant = None if canting is None else _f32c(canting)
        tr = None if canting is None else _f32c(translations.reshape(H, F, 4))
        points = torch.empty((H, F, M, 4), dtype=torch.float32, device=dev)
        normals = torch.empty((H, F, M, 4), dtype=torch.float32, device=dev)
        ori = None
        if orientation is not None:      # fused alignment (a constant here: a learning kinematics takes align_surfaces)
            ori = _f32c(orientation.detach())
            if ori.shape != (H, 4, 4) or ori.device != dev:
                raise ValueError("orientation must be [H,4,4] on the control points' device")
        _lib.call("art_nurbs_fwd", dev,
                  cp.data_ptr(), uv.data_ptr(), uv.stride(0), uv.stride(1), ku.data_ptr(), kv.data_ptr(),
                  None if cant is None else cant.data_ptr(), None if tr is None else tr.data_ptr(),
                  p, q, 1 if uniform else 0, n_unique_u, n_unique_v, H, F, M, nu, nv,
                  None if ori is None else ori.data_ptr(), points.data_ptr(), normals.data_ptr())
        ctx.save_for_backward(cp, uv, ku, kv, cant if cant is not None else cp.new_empty(0),
                              ori if ori is not None else cp.new_empty(0))
        ctx.meta = (p, q, bool(uniform), n_unique_u, n_unique_v, cant is not None, ori is not None)
        return points, normals

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_points, g_normals):
        cp, uv, ku, kv, cant, ori = ctx.saved_tensors
        p, q, uniform, nuq_u, nuq_v, has_cant, has_ori = ctx.meta
        dev = cp.device
        H, F, nu, nv, _ = cp.shape
        M = uv.shape[2]
        g_points, g_normals = _f32c(g_points), _f32c(g_normals)
        g_cp = torch.empty_like(cp)
        _lib.call("art_nurbs_bwd", dev,
                  cp.data_ptr(), uv.data_ptr(), uv.stride(0), uv.stride(1), ku.data_ptr(), kv.data_ptr(),
                  cant.data_ptr() if has_cant else None, p, q, 1 if uniform else 0, nuq_u, nuq_v, H, F, M, nu, nv,
                  ori.data_ptr() if has_ori else None, g_points.data_ptr(), g_normals.data_ptr(), g_cp.data_ptr())
        return (g_cp,) + (None,) * 11


class CantFacets(torch.autograd.Function):
    """The canting rotation of ``points`` and ``normals`` ``[H,F,M,4]`` (either may be None) by the facet bases of ``canting``
    ``[H,F,2,4]``, plus ``translations`` ``[H,F,4]`` (or None) on the points (artist/geometry/transforms.py:276-347,
    artist/nurbs/surfaces.py:674-687; ``art_cant_facets_fwd`` / ``_bwd``, include/artist_hip_canting.h).
    Differentiable w.r.t. all four tensors; the backward is ONE launch that forms only the gradients asked for."""

    @staticmethod
    def forward(ctx, canting, translations, points, normals, inverse=False):
        given = [t for t in (points, normals) if t is not None]
        if not given:
            raise ValueError("CantFacets needs points, normals or both")
        dev = _require_cuda(canting, *given, *(() if translations is None else (translations,)))
        data = given[0]
        if data.dim() != 4 or data.shape[3] != 4 or any(t.shape != data.shape for t in given):
            raise ValueError("points / normals must be [H,F,M,4] (and of one shape)")
        H, F, M = int(data.shape[0]), int(data.shape[1]), int(data.shape[2])
        if tuple(canting.shape) != (H, F, 2, 4):
            raise ValueError(f"canting must be [{H},{F},2,4], got {tuple(canting.shape)}")
        inverse = bool(inverse)
        if translations is not None and (inverse or points is None):
            raise ValueError("translations go with the points of a forward canting only")
        cant = _f32c(canting)
        tr = None if translations is None else _f32c(translations.reshape(H, F, 4))
        pts = None if points is None else _f32c(points)
        nrm = None if normals is None else _f32c(normals)
        out_p = None if pts is None else torch.empty_like(pts)
        out_n = None if nrm is None else torch.empty_like(nrm)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _timed_call("art_cant_facets_fwd", dev, cant.data_ptr(), ptr(tr), ptr(pts), ptr(nrm), 1 if inverse else 0, H * F, M,
                    ptr(out_p), ptr(out_n))
        # the data is read again only by the canting gradient
        keep = ctx.needs_input_grad[0]
        ctx.save_for_backward(cant, pts if keep else None, nrm if keep else None)
        ctx.meta = (inverse, H, F, M, None if translations is None else tuple(translations.shape),
                    points is not None, normals is not None)
        ctx.set_materialize_grads(False)
        return out_p, out_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_p, g_n):
        cant, pts, nrm = ctx.saved_tensors
        inverse, H, F, M, tr_shape, has_p, has_n = ctx.meta
        need_c, need_t, need_p, need_n = ctx.needs_input_grad[:4]
        need_t = need_t and tr_shape is not None
        need_p, need_n = need_p and has_p and g_p is not None, need_n and has_n and g_n is not None
        if (g_p is None and g_n is None) or not (need_c or need_t or need_p or need_n):
            return (None,) * 5
        dev = cant.device
        g_p = None if g_p is None else _f32c(g_p)
        g_n = None if g_n is None else _f32c(g_n)
        gd_p = torch.empty_like(g_p) if need_p else None
        gd_n = torch.empty_like(g_n) if need_n else None
        g_c = torch.empty_like(cant) if need_c else None
        g_t = torch.empty((H, F, 4), dtype=torch.float32, device=dev) if need_t else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        _timed_call("art_cant_facets_bwd", dev, cant.data_ptr(), ptr(pts) if g_p is not None else None,
                    ptr(nrm) if g_n is not None else None, ptr(g_p), ptr(g_n), 1 if inverse else 0, H * F, M,
                    ptr(gd_p), ptr(gd_n), ptr(g_c), ptr(g_t))
        return g_c, None if g_t is None else g_t.reshape(tr_shape), gd_p, gd_n, None


def perform_canting(canting_angles: torch.Tensor, data: torch.Tensor, inverse: bool = False,
                    device: torch.device | None = None) -> torch.Tensor:
    """``artist.geometry.transforms.perform_canting`` (transforms.py:276-347): ``data`` ``[H,F,M,4]`` rotated by the facet bases
    of ``canting_angles`` ``[H,F,2,4]`` - ``data @ R^T``, or ``data @ R`` for ``inverse=True`` (decanting).  Differentiable
    w.r.t. both tensors; fp32 on the GPU (``device`` = None: where ``data`` is)."""
    if device is not None:
        canting_angles, data = canting_angles.to(device), data.to(device)
    return CantFacets.apply(canting_angles, None, data, None, bool(inverse))[0]


def nurbs_eval(control_points, eval_points, knots_u, knots_v, canting, translations, p, q, uniform, n_unique_u, n_unique_v,
               orientation=None):
    """Surface points and normals by the route that reaches every tensor asking for a gradient.  Constants for canting and
    translations: the one fused launch of :class:`NurbsEval`, as ever.  A canting or translation tensor that requires grad:
    the same kernel without them, then :class:`CantFacets`, then :func:`align_surfaces` if ``orientation`` was given - the
    same values bit for bit, and gradients for all three of control points, canting and translations."""
    learns = canting is not None and torch.is_grad_enabled() and (
        canting.requires_grad or (translations is not None and translations.requires_grad))
    if not learns:
        return NurbsEval.apply(control_points, eval_points, knots_u, knots_v, canting, translations, p, q, uniform,
                               n_unique_u, n_unique_v, orientation)
    if translations is None:
        raise ValueError("facet_translations must be given with canting")
    points, normals = NurbsEval.apply(control_points, eval_points, knots_u, knots_v, None, None, p, q, uniform,
                                      n_unique_u, n_unique_v, None)
    points, normals = CantFacets.apply(canting, translations, points, normals, False)
    if orientation is not None:
        shape = points.shape
        points, normals = align_surfaces(points.reshape(shape[0], -1, 4), normals.reshape(shape[0], -1, 4), orientation.detach())
        points, normals = points.reshape(shape), normals.reshape(shape)
    return points, normals


def nurbs_surface_points_and_normals(control_points, eval_points, knots_u, knots_v, degrees, canting=None,
                                     translations=None, uniform=True, n_unique=None, orientation=None):
    p, q = int(degrees[0]), int(degrees[1])
    nu, nv = control_points.shape[2], control_points.shape[3]
    if n_unique is None:
        n_unique = (nu - p + 1, nv - q + 1)
    return nurbs_eval(control_points, eval_points, knots_u, knots_v, canting, translations, p, q,
                      bool(uniform), int(n_unique[0]), int(n_unique[1]), orientation)


class AlignSurfaces(torch.autograd.Function):
    """``points @ orientation^T`` and ``normals @ orientation^T`` in one pass
    (artist/field/heliostat_group_rigid_body.py:217-222, 265-270), differentiable w.r.t. all three inputs."""

    @staticmethod
    def forward(ctx, points, normals, orientation):
        dev = _require_cuda(points, normals, orientation)
        points, normals, orientation = _f32c16(points), _f32c16(normals), _f32c(orientation)
        H, P = points.shape[0], points.shape[1]
        if points.shape != (H, P, 4) or normals.shape != (H, P, 4) or orientation.shape != (H, 4, 4):
            raise ValueError("points/normals must be [H,P,4] and orientation [H,4,4]")
        out_p, out_n = torch.empty_like(points), torch.empty_like(normals)
        _lib.call("art_align_fwd", dev, points.data_ptr(), normals.data_ptr(), orientation.data_ptr(), H, P,
                  out_p.data_ptr(), out_n.data_ptr())
        ctx.save_for_backward(points, normals, orientation)
        return out_p, out_n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out_p, g_out_n):
        points, normals, orientation = ctx.saved_tensors
        dev = points.device
        H, P = points.shape[0], points.shape[1]
        g_out_p, g_out_n = _f32c16(g_out_p), _f32c16(g_out_n)
        g_p, g_n = torch.empty_like(points), torch.empty_like(normals)
        g_m = torch.empty_like(orientation) if ctx.needs_input_grad[2] else None
        _lib.call("art_align_bwd", dev, points.data_ptr(), normals.data_ptr(), orientation.data_ptr(),
                  g_out_p.data_ptr(), g_out_n.data_ptr(), H, P, g_p.data_ptr(), g_n.data_ptr(),
                  None if g_m is None else g_m.data_ptr())
        return g_p, g_n, g_m


def align_surfaces(points: torch.Tensor, normals: torch.Tensor, orientation: torch.Tensor):
    """Aligned ``(points, normals)`` = ``(points @ orientation^T, normals @ orientation^T)``."""
    return AlignSurfaces.apply(points, normals, orientation)
