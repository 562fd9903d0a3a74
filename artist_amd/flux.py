"""The flux epilogue of an optimisation epoch, on MI355X.

Drop-ins for ``artist.flux.bitmap.crop_flux_distributions_around_center`` (artist/flux/bitmap.py:121-246) and
for ``artist.optim.loss.PixelLoss`` / ``KLDivergenceLoss`` (artist/optim/loss.py:251-410): same names,
arguments and return values; the arithmetic runs in ``artist_amd/csrc/flux_kernels.hip`` through
``art_flux_crop_fwd/bwd`` and ``art_flux_loss``.  They consume the ray tracer's ``[H,res_u,res_e]`` bitmaps where
they are, in HBM, and their backward passes are deterministic (the crop's gradient is a gather, not the
atomic scatter of ``grid_sample``'s backward).
"""
from __future__ import annotations

from typing import Any

import torch

from . import _lib
from .ops import _f32c, _require_cuda


def trapezoid_distribution(total_width: int, slope_width: int, plateau_width: int,
                           device: torch.device | None = None) -> torch.Tensor:
    """A one-dimensional trapezoid ``[total_width]``, symmetric about the middle of the axis: 1 on a plateau of
    ``plateau_width`` pixels, falling linearly to 0 over ``slope_width`` pixels on either side (artist/flux/bitmap.py:74-118).
    A trapezoid wider than the axis has its slopes cut off, a narrower one is padded with zeros; ``slope_width == 0`` is the
    hard rectangle.  The aim-point tutorial's target distribution is the outer product of two of these.

    Plain torch (a ``[total_width]`` vector built once per run, not a hot path): works on the CPU and on the GPU.  ``device``
    None is the GPU when there is one, like the reference's ``get_device``."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    total_width = int(total_width)
    pixel = torch.arange(total_width, device=device)
    beyond_plateau = torch.abs(pixel - (total_width - 1) / 2.0) - plateau_width / 2.0
    if slope_width == 0:
        return (beyond_plateau <= 0).to(dtype=torch.float32)
    return 1 - (beyond_plateau / slope_width).clamp(min=0, max=1)


def target_dimensions(solar_tower, target_area_indices: torch.Tensor) -> torch.Tensor:
    """``[B,2]`` (width, height) in metres of each bitmap's target area by GLOBAL index, planar first, cylindrical
    second: planar ``dimensions``, or ``radius * opening_angle`` and ``height`` (bitmap.py:183-216)."""
    tables = []
    from .raytracing import target_area_counts
    n_per_type = target_area_counts(solar_tower)          # (host side: no read of the tower's device tensor)
    if n_per_type[0] > 0:
        tables.append(solar_tower.target_areas[0].dimensions.to(torch.float32))
    if n_per_type[1] > 0:
        cyl = solar_tower.target_areas[1]
        tables.append(torch.stack((cyl.radii.reshape(-1) * cyl.opening_angles.reshape(-1), cyl.heights.reshape(-1)), dim=1)
                      .to(torch.float32))
    table = torch.cat([t.to(target_area_indices.device) for t in tables])
    return table.index_select(0, target_area_indices.long())


class FluxCrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flux, dims, crop_width, crop_height):
        dev = _require_cuda(flux, dims)
        flux, dims = _f32c(flux), _f32c(dims)
        if flux.dim() != 3 or dims.shape != (flux.shape[0], 2):
            raise ValueError("flux must be [B,Hh,W] and the target dimensions [B,2]")
        B, Hh, W = flux.shape
        out = torch.empty_like(flux)
        centers = torch.empty((B, 3), dtype=torch.float32, device=dev)
        _lib.call("art_flux_crop_fwd", dev, flux.data_ptr(), dims.data_ptr(), B, Hh, W, float(crop_width), float(crop_height),
                  out.data_ptr(), centers.data_ptr())
        ctx.save_for_backward(flux, dims, centers)
        ctx.crop = (float(crop_width), float(crop_height))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        flux, dims, centers = ctx.saved_tensors
        dev = flux.device
        B, Hh, W = flux.shape
        grad_out = _f32c(grad_out)
        grad_flux = torch.empty_like(flux)
        workspace = torch.empty((B, 3), dtype=torch.float32, device=dev)
        _lib.call("art_flux_crop_bwd", dev, flux.data_ptr(), dims.data_ptr(), centers.data_ptr(), B, Hh, W, *ctx.crop,
                  grad_out.data_ptr(), grad_flux.data_ptr(), workspace.data_ptr())
        return grad_flux, None, None, None


def crop_flux_distributions_around_center(flux_distributions: torch.Tensor, solar_tower, target_area_indices: torch.Tensor,
                                          crop_width: float = 6, crop_height: float = 6,
                                          device: torch.device | None = None) -> torch.Tensor:
    """Crop a ``crop_width`` x ``crop_height`` metre region centred on each bitmap's centre of mass, resampled to the
    bitmap's own resolution (bitmap.py:121-246; defaults = ``constants.utis_crop_width/height``)."""
    if device is not None:
        flux_distributions = flux_distributions.to(device)
    dims = target_dimensions(solar_tower, target_area_indices.to(flux_distributions.device))
    return FluxCrop.apply(flux_distributions, dims, crop_width, crop_height)


class FluxBlur(torch.autograd.Function):
    """``art_flux_crop_fwd`` in its blur mode (crop size (-1, -1), no target dimensions, the covariances where the crop writes
    its centres).  The operator is its own adjoint: the backward pass is the same call on the upstream gradient."""

    @staticmethod
    def _launch(x: torch.Tensor, covariance: torch.Tensor) -> torch.Tensor:
        B, Hh, W = x.shape
        out = torch.empty_like(x)
        _lib.call("art_flux_crop_fwd", x.device, x.data_ptr(), None, B, Hh, W, -1.0, -1.0, out.data_ptr(), covariance.data_ptr())
        return out

    @staticmethod
    def forward(ctx, flux, covariance):
        ctx.save_for_backward(covariance)
        return FluxBlur._launch(flux, covariance)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        (covariance,) = ctx.saved_tensors
        return FluxBlur._launch(grad_out.contiguous(), covariance), None


def blur_flux(flux: torch.Tensor, covariance: torch.Tensor) -> torch.Tensor:
    """Each bitmap of ``flux [B,Hh,W]`` convolved with its own Gaussian window, ``covariance [B,3]`` =
    ``(S_rr, S_rc, S_cc)`` in pixels^2 (r the bitmap's row, c its column), as ``[B,Hh,W]``: the convolved sun's second half
    (the operator is defined in include/artist_hip.h at ``art_flux_crop_fwd`` and again, in fp64, in
    tests/flux_blur_ref.py).  Differentiable w.r.t. ``flux`` - the window is symmetric about its centre and the bitmap is
    zero-extended, so the gradient is the same blur of the upstream gradient, one launch, the same bits as a forward call on
    it.  The covariance is a constant: one that requires grad is a ``ValueError``.  A covariance that is not finite, not
    positive semi-definite or wider than the kernel's window (``4 sqrt(max(S_rr, S_cc)) > 64``) makes its bitmap NaN - marked
    in the result, no host read.  fp32 on the GPU only; one launch and one allocation (the result): capturable."""
    if covariance.requires_grad:
        raise ValueError("the covariance of blur_flux is a constant (to first order the sun's image does not depend on the "
                         "learned surface): detach it")
    if flux.device.type != "cuda" or covariance.device.type != "cuda":
        raise _lib.ArtistHipError(f"blur_flux runs on the GPU only (got tensors on {flux.device} and {covariance.device}); "
                                  "there is no CPU fallback")
    _require_cuda(flux, covariance)
    if flux.dtype != torch.float32 or covariance.dtype != torch.float32:
        raise ValueError(f"blur_flux takes float32 tensors, got {flux.dtype} and {covariance.dtype}")
    if flux.dim() != 3 or tuple(covariance.shape) != (flux.shape[0], 3):
        raise ValueError(f"flux must be [B,Hh,W] and the covariance [B,3], got {tuple(flux.shape)} and {tuple(covariance.shape)}")
    return FluxBlur.apply(flux.contiguous(), covariance.contiguous())


class DifferentiableFluxBlur(torch.autograd.Function):
    """``FluxBlur`` with the window learned too: the gradient with respect to the covariances is ``art_flux_crop_bwd`` in its
    blur mode (crop size (-1, -1), no target dimensions, the covariances where the crop reads its centres, the gradient
    ``[B,3]`` where it keeps its workspace) - one launch on the sharp bitmaps and the upstream gradient."""

    @staticmethod
    def covariance_gradient(x: torch.Tensor, covariance: torch.Tensor, grad_out: torch.Tensor) -> torch.Tensor:
        B, Hh, W = x.shape
        grad = torch.empty((B, 3), dtype=torch.float32, device=x.device)
        _lib.call("art_flux_crop_bwd", x.device, x.data_ptr(), None, covariance.data_ptr(), B, Hh, W, -1.0, -1.0,
                  grad_out.data_ptr(), None, grad.data_ptr())
        return grad

    @staticmethod
    def forward(ctx, flux, covariance):
        ctx.learns_window = covariance.requires_grad
        ctx.save_for_backward(covariance, *((flux,) if ctx.learns_window else ()))
        return FluxBlur._launch(flux, covariance)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        covariance = ctx.saved_tensors[0]
        grad_out = grad_out.contiguous()
        grad_flux = FluxBlur._launch(grad_out, covariance) if ctx.needs_input_grad[0] else None
        grad_covariance = None
        if ctx.learns_window and ctx.needs_input_grad[1]:
            grad_covariance = DifferentiableFluxBlur.covariance_gradient(ctx.saved_tensors[1], covariance, grad_out)
        return grad_flux, grad_covariance


def differentiable_blur_flux(flux: torch.Tensor, covariance: torch.Tensor) -> torch.Tensor:
    """``blur_flux`` - the same checks, values and bits - differentiable in BOTH arguments: the window learns.
    The gradient with respect to ``flux`` is the same blur of the upstream gradient, as ``blur_flux`` has it; the gradient with
    respect to ``covariance [B,3]`` = ``(S_rr, S_rc, S_cc)`` is one launch of ``art_flux_crop_bwd`` in its blur mode (defined in
    include/artist_hip.h and again, in fp64, in tests/flux_blur_grad_ref.py): the derivative at FIXED tap radii - the radii are
    piecewise constant in the covariance -, deterministic, without atomics.  A covariance whose bitmap is NaN has a NaN
    gradient.  When the covariance requires grad the backward pass keeps the sharp ``flux``: 4 ``Hh W`` bytes per bitmap that
    ``blur_flux`` does not hold; otherwise nothing more is saved and the launches are ``blur_flux``'s.  fp32 on the GPU only
    (``ArtistHipError`` on the CPU: no CPU fallback); capturable."""
    if flux.device.type != "cuda" or covariance.device.type != "cuda":
        raise _lib.ArtistHipError(f"differentiable_blur_flux runs on the GPU only (got tensors on {flux.device} and "
                                  f"{covariance.device}); there is no CPU fallback")
    _require_cuda(flux, covariance)
    if flux.dtype != torch.float32 or covariance.dtype != torch.float32:
        raise ValueError(f"differentiable_blur_flux takes float32 tensors, got {flux.dtype} and {covariance.dtype}")
    if flux.dim() != 3 or tuple(covariance.shape) != (flux.shape[0], 3):
        raise ValueError(f"flux must be [B,Hh,W] and the covariance [B,3], got {tuple(flux.shape)} and {tuple(covariance.shape)}")
    return DifferentiableFluxBlur.apply(flux.contiguous(), covariance.contiguous())


class RadialFluxBlur(torch.autograd.Function):
    """``art_flux_crop_fwd`` in its radial window mode (crop size (-2, -K), the quantile table where the crop reads the target
    dimensions, the metrics where it writes its centres).  The operator is its own adjoint: the backward pass is the same call
    on the upstream gradient."""

    @staticmethod
    def _launch(x: torch.Tensor, metric: torch.Tensor, quantile_table: torch.Tensor) -> torch.Tensor:
        B, Hh, W = x.shape
        out = torch.empty_like(x)
        _lib.call("art_flux_crop_fwd", x.device, x.data_ptr(), quantile_table.data_ptr(), B, Hh, W, -2.0,
                  -float(quantile_table.shape[0] - 1), out.data_ptr(), metric.data_ptr())
        return out

    @staticmethod
    def forward(ctx, flux, metric, quantile_table):
        ctx.save_for_backward(metric, quantile_table)
        return RadialFluxBlur._launch(flux, metric, quantile_table)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        metric, quantile_table = ctx.saved_tensors
        return RadialFluxBlur._launch(grad_out.contiguous(), metric, quantile_table), None, None


def radial_blur_flux(flux: torch.Tensor, metric: torch.Tensor, quantile_table: torch.Tensor) -> torch.Tensor:
    """Each bitmap of ``flux [B,Hh,W]`` convolved with the image of a radial sun shape on its target, as ``[B,Hh,W]``: ``metric
    [B,3]`` = ``(M_rr, M_rc, M_cc)`` in pixels^2/rad^2 (``optics.sun_image_covariance`` of the unit angular covariance
    ``(1, 0, 1)``), ``quantile_table [K+1]`` the sun's table in rad^2 (``scene.radial_quantile_table``), ``1 <= K <= 4096``.  The
    window is the table's density on the ellipses ``(dr, dc) M^-1 (dr, dc)^T = theta^2``, averaged over 4 x 4 sub-pixel points,
    cut at the largest node whose ellipse fits 64 pixels - what lies beyond is dropped, ``optics.radial_window_kept_fraction``
    says how much stays (the operator is defined in include/artist_hip.h at ``art_flux_crop_fwd`` and again,
    in fp64, in tests/radial_blur_ref.py).  Differentiable w.r.t. ``flux`` - the stencil is point-symmetric and the bitmap is
    zero-extended, so the gradient is the same call on the upstream gradient, one launch, the same bits as a forward call on
    it.  Metric and table are constants: one that requires grad is a ``ValueError``.  A metric that is not finite, not positive
    definite, or so wide that not even the table's first annulus fits makes its bitmap NaN, a table that is not finite or
    decreases makes every bitmap NaN - marked in the result, no host read.  fp32 on the GPU only; one launch and one allocation
    (the result): capturable."""
    if metric.requires_grad or quantile_table.requires_grad:
        raise ValueError("the metric and the quantile table of radial_blur_flux are constants (to first order the sun's image does "
                         "not depend on the learned surface): detach them")
    if flux.dtype != torch.float32 or metric.dtype != torch.float32 or quantile_table.dtype != torch.float32:
        raise ValueError(f"radial_blur_flux takes float32 tensors, got {flux.dtype}, {metric.dtype} and {quantile_table.dtype}")
    if flux.dim() != 3 or tuple(metric.shape) != (flux.shape[0], 3) or quantile_table.dim() != 1 or \
            not 2 <= quantile_table.shape[0] <= 4097:
        raise ValueError(f"flux must be [B,Hh,W], the metric [B,3] and the quantile table [K+1] with 1 <= K <= 4096, got "
                         f"{tuple(flux.shape)}, {tuple(metric.shape)} and {tuple(quantile_table.shape)}")
    devices = (flux.device, metric.device, quantile_table.device)
    if any(d.type != "cuda" for d in devices):
        raise _lib.ArtistHipError(f"radial_blur_flux runs on the GPU only (got tensors on {devices[0]}, {devices[1]} and "
                                  f"{devices[2]}); there is no CPU fallback")
    _require_cuda(flux, metric, quantile_table)
    return RadialFluxBlur.apply(flux.contiguous(), metric.contiguous(), quantile_table.contiguous())


class _FluxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction, ground_truth, kind):
        dev = _require_cuda(prediction, ground_truth)
        prediction, ground_truth = _f32c(prediction), _f32c(ground_truth)
        if prediction.shape != ground_truth.shape or prediction.dim() != 3:
            raise ValueError("prediction and ground truth must both be [number_of_samples, res_e, res_u]")
        B = prediction.shape[0]
        npix = prediction.shape[1] * prediction.shape[2]
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        _lib.call("art_flux_loss", dev, prediction.data_ptr(), ground_truth.data_ptr(), B, npix, kind, loss.data_ptr(), None, None)
        ctx.save_for_backward(prediction, ground_truth)
        ctx.kind = kind
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        prediction, ground_truth = ctx.saved_tensors
        dev = prediction.device
        B = prediction.shape[0]
        npix = prediction.shape[1] * prediction.shape[2]
        grad_loss = _f32c(grad_loss)
        grad_prediction = torch.empty_like(prediction)
        _lib.call("art_flux_loss", dev, prediction.data_ptr(), ground_truth.data_ptr(), B, npix, ctx.kind, None,
                  grad_loss.data_ptr(), grad_prediction.data_ptr())
        return grad_prediction, None, None


class FluxCropPixelLoss(torch.autograd.Function):
    """``PixelLoss()(crop_flux_distributions_around_center(flux, ...), ground_truth, reduction_dimensions=(1, 2))`` fused
    (``art_flux_crop_pixel_loss_fwd/bwd``): the same numbers up to the rounding of the sums (< 1e-6), the same bits for every
    batch size, without the cropped bitmaps' round trip through HBM; when a gradient is wanted the forward pass keeps the
    residual ``crop - ground_truth`` and the backward pass is one kernel over it.  Differentiable w.r.t. ``flux``."""

    calls_with_moments = 0          # (tests: how often the bitmaps came with their centre-of-mass sums)

    @staticmethod
    def forward(ctx, flux, dims, ground_truth, crop_width, crop_height):
        dev = _require_cuda(flux, dims, ground_truth)
        flux, dims, ground_truth = _f32c(flux), _f32c(dims), _f32c(ground_truth)
        if flux.dim() != 3 or dims.shape != (flux.shape[0], 2) or ground_truth.shape != flux.shape:
            raise ValueError("flux and ground truth must be [B,Hh,W] and the target dimensions [B,2]")
        B, Hh, W = flux.shape
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        centers = torch.empty((B, 4), dtype=torch.float32, device=dev)
        keep = bool(ctx.needs_input_grad[0])
        residual = torch.empty_like(flux) if keep else None
        unit = torch.empty((B, 2), dtype=torch.float32, device=dev) if keep else None
        from .ops import bitmap_moments
        moments = bitmap_moments(flux)              # bitmaps straight from the tracer bring their centre-of-mass sums along
        if moments is not None and (moments.shape[0] != B or moments.device != dev):
            moments = None
        FluxCropPixelLoss.calls_with_moments += moments is not None
        _lib.call("art_flux_crop_pixel_loss_fwd", dev, flux.data_ptr(), dims.data_ptr(), ground_truth.data_ptr(), B, Hh, W,
                  float(crop_width), float(crop_height), loss.data_ptr(), centers.data_ptr(),
                  residual.data_ptr() if keep else None, unit.data_ptr() if keep else None,
                  None if moments is None else moments.data_ptr())
        if keep:
            ctx.save_for_backward(dims, centers, residual, unit)
        ctx.crop = (float(crop_width), float(crop_height))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        dims, centers, residual, unit = ctx.saved_tensors
        dev = residual.device
        B, Hh, W = residual.shape
        # the gradient of `loss.sum()` arrives as an expanded scalar (stride 0): the kernel reads the one value - no copy to [B]
        stride = 1
        if grad_loss.dtype == torch.float32 and grad_loss.dim() == 1 and grad_loss.stride(0) == 0 and grad_loss.is_cuda:
            stride = 0
        else:
            grad_loss = _f32c(grad_loss)
        grad_flux = torch.empty_like(residual)
        _lib.call("art_flux_crop_pixel_loss_bwd", dev, dims.data_ptr(), centers.data_ptr(), grad_loss.data_ptr(), stride,
                  residual.data_ptr(), unit.data_ptr(), B, Hh, W, *ctx.crop, grad_flux.data_ptr())
        return grad_flux, None, None, None, None


def crop_and_pixel_loss(flux_distributions: torch.Tensor, solar_tower, target_area_indices: torch.Tensor,
                        ground_truth: torch.Tensor, crop_width: float = 6, crop_height: float = 6) -> torch.Tensor:
    """Per-sample pixel loss of the flux cropped around its centre of mass against the measured (cropped) flux: the
    epilogue of ``SurfaceReconstructor``'s epoch (surface_reconstructor.py:575-590, 664-676) in one fused pass."""
    dims = target_dimensions(solar_tower, target_area_indices.to(flux_distributions.device))
    return FluxCropPixelLoss.apply(flux_distributions, dims, ground_truth, crop_width, crop_height)


class FluxCropKLLoss(torch.autograd.Function):
    """``KLDivergenceLoss()(crop_flux_distributions_around_center(flux, ...), ground_truth, reduction_dimensions=(1, 2))``
    as one pass per direction (``art_flux_crop_kl_loss_fwd/bwd``): the cropped bitmaps never reach HBM.  Differentiable
    w.r.t. ``flux``."""

    @staticmethod
    def forward(ctx, flux, dims, ground_truth, crop_width, crop_height):
        dev = _require_cuda(flux, dims, ground_truth)
        flux, dims, ground_truth = _f32c(flux), _f32c(dims), _f32c(ground_truth)
        if flux.dim() != 3 or dims.shape != (flux.shape[0], 2) or ground_truth.shape != flux.shape:
            raise ValueError("flux and ground truth must be [B,Hh,W] and the target dimensions [B,2]")
        B, Hh, W = flux.shape
        loss = torch.empty((B,), dtype=torch.float32, device=dev)
        record = torch.empty((B, 8), dtype=torch.float32, device=dev)
        _lib.call("art_flux_crop_kl_loss_fwd", dev, flux.data_ptr(), dims.data_ptr(), ground_truth.data_ptr(), B, Hh, W,
                  float(crop_width), float(crop_height), loss.data_ptr(), record.data_ptr())
        ctx.save_for_backward(flux, dims, ground_truth, record)
        ctx.crop = (float(crop_width), float(crop_height))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        flux, dims, ground_truth, record = ctx.saved_tensors
        dev = flux.device
        B, Hh, W = flux.shape
        grad_loss = _f32c(grad_loss)
        grad_flux = torch.empty_like(flux)
        workspace = torch.empty((B * Hh * W + 5 * B,), dtype=torch.float32, device=dev)
        _lib.call("art_flux_crop_kl_loss_bwd", dev, flux.data_ptr(), dims.data_ptr(), ground_truth.data_ptr(),
                  record.data_ptr(), grad_loss.data_ptr(), B, Hh, W, *ctx.crop, grad_flux.data_ptr(), workspace.data_ptr())
        return grad_flux, None, None, None, None


def crop_and_kl_loss(flux_distributions: torch.Tensor, solar_tower, target_area_indices: torch.Tensor,
                     ground_truth: torch.Tensor, crop_width: float = 6, crop_height: float = 6) -> torch.Tensor:
    """Per-sample KL divergence of the flux cropped around its centre of mass against the measured (cropped) flux
    (artist/flux/bitmap.py:121-246 + artist/optim/loss.py:321-410) in one fused pass."""
    dims = target_dimensions(solar_tower, target_area_indices.to(flux_distributions.device))
    return FluxCropKLLoss.apply(flux_distributions, dims, ground_truth, crop_width, crop_height)


class _CenterOfMass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bitmaps):
        dev = _require_cuda(bitmaps)
        bitmaps = _f32c(bitmaps)
        if bitmaps.dim() != 3:
            raise ValueError("bitmaps must be [number_of_active_heliostats, bitmap_resolution_u, bitmap_resolution_e]")
        B, Hh, W = bitmaps.shape
        com = torch.empty((B, 3), dtype=torch.float32, device=dev)
        _lib.call("art_flux_center_of_mass", dev, bitmaps.data_ptr(), B, Hh, W, com.data_ptr())
        ctx.save_for_backward(com)
        ctx.shape = (B, Hh, W)
        return com[:, :2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_com):
        (com,) = ctx.saved_tensors
        B, Hh, W = ctx.shape
        dev = com.device
        grad_com = _f32c(grad_com)
        grad = torch.empty((B, Hh, W), dtype=torch.float32, device=dev)
        _lib.call("art_flux_center_of_mass_bwd", dev, com.data_ptr(), grad_com.data_ptr(), B, Hh, W, grad.data_ptr())
        return grad


def get_center_of_mass(bitmaps: torch.Tensor, device: torch.device | None = None) -> torch.Tensor:
    """Bitmap coordinates ``[B,2]`` = (e pixel, u pixel) of each bitmap's centre of mass; (0, 0) for an empty bitmap
    (artist/flux/bitmap.py:12-71).  One streaming pass (``art_flux_center_of_mass``); differentiable."""
    if device is not None:
        bitmaps = bitmaps.to(device)
    return _CenterOfMass.apply(bitmaps)


def bitmap_coordinates_to_target_coordinates(bitmap_coordinates: torch.Tensor, bitmap_resolution, solar_tower,
                                             target_area_indices: torch.Tensor, device: torch.device | None = None) -> torch.Tensor:
    """Pixel coordinates (e, u) -> homogeneous world coordinates ``[B,4]`` on the target surface
    (artist/geometry/coordinates.py:119-249): planar areas linearly, cylindrical ones over angle and height; pixel centres,
    e axis flipped.  ``[B]``-sized arithmetic on the host side of the op (torch, differentiable); unlike the reference no
    branch reads a device tensor, so nothing here waits for the device."""
    from .raytracing import target_area_counts
    bc = bitmap_coordinates if device is None else bitmap_coordinates.to(device)
    dev, dt = bc.device, bc.dtype
    width, height = float(bitmap_resolution[0]), float(bitmap_resolution[1])
    e_norm = (bc[:, 0] + 0.5) / width
    u_norm = (bc[:, 1] + 0.5) / height
    n_planar, n_cyl = target_area_counts(solar_tower)
    tix = target_area_indices.to(dev).long()
    out3 = torch.zeros((bc.shape[0], 3), dtype=dt, device=dev)
    if n_planar > 0:
        planar = solar_tower.target_areas[0]
        pi_ = tix.clamp(0, n_planar - 1)
        centers, dims = planar.centers.to(dev, dt)[pi_][:, :3], planar.dimensions.to(dev, dt)[pi_]
        e_local, u_local = (0.5 - e_norm) * dims[:, 0], (0.5 - u_norm) * dims[:, 1]
        # east and up of the plane are the world's x and z (stacked: a unit vector built from a host list would be a copy to the
        # device, which waits, in every call)
        on_plane = centers + torch.stack((e_local, torch.zeros_like(e_local), u_local), dim=1)
        out3 = torch.where((tix < n_planar)[:, None], on_plane, out3)
    if n_cyl > 0:
        cyl = solar_tower.target_areas[1]
        ci = (tix - n_planar).clamp(0, n_cyl - 1)
        centers, axes, normals = (t.to(dev, dt)[ci][:, :3] for t in (cyl.centers, cyl.axes, cyl.normals))
        radii, heights, opening = (t.to(dev, dt).reshape(-1)[ci] for t in (cyl.radii, cyl.heights, cyl.opening_angles))
        v = torch.cross(axes, normals, dim=-1)
        theta, z = (e_norm - 0.5) * opening, (0.5 - u_norm) * heights
        on_cyl = centers + radii[:, None] * torch.cos(theta)[:, None] * normals + radii[:, None] * torch.sin(theta)[:, None] * v \
            + z[:, None] * axes
        out3 = torch.where((tix >= n_planar)[:, None], on_cyl, out3)
    return torch.cat((out3, torch.ones((bc.shape[0], 1), dtype=dt, device=dev)), dim=1)


class FocalSpotLoss:
    """Distance between the predicted and the ground-truth focal spot on the target area, per sample
    (artist/optim/loss.py:124-250): centres of mass of both bitmaps (``get_center_of_mass``) mapped to world coordinates."""

    def __init__(self, scenario) -> None:
        self.loss_function = None
        self.scenario = scenario

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        expected_kwargs = ["device", "target_area_indices"]
        errors = [f"Please add '{key}' as keyword argument." for key in expected_kwargs if key not in kwargs]
        if errors:                                   # same message as artist/optim/loss.py:187-196
            raise ValueError(f"The focal spot loss expects {expected_kwargs} as keyword arguments. " + " ".join(errors))
        tower = self.scenario.solar_tower
        resolution = (prediction.shape[2], prediction.shape[1])             # (width, height), loss.py:212-216
        spots = [bitmap_coordinates_to_target_coordinates(get_center_of_mass(b), resolution, tower, kwargs["target_area_indices"])
                 for b in (prediction, ground_truth)]
        return torch.norm(spots[0][:, :3] - spots[1][:, :3], dim=1)


def _check_reduction(kwargs: dict, what: str) -> None:
    if "reduction_dimensions" not in kwargs:          # same messages as artist/optim/loss.py:300-311, 376-383
        if what == "pixel":
            raise ValueError("The vector loss expects ['reduction_dimensions'] as keyword arguments. "
                             "Please add 'reduction_dimensions' as keyword argument.")
        if what != "kl":                                # a gain-invariant loss (the reference has none): named in full
            raise ValueError(f"The {what} loss expects 'reduction_dimensions' as keyword argument. Please add this argument.")
        raise ValueError("The KL-divergence loss expects 'reduction_dimensions' as keyword argument. "
                         "Please add this argument.")
    if tuple(int(d) for d in kwargs["reduction_dimensions"]) not in ((1, 2), (-2, -1)):
        raise NotImplementedError("the fused flux losses reduce over the two bitmap dimensions (1, 2) - the only "
                                  "reduction ARTIST's optimisers use")


class PixelLoss:
    """``sum (prediction - ground_truth)^2 / sum ground_truth`` per sample (artist/optim/loss.py:251-318)."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "pixel")
        return _FluxLoss.apply(prediction, ground_truth, 0)


class KLDivergenceLoss:
    """``D_KL(ground truth || prediction)`` of the L1-normalised bitmaps per sample (artist/optim/loss.py:321-410)."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "kl")
        return _FluxLoss.apply(prediction, ground_truth, 1)


# The gain-invariant losses (no counterpart in the reference): a measured flux image is a camera frame whose
# gain against the traced flux is unknown, so these compare SHAPES - multiplying the prediction or the ground truth by a
# positive number changes none of them - and, unlike the KL divergence, all four are bounded.
class JensenShannonLoss:
    """Jensen-Shannon divergence of the L1-normalised bitmaps per sample (``art_flux_loss`` kind 2), in about ``[0, ln 2]``:
    ``1/2 D_KL(g^ || m) + 1/2 D_KL(p^ || m)`` with ``m = (p^ + g^) / 2`` and the ``+ 1e-12`` of ``KLDivergenceLoss`` inside every
    logarithm.  A prediction that is empty costs about ``ln(2) / 2`` where the KL divergence costs about 27.6."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "Jensen-Shannon")
        return _FluxLoss.apply(prediction, ground_truth, 2)


class ShapePixelLoss:
    """``PixelLoss`` of the two bitmaps each scaled to unit mean, per sample (``art_flux_loss`` kind 3):
    ``K sum (p^ - g^)^2`` for bitmaps of ``K`` pixels, ``p^`` and ``g^`` L1-normalised."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "shape pixel")
        return _FluxLoss.apply(prediction, ground_truth, 3)


class TotalVariationLoss:
    """Total variation distance of the L1-normalised bitmaps per sample (``art_flux_loss`` kind 4): ``1/2 sum |p^ - g^|`` in
    ``[0, 1]``, the share of the flux that lies in the wrong place."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "total variation")
        return _FluxLoss.apply(prediction, ground_truth, 4)


class CosineFluxLoss:
    """One minus the cosine similarity of the flattened bitmaps per sample (``art_flux_loss`` kind 5): what
    ``artist_amd.losses.CosineSimilarityLoss`` gives on ``prediction.flatten(1)``, ``ground_truth.flatten(1)``, in one pass over
    the bitmaps."""

    def __call__(self, prediction: torch.Tensor, ground_truth: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        _check_reduction(kwargs, "cosine flux")
        return _FluxLoss.apply(prediction, ground_truth, 5)
