"""``artist.scenario.surface_generator.SurfaceGenerator`` on the gfx950 kernels ``art_surface_fit_prepare / _loss_grad / _run``.

Same constructor and method names as the reference class (artist/scenario/surface_generator.py:16-436).  ``fit_nurbs`` fits one
facet as the reference does; ``fit_nurbs_batch`` - the capability the reference lacks - fits all facets of a field in one
``prepare`` launch and one ``run`` launch per chunk of epochs, one workgroup per facet, without a host-device synchronisation;
``generate_fitted_surface_config`` goes through it.  The C ABI is declared in ``include/artist_hip_surface_fit.h``; there is no
CPU fallback.

One deliberate deviation: the reference hands ONE scheduler object to every facet's fit in turn, so a ``ReduceLROnPlateau``
carries ``best`` / ``num_bad_epochs`` / ``cooldown_counter`` from one facet into the next.  ``generate_fitted_surface_config``
here starts every facet with fresh scheduler state by default (``independent_facets=True``: the facets are fitted at once);
``independent_facets=False`` keeps the reference's facet-after-facet order with the state carried over.
"""
from __future__ import annotations

import dataclasses
import logging
import math

import torch

from . import _lib
from .nurbs import NURBSSurfaces, create_planar_nurbs_control_points
from .ops import _f32c, _require_cuda, _timed_call
from .optim import Adam as _HipAdam

__all__ = ["SurfaceGenerator", "FittedFacet", "FIT_NURBS_FROM_POINTS", "FIT_NURBS_FROM_NORMALS"]

log = logging.getLogger(__name__)

FIT_NURBS_FROM_POINTS = "point_cloud"        # artist.util.constants.fit_nurbs_from_points
FIT_NURBS_FROM_NORMALS = "deflectometry"     # artist.util.constants.fit_nurbs_from_normals
_METHODS = {FIT_NURBS_FROM_POINTS: 0, FIT_NURBS_FROM_NORMALS: 1}
_MAX_EPOCHS_PER_LAUNCH = 1024


@dataclasses.dataclass
class FittedFacet:
    """One facet of a surface configuration: the fields of the reference's ``FacetConfig`` as plain data."""
    facet_key: str
    control_points: torch.Tensor          # [nu, nv, 3]
    degrees: torch.Tensor                 # [2]
    translation_vector: torch.Tensor      # [4]
    canting: torch.Tensor                 # [2, 4]


def _check_method(fit_method: str) -> int:
    if fit_method not in _METHODS:
        raise NotImplementedError(f"The conversion method '{fit_method}' is not yet supported in ARTIST.")
    return _METHODS[fit_method]


def adam_hyperparameters(optimizer) -> dict | None:
    """The hyper-parameters the fused path runs with, read from ``optimizer.defaults`` (the reference clears the parameter
    groups and adds a fresh one, so the defaults are what it steps with); ``None`` for an optimiser that is not Adam (generic
    path).  ``None`` as optimiser means ``Adam(lr=1e-3)``."""
    if optimizer is None:
        return dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)
    if type(optimizer) not in (torch.optim.Adam, _HipAdam):
        return None
    d = optimizer.defaults
    for flag in ("amsgrad", "capturable", "differentiable", "decoupled_weight_decay"):
        if d.get(flag):
            raise ValueError(f"SurfaceGenerator fits with plain Adam: {flag}=True is not supported")
    if isinstance(d["lr"], torch.Tensor):
        raise ValueError("SurfaceGenerator needs a Python float learning rate, not a tensor")
    return dict(lr=float(d["lr"]), betas=(float(d["betas"][0]), float(d["betas"][1])), eps=float(d["eps"]),
                weight_decay=float(d["weight_decay"]), maximize=bool(d.get("maximize", False)))


def plateau_hyperparameters(scheduler) -> dict | None:
    """Parameters and current state of a ``ReduceLROnPlateau``; ``None`` for any other scheduler (generic path).  Without a
    scheduler: ``dict(use=False)``."""
    if scheduler is None:
        return dict(use=False, mode_max=False, factor=0.1, patience=10, threshold=1e-4, threshold_abs=False, cooldown=0,
                    min_lr=0.0, eps=1e-8, best=math.inf, num_bad_epochs=0, cooldown_counter=0)
    if not isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
        return None
    if scheduler.mode not in ("min", "max") or scheduler.threshold_mode not in ("rel", "abs"):
        raise ValueError(f"unknown ReduceLROnPlateau mode {scheduler.mode!r} / threshold mode {scheduler.threshold_mode!r}")
    min_lrs = scheduler.min_lrs
    return dict(use=True, mode_max=scheduler.mode == "max", factor=float(scheduler.factor), patience=int(scheduler.patience),
                threshold=float(scheduler.threshold), threshold_abs=scheduler.threshold_mode == "abs",
                cooldown=int(scheduler.cooldown), min_lr=float(min_lrs[0] if isinstance(min_lrs, (list, tuple)) else min_lrs),
                eps=float(scheduler.eps), best=float(scheduler.best), num_bad_epochs=int(scheduler.num_bad_epochs),
                cooldown_counter=int(scheduler.cooldown_counter))


def _net_block_error(nu: int, nv: int, p: int, q: int, epochs: int):
    """``on_error`` of the loop kernels' calls.  The number of points is no limit (beyond 2^20 rows per facet, which is
    ``ART_EINVAL``): a facet whose per-point arrays do not fit in LDS is evaluated in chunks.  What has to fit in a CU's 160 KiB
    is the net's own block, and ``ART_EUNSUPPORTED`` says that it does not."""
    def on_error(code: int, name: str) -> None:
        if code != _lib.ART_EUNSUPPORTED:
            return _lib.check(code, name)
        ncells, pq = (nu - p) * (nv - q), (p + 1) * (q + 1)
        parts = {"control net and two Adam moments": 9 * nu * nv, "cell partial sums": 3 * ncells * pq,
                 "bias-correction tables": 3 * epochs, "cell offsets": ncells + 3}
        text = ", ".join(f"{k} {4 * v / 1024:.1f} KiB" for k, v in parts.items())
        raise _lib.ArtistHipError(
            f"{name}: the LDS block of a {nu} x {nv} net of degrees ({p}, {q}) does not fit in 160 KiB beside one chunk of 64 "
            f"points ({text}; the number of points per facet does not enter: they are streamed in chunks). "
            f"Use a smaller net{' or fewer epochs per launch' if epochs else ''}. (code {code})")
    return on_error


class _Prepared:
    """Buffers of ``art_surface_fit_prepare`` for a batch: what the loop kernels read, plus the evaluation points and the
    initial nets.  Any ``N`` up to 2^20 rows per facet; nothing but these buffers is sized by it."""

    def __init__(self, points: torch.Tensor, n_valid, nu: int, nv: int, p: int, q: int, knots_u, knots_v):
        dev = _require_cuda(points)
        if points.dim() != 3 or points.shape[2] != 4 or points.shape[1] < 1:
            raise ValueError(f"surface points must be [B, N, 4] with N >= 1, got {tuple(points.shape)}")
        self.points = _f32c(points)
        self.B, self.N = int(points.shape[0]), int(points.shape[1])
        self.nu, self.nv, self.p, self.q, self.device = nu, nv, p, q, dev
        if n_valid is not None:
            n_valid = n_valid.to(device=dev, dtype=torch.int32).contiguous()
            if n_valid.shape != (self.B,):
                raise ValueError(f"n_valid must be [B] = [{self.B}], got {tuple(n_valid.shape)}")
        self.n_valid = n_valid
        W = int(_lib.lib().art_surface_fit_table_words(p, q))
        if W < 0:
            raise ValueError(f"NURBS degrees must be in 1..7, got ({p}, {q})")
        ncells = (nu - p) * (nv - q)
        self.eval_uv = torch.empty((self.B, self.N, 2), dtype=torch.float32, device=dev)
        self.initial_control_points = torch.empty((self.B, nu, nv, 3), dtype=torch.float32, device=dev)
        self.perm = torch.empty((self.B, self.N), dtype=torch.int32, device=dev)
        self.cell_start = torch.empty((self.B, max(ncells, 0) + 1), dtype=torch.int32, device=dev)
        self.table = torch.empty((self.B, self.N, W), dtype=torch.float32, device=dev)
        _timed_call("art_surface_fit_prepare", dev, self.points.data_ptr(), self._nv_ptr(), knots_u.data_ptr(), knots_v.data_ptr(),
                    self.B, self.N, nu, nv, p, q, self.eval_uv.data_ptr(), self.initial_control_points.data_ptr(), self.perm.data_ptr(),
                    self.cell_start.data_ptr(), self.table.data_ptr())

    def _nv_ptr(self):
        return None if self.n_valid is None else self.n_valid.data_ptr()

    def loss_grad(self, control_points: torch.Tensor, targets: torch.Tensor, method: int, with_points: bool = False):
        """``(loss [B], grad [B,nu,nv,3])`` (+ points, normals ``[B,N,4]`` in the original row order)."""
        cp = _f32c(control_points).reshape(self.B, self.nu, self.nv, 3)
        loss = torch.empty((self.B,), dtype=torch.float32, device=self.device)
        grad = torch.empty_like(cp)
        pts = torch.zeros((self.B, self.N, 4), dtype=torch.float32, device=self.device) if with_points else None
        nrm = torch.zeros_like(pts) if with_points else None
        _timed_call("art_surface_fit_loss_grad", self.device, cp.data_ptr(), targets.data_ptr(), self._nv_ptr(), self.perm.data_ptr(),
                    self.cell_start.data_ptr(), self.table.data_ptr(), self.B, self.N, self.nu, self.nv, self.p, self.q, method,
                    loss.data_ptr(), grad.data_ptr(), None if pts is None else pts.data_ptr(), None if nrm is None else nrm.data_ptr(),
                    on_error=_net_block_error(self.nu, self.nv, self.p, self.q, 0))
        return (loss, grad, pts, nrm) if with_points else (loss, grad)


class _FitState:
    """Per-facet optimiser / scheduler / stop state of ``art_surface_fit_run`` (layout: include/artist_hip_surface_fit.h)."""

    def __init__(self, control_points: torch.Tensor, lr: float, sched: dict):
        dev = control_points.device
        B = control_points.shape[0]
        self.control_points = control_points
        self.exp_avg = torch.zeros_like(control_points)
        self.exp_avg_sq = torch.zeros_like(control_points)
        self.f64 = torch.empty((B, 2), dtype=torch.float64, device=dev)
        self.f64[:, 0].fill_(lr)
        self.f64[:, 1].fill_(sched["best"])
        self.i32 = torch.zeros((B, 5), dtype=torch.int32, device=dev)
        if sched["num_bad_epochs"]:
            self.i32[:, 1].fill_(sched["num_bad_epochs"])
        if sched["cooldown_counter"]:
            self.i32[:, 2].fill_(sched["cooldown_counter"])
        self.last_loss = torch.full((B,), math.inf, dtype=torch.float32, device=dev)

    lr = property(lambda self: self.f64[:, 0])
    best = property(lambda self: self.f64[:, 1])
    step = property(lambda self: self.i32[:, 0])
    num_bad_epochs = property(lambda self: self.i32[:, 1])
    cooldown_counter = property(lambda self: self.i32[:, 2])
    epochs_run = property(lambda self: self.i32[:, 3])
    done = property(lambda self: self.i32[:, 4])


def run_epochs(prep: _Prepared, state: _FitState, targets: torch.Tensor, method: int, epochs: int, tolerance: float,
               max_epoch: int, adam: dict, sched: dict) -> None:
    """``epochs`` epochs on every facet that has not stopped, in launches of at most 1024 epochs."""
    while epochs > 0:
        chunk = min(epochs, _MAX_EPOCHS_PER_LAUNCH)
        _timed_call("art_surface_fit_run", prep.device,
                    state.control_points.data_ptr(), state.exp_avg.data_ptr(), state.exp_avg_sq.data_ptr(), state.f64.data_ptr(),
                    state.i32.data_ptr(), state.last_loss.data_ptr(), targets.data_ptr(), prep._nv_ptr(), prep.perm.data_ptr(),
                    prep.cell_start.data_ptr(), prep.table.data_ptr(), prep.B, prep.N, prep.nu, prep.nv, prep.p, prep.q, method,
                    chunk, float(tolerance), int(max_epoch), adam["betas"][0], adam["betas"][1], adam["eps"], adam["weight_decay"],
                    1 if adam["maximize"] else 0, 1 if sched["use"] else 0, 1 if sched["mode_max"] else 0, sched["factor"],
                    sched["patience"], sched["threshold"], 1 if sched["threshold_abs"] else 0, sched["cooldown"], sched["min_lr"],
                    sched["eps"], on_error=_net_block_error(prep.nu, prep.nv, prep.p, prep.q, chunk))
        epochs -= chunk


class _FitLoss(torch.autograd.Function):
    """Per-facet fit loss ``[B]`` of control nets ``[B,nu,nv,3]`` (generic path: any optimiser steps it in a host loop)."""

    @staticmethod
    def forward(ctx, control_points, prep, targets, method):
        loss, grad = prep.loss_grad(control_points.detach(), targets, method)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        (grad,) = ctx.saved_tensors
        return grad * grad_loss.reshape(-1, 1, 1, 1), None, None, None


class SurfaceGenerator:
    """A surface generator for fitted and ideal surfaces (artist/scenario/surface_generator.py:16-69)."""

    def __init__(self, number_of_control_points: torch.Tensor = torch.tensor([10, 10]),
                 degrees: torch.Tensor = torch.tensor([3, 3]), device: torch.device | None = None) -> None:
        self._n_cp = (int(number_of_control_points[0]), int(number_of_control_points[1]))
        self._deg = (int(degrees[0]), int(degrees[1]))
        self._degrees_host = torch.tensor(self._deg)
        if device is not None:
            number_of_control_points, degrees = number_of_control_points.to(device), degrees.to(device)
        self.number_of_control_points = number_of_control_points
        self.degrees = degrees

    # ---- the batch path ------------------------------------------------------------------------------------------------------

    def _surfaces(self, control_points: torch.Tensor) -> NURBSSurfaces:
        # (the host copy of the degrees: reading a device tensor would synchronise)
        return NURBSSurfaces(degrees=self._degrees_host, control_points=control_points, device=control_points.device)

    def prepare(self, surface_points: torch.Tensor, n_valid: torch.Tensor | None = None) -> _Prepared:
        """``art_surface_fit_prepare`` for ``surface_points [B,N,4]``: normalised evaluation points, initial nets and the
        per-point tables of the loop kernels."""
        dev = _require_cuda(surface_points)
        (nu, nv), (p, q) = self._n_cp, self._deg
        knots = self._surfaces(torch.empty((1, 1, nu, nv, 3), dtype=torch.float32, device=dev))
        return _Prepared(surface_points, n_valid, nu, nv, p, q, _f32c(knots.knot_vectors_u[0, 0]), _f32c(knots.knot_vectors_v[0, 0]))

    def fit_nurbs_batch(self, surface_points: torch.Tensor, surface_normals: torch.Tensor, n_valid: torch.Tensor | None = None,
                        optimizer: torch.optim.Optimizer | None = None, scheduler=None,
                        fit_method: str = FIT_NURBS_FROM_NORMALS, tolerance: float = 1e-10, max_epoch: int = 400,
                        epochs_per_launch: int | None = None, device: torch.device | None = None):
        """Fit ``B`` independent facets at once: ``surface_points``, ``surface_normals`` ``[B,N,4]``, of which the first
        ``n_valid[b]`` rows of facet ``b`` count (all when ``None``).  Returns ``(NURBSSurfaces with control points
        [B,1,nu,nv,3], epochs_run [B] int32, final_loss [B])``; ``final_loss`` is the loss the last epoch computed before its
        update, as the reference's loop compares it.  Hyper-parameters come from ``optimizer.defaults`` (Adam; ``None``:
        ``lr=1e-3``) and from a ``ReduceLROnPlateau`` (parameters only - every facet starts with fresh scheduler state; the
        scheduler object is not modified).  One ``prepare`` launch and one ``run`` launch per ``epochs_per_launch`` epochs
        (default: all), no host-device synchronisation - a generator's first call included."""
        method = _check_method(fit_method)
        dev = _require_cuda(surface_points, surface_normals)
        adam, sched = adam_hyperparameters(optimizer), plateau_hyperparameters(scheduler)
        if adam is None or sched is None:
            raise TypeError("fit_nurbs_batch runs Adam with an optional ReduceLROnPlateau; other optimisers and schedulers go "
                            "through fit_nurbs, facet by facet")
        if surface_normals.shape != surface_points.shape:
            raise ValueError("surface points and normals differ in shape")
        if sched["use"]:
            sched = dict(sched, best=-math.inf if sched["mode_max"] else math.inf, num_bad_epochs=0, cooldown_counter=0)
        prep = self.prepare(surface_points, n_valid)
        targets = prep.points if method == 0 else _f32c(surface_normals)
        state = _FitState(prep.initial_control_points.clone(), adam["lr"], sched)
        total = int(max_epoch) + 1                       # epochs 0 .. max_epoch (surface_generator.py:196)
        per = total if epochs_per_launch is None else max(1, int(epochs_per_launch))
        done = 0
        while done < total:
            n = min(per, total - done)
            run_epochs(prep, state, targets, method, n, tolerance, max_epoch, adam, sched)
            done += n
        surfaces = self._surfaces(state.control_points.reshape(prep.B, 1, prep.nu, prep.nv, 3))
        surfaces.fit_state = state
        return surfaces, state.epochs_run, state.last_loss

    # ---- the reference's interface -------------------------------------------------------------------------------------------

    def fit_nurbs(self, surface_points: torch.Tensor, surface_normals: torch.Tensor, optimizer: torch.optim.Optimizer,
                  scheduler=None, fit_method: str = FIT_NURBS_FROM_NORMALS, tolerance: float = 1e-10, max_epoch: int = 400,
                  device: torch.device | None = None) -> NURBSSurfaces:
        """Fit one NURBS surface to ``surface_points`` / ``surface_normals`` ``[N,4]`` (surface_generator.py:71-223); returns
        ``NURBSSurfaces`` with control points ``[1,1,nu,nv,3]``.

        ``torch.optim.Adam`` / ``artist_amd.optim.Adam`` with no scheduler or a ``ReduceLROnPlateau`` run as one launch;
        the scheduler's ``best`` / ``num_bad_epochs`` / ``cooldown_counter`` are read in and written back, the optimiser's
        parameter group is replaced by one holding the fitted control points, as the reference leaves them.  Any other
        optimiser or scheduler is stepped in a host loop over the fused loss-and-gradient kernel."""
        method = _check_method(fit_method)
        dev = _require_cuda(surface_points, surface_normals)
        if surface_points.dim() != 2 or surface_points.shape[1] != 4 or surface_normals.shape != surface_points.shape:
            raise ValueError(f"surface points and normals must be [N, 4], got {tuple(surface_points.shape)} and "
                             f"{tuple(surface_normals.shape)}")
        adam, sched = adam_hyperparameters(optimizer), plateau_hyperparameters(scheduler)
        prep = self.prepare(surface_points.unsqueeze(0))
        targets = prep.points if method == 0 else _f32c(surface_normals.unsqueeze(0))
        (nu, nv) = self._n_cp
        if adam is None or sched is None:
            return self._fit_generic(prep, targets, method, optimizer, scheduler, tolerance, max_epoch)
        state = _FitState(prep.initial_control_points.clone(), adam["lr"], sched)
        run_epochs(prep, state, targets, method, int(max_epoch) + 1, tolerance, max_epoch, adam, sched)
        surfaces = self._surfaces(state.control_points.reshape(1, 1, nu, nv, 3))
        surfaces.fit_state = state
        if optimizer is not None:
            optimizer.param_groups.clear()
            optimizer.add_param_group({"params": surfaces.control_points.requires_grad_()})
        if scheduler is not None or optimizer is not None:
            lr, best = (float(x) for x in state.f64[0].tolist())                     # (one read-back: the caller's objects)
            _, num_bad, cooldown_counter, epochs_run, _ = state.i32[0].tolist()
            if optimizer is not None:
                optimizer.param_groups[0]["lr"] = lr
            if scheduler is not None:
                scheduler.best, scheduler.num_bad_epochs, scheduler.cooldown_counter = best, num_bad, cooldown_counter
                scheduler.last_epoch += epochs_run
                scheduler._last_lr = [lr]
        return surfaces

    def _fit_generic(self, prep: _Prepared, targets, method, optimizer, scheduler, tolerance, max_epoch) -> NURBSSurfaces:
        (nu, nv) = self._n_cp
        surfaces = self._surfaces(prep.initial_control_points.clone().reshape(1, 1, nu, nv, 3))
        optimizer.param_groups.clear()
        optimizer.add_param_group({"params": surfaces.control_points.requires_grad_()})
        loss, epoch = torch.inf, 0
        while loss > tolerance and epoch <= max_epoch:
            optimizer.zero_grad()
            loss = _FitLoss.apply(surfaces.control_points.reshape(1, nu, nv, 3), prep, targets, method).sum()
            loss.backward()
            optimizer.step()
            if scheduler:
                if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
                    scheduler.step(loss.abs().mean().detach())
                else:
                    scheduler.step()
            if epoch % 100 == 0:
                log.info(f"Epoch: {epoch}, Loss: {loss.abs().mean().item()}, LR: {optimizer.param_groups[0]['lr']}.")
            epoch += 1
        return surfaces

    def generate_fitted_surface_config(self, heliostat_name: str, facet_translation_vectors: torch.Tensor, canting: torch.Tensor,
                                       surface_points_with_facets_list: list[torch.Tensor],
                                       surface_normals_with_facets_list: list[torch.Tensor], optimizer: torch.optim.Optimizer,
                                       scheduler=None, deflectometry_step_size: int = 100,
                                       fit_method: str = FIT_NURBS_FROM_NORMALS, tolerance: float = 1e-10, max_epoch: int = 400,
                                       device: torch.device | None = None, independent_facets: bool = True) -> list[FittedFacet]:
        """Fitted control points per facet (surface_generator.py:225-376): the facets' point and normal lists are truncated to
        the shortest facet, strided by ``deflectometry_step_size``, converted to 4D and fitted; the facet translation is added
        to the fitted net (zero translations for the point-cloud method, which learns them).  Returns a list of
        :class:`FittedFacet` - plain data in place of the reference's ``SurfaceConfig``.  The default stride of 100 is the
        reference's (an eager fit is slow); here ``deflectometry_step_size=1`` - every measured point, up to 2^20 per facet -
        is one launch like any other, with the same ordered sums (cost: DESIGN.md 4.7).

        Scheduler state: the reference passes one scheduler object to every facet's fit in turn, so ``best`` /
        ``num_bad_epochs`` of a ``ReduceLROnPlateau`` carry over from one facet into the next.  Here, by default
        (``independent_facets=True``) or without a scheduler, all facets are fitted at once, each with fresh scheduler
        state; ``independent_facets=False`` keeps the reference's facet-after-facet order with the shared state."""
        method = _check_method(fit_method)
        log.info("Beginning generation of the fitted surface configuration.")
        n_points = min(t.shape[0] for t in surface_points_with_facets_list)
        n_normals = min(t.shape[0] for t in surface_normals_with_facets_list)
        points = torch.stack([t[:n_points] for t in surface_points_with_facets_list])[:, ::deflectometry_step_size]
        normals = torch.stack([t[:n_normals] for t in surface_normals_with_facets_list])[:, ::deflectometry_step_size]
        dev = _require_cuda(points, normals)
        if points.shape[-1] != 3 or normals.shape[-1] != 3:
            raise ValueError(f"Expected 3D points and directions but got {tuple(points.shape)} and {tuple(normals.shape)}!")
        if method == 0:
            facet_translation_vectors = torch.zeros(facet_translation_vectors.shape, device=dev)
        points = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1)
        normals = torch.cat([normals, torch.zeros_like(normals[..., :1])], dim=-1)
        log.info(f"Generating NURBS surface for heliostat: {heliostat_name}.")
        fused = adam_hyperparameters(optimizer) is not None and plateau_hyperparameters(scheduler) is not None
        if fused and (scheduler is None or independent_facets):
            surfaces, _, _ = self.fit_nurbs_batch(points, normals, None, optimizer, scheduler, fit_method, tolerance, max_epoch)
            nets = surfaces.control_points[:, 0]
        else:
            nets = torch.stack([self.fit_nurbs(points[i], normals[i], optimizer, scheduler, fit_method, tolerance, max_epoch)
                                .control_points[0, 0].detach() for i in range(points.shape[0])])
        facets = [FittedFacet(facet_key=f"facet_{i + 1}",
                              control_points=(nets[i] + facet_translation_vectors[i, :3]).detach(), degrees=self.degrees,
                              translation_vector=facet_translation_vectors[i], canting=canting[i])
                  for i in range(points.shape[0])]
        log.info("Surface configuration based on fit complete!")
        return facets

    def generate_ideal_surface_config(self, facet_translation_vectors: torch.Tensor, canting: torch.Tensor,
                                      device: torch.device | None = None) -> list[FittedFacet]:
        """Flat, canted control nets per facet (surface_generator.py:378-436) as a list of :class:`FittedFacet`."""
        device = canting.device if device is None else device
        control_points = create_planar_nurbs_control_points(self.number_of_control_points, canting, device=device)
        return [FittedFacet(facet_key=f"facet_{i + 1}", control_points=control_points[i], degrees=self.degrees,
                            translation_vector=facet_translation_vectors[i], canting=canting[i])
                for i in range(facet_translation_vectors.shape[0])]
