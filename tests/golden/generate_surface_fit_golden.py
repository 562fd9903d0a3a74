#!/usr/bin/env python3
"""Fixtures of the NURBS surface fit (runs ONLY in the build container, like generate_golden.py, whose reference import recipe
it uses).

TEST INFRASTRUCTURE - not part of the product.  The measured deflectometry files are not available, so the point clouds are
synthetic and seeded (tests/surface_fit_ref.py::synthetic_facet: a canted, slightly paraboloidal 1.6 m x 1.3 m facet with a few
sinusoidal dents of ~1e-4 m at random non-grid positions, analytic unit normals).  Per case the REFERENCE's own
``SurfaceGenerator.fit_nurbs`` runs on the CPU with ``torch.optim.Adam(lr=1e-3)``, in fp32 and in fp64, once without a scheduler
and once with ``ReduceLROnPlateau(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")`` (the tutorial's scheduler with
a patience small enough for at least two reductions inside the run - asserted).

  surface_fit_<N>_<nu>x<nv>_d<p>_<method>.npz   N in {37, 800}; nets 5x5 / degree 2 and 10x10 / degree 3; both fit methods.
      ``points``, ``normals`` [N,4]; ``eval_points`` [N,2] (normalised, fp32), ``cp_initial``; ``record_epochs``; and per
      scheduler tag t in {"none", "plateau"}: ``loss_<t>`` [E], ``lr_<t>`` [E] (the rate each epoch stepped with; fp64 run:
      ``lr64_<t>`` - asserted equal), ``epochs_run_<t>``, ``cp_<t>`` [R,nu,nv,3] and ``grad_<t>`` [R,nu,nv,3] at the recorded
      epochs (before that epoch's update), ``cp_final_<t>``, and the same from the fp64 run (``loss64_``, ``cp64_``, ``grad64_``,
      ``cp64_final_``).
  surface_fit_early_stop.npz    the 37-point 5x5 points case with ``tolerance`` set so that the reference stops early
      (``tolerance``, ``epochs_run``, ``cp_final``, ``loss``); fp32 and fp64 agree on the stop epoch (asserted).
  surface_fit_four_facets.npz   the reference's ``generate_fitted_surface_config`` on four facets of unequal length,
      ``scheduler=None``: ``points_<i>``, ``normals_<i>`` [n_i,3], ``translations``, ``canting``, ``step_size``, ``max_epoch``,
      ``control_points`` [4,nu,nv,3] (fp32) and ``control_points64``.

Usage:  PYTHONPATH=<repo root> python tests/golden/generate_surface_fit_golden.py
"""
from __future__ import annotations

import pathlib
import sys

import generate_golden as gg  # noqa: E402  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import surface_fit_ref as sfr  # noqa: E402

RECORD = [0, 1, 2, 10, 50]
MAX_EPOCH = 400
PLATEAU = dict(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")
CASES = [(n, net, deg, method) for n in (37, 800) for net, deg in ((5, 2), (10, 3)) for method in (sfr.POINTS, sfr.NORMALS)]
SEEDS = {37: 5, 800: 9}


def reference_fit(points, normals, net, deg, method, dtype, plateau, tolerance=1e-10, max_epoch=MAX_EPOCH):
    """The reference's fit_nurbs with a recording Adam; returns a dict like surface_fit_ref.fit."""
    from artist.scenario.surface_generator import SurfaceGenerator

    torch.set_default_dtype(dtype)
    try:
        log = dict(loss=[], lr=[], cp_at={}, grad_at={})

        class RecordingAdam(torch.optim.Adam):
            def step(self, closure=None):
                prm = self.param_groups[0]["params"][0]
                epoch = len(log["lr"])
                log["lr"].append(float(self.param_groups[0]["lr"]))
                log["cp_at"][epoch] = gg.npy(prm)[0, 0].copy()
                log["grad_at"][epoch] = gg.npy(prm.grad)[0, 0].copy()
                return super().step(closure)

        mse_forward = torch.nn.MSELoss.forward

        def recording_forward(self, a, b):
            out = mse_forward(self, a, b)
            log["loss"].append(float(out.detach()))
            return out

        torch.nn.MSELoss.forward = recording_forward
        try:
            gen = SurfaceGenerator(torch.tensor([net, net]), torch.tensor([deg, deg]), device=gg.CPU)
            opt = RecordingAdam([torch.zeros(1, requires_grad=True)], lr=1e-3)
            sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU) if plateau else None
            surf = gen.fit_nurbs(torch.from_numpy(points).to(dtype), torch.from_numpy(normals).to(dtype), opt, sched,
                                 fit_method=method, tolerance=tolerance, max_epoch=max_epoch, device=gg.CPU)
        finally:
            torch.nn.MSELoss.forward = mse_forward
        E = len(log["lr"])
        assert len(log["loss"]) == E
        return dict(loss=np.asarray(log["loss"]), lr=np.asarray(log["lr"]), epochs_run=E, cp=gg.npy(surf.control_points)[0, 0].copy(),
                    cp_at=log["cp_at"], grad_at=log["grad_at"])
    finally:
        torch.set_default_dtype(torch.float32)


def case_fixture(n, net, deg, method):
    points, normals = sfr.synthetic_facet(n, SEEDS[n])
    out = dict(points=points, normals=normals, degrees=np.asarray([deg, deg]), net=np.asarray([net, net]), max_epoch=np.int64(MAX_EPOCH))
    ev = torch.from_numpy(points[:, :2].copy())
    from artist.geometry import coordinates
    out["eval_points"] = gg.npy(coordinates.normalize_points(ev))
    for tag, plateau in (("none", False), ("plateau", True)):
        r32 = reference_fit(points, normals, net, deg, method, torch.float32, plateau)
        r64 = reference_fit(points, normals, net, deg, method, torch.float64, plateau)
        assert r32["epochs_run"] == r64["epochs_run"] == MAX_EPOCH + 1, (r32["epochs_run"], r64["epochs_run"])
        assert np.array_equal(r32["lr"], r64["lr"]), f"fp32 and fp64 reference runs disagree on the lr schedule: {n} {net} {method} {tag}"
        if plateau:
            drops = int((np.diff(r32["lr"]) < 0).sum())
            assert drops >= 2, f"only {drops} lr reductions: {n} {net} {method}"
        rec = RECORD + [r32["epochs_run"] - 1]
        out["record_epochs"] = np.asarray(rec)
        out["cp_initial"] = r32["cp_at"][0].astype(np.float32)
        for key, r in (("", r32), ("64", r64)):
            out[f"loss{key}_{tag}"] = r["loss"]
            out[f"lr{key}_{tag}"] = r["lr"]
            out[f"cp{key}_{tag}"] = np.stack([r["cp_at"][e] for e in rec])
            out[f"grad{key}_{tag}"] = np.stack([r["grad_at"][e] for e in rec])
            out[f"cp{key}_final_{tag}"] = r["cp"]
        out[f"epochs_run_{tag}"] = np.int64(r32["epochs_run"])
    return out


def early_stop_fixture():
    n, net, deg, method = 37, 5, 2, sfr.POINTS
    points, normals = sfr.synthetic_facet(n, SEEDS[n])
    full32 = reference_fit(points, normals, net, deg, method, torch.float32, False)
    full64 = reference_fit(points, normals, net, deg, method, torch.float64, False)
    # a tolerance halfway (geometrically) between two consecutive losses around epoch 60, where both runs still fall clearly
    k = 60
    tol = float(np.sqrt(full32["loss"][k] * full32["loss"][k - 1]))
    for full in (full32, full64):
        assert full["loss"][k] < tol * 0.999 and full["loss"][k - 1] > tol * 1.001 and np.all(full["loss"][:k] > tol), "pick another epoch"
    r32 = reference_fit(points, normals, net, deg, method, torch.float32, False, tolerance=tol)
    r64 = reference_fit(points, normals, net, deg, method, torch.float64, False, tolerance=tol)
    assert r32["epochs_run"] == r64["epochs_run"] == k + 1 < MAX_EPOCH, (r32["epochs_run"], r64["epochs_run"])
    return dict(points=points, normals=normals, degrees=np.asarray([deg, deg]), net=np.asarray([net, net]), tolerance=np.float64(tol),
                max_epoch=np.int64(MAX_EPOCH), epochs_run=np.int64(r32["epochs_run"]), cp_final=r32["cp"], cp64_final=r64["cp"],
                loss=r32["loss"], loss64=r64["loss"])


def four_facets_fixture():
    from artist.scenario.surface_generator import SurfaceGenerator
    from artist.util import constants

    lengths, step, max_epoch, net, deg = [372, 405, 391, 388], 10, 100, 10, 3
    out = dict(step_size=np.int64(step), max_epoch=np.int64(max_epoch), degrees=np.asarray([deg, deg]), net=np.asarray([net, net]),
               lengths=np.asarray(lengths))
    pts, nrm = [], []
    for i, length in enumerate(lengths):
        p, nn = sfr.synthetic_facet(length, 100 + i)
        out[f"points_{i}"], out[f"normals_{i}"] = p[:, :3].copy(), nn[:, :3].copy()
        pts.append(p[:, :3].copy())
        nrm.append(nn[:, :3].copy())
    transl = np.asarray([[-0.8, 0.65, 0.04, 0.0], [0.8, 0.65, 0.04, 0.0], [-0.8, -0.65, 0.04, 0.0], [0.8, -0.65, 0.04, 0.0]], dtype=np.float32)
    canting = np.tile(np.asarray([[[0.8, 0.0, 0.0, 0.0], [0.0, 0.65, 0.0, 0.0]]], dtype=np.float32), (4, 1, 1))
    out["translations"], out["canting"] = transl, canting
    for key, dtype in (("", torch.float32), ("64", torch.float64)):
        torch.set_default_dtype(dtype)
        try:
            gen = SurfaceGenerator(torch.tensor([net, net]), torch.tensor([deg, deg]), device=gg.CPU)
            opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
            cfg = gen.generate_fitted_surface_config(
                "synthetic", torch.from_numpy(transl).to(dtype), torch.from_numpy(canting).to(dtype),
                [torch.from_numpy(a).to(dtype) for a in pts], [torch.from_numpy(a).to(dtype) for a in nrm], opt, None,
                deflectometry_step_size=step, fit_method=constants.fit_nurbs_from_normals, max_epoch=max_epoch, device=gg.CPU)
        finally:
            torch.set_default_dtype(torch.float32)
        out[f"control_points{key}"] = np.stack([gg.npy(f.control_points) for f in cfg.facet_list])
    return out


def main():
    for n, net, deg, method in CASES:
        gg.save(f"surface_fit_{n}_{net}x{net}_d{deg}_{method}", case_fixture(n, net, deg, method))
    gg.save("surface_fit_early_stop", early_stop_fixture())
    gg.save("surface_fit_four_facets", four_facets_fixture())


if __name__ == "__main__":
    main()
