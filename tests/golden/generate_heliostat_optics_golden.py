#!/usr/bin/env python3
"""Golden vectors for per-heliostat reflectivity and extinction (runs ONLY in the build container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  The reference's ``trace_rays`` takes ONE ``ray_extinction_factor`` and ONE
``mirror_reflectivity`` for the whole field (artist/raytracing/heliostat_ray_tracer.py:482-487), so it pins a per-heliostat
pair exactly: the field is traced once per heliostat ``h`` with the scalars ``(eps_h, rho_h)`` and row ``h`` is kept.  The
import recipe, the scenario builder and the helpers are those of generate_golden.py (imported, unchanged).

Two small fields in the style of ``small_blocking``, two planar targets each, 64 x 64 bitmaps, 8 x 8 points per facet, 6 rays:

* ``off`` (no blocking): two heliostats, EACH ACTIVATED TWICE - four active heliostat samples with their own rays, factors and
  targets.  The reference's sampler needs a uniform replica count (artist/raytracing/sampling.py:133-135: with the mask
  1 2 1 it drops the last sample), so "one heliostat twice, the others once" cannot be traced by it.
* ``on`` (blocking): the column of four heliostats of ``small_blocking``, each active once.  With blocking the reference
  cannot trace a heliostat that is activated twice at all (heliostat_ray_tracer.py:174 assigns the active surfaces to
  ``surfaces[mask]``, one row per DISTINCT heliostat).  The product order of the intensities includes ``(1 - blocked)``.

Per case: all inputs with the distortions stored, the per-heliostat bitmaps, the three factors (the intercept factor counts
``intensity > 0``, so it is 0 for the row whose reflectivity is 0), the per-target sums, the bitmaps with the scalars (0, 1),
and the autograd gradient of ``sum(weights * flux)`` with respect to the aligned surface points - the sum over ``h`` of the
gradient of row ``h``'s share in the trace with heliostat ``h``'s scalars, rectangles in the graph as in ``small_blocking``.
Everything in fp32, and flux, per-target sums and gradient once more from an fp64 run on the fp32 run's rays (the yardstick).

Usage:  python tests/golden/generate_heliostat_optics_golden.py      (writes tests/golden/heliostat_optics.npz)
"""
from __future__ import annotations

import generate_golden as g      # the import recipe and the scenario builder; through it the reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

npy, CPU = g.npy, g.CPU

TARGETS = dict(target_centers=[[0.0, 0.0, 55.0, 1.0], [1.0, 0.0, 47.0, 1.0]],
               target_normals=[[0.0, 1.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], target_dims=[[8.0, 8.0], [6.0, 5.0]])
COMMON = dict(n_cp=(6, 6), degrees=(3, 3), n_eval=8, n_rays=6, resolution=[64, 64], curvature=1e-3, **TARGETS)
CASES = {
    "off": dict(COMMON, n_heliostats=2, active_mask=[2, 2], blocking=False, target_idx=[0, 1, 1, 0],
                positions=[[-20.0, 90.0, 0.0, 1.0], [35.0, 120.0, 0.0, 1.0]]),
    "on": dict(COMMON, n_heliostats=4, active_mask=[1, 1, 1, 1], blocking=True, target_idx=[0, 1, 1, 0],
               positions=[[0.0, 140.0, 0.0, 1.0], [0.0, 137.0, 0.0, 1.0], [1.2, 134.0, 0.0, 1.0], [30.0, 120.0, 0.0, 1.0]]),
}
EXTINCTION = [0.0, 0.3, 0.12, 0.05]          # eps_h, distinct, in [0, 0.3]
REFLECTIVITY = [1.0, 0.5, 0.0, 0.85]         # rho_h, distinct, in [0.5, 1] and one zero: the row without weight
WEIGHT_SEED = 1234


def run(case, dtype, distortions_f32=None):
    b = g.build(case, dtype)
    scenario, group = b["scenario"], b["group"]
    mask = torch.tensor(case["active_mask"], dtype=torch.int32)
    H = int(mask.sum())
    target_idx = torch.tensor(case["target_idx"], dtype=torch.int64)
    incident = torch.nn.functional.normalize(torch.tensor([[0.0, 1.0, 0.0, 0.0]] * H, dtype=dtype), dim=1)
    res = torch.tensor(case["resolution"])
    group.activate_heliostats(active_heliostats_mask=mask, device=CPU)
    aim = scenario.solar_tower.get_centers_of_target_areas(target_area_indices=target_idx, device=CPU)
    with torch.no_grad():
        orientation = group.kinematics.incident_ray_directions_to_orientations(
            incident_ray_directions=incident, aim_points=aim, device=CPU)
        points = group.active_surface_points @ orientation.transpose(1, 2)
        normals = group.active_surface_normals @ orientation.transpose(1, 2)
    points = points.detach().clone().requires_grad_(True)
    normals = normals.detach().clone()
    group.active_surface_points, group.active_surface_normals = points, normals

    captured = []
    builder = g.ref_blocking.create_blocking_primitives_rectangles_by_index

    def capturing_builder(*a, **k):
        captured.append(builder(*a, **k))
        return captured[-1]

    g.ref_blocking.create_blocking_primitives_rectangles_by_index = capturing_builder
    try:
        rt = g.HeliostatRayTracer(scenario=scenario, heliostat_group=group, blocking_active=case["blocking"], batch_size=100,
                                  random_seed=7, bitmap_resolution=res, dni=None)
        assert list(rt.distortions_sampler) == list(range(H)), "the reference's sampler drops a heliostat sample"
        du32, de32 = rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e
        if distortions_f32 is not None:
            du32, de32 = distortions_f32
        rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e = du32.to(dtype), de32.to(dtype)
        weights = torch.rand((H, int(res[0]), int(res[1])), generator=torch.Generator().manual_seed(WEIGHT_SEED),
                             dtype=torch.float32).to(dtype)

        def trace(eps, rho):
            return rt.trace_rays(incident_ray_directions=incident, active_heliostats_mask=mask, target_area_indices=target_idx,
                                 ray_extinction_factor=eps, mirror_reflectivity=rho, device=CPU)

        rows, factors = [], []
        gradient = torch.zeros_like(points)
        for h in range(H):
            flux, intercept, on_target, blocking = trace(EXTINCTION[h], REFLECTIVITY[h])
            (gradient_h,) = torch.autograd.grad((flux[h] * weights[h]).sum(), points, allow_unused=True,
                                                 retain_graph=True)     # (the rectangles' graph is the constructor's: shared)
            if gradient_h is not None:
                gradient += gradient_h
            rows.append(flux[h].detach())
            factors.append(torch.stack((intercept[h], on_target[h], blocking[h])))
        flux = torch.stack(rows)
        factors = torch.stack(factors, dim=1)                                   # [3,H]
        with torch.no_grad():
            per_target = rt.get_bitmaps_per_target(flux, target_idx, device=CPU)
            flux_unit = trace(0.0, 1.0)[0]
    finally:
        g.ref_blocking.create_blocking_primitives_rectangles_by_index = builder
    out = dict(aligned_points=npy(points), aligned_normals=npy(normals), incident=npy(incident), target_idx=npy(target_idx),
               active_mask=npy(mask), target_centers=npy(b["planar"].centers), target_normals=npy(b["planar"].normals),
               target_dims=npy(b["planar"].dimensions), resolution=npy(res), ray_magnitude=np.float64(float(rt.ray_magnitude)),
               distortions_u=npy(du32), distortions_e=npy(de32), loss_weights=npy(weights), flux=npy(flux), flux_unit=npy(flux_unit),
               intercept=npy(factors[0]), on_target=npy(factors[1]), blocking=npy(factors[2]), per_target=npy(per_target),
               grad_aligned_points=npy(gradient))
    if case["blocking"]:
        corners, spans, pnormals = captured[-1]
        out.update(prim_corners=npy(corners), prim_spans=npy(spans), prim_normals=npy(pnormals),
                   blocking_surfaces=npy(rt.blocking_heliostat_surfaces_active))
    torch.set_default_dtype(torch.float32)
    return out, (du32, de32)


def main():
    arrays = dict(extinction=np.asarray(EXTINCTION, dtype=np.float32), reflectivity=np.asarray(REFLECTIVITY, dtype=np.float32),
                  weight_seed=np.int64(WEIGHT_SEED))
    for name, case in CASES.items():
        out32, drawn = run(case, torch.float32)
        out64, _ = run(case, torch.float64, distortions_f32=drawn)
        zero = REFLECTIVITY.index(0.0)
        assert not out32["flux"][zero].any() and out32["intercept"][zero] == 0 and out32["on_target"][zero] > 0
        assert all(np.isfinite(v).all() for v in out32.values() if np.asarray(v).dtype.kind == "f")
        assert (out32["flux"].sum(axis=(1, 2)) > 0).sum() == len(EXTINCTION) - 1, "a heliostat with weight misses its target"
        if case["blocking"]:
            print(f"{name}: unblocked fractions {out32['blocking']}")
            assert out32["blocking"].min() < 0.9, "the case does not block"
        for key, value in out32.items():
            arrays[f"{name}_{key}"] = value
        for key in ("flux", "per_target", "grad_aligned_points"):
            arrays[f"{name}_{key}_f64"] = np.asarray(out64[key], dtype=np.float64)
            print(f"{name}: {key}: fp32 vs fp64 {rel_l2(out32[key], out64[key]):.2e}")
        print(f"{name}: intercept {out32['intercept']}, on target {out32['on_target']}")
    path = g.OUT_DIR / "heliostat_optics.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    print(f"wrote {path.name}: {size / 1024:.1f} KiB, keys={len(arrays)}")
    assert size < (1 << 20)


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


if __name__ == "__main__":
    main()
