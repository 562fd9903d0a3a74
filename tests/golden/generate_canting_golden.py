#!/usr/bin/env python3
"""Fixture of the canting gradients (runs ONLY in the build container, like generate_golden.py, whose reference import recipe
and helpers it uses).

TEST INFRASTRUCTURE - not part of the product.  Writes tests/golden/canting.npz:

  Per case <c> in CASES, from the reference's own ``NURBSSurfaces.calculate_surface_points_and_normals(evaluation_points,
  canting, facet_translations)`` (artist/nurbs/surfaces.py:475-689) with ``canting`` / ``facet_translations`` / control points
  as autograd leaves, activated by ``repeat_interleave(mask)`` as ``HeliostatGroup.activate_heliostats`` does
  (artist/field/heliostat_group.py:258-272):
    inputs      <c>_degrees, <c>_cp [Hb,F,nu,nv,3], <c>_uv [H,F,M,2], <c>_canting [Hb,F,2,4], <c>_translations [Hb,F,4],
                <c>_mask [Hb] (H = mask.sum()), <c>_wp, <c>_wn [H,F,M,4] (seeded upstream weights)
    results     in fp32 (<c>_<key>) and fp64 (<c>_<key>_f64, the same fp32 inputs upcast): points, normals, the un-canted
                points0 / normals0 (canting = None), and grad_canting, grad_translations, grad_cp of
                ((points * wp).sum() + (normals * wn).sum()) w.r.t. the three leaves
    <c>_grads_finite   1 when every reference gradient is finite in both precisions; 0 marks the case forward-only
  Direct ``perform_canting`` calls (artist/geometry/transforms.py:276-347) per case, on random data whose w is neither 0
  nor 1: <c>_pc_data, <c>_pc_w, <c>_pc_fwd, <c>_pc_inv, and for the inverse the gradients of (pc_inv * pc_w).sum():
  <c>_pc_inv_grad_canting, <c>_pc_inv_grad_data (+ _f64 each).

  descent_*   the end-to-end descent check of tests/test_gpu_canting.py through the reference's own pipeline on the CPU (NURBS
              -> alignment -> HeliostatRayTracer.trace_rays -> squared pixel loss, the scenario ``smoke()`` builds): the
              fraction of the loss that the first-order prediction of the step promises (descent_fraction) and the
              reference's ratio measured / predicted decrease at that step (descent_ref_ratio), plus the tilt and the facet.

Usage:  PYTHONPATH=<repo root> python tests/golden/generate_canting_golden.py
"""
from __future__ import annotations

import generate_golden as gg  # noqa: E402  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402
from artist.geometry.transforms import perform_canting  # noqa: E402
from artist.nurbs import NURBSSurfaces  # noqa: E402
from artist.nurbs.utils import create_nurbs_evaluation_grid, create_planar_nurbs_control_points  # noqa: E402
from artist.raytracing.heliostat_ray_tracer import HeliostatRayTracer  # noqa: E402

CPU = gg.CPU
E_LEN, N_LEN = 0.8025, 0.6375


def _planar_net(canting, n_cp, z_noise, curvature, gen):
    """[Hb,F,nu,nv,3] planar nets sized by the canting vectors, with a little noise and a paraboloid on z."""
    Hb = canting.shape[0]
    cp = torch.stack([create_planar_nurbs_control_points(torch.tensor(n_cp), canting[h], device=CPU) for h in range(Hb)]).float()
    if z_noise:
        cp[..., 2] += z_noise * torch.randn(cp[..., 2].shape, generator=gen)
    if curvature:
        cp[..., 2] += curvature * (cp[..., 0] ** 2 + cp[..., 1] ** 2)
    return cp


def _canting(Hb, F, gen, mrad=3e-3):
    """Facet vectors of real length along east / north with mrad-scale z components."""
    c = torch.zeros(Hb, F, 2, 4)
    c[..., 0, 0], c[..., 1, 1] = E_LEN, N_LEN
    c[..., 0, 2] = E_LEN * mrad * (2 * torch.rand(Hb, F, generator=gen) - 1)
    c[..., 1, 2] = N_LEN * mrad * (2 * torch.rand(Hb, F, generator=gen) - 1)
    return c


def _translations(Hb, F, gen):
    base = torch.tensor(gg.FACET_TRANSLATIONS)[torch.arange(F) % 4]
    t = base.unsqueeze(0).repeat(Hb, 1, 1).clone()
    t[..., 2] = 0.02 * torch.rand(Hb, F, generator=gen)
    return t


def make_cases():
    gen = torch.Generator().manual_seed(23)
    cases = {}
    # (a) one heliostat, two facets, 5 x 7 points, degree 3, 6 x 6 net
    cant = _canting(1, 2, gen)
    cases["a"] = dict(degrees=(3, 3), grid=(5, 7), canting=cant, translations=_translations(1, 2, gen),
                      cp=_planar_net(cant, (6, 6), 1e-3, 2e-3, gen), mask=[1])
    # (b) three heliostats, four facets, 8 x 8 points, degree 2, 5 x 5 net; heliostat 1's n is not orthogonal to its e
    cant = _canting(3, 4, gen)
    cant[1, :, 1, 0] = 0.15 * N_LEN * (1 + torch.arange(4.0))      # n leans into e by 0.15 .. 0.6 of its length
    cases["b"] = dict(degrees=(2, 2), grid=(8, 8), canting=cant, translations=_translations(3, 4, gen),
                      cp=_planar_net(cant, (5, 5), 1e-3, 1e-3, gen), mask=[1, 1, 1])
    # (c) exactly flat facets
    cant = _canting(1, 4, gen)
    cases["c"] = dict(degrees=(3, 3), grid=(4, 4), canting=cant, translations=_translations(1, 4, gen),
                      cp=_planar_net(cant, (6, 6), 0.0, 0.0, gen), mask=[1])
    # (d) two heliostats, the second listed twice: the gradients of its replicas add up in its row
    cant = _canting(2, 4, gen)
    cases["d"] = dict(degrees=(3, 3), grid=(6, 6), canting=cant, translations=_translations(2, 4, gen),
                      cp=_planar_net(cant, (6, 6), 1e-3, 2e-3, gen), mask=[1, 2])
    # (e) facet 1 degenerate: n parallel to e (e x n = 0 exactly, both clamps of the basis are met)
    cant = _canting(1, 2, gen)
    cant[0, 1, 0] = torch.tensor([E_LEN, 0.0, 0.0, 0.0])
    cant[0, 1, 1] = torch.tensor([N_LEN, 0.0, 0.0, 0.0])
    cases["e"] = dict(degrees=(3, 3), grid=(4, 5), canting=cant, translations=_translations(1, 2, gen),
                      cp=_planar_net(_canting(1, 2, gen), (6, 6), 1e-3, 2e-3, gen), mask=[1])
    for case in cases.values():
        mask = torch.tensor(case["mask"], dtype=torch.int32)
        H, F = int(mask.sum()), case["canting"].shape[1]
        uv = create_nurbs_evaluation_grid(torch.tensor(case["grid"]), device=CPU).float()
        M = uv.shape[0]
        case.update(mask=mask, uv=uv[None, None].expand(H, F, -1, -1).contiguous(),
                    wp=torch.rand(H, F, M, 4, generator=gen) - 0.5, wn=torch.rand(H, F, M, 4, generator=gen) - 0.5,
                    pc_data=torch.randn(case["canting"].shape[0], F, 9, 4, generator=gen) * torch.tensor([1.0, 1.0, 0.1, 1.0])
                    + torch.tensor([0.0, 0.0, 0.0, 0.5]),
                    pc_w=torch.rand(case["canting"].shape[0], F, 9, 4, generator=gen) - 0.5)
    return cases


def run_case(case, dtype):
    torch.set_default_dtype(dtype)
    rep = lambda t: t.repeat_interleave(case["mask"], dim=0)  # noqa: E731
    cp, cant, tr = (case[k].to(dtype).clone().requires_grad_(True) for k in ("cp", "canting", "translations"))
    degrees, uv = torch.tensor(case["degrees"]), case["uv"].to(dtype)
    pts, nrm = NURBSSurfaces(degrees, rep(cp), device=CPU).calculate_surface_points_and_normals(uv, rep(cant), rep(tr), device=CPU)
    ((pts * case["wp"].to(dtype)).sum() + (nrm * case["wn"].to(dtype)).sum()).backward()
    with torch.no_grad():
        pts0, nrm0 = NURBSSurfaces(degrees, rep(cp).detach(), device=CPU).calculate_surface_points_and_normals(uv, None, None, device=CPU)
    out = dict(points=pts, normals=nrm, points0=pts0, normals0=nrm0, grad_canting=cant.grad, grad_translations=tr.grad,
               grad_cp=cp.grad)
    # direct calls
    data = case["pc_data"].to(dtype)
    c2 = case["canting"].to(dtype).clone().requires_grad_(True)
    d2 = data.clone().requires_grad_(True)
    out["pc_fwd"] = perform_canting(case["canting"].to(dtype), data, device=CPU)
    inv = perform_canting(c2, d2, inverse=True, device=CPU)
    (inv * case["pc_w"].to(dtype)).sum().backward()
    out.update(pc_inv=inv, pc_inv_grad_canting=c2.grad, pc_inv_grad_data=d2.grad)
    torch.set_default_dtype(torch.float32)
    return {k: gg.npy(v) for k, v in out.items()}


# ---- the end-to-end descent check through the reference's pipeline -----------------------------------------------------------
DESCENT_CASE = dict(n_heliostats=2, n_cp=(6, 6), degrees=(3, 3), n_eval=16, n_rays=8, resolution=[64, 64], **gg.RECEIVER)
DESCENT_TILT, DESCENT_FACET = 2e-3, (0, 1)


def descent_reference():
    b = gg.build(DESCENT_CASE, torch.float32)
    torch.set_default_dtype(torch.float32)
    scenario, group = b["scenario"], b["group"]
    degrees, cp, uv_full, canting_h, transl_h = b["nurbs_inputs"]
    mask = torch.ones(2, dtype=torch.int32)
    tix = torch.zeros(2, dtype=torch.int64)
    incident = torch.tensor([[0.0, 1.0, 0.0, 0.0]]).repeat(2, 1)
    group.activate_heliostats(active_heliostats_mask=mask, device=CPU)
    aim = scenario.solar_tower.get_centers_of_target_areas(target_area_indices=tix, device=CPU)
    with torch.no_grad():
        orientation = group.kinematics.incident_ray_directions_to_orientations(incident_ray_directions=incident, aim_points=aim,
                                                                                device=CPU)

    def flux_of(canting):
        pts, nrm = NURBSSurfaces(degrees, cp, device=CPU).calculate_surface_points_and_normals(uv_full, canting, transl_h, device=CPU)
        group.active_surface_points = pts.reshape(2, -1, 4) @ orientation.transpose(1, 2)
        group.active_surface_normals = nrm.reshape(2, -1, 4) @ orientation.transpose(1, 2)
        rt = HeliostatRayTracer(scenario=scenario, heliostat_group=group, blocking_active=False, batch_size=100, random_seed=7,
                                bitmap_resolution=torch.tensor([64, 64]))
        return rt.trace_rays(incident_ray_directions=incident, active_heliostats_mask=mask, target_area_indices=tix, device=CPU)[0]

    with torch.no_grad():
        target = flux_of(canting_h)
    h, f = DESCENT_FACET
    tilted = canting_h.clone()
    tilted[h, f, 1, 2] += DESCENT_TILT * float(torch.linalg.norm(canting_h[h, f, 1]))
    tilted.requires_grad_(True)
    loss = ((flux_of(tilted) - target) ** 2).sum()
    (grad,) = torch.autograd.grad(loss, tilted)
    fraction = 0.01
    while True:
        eta = fraction * float(loss) / float((grad * grad).sum())
        with torch.no_grad():
            stepped = ((flux_of(tilted.detach() - eta * grad) - target) ** 2).sum()
        ratio = float(loss - stepped) / (fraction * float(loss))
        print(f"descent: fraction {fraction:g}, eta {eta:.3e}, loss {float(loss):.6e} -> {float(stepped):.6e}, ratio {ratio:.4f}")
        if 0.8 <= ratio <= 1.2 or fraction < 1e-4:
            break
        fraction *= 0.5
    return dict(descent_fraction=np.float64(fraction), descent_ref_ratio=np.float64(ratio), descent_ref_eta=np.float64(eta),
                descent_ref_loss=np.float64(float(loss)), descent_tilt=np.float64(DESCENT_TILT),
                descent_facet=np.asarray(DESCENT_FACET, dtype=np.int64))


def main():
    out = {}
    for name, case in make_cases().items():
        for key in ("cp", "uv", "canting", "translations", "mask", "wp", "wn", "pc_data", "pc_w"):
            out[f"{name}_{key}"] = gg.npy(case[key])
        out[f"{name}_degrees"] = np.asarray(case["degrees"], dtype=np.int64)
        r32, r64 = run_case(case, torch.float32), run_case(case, torch.float64)
        finite = all(np.isfinite(r[k]).all() for r in (r32, r64) for k in r if "grad" in k)
        out[f"{name}_grads_finite"] = np.int64(1 if finite else 0)
        print(f"case {name}: gradients finite: {finite}")
        for k in r32:
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64, k
            out[f"{name}_{k}"], out[f"{name}_{k}_f64"] = r32[k], r64[k]
            if "grad" in k and finite:
                d = np.linalg.norm(r32[k] - r64[k]) / max(np.linalg.norm(r64[k]), 1e-300)
                print(f"   {k}: fp32 vs fp64 rel-L2 {d:.2e}")
    out.update(descent_reference())
    assert not any(v.dtype == object for v in out.values())
    gg.save("canting", out)


if __name__ == "__main__":
    main()
