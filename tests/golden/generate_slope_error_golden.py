#!/usr/bin/env python3
"""Golden vectors for mirror slope errors (runs ONLY in the build container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  The tilt of the normals (``artist_amd.optics.tilt_normals``) is
the project's own formula; the reference pins what stands around it: its ``trace_rays`` on the tilted and aligned normals, and
its autograd from ``sum(weights * flux)`` back through the trace, the alignment ``@ orientation^T`` and the tilt to sigma.  The
import recipe, the scenario builder and the helpers are those of generate_golden.py (imported, unchanged); the two fields,
``off`` (two heliostats each activated twice, no blocking) and ``on`` (the blocking column of four), are those of
generate_heliostat_optics_golden.py - ``off`` moved closer to the tower, see ``CASES`` - with 8 x 8 points per facet, 6 rays,
64 x 64 bitmaps and two planar targets.

Per case: zeta ``[N, P, 2]`` (``torch.randn`` on the CPU, seeded; one realisation per heliostat of the group, shared by its
activations), sigma ``[N]``, the group's nets and canonical surfaces, the orientations, canonical and aligned points and normals of
the active heliostats, the distortions; flux, per-target sums and the three factors; the gradients of ``sum(weights * flux)``
with respect to sigma ``[N]``, to the slopes ``sigma_h * zeta`` as a leaf ``[H, P, 2]`` and to the aligned points.  Everything in
fp32, and flux, per-target sums and the gradients once more from an fp64 run on the fp32 run's rays and zeta (the yardstick).

The loss curves (``off``, fp64): the mean squared pixel difference to the bitmaps at the true sigma, along each sigma axis at 13
values over [0, 3] mrad with the other sigma at its truth.  Each curve must fall strictly to 0 at the truth and rise strictly
beyond it: the problem the learning test poses is identifiable.

Usage:  python tests/golden/generate_slope_error_golden.py      (writes tests/golden/slope_error.npz)
"""
from __future__ import annotations

import generate_golden as g      # the import recipe and the scenario builder; through it the reference

import numpy as np  # noqa: E402
import torch  # noqa: E402
from generate_heliostat_optics_golden import CASES as OPTICS_CASES, rel_l2  # noqa: E402

from artist_amd.optics import tilt_normals  # noqa: E402

npy, CPU = g.npy, g.CPU

# ``off`` stands closer to the tower than in generate_heliostat_optics_golden.py (there 90 m and 120 m north): at that range
# 3 mrad of slope throw a ray further than the image is wide, the loss curve along sigma_1 flattens beyond 1.5 mrad and is no
# longer monotone (0.11677 -> 0.11658), and the reference's own fp32 gradient is 6e-2 from its fp64 one.  At 60 m and 75 m both
# curves are strictly monotone and the yardstick is 1e-4.
CASES = dict(off=dict(OPTICS_CASES["off"], positions=[[-12.0, 60.0, 0.0, 1.0], [20.0, 75.0, 0.0, 1.0]]), on=OPTICS_CASES["on"])
SIGMA = dict(off=[1.5e-3, 0.5e-3], on=[1.5e-3, 0.5e-3, 1.0e-3, 2.0e-3])      # rad, per heliostat of the group
ZETA_SEED = 4321
CURVE = np.linspace(0.0, 3.0e-3, 13)                                           # holds 0.5 and 1.5 mrad


def smooth_weights(H, height, width):
    """``[H, height, width]`` fp32 loss weights: a plane per heliostat sample, each with its own slope, plus a shallow bowl.

    Not noise, unlike generate_heliostat_optics_golden.py's: here the code under test computes the normals itself, so they differ
    from the fixture's in the last bit (1.8e-7 measured), which moves a ray's landing point by 2e-4 pixels.  The bilinear splat is
    continuous in that point but its derivative jumps at every pixel border by the second difference of the weights; with
    6144 rays two or three cross a border, and under noise weights - a jump as large as the derivative itself - that alone
    puts the reference's own fp32 gradient 1e-2 to 6e-2 from its fp64 one, whatever the code.  Under a plane the derivative
    has no jump at all; the bowl (second difference 5e-5 against a slope of 1e-2 per pixel) keeps the curvature of the spot in
    the sum at jumps of half a percent."""
    i = (torch.arange(height, dtype=torch.float64) - 0.5 * (height - 1))[None, :, None] / height
    j = (torch.arange(width, dtype=torch.float64) - 0.5 * (width - 1))[None, None, :] / width
    h = torch.arange(H, dtype=torch.float64)[:, None, None]
    return (1.0 + (0.5 + 0.25 * h) * j + (0.5 * h - 0.75) * i + 0.1 * (i * i + j * j)).float()


def run(name, case, dtype, drawn=None, sigma=None, gradients=True):
    """The reference's trace of case ``name`` with the normals tilted by ``sigma`` (default: the truth)."""
    b = g.build(case, dtype)
    scenario, group = b["scenario"], b["group"]
    mask = torch.tensor(case["active_mask"], dtype=torch.int32)
    N, H = len(case["active_mask"]), int(mask.sum())
    target_idx = torch.tensor(case["target_idx"], dtype=torch.int64)
    incident = torch.nn.functional.normalize(torch.tensor([[0.0, 1.0, 0.0, 0.0]] * H, dtype=dtype), dim=1)
    res = torch.tensor(case["resolution"])
    P = b["P"]
    zeta = torch.randn((N, P, 2), generator=torch.Generator().manual_seed(ZETA_SEED), dtype=torch.float32)
    sigma = torch.tensor(SIGMA[name] if sigma is None else sigma, dtype=dtype).requires_grad_(gradients)
    group.activate_heliostats(active_heliostats_mask=mask, device=CPU)
    aim = scenario.solar_tower.get_centers_of_target_areas(target_area_indices=target_idx, device=CPU)
    with torch.no_grad():
        orientation = group.kinematics.incident_ray_directions_to_orientations(
            incident_ray_directions=incident, aim_points=aim, device=CPU)
        canonical_points = group.active_surface_points.detach().clone()
        canonical_normals = group.active_surface_normals.detach().clone()
        points = canonical_points @ orientation.transpose(1, 2)
    slopes = sigma.repeat_interleave(mask)[:, None, None] * zeta.to(dtype).repeat_interleave(mask, dim=0)
    if gradients:
        slopes.retain_grad()
    normals = tilt_normals(canonical_normals, slopes) @ orientation.transpose(1, 2)
    points = points.detach().clone().requires_grad_(gradients)
    group.active_surface_points, group.active_surface_normals = points, normals

    rt = g.HeliostatRayTracer(scenario=scenario, heliostat_group=group, blocking_active=case["blocking"], batch_size=100,
                              random_seed=7, bitmap_resolution=res, dni=None)
    assert list(rt.distortions_sampler) == list(range(H)), "the reference's sampler drops a heliostat sample"
    du32, de32 = rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e
    if drawn is not None:
        du32, de32 = drawn
    rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e = du32.to(dtype), de32.to(dtype)
    weights = smooth_weights(H, int(res[0]), int(res[1])).to(dtype)
    with torch.set_grad_enabled(gradients):
        flux, intercept, on_target, blocking = rt.trace_rays(incident_ray_directions=incident, active_heliostats_mask=mask,
                                                             target_area_indices=target_idx, device=CPU)
    if not gradients:
        torch.set_default_dtype(torch.float32)
        return dict(flux=npy(flux)), (du32, de32)
    (flux * weights).sum().backward()
    with torch.no_grad():
        per_target = rt.get_bitmaps_per_target(flux.detach(), target_idx, device=CPU)
    degrees, nets, _, canting, translations = b["nurbs_inputs"]
    out = dict(zeta=npy(zeta), sigma=npy(sigma).astype(np.float32), positions=npy(group.positions), control_points=npy(nets),
               canting=npy(canting), facet_translations=npy(translations), degrees=npy(degrees),
               surface_points=npy(group.surface_points), surface_normals=npy(group.surface_normals),
               orientation=npy(orientation), aim_points=npy(aim), canonical_points=npy(canonical_points),
               canonical_normals=npy(canonical_normals), aligned_points=npy(points), aligned_normals=npy(normals),
               incident=npy(incident), target_idx=npy(target_idx), active_mask=npy(mask), target_centers=npy(b["planar"].centers),
               target_normals=npy(b["planar"].normals), target_dims=npy(b["planar"].dimensions), resolution=npy(res),
               ray_magnitude=np.float64(float(rt.ray_magnitude)), distortions_u=npy(du32), distortions_e=npy(de32),
               loss_weights=npy(weights), flux=npy(flux), intercept=npy(intercept), on_target=npy(on_target), blocking=npy(blocking),
               per_target=npy(per_target), grad_sigma=npy(sigma.grad), grad_slopes=npy(slopes.grad), grad_aligned_points=npy(points.grad))
    if case["blocking"]:
        out.update(blocking_surfaces=npy(rt.blocking_heliostat_surfaces_active))
    torch.set_default_dtype(torch.float32)
    return out, (du32, de32)


def loss_curves(case, drawn, truth_flux):
    """``[N, 13]`` fp64: the mean squared pixel difference to ``truth_flux`` with sigma_h at ``CURVE`` and the others true."""
    truth = SIGMA["off"]
    curves = np.zeros((len(truth), len(CURVE)))
    for h in range(len(truth)):
        for k, value in enumerate(CURVE):
            sigma = list(truth)
            sigma[h] = float(value)
            flux = run("off", case, torch.float64, drawn=drawn, sigma=sigma, gradients=False)[0]["flux"]
            curves[h, k] = float(np.mean((flux - truth_flux) ** 2))
        at = int(np.argmin(np.abs(CURVE - truth[h])))
        assert abs(CURVE[at] - truth[h]) < 1e-12 and curves[h, at] == 0.0, (h, curves[h])
        assert (np.diff(curves[h, :at + 1]) < 0).all() and (np.diff(curves[h, at:]) > 0).all(), (h, curves[h])
        print(f"off: loss curve along sigma_{h} (truth {truth[h]}): {curves[h]}")
    return curves


GRADIENTS = ("grad_sigma", "grad_slopes", "grad_aligned_points")


def main():
    arrays = dict(zeta_seed=np.int64(ZETA_SEED), curve_sigma=CURVE)
    for name, case in CASES.items():
        out32, drawn = run(name, case, torch.float32)
        out64, _ = run(name, case, torch.float64, drawn=drawn)
        assert all(np.isfinite(v).all() for v in out32.values() if np.asarray(v).dtype.kind == "f")
        assert (out32["flux"].sum(axis=(1, 2)) > 0).all(), "a heliostat misses its target"
        assert out32["grad_sigma"].all() and out32["grad_slopes"].any(axis=(1, 2)).all()
        if case["blocking"]:
            print(f"{name}: unblocked fractions {out32['blocking']}")
            assert out32["blocking"].min() < 0.9, "the case does not block"
        for key, value in out32.items():
            arrays[f"{name}_{key}"] = value
        for key in ("flux", "per_target") + GRADIENTS:
            arrays[f"{name}_{key}_f64"] = np.asarray(out64[key], dtype=np.float64)
            print(f"{name}: {key}: fp32 vs fp64 {rel_l2(out32[key], out64[key]):.2e}")
        print(f"{name}: d loss / d sigma {out64['grad_sigma']}; intercept {out32['intercept']}, on target {out32['on_target']}")
        if name == "off":
            arrays["off_loss_curves"] = loss_curves(case, drawn, out64["flux"])
    path = g.OUT_DIR / "slope_error.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    print(f"wrote {path.name}: {size / 1024:.1f} KiB, keys={len(arrays)}")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
