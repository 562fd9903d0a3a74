#!/usr/bin/env python3
"""The gradient of the convolved sun's window, timed on the bench's synthetic field.

One process, the field of bench.py (default 1000 heliostats, 4 x 50 x 50 points each, 256 x 256 bitmaps, one planar receiver), the
protocol of tools/flux_blur_bench.py:

* ``window_gradient``: ``art_flux_crop_bwd`` in its blur mode alone - the field's chief-ray bitmaps, its covariances with a
  1.5 mrad optical error, a dense upstream gradient;
* ``blur_field`` / ``blur_dense``: ``artist_amd.flux.blur_flux`` alone, on the same covariances, in the same run;
* ``convolved_constant_forward_backward`` / ``convolved_learned_forward_backward``: trace of the chief rays +
  ``optics.sun_image_covariance`` + the blur, forward, and backward from a dense upstream gradient to the surface points and
  normals - with constant optical errors (``blur_flux``) and with optical errors that learn (``differentiable_blur_flux``).

The variants run interleaved, round by round; every shape is warmed up twice; times are device events around ``--steps`` calls,
the median over ``--rounds`` rounds.  ``bar_met``: the gradient call takes at most 4 times ``blur_flux`` on the same bitmaps
(``blur_field``), in the same run.

usage:  python tools/flux_blur_grad_bench.py [--heliostats 1000] [--rounds 7] [--steps 5] [--out profiles/flux_blur_grad_bench.json]
"""
import argparse
import json
import pathlib
import statistics
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--heliostats", type=int, default=1000)
    ap_.add_argument("--n-eval", type=int, default=50)
    ap_.add_argument("--rounds", type=int, default=7)
    ap_.add_argument("--steps", type=int, default=5)
    ap_.add_argument("--optical-error", type=float, default=1.5e-3)
    ap_.add_argument("--out", default=str(ROOT / "profiles" / "flux_blur_grad_bench.json"))
    args = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flux_blur_grad_bench.py measures on the GPU; there is none")
    from artist_amd import NURBSSurfaces, ops, optics, scene
    from artist_amd.flux import DifferentiableFluxBlur, blur_flux, differentiable_blur_flux
    dev = torch.device("cuda:0")
    H, n_eval, res = args.heliostats, args.n_eval, 256
    P = 4 * n_eval * n_eval
    scenario, uv = scene.build_synthetic_scenario(H, n_rays=100, n_cp=(10, 10), n_eval=n_eval, device=dev)
    group = scenario.heliostat_field.heliostat_groups[0]
    group.activate_heliostats(torch.ones(H, dtype=torch.int32, device=dev))
    tix = torch.zeros(H, dtype=torch.long, device=dev)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=dev).repeat(H, 1)
    orientation = scene.ideal_orientations(group.active_positions, scenario.solar_tower.get_centers_of_target_areas(tix), inc)
    with torch.no_grad():
        points, normals = NURBSSurfaces(group.nurbs_degrees, group.active_nurbs_control_points, device=dev) \
            .calculate_surface_points_and_normals(uv[:1].expand(H, -1, -1, -1), group.active_canting,
                                                  group.active_facet_translations, orientations=orientation)
    points = points.reshape(H, P, 4).contiguous().requires_grad_(True)
    normals = normals.reshape(H, P, 4).contiguous().requires_grad_(True)
    planar = scenario.solar_tower.target_areas[0]
    tables = (planar.centers, planar.normals, planar.dimensions)
    sun = scenario.light_sources.light_source_list[0]
    tril = sun.distribution.scale_tril.float()
    C = tril @ tril.T
    sigma = torch.full((H,), args.optical_error, device=dev, requires_grad=True)
    upstream = torch.rand((H, res, res), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    zeros = torch.zeros((H, 1, P, 2), device=dev)

    def angular(errors):
        variance = errors * errors
        return torch.stack((C[0, 0] + variance, C[0, 1].expand_as(variance), C[1, 1] + variance), dim=1)

    def trace():
        return ops.trace_rays(points, normals, inc, zeros[..., 0], zeros[..., 1], tix, *tables, 100.0, 0.0, 0.935, (res, res),
                              points_per_facet=n_eval * n_eval)[0]

    def convolved_constant():
        return blur_flux(trace(), optics.sun_image_covariance(points, normals, inc, tix, *tables, angular(sigma.detach()), (res, res)))

    def convolved_learned():
        return differentiable_blur_flux(trace(), optics.sun_image_covariance(points, normals, inc, tix, *tables, angular(sigma),
                                                                             (res, res), differentiable=True))

    with torch.no_grad():
        sharp = trace()
        covariance = optics.sun_image_covariance(points, normals, inc, tix, *tables, angular(sigma.detach()), (res, res))

    def backward_of(forward):
        def run():
            points.grad = normals.grad = sigma.grad = None
            forward().backward(upstream)
        return run

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    variants = {
        "window_gradient": no_grad(lambda: DifferentiableFluxBlur.covariance_gradient(sharp, covariance, upstream)),
        "blur_field": no_grad(lambda: blur_flux(sharp, covariance)),
        "blur_dense": no_grad(lambda: blur_flux(upstream, covariance)),
        "convolved_constant_forward_backward": backward_of(convolved_constant),
        "convolved_learned_forward_backward": backward_of(convolved_learned),
    }
    for fn in variants.values():          # warm-up: every shape, twice
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.steps):
                fn()
            end.record()
            end.synchronize()
            times[name].append(start.elapsed_time(end) / args.steps)
    ops.check_async_errors(dev)
    ms = {name: dict(median=statistics.median(v), min=min(v), max=max(v)) for name, v in times.items()}
    gradient, blur = ms["window_gradient"]["median"], ms["blur_dense"]["median"]
    constant, learned = (ms[f"convolved_{k}_forward_backward"]["median"] for k in ("constant", "learned"))
    result = dict(tool="flux_blur_grad_bench", device=torch.cuda.get_device_name(0), heliostats=H, points_per_heliostat=P,
                  resolution=res, rounds=args.rounds, steps=args.steps, optical_error_rad=args.optical_error,
                  covariance_px2=dict(min=covariance.min(0).values.tolist(), max=covariance.max(0).values.tolist()),
                  ms=ms, window_gradient_ms=gradient, blur_dense_ms=blur, blur_field_ms=ms["blur_field"]["median"],
                  window_gradient_over_blur_dense=gradient / blur, window_gradient_over_blur_field=gradient / ms["blur_field"]["median"],
                  bar=4.0, bar_met=bool(gradient <= 4.0 * ms["blur_field"]["median"]),
                  convolved_constant_forward_backward_ms=constant, convolved_learned_forward_backward_ms=learned,
                  learned_over_constant=learned / constant)
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
