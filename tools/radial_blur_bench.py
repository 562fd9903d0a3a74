#!/usr/bin/env python3
"""The convolved sun for a radial shape against the sampled one, timed on the bench's synthetic field.

One process, the field of bench.py (default 1000 heliostats, 4 x 50 x 50 points each, 256 x 256 bitmaps, one planar receiver)
under a pillbox sun of 4.65 mrad:

* ``radial_blur``: ``artist_amd.flux.radial_blur_flux`` alone on the field's own chief-ray bitmaps and metrics (tiles without flux
  leave early) and on dense bitmaps (an upstream gradient: no tile leaves early) - ms per call, and the fp32 FMAs per second
  over the stencils' non-zero taps (``taps_per_pixel``: counted from the operator's definition by a delta's response).
* ``convolved``: trace of the chief rays (R = 1, ray magnitude R) + ``optics.sun_image_covariance`` of the unit covariance +
  ``radial_blur_flux``, forward, and backward from a dense upstream gradient to the surface points and normals.
* ``sampled_r100``: the sampled trace (``art_trace_fwd`` / ``art_trace_bwd``, code this feature does not touch) with 100 rays per
  point of the same sun from the HIP radial sampler, drawn outside the timed region, forward and backward from the same gradient.

The variants run interleaved, round by round (machines differ by 10-20 % on the same binary; only numbers of one run compare);
every shape is warmed up twice first; times are device events around ``--steps`` calls, median and min to max over ``--rounds``.
``bar_met``: the slowest convolved forward + backward round is faster than the fastest sampled R = 100 forward + backward round.

usage:  python tools/radial_blur_bench.py [--heliostats 1000] [--rounds 7] [--steps 5] [--out profiles/radial_blur_bench.json]
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
    ap_.add_argument("--half-angle", type=float, default=4.65e-3)
    ap_.add_argument("--out", default=str(ROOT / "profiles" / "radial_blur_bench.json"))
    args = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("radial_blur_bench.py measures on the GPU; there is none")
    from artist_amd import NURBSSurfaces, ops, optics, scene
    from artist_amd.flux import radial_blur_flux
    dev = torch.device("cuda:0")
    H, n_eval, res, rays = args.heliostats, args.n_eval, 256, 100
    P = 4 * n_eval * n_eval
    scenario, uv = scene.build_synthetic_scenario(H, n_rays=rays, n_cp=(10, 10), n_eval=n_eval, device=dev)
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
    table = scene.Sun(rays, dict(distribution_type="pillbox", half_angle=args.half_angle), device=dev).quantile_table
    unit = torch.tensor([1.0, 0.0, 1.0], device=dev)
    upstream = torch.rand((H, res, res), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    distortions = {1: torch.zeros((H, 1, P, 2), device=dev),
                   rays: ops.sample_radial_distortions(range(H), rays, P, 7, (0.0, 0.0), table, dev)}

    def trace(n, magnitude):
        d = distortions[n]
        return ops.trace_rays(points, normals, inc, d[..., 0], d[..., 1], tix, *tables, magnitude, 0.0, 0.935, (res, res),
                              points_per_facet=n_eval * n_eval)[0]

    def convolved_forward():
        sharp = trace(1, float(rays))
        return radial_blur_flux(sharp, optics.sun_image_covariance(points, normals, inc, tix, *tables, unit, (res, res)), table)

    with torch.no_grad():
        sharp = trace(1, float(rays))
        metric = optics.sun_image_covariance(points, normals, inc, tix, *tables, unit, (res, res))
        # the stencils' non-zero taps, from the operator itself: the response to a delta at the centre
        delta = torch.zeros((H, res, res), device=dev)
        delta[:, res // 2, res // 2] = 1.0
        taps = (radial_blur_flux(delta, metric, table) != 0).flatten(1).sum(1).double()
        del delta
    nonzero_fraction = float((sharp != 0).float().mean())
    kept = optics.radial_window_kept_fraction(metric, table)

    def backward_of(forward):
        def run():
            points.grad = normals.grad = None
            forward().backward(upstream)
        return run

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    variants = {
        "radial_blur_field": no_grad(lambda: radial_blur_flux(sharp, metric, table)),
        "radial_blur_dense": no_grad(lambda: radial_blur_flux(upstream, metric, table)),
        "convolved_forward": no_grad(convolved_forward),
        "convolved_forward_backward": backward_of(convolved_forward),
        "sampled_r100_forward": no_grad(lambda: trace(rays, 1.0)),
        "sampled_r100_forward_backward": backward_of(lambda: trace(rays, 1.0)),
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
    scale = 1000.0 / H
    fmas_dense = float(taps.sum()) * res * res          # every pixel meets every non-zero tap (edges aside)
    blur = {name: dict(ms=ms[name]["median"], ms_per_1000_bitmaps=ms[name]["median"] * scale) for name in
            ("radial_blur_field", "radial_blur_dense")}
    blur["radial_blur_dense"]["fma_per_second"] = fmas_dense / (ms["radial_blur_dense"]["median"] * 1e-3)
    convolved, r100 = ms["convolved_forward_backward"], ms["sampled_r100_forward_backward"]
    half_extents = (metric[:, [0, 2]].double() * float(table[1])).sqrt()
    result = dict(tool="radial_blur_bench", device=torch.cuda.get_device_name(0), heliostats=H, points_per_heliostat=P, resolution=res,
                  rounds=args.rounds, steps=args.steps, half_angle=args.half_angle,
                  nonzero_fraction_of_chief_ray_bitmaps=nonzero_fraction,
                  half_extents_px=dict(min=half_extents.min(0).values.tolist(), max=half_extents.max(0).values.tolist()),
                  taps_per_pixel=dict(min=float(taps.min()), mean=float(taps.mean()), max=float(taps.max())),
                  kept_fraction=dict(min=float(kept.min()), max=float(kept.max())), fma_dense=fmas_dense,
                  radial_blur=blur, ms=ms,
                  convolved_forward_backward_ms=convolved["median"], sampled_r100_forward_backward_ms=r100["median"],
                  convolved_over_sampled_r100=convolved["median"] / r100["median"], bar_met=bool(convolved["max"] < r100["min"]))
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
