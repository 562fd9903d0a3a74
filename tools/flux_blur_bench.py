#!/usr/bin/env python3
"""The convolved sun against the sampled one, timed on the bench's synthetic field.

One process, the field of bench.py (default 1000 heliostats, 4 x 50 x 50 points each, 256 x 256 bitmaps, one planar receiver):

* ``blur``: ``artist_amd.flux.blur_flux`` alone on the field's own chief-ray bitmaps and covariances (tiles without flux leave
  early) and on dense bitmaps (an upstream gradient: no tile leaves early) - ms per call, and the achieved GB/s against ONE read and
  ONE write of the bitmaps, the traffic the fused kernel is built for; ``hbm_floor_fraction`` is that traffic at ``--hbm-gbps``
  (default 8000, the MI355X's nominal HBM3E rate) over the measured time.
* ``convolved``: trace of the chief rays (R = 1, ray magnitude R) + ``optics.sun_image_covariance`` + ``blur_flux``, forward, and
  backward from a dense upstream gradient to the surface points and normals.
* ``sampled_r10`` / ``sampled_r100``: the sampled trace (``art_trace_fwd`` / ``art_trace_bwd``, code this feature does not touch) with
  10 and 100 rays per point from the HIP sampler, forward and backward from the same upstream gradient.

The variants run interleaved, round by round (machines differ by 10-20 % on the same binary; only numbers of one run compare);
every shape is warmed up first; times are device events around ``--steps`` calls, the median over ``--rounds`` rounds.
``bar_met``: convolved forward + backward takes less time than sampled R = 100 forward + backward - the feature's only bar.

usage:  python tools/flux_blur_bench.py [--heliostats 1000] [--rounds 7] [--steps 5] [--out profiles/flux_blur_bench.json]
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
    ap_.add_argument("--hbm-gbps", type=float, default=8000.0)
    ap_.add_argument("--out", default=str(ROOT / "profiles" / "flux_blur_bench.json"))
    args = ap_.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flux_blur_bench.py measures on the GPU; there is none")
    from artist_amd import NURBSSurfaces, ops, optics, scene
    from artist_amd.flux import blur_flux
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
    angular = torch.stack((C[0, 0], C[0, 1], C[1, 1]))
    sigma = float(tril[0, 0])
    upstream = torch.rand((H, res, res), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    zeros = torch.zeros((H, 1, P, 2), device=dev)
    distortions = {1: zeros}
    for rays in (10, 100):
        distortions[rays] = ops.sample_distortions(range(H), rays, P, 7, (0.0, 0.0), ((sigma, 0.0), (0.0, sigma)), dev)

    def trace(rays, magnitude):
        d = distortions[rays]
        return ops.trace_rays(points, normals, inc, d[..., 0], d[..., 1], tix, *tables, magnitude, 0.0, 0.935, (res, res),
                              points_per_facet=n_eval * n_eval)[0]

    def convolved_forward():
        sharp = trace(1, 100.0)
        return blur_flux(sharp, optics.sun_image_covariance(points, normals, inc, tix, *tables, angular, (res, res)))

    with torch.no_grad():
        sharp = trace(1, 100.0)
        covariance = optics.sun_image_covariance(points, normals, inc, tix, *tables, angular, (res, res))
    nonzero_fraction = float((sharp != 0).float().mean())

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
        "blur_field": no_grad(lambda: blur_flux(sharp, covariance)),
        "blur_dense": no_grad(lambda: blur_flux(upstream, covariance)),
        "convolved_forward": no_grad(convolved_forward),
        "convolved_forward_backward": backward_of(convolved_forward),
        "sampled_r10_forward": no_grad(lambda: trace(10, 1.0)),
        "sampled_r10_forward_backward": backward_of(lambda: trace(10, 1.0)),
        "sampled_r100_forward": no_grad(lambda: trace(100, 1.0)),
        "sampled_r100_forward_backward": backward_of(lambda: trace(100, 1.0)),
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
    traffic = 2 * H * res * res * 4
    floor_ms = traffic / (args.hbm_gbps * 1e9) * 1e3
    blur = {name: dict(ms=ms[name]["median"], ms_per_1000_bitmaps=ms[name]["median"] * scale,
                       achieved_gbps=traffic / (ms[name]["median"] * 1e-3) / 1e9, hbm_floor_fraction=floor_ms / ms[name]["median"])
            for name in ("blur_field", "blur_dense")}
    convolved, r100, r10 = (ms[f"{k}_forward_backward"]["median"] for k in ("convolved", "sampled_r100", "sampled_r10"))
    result = dict(tool="flux_blur_bench", device=torch.cuda.get_device_name(0), heliostats=H, points_per_heliostat=P, resolution=res,
                  rounds=args.rounds, steps=args.steps, hbm_gbps_assumed=args.hbm_gbps, traffic_bytes_one_read_one_write=traffic,
                  nonzero_fraction_of_chief_ray_bitmaps=nonzero_fraction,
                  covariance_px2=dict(min=covariance.min(0).values.tolist(), max=covariance.max(0).values.tolist()),
                  blur=blur, ms=ms,
                  convolved_forward_backward_ms=convolved, sampled_r100_forward_backward_ms=r100, sampled_r10_forward_backward_ms=r10,
                  convolved_over_sampled_r100=convolved / r100, convolved_over_sampled_r10=convolved / r10, bar_met=bool(convolved < r100))
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
