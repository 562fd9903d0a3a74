#!/usr/bin/env python3
"""What mirror slope errors cost, each figure beside the path it stands next to, timed in the same process:

* ``epoch``: one epoch on the metric field (``--heliostats`` x ``--rays`` x 4 x ``--n-eval``^2 points, 256 x 256 bitmaps) -
  control points -> surfaces -> alignment -> trace -> crop and pixel loss -> backward -> Adam - three ways.  ``without`` is the
  parent commit's path, the same launches: the fused evaluate-and-align launch.  ``staged`` leaves the fused launch (evaluation,
  then ``art_align_fwd``) without a tilt: what the route costs by itself.  ``with`` is ``staged`` with the normals tilted by
  ``sigma_h * zeta`` in between, sigma learning beside the control points;
* ``tilt``: ``optics.tilt_normals`` forward and backward alone on ``[--tilt-heliostats, --tilt-points, 4]`` normals, and the
  alignment launches they sit next to (``art_align_fwd`` + ``art_align_bwd``) on the same shapes;
* ``draw``: one zeta draw for the metric field (``optics.slope_sample``).

HIP events around each call, ``--warmup`` calls first, then the median of ``--runs``, the paths of a part alternating.  Prints
one JSON line; ``--out`` also writes it to a file.
"""
import argparse
import json
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch  # noqa: E402


def timed(calls: dict, warmup: int, runs: int) -> dict:
    """Median milliseconds of each call in ``calls`` (name -> function), alternating between them run by run."""
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    samples = {name: [] for name in calls}
    for _ in range(runs):
        for name, call in calls.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            call()
            end.record()
            end.synchronize()
            samples[name].append(start.elapsed_time(end))
    return {name: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), runs=len(v)) for name, v in samples.items()}


def part_epoch(args, dev) -> dict:
    from artist_amd import HeliostatRayTracer, NURBSSurfaces, crop_and_pixel_loss, ops, scene
    from artist_amd.optim import Adam
    H = args.heliostats
    scenario, uv = scene.build_synthetic_scenario(H, n_rays=args.rays, n_eval=args.n_eval, device=dev)
    tower, group = scenario.solar_tower, scenario.heliostat_field.heliostat_groups[0]
    group.slope_errors = torch.full((H,), 1e-3, device=dev)
    mask = torch.ones(H, dtype=torch.int32, device=dev)
    targets = torch.zeros(H, dtype=torch.long, device=dev)
    incident = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=dev).repeat(H, 1)
    group.activate_heliostats(mask, dev)
    orientation = scene.ideal_orientations(group.active_positions, tower.get_centers_of_target_areas(targets), incident)
    zeta = group.active_slope_sample.reshape(H, 4, -1, 2)
    nets = group.active_nurbs_control_points.clone().requires_grad_(True)
    sigma = group.slope_errors.clone().requires_grad_(True)
    surfaces = NURBSSurfaces(group.nurbs_degrees, nets, device=dev)
    with torch.no_grad():
        points, normals = surfaces.calculate_surface_points_and_normals(uv, group.active_canting, group.active_facet_translations,
                                                                        orientations=orientation)
        group.active_surface_points, group.active_surface_normals = points.reshape(H, -1, 4), normals.reshape(H, -1, 4)
    tracer = HeliostatRayTracer(scenario, group, blocking_active=False)
    truth = torch.rand((H, 256, 256), generator=torch.Generator().manual_seed(1)).to(dev) + 0.1
    optimizers = dict(without=Adam([nets], lr=1e-6), staged=Adam([nets], lr=1e-6), **{"with": Adam([nets, sigma], lr=1e-6)})

    def epoch(path):
        def run():
            optimizers[path].zero_grad(set_to_none=True)
            net = NURBSSurfaces(group.nurbs_degrees, nets, device=dev)
            if path == "without":
                points, normals = net.calculate_surface_points_and_normals(uv, group.active_canting, group.active_facet_translations,
                                                                           orientations=orientation)
                points, normals = points.reshape(H, -1, 4), normals.reshape(H, -1, 4)
            else:
                points, normals = net.calculate_surface_points_and_normals(uv, group.active_canting, group.active_facet_translations)
                if path == "with":
                    normals = group.tilted_normals(normals, sigma.reshape(H, 1), zeta)
                points, normals = ops.align_surfaces(points.reshape(H, -1, 4), normals.reshape(H, -1, 4), orientation)
            group.active_surface_points, group.active_surface_normals = points, normals
            flux, *_ = tracer.trace_rays(incident, mask, targets)
            crop_and_pixel_loss(flux, tower, targets, truth).sum().backward()
            optimizers[path].step()
        return run

    out = timed({name: epoch(name) for name in ("without", "staged", "with")}, args.warmup, args.runs)
    out.update(heliostats=H, rays=args.rays, points=int(group.active_surface_points.shape[1]),
               without_is="the parent commit's path: the fused evaluate-and-align launch, the same launches")
    return out


def part_tilt(args, dev) -> dict:
    from artist_amd import ops, optics
    H, P = args.tilt_heliostats, args.tilt_points
    generator = torch.Generator().manual_seed(2)
    normals = torch.cat((0.05 * torch.randn(H, P, 2, generator=generator), torch.ones(H, P, 1)), dim=-1)
    normals = torch.cat((torch.nn.functional.normalize(normals, dim=-1), torch.zeros(H, P, 1)), dim=-1).to(dev).requires_grad_(True)
    points = torch.randn(H, P, 4, generator=generator).to(dev).requires_grad_(True)
    zeta = torch.randn(H, P, 2, generator=generator).to(dev)
    sigma = torch.full((H, 1, 1), 1e-3, device=dev, requires_grad=True)
    orientation = torch.eye(4, device=dev).repeat(H, 1, 1)
    gradient = torch.randn(H, P, 4, generator=generator).to(dev)
    tilted = optics.tilt_normals(normals, sigma * zeta)
    aligned = ops.align_surfaces(points, normals, orientation)

    def backward(outputs, inputs, gradients):
        return lambda: torch.autograd.grad(outputs, inputs, gradients, retain_graph=True)

    with torch.no_grad():
        forward = timed({"tilt_forward": lambda: optics.tilt_normals(normals, sigma * zeta),
                         "align_forward": lambda: ops.align_surfaces(points, normals, orientation)}, args.warmup, args.runs)
    out = dict(forward, **timed({"tilt_backward": backward([tilted], [normals, sigma], [gradient]),
                                 "align_backward": backward(list(aligned), [points, normals], [gradient, gradient])},
                                args.warmup, args.runs))
    out.update(heliostats=H, points=P, normals_bytes=H * P * 16)
    return out


def part_draw(args, dev) -> dict:
    from artist_amd import optics
    H, P = args.heliostats, 4 * args.n_eval * args.n_eval
    rows = list(range(H))
    out = timed({"zeta_draw": lambda: optics.slope_sample(rows, P, 7, dev)}, args.warmup, args.runs)
    out.update(heliostats=H, points=P, sample_bytes=H * P * 8)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--heliostats", type=int, default=1000)
    ap.add_argument("--rays", type=int, default=100)
    ap.add_argument("--n-eval", type=int, default=50)
    ap.add_argument("--tilt-heliostats", type=int, default=1000)
    ap.add_argument("--tilt-points", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--parts", nargs="*", default=["epoch", "tilt", "draw"], choices=["epoch", "tilt", "draw"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("slope_error_bench measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(dev), warmup=args.warmup, runs=args.runs)
    for part in args.parts:
        result[part] = dict(epoch=part_epoch, tilt=part_tilt, draw=part_draw)[part](args, dev)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
