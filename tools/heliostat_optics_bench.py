#!/usr/bin/env python3
"""What per-heliostat optics cost, each figure beside the path it replaces, timed in the same process:

* ``scale``: trace forward + backward with the factors as floats (the kernel applies them) and as tensors ``[H]`` (the kernel
  runs with 0 / 1, one element-wise pass scales the ``[H,256,256]`` bitmaps, its backward scales the gradient), and that pass
  alone on the traced bitmaps;
* ``per_target``: ``trace_rays_per_target`` with floats (the fused per-target mode) and with tensors (trace per heliostat,
  scale, ``art_per_target_sum``), forward only, for each ``--per-target-heliostats``;
* ``draw``: a distortion draw of the ``"hip"`` sampler without and with ``optical_errors`` (cache cleared before each).

HIP events around each call, ``--warmup`` calls first, then the median of ``--runs``, the two paths of a pair alternating.  Prints
one JSON line; ``--out`` also writes it to a file.  Under ``rocprofv3 --kernel-trace --stats -- python tools/...`` the kernels
carry their entry points' names; pick the parts with ``--parts``.
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


def field(H: int, R: int, n_eval: int, dev):
    from artist_amd import HeliostatRayTracer
    from artist_amd.scene import build_synthetic_scenario
    scenario, _ = build_synthetic_scenario(H, n_rays=R, n_eval=n_eval, device=dev)
    scenario.light_sources.light_source_list[0].sampler = "hip"
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=dev)
    group.activate_heliostats(mask)
    targets = torch.zeros(H, dtype=torch.long, device=dev)
    incident = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=dev).repeat(H, 1)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(targets), incident, mask)
    tracer = HeliostatRayTracer(scenario, group, blocking_active=False)
    generator = torch.Generator(device="cpu").manual_seed(3)
    extinction = (0.3 * torch.rand(H, generator=generator)).to(dev)
    reflectivity = (0.5 + 0.5 * torch.rand(H, generator=generator)).to(dev)
    return scenario, group, tracer, (incident, mask, targets), extinction, reflectivity


def part_scale(args, dev) -> dict:
    H = args.heliostats
    _, group, tracer, call_arguments, extinction, reflectivity = field(H, args.rays, args.n_eval, dev)
    points = group.active_surface_points.detach().requires_grad_(True)
    group.active_surface_points = points
    weights = torch.rand((H, 256, 256), device=dev)

    def step(eps, rho):
        def run():
            points.grad = None
            flux, *_ = tracer.trace_rays(*call_arguments, ray_extinction_factor=eps, mirror_reflectivity=rho)
            (flux * weights).sum().backward()
        return run

    flux = tracer.trace_rays(*call_arguments, ray_extinction_factor=0.0, mirror_reflectivity=1.0)[0].detach()
    w = ((1.0 - extinction) * reflectivity).view(-1, 1, 1)
    out = timed({"trace_fwd_bwd_floats": step(0.1, 0.9), "trace_fwd_bwd_tensors": step(extinction, reflectivity),
                 "scale_pass_alone": lambda: flux * w}, args.warmup, args.runs)
    out["bitmap_bytes"] = int(flux.numel() * 4)
    out["heliostats"], out["rays"], out["points"] = H, args.rays, int(points.shape[1])
    return out


def part_per_target(args, dev) -> dict:
    out = {}
    for H in args.per_target_heliostats:
        _, _, tracer, call_arguments, extinction, reflectivity = field(H, args.per_target_rays, args.n_eval, dev)
        with torch.no_grad():
            out[f"H{H}"] = timed({
                "fused_mode_floats": lambda: tracer.trace_rays_per_target(*call_arguments, ray_extinction_factor=0.1,
                                                                          mirror_reflectivity=0.9),
                "scaled_route_tensors": lambda: tracer.trace_rays_per_target(*call_arguments, ray_extinction_factor=extinction,
                                                                             mirror_reflectivity=reflectivity)},
                args.warmup, args.runs)
        out[f"H{H}"]["rays"] = args.per_target_rays
        del tracer
        torch.cuda.empty_cache()
    return out


def part_draw(args, dev) -> dict:
    from artist_amd.scene import Sun
    H, P = args.heliostats, 4 * args.n_eval * args.n_eval
    out = {}
    for kind in ("normal", "pillbox"):
        sun = Sun(args.rays, dict(distribution_type=kind), device=dev, sampler="hip")
        errors = torch.full((H,), 2e-3, device=dev)

        def draw(optical_errors):
            def run():
                sun.clear_distortion_cache()
                sun.get_distortions(number_of_points=P, number_of_active_heliostats=H, optical_errors=optical_errors)
            return run

        out[kind] = timed({"plain_draw": draw(None), "draw_with_optical_errors": draw(errors)}, args.warmup, args.runs)
        sun.clear_distortion_cache()
        torch.cuda.empty_cache()
    out["sample_bytes"] = H * args.rays * P * 8
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--heliostats", type=int, default=1000)
    ap.add_argument("--rays", type=int, default=100)
    ap.add_argument("--n-eval", type=int, default=50)
    ap.add_argument("--per-target-heliostats", type=int, nargs="*", default=[1000, 10000])
    ap.add_argument("--per-target-rays", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--parts", nargs="*", default=["scale", "per_target", "draw"], choices=["scale", "per_target", "draw"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("heliostat_optics_bench measures on the GPU; there is none")
    dev = torch.device("cuda:0")
    result = dict(device=torch.cuda.get_device_name(dev), warmup=args.warmup, runs=args.runs)
    for part in args.parts:
        result[part] = dict(scale=part_scale, per_target=part_per_target, draw=part_draw)[part](args, dev)
        torch.cuda.empty_cache()
    line = json.dumps(result)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
