#!/usr/bin/env python3
"""Cost of drawing the sun-shape distortions -> profiles/sampler_bench.json.

  * one draw with the HIP sampler (art_sample_distortions) at the metric field and at one rank's share (125 rows): ms from
    device events, GB/s of the [n,R,P,2] fp32 buffer it writes, fraction of the 6.1 TB/s plain-store rate;
  * the torch per-row recipe (Sun(sampler="torch").get_distortions_rows) at the same sizes: host clock around a synchronised
    draw (it synchronises by itself);
  * a HeliostatRayTracer construction that hits the per-sun cache: host time and the number of sampler launches (0);
  * a reference-shaped epoch (artist/optim/surface_reconstructor.py:557: a new tracer every epoch), trace_rays + backward,
    the tracer rebuilt every step: with a sample drawn once before the loop, with the torch sampler, with the HIP sampler
    without the cache and with it; and, for scale, one tracer reused by every step.

  * --shape pillbox | buie: instead of the above, the radial kernel (art_sample_radial_distortions, the shape's quantile
    table) next to the Gaussian kernel at the same two sizes, both from device events, alternating in one process
    -> profiles/sunshape_bench.json.

usage: python tools/sampler_bench.py [--heliostats 1000 --rays 100 --n-eval 50 --steps 10 --warmup 3 --epoch-steps 30]
                                     [--no-epoch] [--shape normal|pillbox|buie] [--out FILE]
"""
import argparse
import json
import pathlib
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WRITE_RATE = 6.1e12            # B/s: plain-store rate of MI355X_MICROARCH.md (measured copy peak 6.29 TB/s)


def event_ms(fn, steps, warmup):
    """Median and mean device-event time of ``fn`` over ``steps`` calls after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": ms[len(ms) // 2], "mean_ms": sum(ms) / len(ms), "min_ms": ms[0], "max_ms": ms[-1]}


def wall_ms(fn, steps, warmup):
    """Host time per call of ``fn`` over ``steps`` calls, synchronised before and after the window."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


class DrawnOnce:
    """A light source that hands out one sample drawn before the loop (the epoch's baseline: no draw, no cache lookup)."""

    def __init__(self, sun, u, e):
        self.number_of_rays, self.distribution = sun.number_of_rays, sun.distribution
        self.u, self.e = u, e

    def get_distortions(self, number_of_points, number_of_active_heliostats, random_seed=7):
        return self.u, self.e

    def get_distortions_rows(self, rows, number_of_points, number_of_active_heliostats, random_seed=7):
        return self.u, self.e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heliostats", type=int, default=1000)
    ap.add_argument("--rays", type=int, default=100)
    ap.add_argument("--n-eval", type=int, default=50)
    ap.add_argument("--share", type=int, default=125, help="rows of one rank's share")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--epoch-steps", type=int, default=30)
    ap.add_argument("--no-epoch", action="store_true", help="draws only (the profiler run)")
    ap.add_argument("--shape", choices=("normal", "pillbox", "buie"), default="normal",
                    help="a radial shape: time its kernel against the Gaussian kernel, draws only")
    ap.add_argument("--out", default=None, help="default: profiles/sampler_bench.json (sunshape_bench.json with --shape)")
    args = ap.parse_args()
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("sampler_bench.json" if args.shape == "normal" else "sunshape_bench.json"))
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench needs a GPU")
    from artist_amd import HeliostatRayTracer, _lib, ops
    from artist_amd.scene import Sun, build_synthetic_scenario

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H, R, P = args.heliostats, args.rays, 4 * args.n_eval * args.n_eval
    res = {"field": {"heliostats": H, "rays": R, "points": P}, "device": torch.cuda.get_device_name(dev),
           "write_rate_TBps": WRITE_RATE / 1e12, "draws": {}}

    handle = _lib.lib()
    real = handle.art_sample_distortions
    launches = [0]

    def counted(*a):
        launches[0] += 1
        return real(*a)

    handle.art_sample_distortions = counted

    sun = Sun(R, device=dev)
    law = sun._host_law()
    sizes = (("field", list(range(H))), ("rank_share", list(range(0, H, max(1, H // args.share)))[:args.share]))
    if args.shape != "normal":
        return finish(shape_pair(res, args, ops, Sun(R, dict(distribution_type=args.shape), device=dev), law, sizes, R, P, dev),
                      args.out)
    for label, rows in sizes:
        nbytes = len(rows) * R * P * 8
        hip = event_ms(lambda: ops.sample_distortions(rows, R, P, 7, *law, dev), args.steps, args.warmup)
        sun.sampler = "torch"
        torch_ms = wall_ms(lambda: sun.get_distortions_rows(rows, P, H, 7), max(2, args.steps // 2), 1)
        res["draws"][label] = {
            "rows": len(rows), "bytes": nbytes, "hip": hip, "hip_GBps": nbytes / hip["median_ms"] / 1e6,
            "hip_fraction_of_write_rate": nbytes / (hip["median_ms"] * 1e-3) / WRITE_RATE,
            "hip_write_floor_ms": nbytes / WRITE_RATE * 1e3, "torch_per_row_wall_ms": torch_ms,
            "torch_over_hip": torch_ms / hip["median_ms"]}
        print(f"[sampler] {label}: {len(rows)} rows, hip {hip['median_ms']:.3f} ms "
              f"({res['draws'][label]['hip_fraction_of_write_rate']:.2f} of the write rate), torch {torch_ms:.3f} ms", flush=True)
        torch.cuda.empty_cache()
    if args.no_epoch:
        return finish(res, args.out)

    # ---- tracer construction and the reference-shaped epoch on the synthetic field ----------------------------------
    scenario, _ = build_synthetic_scenario(H, n_rays=R, n_eval=args.n_eval, device=dev)
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=dev)
    group.activate_heliostats(mask)
    tix = torch.zeros(H, dtype=torch.long, device=dev)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=dev).repeat(H, 1)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
    points = group.active_surface_points.detach().clone().requires_grad_(True)
    normals = group.active_surface_normals.detach().clone().requires_grad_(True)
    sun = scenario.light_sources.light_source_list[0]

    sun.sampler = "hip"
    rt = HeliostatRayTracer(scenario, group, blocking_active=False)            # fills the cache
    torch.cuda.synchronize()
    before = launches[0]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        rt = HeliostatRayTracer(scenario, group, blocking_active=False)
    host_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    res["cache_hit_construction"] = {"host_ms": host_ms, "sampler_launches": launches[0] - before,
                                     "constructions": args.steps}
    print(f"[sampler] cache-hit construction {host_ms:.3f} ms host, {launches[0] - before} sampler launches", flush=True)
    del rt

    def trace_backward(rt):
        group.active_surface_points, group.active_surface_normals = points, normals
        flux, *_ = rt.trace_rays(inc, mask, tix)
        flux.sum().backward()
        points.grad = normals.grad = None

    sources = scenario.light_sources.light_source_list
    sun.sampler = "hip"
    u, e = sun.get_distortions(P, H)
    drawn = DrawnOnce(sun, u.clone(), e.clone())        # (a buffer of its own: the cache below may replace the sun's)
    del u, e

    def variant(label):
        """One step of the reference-shaped epoch: a NEW tracer, its trace_rays, the backward."""
        if label == "tracer_reused":
            return lambda: trace_backward(reused)
        sources[0] = drawn if label == "drawn_once" else sun
        sun.sampler = "torch" if label == "torch_sampler" else "hip"
        no_cache = label == "hip_no_cache"

        def step():
            if no_cache:
                sun.clear_distortion_cache()
            trace_backward(HeliostatRayTracer(scenario, group, blocking_active=False))
        return step

    reused = HeliostatRayTracer(scenario, group, blocking_active=False)
    epochs = {}
    order = ["drawn_once", "hip_cache", "tracer_reused", "torch_sampler", "hip_no_cache", "drawn_once", "hip_cache"]
    for label in order:                                 # drawn_once / hip_cache twice, alternating: the same-run spread
        fn = variant(label)
        for _ in range(args.warmup):
            fn()
        before = launches[0]
        ms = wall_ms(fn, args.epoch_steps, 0)
        epochs.setdefault(label, []).append(ms)
        epochs.setdefault(label + "_sampler_launches_per_step", []).append((launches[0] - before) / args.epoch_steps)
        sources[0] = sun
        torch.cuda.empty_cache()
    mean = lambda k: sum(epochs[k]) / len(epochs[k])    # noqa: E731
    epochs["hip_cache_over_drawn_once"] = mean("hip_cache") / mean("drawn_once")
    epochs["what"] = ("ms per step, host clock over K steps between synchronisations (a list: one entry per repeat); a step = "
                      "a new HeliostatRayTracer + trace_rays + flux.sum().backward(), blocking off.  drawn_once: the tracer is "
                      "rebuilt but its light source hands out a sample drawn before the loop; tracer_reused: one tracer for "
                      "all steps (no rebuild at all); torch_sampler / hip_no_cache / hip_cache: the sun draws for every new "
                      "tracer, hip_cache reuses its kept sample")
    res["reference_epoch"] = epochs
    print("[sampler] epoch ms: " + ", ".join(f"{k} {v}" for k, v in epochs.items() if k != "what"), flush=True)
    return finish(res, args.out)


def shape_pair(res, args, ops, shape_sun, law, sizes, R, P, dev):
    """The radial kernel and the Gaussian kernel, two rounds each in turn (the same-run spread), per size."""
    table = shape_sun.quantile_table
    res["shape"] = {"distribution_type": args.shape, "K": int(table.shape[0]) - 1, "lds_bytes_per_workgroup": 8 * (int(table.shape[0]) - 1)}
    for label, rows in sizes:
        nbytes = len(rows) * R * P * 8
        rows_t = torch.tensor(rows, dtype=torch.int64, device=dev)
        kernels = {"gaussian": lambda: ops.sample_distortions(rows_t, R, P, 7, *law, dev),
                   "radial": lambda: ops.sample_radial_distortions(rows_t, R, P, 7, (0.0, 0.0), table, dev)}
        rounds = {name: [] for name in kernels}
        for _ in range(2):
            for name, fn in kernels.items():
                rounds[name].append(event_ms(fn, args.steps, args.warmup))
                torch.cuda.empty_cache()
        entry = {"rows": len(rows), "bytes": nbytes, "write_floor_ms": nbytes / WRITE_RATE * 1e3}
        for name, got in rounds.items():
            median = min(r["median_ms"] for r in got)
            entry[name] = {"rounds": got, "median_ms": median, "GBps": nbytes / median / 1e6,
                           "fraction_of_write_rate": nbytes / (median * 1e-3) / WRITE_RATE}
        entry["radial_over_gaussian"] = entry["radial"]["median_ms"] / entry["gaussian"]["median_ms"]
        res["draws"][label] = entry
        print(f"[sampler] {label}: {len(rows)} rows, gaussian {entry['gaussian']['median_ms']:.3f} ms, {args.shape} "
              f"{entry['radial']['median_ms']:.3f} ms (ratio {entry['radial_over_gaussian']:.3f})", flush=True)
    res["what"] = ("ms per draw from device events; per kernel two rounds of --steps draws, alternating gaussian / radial, "
                   "median_ms = the lower of the two round medians; rows travel as a device tensor in both")
    return res


def finish(res, out):
    out = pathlib.Path(out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
