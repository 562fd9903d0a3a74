#!/usr/bin/env python3
"""Cost of shading: the blocking bench's field (40 columns x 25 rows, 4.2 m x 5 m pitch) under a low sun (15 degrees above
the southern horizon), forward and forward + backward, blocking only against blocking + shading; also the cull and the
table kernels on their own and the lengths of the lists, once per value of ``artist_amd.ops.SHADING_SLOTS`` asked for (a
heliostat with more possible shaders than slots comes back NaN, and its overflowed row is read in full: such a run measures
the overflow, not shading).  Prints one JSON line (kept in profiles/shading_bench.json).

    python tools/shading_bench.py [--heliostats 1000] [--rays 100] [--steps 5] [--slots 8,16] [--out profiles/shading_bench.json]
"""
import argparse
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from artist_amd import HeliostatRayTracer, ops  # noqa: E402
from artist_amd.blocking import ShadingTables, create_blocking_primitives_rectangles_by_index, shading_cull  # noqa: E402
from artist_amd.scene import build_synthetic_scenario  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, steps):
    """Mean milliseconds per call over ``steps`` calls between two events on the stream, after two warm-up calls."""
    for _ in range(2):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heliostats", type=int, default=1000)
    ap.add_argument("--rays", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--slots", default="8,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    H, R = args.heliostats, args.rays
    scenario, _ = build_synthetic_scenario(H, n_rays=R, device=dev)
    g = scenario.heliostat_field.heliostat_groups[0]
    i = torch.arange(H, device=dev)
    g.positions = torch.stack([((i % 40) - 19.5) * 4.2, 60.0 + (i // 40) * 5.0, torch.zeros(H, device=dev), torch.ones(H, device=dev)], dim=1)
    mask = torch.ones(H, dtype=torch.int32, device=dev)
    g.activate_heliostats(mask)
    tix = torch.zeros(H, dtype=torch.long, device=dev)
    inc = torch.nn.functional.normalize(torch.tensor([[0.0, 0.9659, -0.2588, 0.0]], device=dev), dim=1).repeat(H, 1)
    g.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
    pts = g.active_surface_points.detach().requires_grad_(True)
    g.active_surface_points = pts
    result = {"H": H, "R": R, "P": int(pts.shape[1]), "rays": H * R * int(pts.shape[1]), "sun_elevation_deg": 15.0,
              "device": torch.cuda.get_device_name(0)}
    for slots in (int(v) for v in args.slots.split(",")):
        ops.SHADING_SLOTS = slots
        result[f"slots_{slots}"] = measure(args, scenario, g, mask, tix, inc, pts, H)
    line = json.dumps(result)
    print(line)
    if args.out:
        pathlib.Path(args.out).write_text(line + "\n")


def measure(args, scenario, g, mask, tix, inc, pts, H):
    out = {"shading_slots": ops.SHADING_SLOTS}
    for label, kw in (("blocking", dict(blocking_active=True)), ("blocking_and_shading", dict(blocking_active=True, shading_active=True)),
                      ("shading_only", dict(blocking_active=False, shading_active=True))):
        rt = HeliostatRayTracer(scenario, g, **kw)
        rt.lbvh_compat = False
        flux, intercept, on_target, unblocked = rt.trace_rays(inc, mask, tix)
        w = torch.rand_like(flux)

        def fwd():
            return rt.trace_rays(inc, mask, tix)[0]

        def fwd_bwd():
            pts.grad = None
            (rt.trace_rays(inc, mask, tix)[0] * w).sum().backward(retain_graph=True)   # the rectangles hang off the constructor's graph

        row = {"fwd_ms": timed(fwd, args.steps), "fwd_bwd_ms": timed(fwd_bwd, args.steps),
               "mean_free_fraction": float(torch.nan_to_num(unblocked, nan=0.0).mean()), "flux_sum": float(torch.nan_to_num(flux.detach()).sum()),
               "heliostats_nan": int(torch.isnan(unblocked).sum())}
        fwd()
        counts = ops._LAST_BLOCKING[1]
        row.update(candidates_max=int(counts.max()), candidates_mean=float(counts.float().mean()),
                   heliostats_beyond_32=int((counts > 32).sum()))
        if rt.shading_active:
            found = rt._shading[1]
            row.update(shaders_max=int(found.max()), shaders_mean=float(found.float().mean()),
                       heliostats_beyond_slots=int((found > ops.SHADING_SLOTS).sum()))
        out[label] = row
    # the new kernels on their own
    corners = create_blocking_primitives_rectangles_by_index(pts.detach())[0]
    owner = torch.arange(H, dtype=torch.int32, device=dev)
    scatter = rt._max_scatter_angle()
    out["cull_ms"] = timed(lambda: shading_cull(corners, owner, inc, scatter), 20)
    idx, _ = shading_cull(corners, owner, inc, scatter)
    out["tables_fwd_ms"] = timed(lambda: ShadingTables.apply(corners, owner, inc, idx), 20)
    leaf = corners.clone().requires_grad_(True)

    def tables_fwd_bwd():
        leaf.grad = None
        c, s, n = ShadingTables.apply(leaf, owner, inc, idx)
        (c.sum() + s.sum() + n.sum()).backward()

    out["tables_fwd_bwd_ms"] = timed(tables_fwd_bwd, 20)
    ops.check_async_errors(dev)
    return out


if __name__ == "__main__":
    main()
