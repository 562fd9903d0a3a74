#!/usr/bin/env python3
"""Wall time per reconstruction epoch, eager against replayed from an ``artist_amd.EpochGraph``.

The epoch is NURBS (control points as the leaf, fused alignment) -> trace_rays -> crop + pixel loss -> backward, followed by
the eager ``artist_amd.optim.Adam.step()`` in BOTH variants (the optimiser step stays outside the graph).  A measurement is N
epochs enqueued back to back and one device synchronisation at the end, wall clock; the two variants alternate inside one
process, warm-up comes before timing, no profiler.  Fields of 1, 4, 40 and 125 heliostats with 10^4 points each, 10 and 100 rays
per point, 256 x 256 bitmaps, blocking off and on - with blocking on the epoch is not captured (the library refuses it), so only
the eager times are recorded there.  Every repeat is kept so that the spread can be seen.

Also recorded: the library entry points an eager epoch calls, counted by wrapping the ctypes handle for one epoch (each is
one or more kernel launches; torch's own kernels - the loss sum, its backward - are not in that number).

usage: python tools/graph_bench.py [--out profiles/graph_bench.json] [--epochs 40] [--repeats 5] [--fields 1,4,40,125]
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEV = torch.device("cuda:0")


class Epoch:
    def __init__(self, H, R, blocking, resolution=256, n_eval=50):
        from artist_amd import HeliostatRayTracer, NURBSSurfaces, scene
        from artist_amd.optim import Adam
        self.H = H
        scenario, self.uv = scene.build_synthetic_scenario(H, n_rays=R, n_cp=(6, 6), n_eval=n_eval, device=DEV)
        self.tower = scenario.solar_tower
        self.group = group = scenario.heliostat_field.heliostat_groups[0]
        self.mask = torch.ones(H, dtype=torch.int32, device=DEV)
        self.tix = torch.zeros(H, dtype=torch.long, device=DEV)
        self.inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
        group.activate_heliostats(self.mask, DEV)
        self.orientation = scene.ideal_orientations(group.active_positions, self.tower.get_centers_of_target_areas(self.tix), self.inc)
        self.cp = group.active_nurbs_control_points.clone().requires_grad_(True)
        with torch.no_grad():       # the tracer takes its blocking rectangles from the aligned surfaces it finds
            pts, nrm = NURBSSurfaces(group.nurbs_degrees, self.cp, device=DEV).calculate_surface_points_and_normals(
                self.uv, group.active_canting, group.active_facet_translations, orientations=self.orientation)
            group.active_surface_points, group.active_surface_normals = pts.reshape(H, -1, 4), nrm.reshape(H, -1, 4)
        self.tracer = HeliostatRayTracer(scenario, group, blocking_active=blocking,
                                         bitmap_resolution=torch.tensor([resolution, resolution]))
        self.truth = torch.rand((H, resolution, resolution), generator=torch.Generator().manual_seed(1)).to(DEV) + 0.1
        self.optimizer = Adam([self.cp], lr=1e-5)

    def step(self):
        from artist_amd import NURBSSurfaces, crop_and_pixel_loss
        group, H = self.group, self.H
        pts, nrm = NURBSSurfaces(group.nurbs_degrees, self.cp, device=DEV).calculate_surface_points_and_normals(
            self.uv, group.active_canting, group.active_facet_translations, orientations=self.orientation)
        group.active_surface_points, group.active_surface_normals = pts.reshape(H, -1, 4), nrm.reshape(H, -1, 4)
        flux, *_ = self.tracer.trace_rays(self.inc, self.mask, self.tix)
        loss = crop_and_pixel_loss(flux, self.tower, self.tix, self.truth).sum()
        loss.backward()
        return loss


def count_library_calls(epoch):
    from artist_amd import _lib
    handle, calls, saved = _lib.lib(), [], {}
    for name in _lib.SIGNATURES:
        if name.startswith("art_") and name not in ("art_abi_version", "art_last_hip_error", "art_strerror"):
            saved[name] = getattr(handle, name)

            def wrapped(*args, _real=saved[name], _name=name):
                calls.append(_name)
                return _real(*args)
            setattr(handle, name, wrapped)
    try:
        epoch.optimizer.zero_grad(set_to_none=True)
        epoch.step()
        epoch.optimizer.step()
        torch.cuda.synchronize()
    finally:
        for name, real in saved.items():
            setattr(handle, name, real)
    return calls


def timed(run_epoch, epochs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        run_epoch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / epochs * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_bench.json"))
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fields", default="1,4,40,125")
    ap.add_argument("--rays", default="10,100")
    args = ap.parse_args()
    from artist_amd import EpochGraph, ops
    results = []
    for H in (int(v) for v in args.fields.split(",")):
        for R in (int(v) for v in args.rays.split(",")):
            for blocking in (False, True):
                epoch = Epoch(H, R, blocking)
                calls = count_library_calls(epoch)

                def eager():
                    epoch.optimizer.zero_grad(set_to_none=True)
                    epoch.step()
                    epoch.optimizer.step()

                for _ in range(3):
                    eager()
                graph, refused, captured = None, None, None
                if blocking:                                     # not captured: the eager times are the record
                    refused = "blocking under graph capture is refused by the library"
                else:
                    # a field of its own: the eager epoch's leaf has an AccumulateGrad node on the default stream by now
                    # (EpochGraph, "Fresh leaves")
                    captured = Epoch(H, R, blocking)
                    graph = EpochGraph(captured.step, warmup=2)

                def replayed():
                    graph.replay()
                    captured.optimizer.step()

                for _ in range(3 if graph is not None else 0):
                    replayed()
                t_eager, t_replay = [], []
                for _ in range(args.repeats):                    # the variants alternate
                    t_eager.append(timed(eager, args.epochs))
                    if graph is not None:
                        t_replay.append(timed(replayed, args.epochs))
                ops.check_async_errors(DEV)
                row = dict(heliostats=H, rays=R, points=int(epoch.group.active_surface_points.shape[1]), blocking=blocking,
                           epochs_per_repeat=args.epochs, eager_us=t_eager, replay_us=t_replay or None, replay_refused=refused,
                           eager_median_us=statistics.median(t_eager),
                           replay_median_us=statistics.median(t_replay) if t_replay else None,
                           eager_spread_us=max(t_eager) - min(t_eager),
                           ratio=statistics.median(t_eager) / statistics.median(t_replay) if t_replay else None,
                           library_calls_per_eager_epoch=len(calls), library_calls=calls)
                results.append(row)
                print(json.dumps({k: v for k, v in row.items() if k != "library_calls"}), flush=True)
                if graph is not None:
                    graph.close()
                del graph, epoch, captured
                torch.cuda.empty_cache()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results), indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
