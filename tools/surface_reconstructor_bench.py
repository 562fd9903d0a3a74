#!/usr/bin/env python3
"""Wall time per epoch of ``artist_amd.optim.SurfaceReconstructor`` against the hand-assembled epoch that ``bench.py`` times.

Two sizes: the fixture's (tests/golden/surface_reconstructor_class_epochs.npz: three heliostats of test_blocking.h5 with three
training samples each, 10 x 10 points per facet, 3 rays, 64 x 64 bitmaps) and 40 heliostats x 4 samples on the synthetic field
(three training samples each = 120 traced samples of 10^4 points, 10 rays per point, 256 x 256 bitmaps).

* ``class``: an epoch as ``reconstruct_surfaces`` runs it between two validations - zero_grad, ``predict_flux``, ``epoch_loss``
  (PixelLoss, constraint, both regularisers), backward, multiplier, edge lock, ``Adam.step()``, the epoch's six scalars in one
  ``tolist()`` (the synchronisation that ends the epoch), scheduler.
* ``class+validation``: the same epoch followed by ``validate`` (and so by a re-activation in the next epoch).
* ``class, epoch_graph`` / ``class+validation, epoch_graph``: the same two with the training step replayed from the
  ``EpochGraph`` that ``epoch_graph=True`` builds (``build_epoch_graph``): zero_grad, ``replay()``, multiplier (in place), edge
  lock, ``Adam.step()``, the six scalars, scheduler.  Also recorded: the build (warm-up + capture) in ms and in eager epochs.
* ``assembled``: the epoch of ``bench.py``'s kind with one control net PER SAMPLE: fused NURBS + alignment, trace, fused
  crop + pixel loss, sum, backward, ``Adam.step()`` with the edge lock in the kernel, ``loss.item()``.  No constraint, no
  regularisers, no scheduler: the floor of what the kernels cost at this size.

A measurement is the host clock around ONE epoch, which ends in a device synchronisation; warm-up epochs come first and are not
counted; the variants alternate in blocks inside one process; every epoch's time is kept, median and spread are reported.  Also
recorded: the synchronising calls of one epoch, counted with ``torch.cuda.set_sync_debug_mode("warn")``, and
``reconstruct_surfaces`` as a whole (prepare, epochs, two validations, ``update_surfaces``) per epoch, eagerly and with
``epoch_graph=True``.  ``replay_within_eager_spread``: the replayed epoch's median does not exceed the eager median of the same
call by more than that call's eager p90 - p10.

``--parameters`` (repeatable; one choice per occurrence, its names separated by commas, e.g. ``--parameters
nurbs_control_points --parameters canting --parameters nurbs_control_points,canting,facet_translations``): instead of the
above, the ``class`` epoch and its replayed form for every choice of ``SurfaceReconstructor(parameters=...)``, the choices
alternating in blocks inside one process, at both sizes.  One record per choice is written under ``"parameters"`` into the
existing file, beside the records that are there; the record of the default choice is compared with the file's own ``class``
records (``not_above_recorded_p90``: its median does not exceed their p90; ``within_recorded_spread``: nor is it below their
p10 - epochs at these sizes are host time, which differs between sessions by more than a session's own spread).

usage: python tools/surface_reconstructor_bench.py [--out profiles/surface_reconstructor_bench.json] [--epochs 30] [--blocks 3]
                                                   [--parameters NAMES]...
"""
import argparse
import json
import pathlib
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEV = torch.device("cuda:0")
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
SUNS = [[0.0, 0.8, -0.6, 0.0], [0.1, 1.0, -0.2, 0.0], [-0.25, 0.9, -0.35, 0.0], [0.2, 0.85, -0.5, 0.0]]


def configuration(max_epoch):
    return dict(optimization=dict(initial_learning_rate=1e-6, tolerance=0.0, max_epoch=max_epoch, batch_size=30, log_step=0,
                                  early_stopping_delta=1e-9, early_stopping_patience=10 ** 6, early_stopping_window=10),
                scheduler=dict(scheduler_type="exponential", gamma=0.999),
                constraints=dict(rho_flux_integral=1.0, energy_tolerance=0.01, weight_smoothness=0.005, weight_ideal_surface=0.005))


def fixture_case():
    """(scenario factory, six parser tensors, points per facet, resolution) at the fixture's size."""
    from artist_amd.scenario import Scenario, open_scenario_file
    d = dict(np.load(ROOT / "tests" / "golden" / "surface_reconstructor_class_epochs.npz"))
    points = torch.tensor([int(v) for v in d["points_per_facet"]])

    def scenario():
        with open_scenario_file(ROOT / "tests" / "golden" / "scenarios" / "test_blocking.h5") as scenario_file:
            s = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file, number_of_surface_points_per_facet=points, device=DEV)
        s.set_number_of_rays(number_of_rays=int(d["n_rays"]))
        return s

    t = lambda key, dtype=torch.float32: torch.as_tensor(d[key], dtype=dtype).to(DEV)  # noqa: E731
    six = (t("parser_flux_measured"), t("parser_focal_spots"), t("parser_incident_ray_directions"), t("parser_motor_positions"),
           t("parser_mask", torch.int32), t("parser_target_area_indices", torch.long))
    return scenario, six, points, torch.tensor([int(v) for v in d["resolution"]])


def synthetic_case(heliostats=40, samples=4, rays=10, n_eval=50, resolution=256):
    from artist_amd.scene import build_synthetic_scenario

    def scenario():
        return build_synthetic_scenario(heliostats, n_rays=rays, n_cp=(10, 10), n_eval=n_eval, device=DEV)[0]

    n = heliostats * samples
    incident = torch.nn.functional.normalize(torch.tensor(SUNS[:samples]), dim=1).repeat(heliostats, 1).to(DEV)
    measured = (torch.rand((n, resolution, resolution), generator=torch.Generator().manual_seed(1)) + 0.1).to(DEV)
    six = (measured, torch.zeros(n, 4, device=DEV), incident, torch.zeros(n, 2, device=DEV),
           torch.full((heliostats,), samples, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV))
    return scenario, six, torch.tensor([n_eval, n_eval]), torch.tensor([resolution, resolution])


class ClassEpoch:
    def __init__(self, case, max_epoch=10 ** 6, parameters=None):
        from artist_amd import CalibrationSamples, PixelLoss
        from artist_amd.optim import SurfaceReconstructor
        scenario, six, points, resolution = case
        self.reconstructor = SurfaceReconstructor(
            ddp_setup=DDP, scenario=scenario(), data={"data_parser": CalibrationSamples(six), "heliostat_data_mapping": []},
            optimization_configuration=configuration(max_epoch), number_of_surface_points=points, bitmap_resolution=resolution,
            device=DEV, **({} if parameters is None else dict(parameters=parameters)))
        self.loss_definition = PixelLoss()
        self.state = None

    def prepare(self):
        self.state = self.reconstructor.prepare(0, DEV)

    def step(self, validate=False):
        r, state = self.reconstructor, self.state
        state.optimizer.zero_grad()
        loss = r.epoch_loss(state, r.predict_flux(state, DEV), self.loss_definition, DEV)
        loss.total.backward()
        r.update_multiplier(state, loss.violation)
        r._synchronize_and_lock_learnables(state, DEV)
        state.optimizer.step()
        scalars = loss.scalars().tolist()
        state.scheduler.step()
        if validate:
            r.validate(state, DEV)
        return scalars[0]


class GraphEpoch(ClassEpoch):
    """The class epoch as ``reconstruct_surfaces`` runs it with ``epoch_graph=True``: the training step is a replay."""

    def prepare(self):
        super().prepare()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.graph = self.reconstructor.build_epoch_graph(self.state, self.loss_definition, DEV)
        torch.cuda.synchronize()
        self.build_ms = 1e3 * (time.perf_counter() - t0)

    def step(self, validate=False):
        r, state = self.reconstructor, self.state
        state.optimizer.zero_grad()
        scalars, _, _, violation = self.graph.replay()
        r.update_multiplier(state, violation)
        r._synchronize_and_lock_learnables(state, DEV)
        state.optimizer.step()
        scalars = scalars.tolist()
        state.scheduler.step()
        if validate:
            r.validate(state, DEV)
        return scalars[0]


class AssembledEpoch:
    """bench.py's epoch at the same number of traced samples: one control net per sample."""

    def __init__(self, case):
        from artist_amd import HeliostatRayTracer, training
        from artist_amd.optim import Adam
        from artist_amd.scene import ideal_orientations
        scenario, six, points, resolution = case
        self.scenario = scenario = scenario()
        self.group = group = scenario.heliostat_field.heliostat_groups[0]
        split = training.train_test_split(six[4], six[0], six[1], six[2], six[3], six[5], device=DEV)
        self.mask, self.incident, self.targets = split.active_heliostats_mask_train, split.incident_ray_directions_train, split.target_area_indices_train
        self.measured = split.flux_measured_train
        group.activate_heliostats(self.mask, DEV)
        aim = scenario.solar_tower.get_centers_of_target_areas(self.targets)
        with torch.no_grad():
            if group.kinematics is not None:
                self.orientation = group.kinematics.incident_ray_directions_to_orientations(self.incident, aim, device=DEV)
            else:
                self.orientation = ideal_orientations(group.active_positions, aim, self.incident)
        self.cp = group.active_nurbs_control_points.detach().clone().requires_grad_(True)
        self.samples = self.cp.shape[0]
        from artist_amd import create_nurbs_evaluation_grid
        self.uv = create_nurbs_evaluation_grid(points, device=DEV)[None, None].expand(self.samples, group.number_of_facets_per_heliostat, -1, -1)
        self._evaluate()
        self.tracer = HeliostatRayTracer(scenario, group, blocking_active=False, random_seed=0, bitmap_resolution=resolution)
        self.optimizer = Adam([self.cp], lr=1e-6, lock_outer_edges=True)

    def _evaluate(self):
        from artist_amd import NURBSSurfaces
        group = self.group
        pts, nrm = NURBSSurfaces(group.nurbs_degrees, self.cp, device=DEV).calculate_surface_points_and_normals(
            self.uv, group.active_canting, group.active_facet_translations, orientations=self.orientation)
        group.active_surface_points, group.active_surface_normals = pts.reshape(self.samples, -1, 4), nrm.reshape(self.samples, -1, 4)

    def prepare(self):
        pass

    def step(self, validate=False):
        from artist_amd import crop_and_pixel_loss
        self.optimizer.zero_grad()
        self._evaluate()
        flux, *_ = self.tracer.trace_rays(self.incident, self.mask, self.targets)
        loss = crop_and_pixel_loss(flux, self.scenario.solar_tower, self.targets, self.measured).sum()
        loss.backward()
        self.optimizer.step()
        return loss.item()


def summary(times_ms):
    q = statistics.quantiles(times_ms, n=10) if len(times_ms) >= 10 else [min(times_ms)] * 9
    return dict(median_ms=statistics.median(times_ms), min_ms=min(times_ms), p10_ms=q[0], p90_ms=q[-1], max_ms=max(times_ms),
                epochs=len(times_ms))


def count_syncs(fn):
    """The synchronising calls torch reports during ``fn()``."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return len([w for w in caught if "synchroniz" in str(w.message).lower()])


def measure(name, case, epochs, blocks, warmup):
    variants = {"class": (ClassEpoch(case), False), "class, epoch_graph": (GraphEpoch(case), False),
                "class+validation": (ClassEpoch(case), True), "class+validation, epoch_graph": (GraphEpoch(case), True),
                "assembled": (AssembledEpoch(case), False)}
    times = {key: [] for key in variants}
    for key, (epoch, validate) in variants.items():
        epoch.prepare()
        for _ in range(warmup):
            epoch.step(validate)
    for _ in range(blocks):                              # alternating blocks inside one process
        for key, (epoch, validate) in variants.items():
            torch.cuda.synchronize()
            for _ in range(epochs):
                t0 = time.perf_counter()
                epoch.step(validate)
                torch.cuda.synchronize()
                times[key].append(1e3 * (time.perf_counter() - t0))
    result = {key: summary(v) | dict(all_ms=[round(x, 4) for x in v]) for key, v in times.items()}
    result["synchronising_calls"] = {
        "epoch (the loop's tolist)": count_syncs(lambda: variants["class"][0].step(False)),
        "epoch + validation": count_syncs(lambda: variants["class+validation"][0].step(True)),
        "epoch after a validation (re-activation)": count_syncs(lambda: variants["class+validation"][0].step(False)),
        "assembled": count_syncs(lambda: variants["assembled"][0].step(False)),
        "epoch_graph: epoch (the loop's tolist)": count_syncs(lambda: variants["class, epoch_graph"][0].step(False)),
        "epoch_graph: epoch + validation": count_syncs(lambda: variants["class+validation, epoch_graph"][0].step(True)),
        "epoch_graph: epoch after a validation (no re-activation)": count_syncs(lambda: variants["class+validation, epoch_graph"][0].step(False))}
    for eager, replayed in (("class", "class, epoch_graph"), ("class+validation", "class+validation, epoch_graph")):
        e, g = result[eager], result[replayed]
        g["eager_median_ms"], g["eager_over_replayed"] = e["median_ms"], e["median_ms"] / g["median_ms"]
        g["eager_p90_minus_p10_ms"] = e["p90_ms"] - e["p10_ms"]
        g["replay_within_eager_spread"] = g["median_ms"] <= e["median_ms"] + g["eager_p90_minus_p10_ms"]
        g["build_ms"] = variants[replayed][0].build_ms
        g["build_in_eager_epochs"] = g["build_ms"] / e["median_ms"]
    # the whole call: prepare, max_epoch + 1 epochs, validations after the first and the last but one, update_surfaces
    run_epochs = max(epochs, 4)
    whole = ClassEpoch(case, max_epoch=run_epochs - 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, histories = whole.reconstructor.reconstruct_surfaces(whole.loss_definition, DEV)
    torch.cuda.synchronize()
    result["reconstruct_surfaces"] = dict(total_ms=1e3 * (time.perf_counter() - t0), epochs=len(histories[0][0]["total_loss"]))
    result["reconstruct_surfaces"]["ms_per_epoch"] = result["reconstruct_surfaces"]["total_ms"] / result["reconstruct_surfaces"]["epochs"]
    whole = ClassEpoch(case, max_epoch=run_epochs - 1)
    whole.reconstructor.epoch_graph = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, histories = whole.reconstructor.reconstruct_surfaces(whole.loss_definition, DEV)
    torch.cuda.synchronize()
    result["reconstruct_surfaces, epoch_graph"] = dict(total_ms=1e3 * (time.perf_counter() - t0), epochs=len(histories[0][0]["total_loss"]))
    result["reconstruct_surfaces, epoch_graph"]["ms_per_epoch"] = \
        result["reconstruct_surfaces, epoch_graph"]["total_ms"] / result["reconstruct_surfaces, epoch_graph"]["epochs"]
    print(f"[{name}] " + ", ".join(f"{key}: median {v['median_ms']:.3f} ms (min {v['min_ms']:.3f}, p10 {v['p10_ms']:.3f}, p90 {v['p90_ms']:.3f}, "
                                   f"max {v['max_ms']:.3f})" for key, v in result.items() if "median_ms" in v), flush=True)
    print(f"[{name}] synchronising calls: {result['synchronising_calls']}; reconstruct_surfaces: {result['reconstruct_surfaces']}; "
          f"with epoch_graph: {result['reconstruct_surfaces, epoch_graph']}", flush=True)
    for key in ("class, epoch_graph", "class+validation, epoch_graph"):
        print(f"[{name}] {key}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in result[key].items()
                                                if k not in ("all_ms",)), flush=True)
    return result


def measure_parameters(name, case, choices, epochs, blocks, warmup):
    """The class epoch, eager and replayed, per choice of ``parameters``: ``{label: {"class": ..., "class, epoch_graph": ...}}``."""
    variants = {}
    for choice in choices:
        label = ",".join(choice)
        variants[label, "class"] = ClassEpoch(case, parameters=choice)
        variants[label, "class, epoch_graph"] = GraphEpoch(case, parameters=choice)
    times = {key: [] for key in variants}
    for epoch in variants.values():
        epoch.prepare()
        for _ in range(warmup):
            epoch.step(False)
    for _ in range(blocks):                              # alternating blocks inside one process
        for key, epoch in variants.items():
            torch.cuda.synchronize()
            for _ in range(epochs):
                t0 = time.perf_counter()
                epoch.step(False)
                torch.cuda.synchronize()
                times[key].append(1e3 * (time.perf_counter() - t0))
    result = {}
    for (label, kind), v in times.items():
        result.setdefault(label, {})[kind] = summary(v)
        print(f"[{name}] parameters={label}, {kind}: median {result[label][kind]['median_ms']:.3f} ms (p10 "
              f"{result[label][kind]['p10_ms']:.3f}, p90 {result[label][kind]['p90_ms']:.3f})", flush=True)
    return result


def main_parameters(args):
    """One record per choice into the existing file, beside what is there."""
    from artist_amd.surface_reconstructor import canonical_parameters
    choices = []
    for given in args.parameters:
        choice = canonical_parameters([part.strip() for part in given.split(",") if part.strip()])
        if choice not in choices:
            choices.append(choice)
    path = pathlib.Path(args.out)
    out = json.loads(path.read_text()) if path.exists() else {}
    cases = dict(fixture=("fixture: 3 heliostats x 3 training samples, 400 points, 3 rays, 64 x 64", fixture_case),
                 synthetic_40x4=("synthetic: 40 heliostats x 3 training samples, 10^4 points, 10 rays, 256 x 256", synthetic_case))
    records = out.setdefault("parameters", {})
    for size, (name, case) in cases.items():
        measured = measure_parameters(name, case(), choices, args.epochs, args.blocks, args.warmup)
        default = measured.get("nurbs_control_points")
        for label, record in measured.items():
            if default is not None and label != "nurbs_control_points":
                for kind in record:
                    record[kind]["over_default_ms"] = record[kind]["median_ms"] - default[kind]["median_ms"]
            elif label == "nurbs_control_points":
                for kind in record:                  # against the record that is in the file: the commit before this choice existed
                    recorded = out.get(size, {}).get(kind)
                    if recorded is not None:
                        record[kind].update(recorded_median_ms=recorded["median_ms"], recorded_p10_ms=recorded["p10_ms"],
                                            recorded_p90_ms=recorded["p90_ms"],
                                            not_above_recorded_p90=record[kind]["median_ms"] <= recorded["p90_ms"],
                                            within_recorded_spread=recorded["p10_ms"] <= record[kind]["median_ms"] <= recorded["p90_ms"])
            records.setdefault(label, dict(device=torch.cuda.get_device_name(DEV), epochs_per_block=args.epochs, blocks=args.blocks,
                                           warmup=args.warmup))[size] = record
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "surface_reconstructor_bench.json"))
    ap.add_argument("--epochs", type=int, default=30, help="timed epochs per block and variant")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parameters", action="append", default=None, metavar="NAMES",
                    help="a choice of SurfaceReconstructor(parameters=...), names separated by commas; repeatable: one record per choice")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_reconstructor_bench.py measures on the GPU; no GPU found")
    if args.parameters:
        return main_parameters(args)
    out = dict(device=torch.cuda.get_device_name(DEV), epochs_per_block=args.epochs, blocks=args.blocks, warmup=args.warmup,
               fixture=measure("fixture: 3 heliostats x 3 training samples, 400 points, 3 rays, 64 x 64", fixture_case(), args.epochs,
                               args.blocks, args.warmup),
               synthetic_40x4=measure("synthetic: 40 heliostats x 3 training samples, 10^4 points, 10 rays, 256 x 256", synthetic_case(),
                                      args.epochs, args.blocks, args.warmup))
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
