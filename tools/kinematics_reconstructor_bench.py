#!/usr/bin/env python3
"""What does an epoch of ``artist_amd.optim.KinematicsReconstructor`` cost?  

Both modes - flux-driven with ``FocalSpotLoss``, alignment-driven with ``AngleLoss`` - at two sizes:

* ``fixture``: the case of tests/golden/kinematics_reconstructor_class_*.npz - six heliostats of test_blocking.h5, four of them with
  three training samples and one test sample, 400 surface points, 3 rays, 64 x 64 bitmaps.
* ``synthetic_100x4``: 100 heliostats of the synthetic field with ideal actuators, four samples each (three for training), 10^4
  surface points, 10 rays, 256 x 256 bitmaps; measured from the true (zero) deviations, started 3e-3 rad away.

An epoch is what the loop of ``reconstruct_kinematics`` does: ``zero_grad``, ``epoch_loss``, ``backward``, (``nan_to_num_``),
``step``, ``loss.item()``, the scheduler - and, as ``<method>, epoch_graph``, the same with ``epoch_loss`` + ``backward`` replayed from
the ``EpochGraph`` that ``epoch_graph=True`` builds (``build_epoch_graph``), eager and replayed alternating in one process; the
build (warm-up + capture) is recorded in ms and in eager epochs, and ``replay_within_eager_spread`` says whether the replayed
median stays within the eager median plus the eager p90 - p10 of the same call.  A measurement is the host clock around ONE epoch, which ends in the loop's read of the
loss; warm-up epochs come first and are not counted; every epoch's time is kept, median and spread are reported.  Also recorded:
the calls into the library per epoch by entry point (each is one kernel launch or a few), and the synchronising calls of one
epoch, of an epoch with its validation and of the epoch after a validation, counted with ``torch.cuda.set_sync_debug_mode("warn")``.

``--parameters a,b,...`` ("More kinematic parameters") measures something else: per size and mode the epoch that
learns the rotation deviations alone beside the epoch that learns the given tensors (``KINEMATICS_PARAMETER_NAMES``), eager and
replayed, all alternating in one process.  A name that a variant cannot learn is left out of that variant and said so
(``left_out``): the translation deviations in the alignment-driven mode, the actuator parameters on the synthetic field's ideal
actuators.  The fixture's two extra tensors keep the file's values.  Written to ``--out``, by default
profiles/kinematics_parameters_bench.json.

usage: python tools/kinematics_reconstructor_bench.py [--out profiles/kinematics_reconstructor_bench.json] [--epochs 30] [--blocks 3]
                                                      [--parameters rotation_deviations,translation_deviations,actuator_parameters]
"""
import argparse
import collections
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
SUNS = [[0.1, 1.0, -0.2, 0.0], [-0.25, 0.9, -0.35, 0.0], [0.3, 0.8, -0.3, 0.0], [0.0, 1.0, -0.5, 0.0]]
METHODS = ("raytracing", "alignment")
CONFIGURATION = dict(optimization=dict(initial_learning_rate_rotation_deviation=1e-6, tolerance=0.0, max_epoch=10 ** 6, batch_size=30,
                                       log_step=0, early_stopping_delta=1e-9, early_stopping_patience=10 ** 6, early_stopping_window=10),
                     scheduler=dict(scheduler_type="exponential", gamma=0.999))


def fixture_case(method):
    """(scenario, six parser tensors, resolution) at the fixture's size, the deviations at the reference's start."""
    from artist_amd.scenario import Scenario, open_scenario_file
    name = "flux" if method == "raytracing" else "alignment"
    d = dict(np.load(ROOT / "tests" / "golden" / f"kinematics_reconstructor_class_{name}.npz"))
    points = torch.tensor([int(v) for v in d["points_per_facet"]])
    with open_scenario_file(ROOT / "tests" / "golden" / "scenarios" / "test_blocking.h5") as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file, number_of_surface_points_per_facet=points, device=DEV)
    scenario.set_number_of_rays(number_of_rays=int(d["n_rays"]))
    t = lambda key, dtype=torch.float32: torch.as_tensor(d[key], dtype=dtype).to(DEV)  # noqa: E731
    scenario.heliostat_field.heliostat_groups[0].kinematics.rotation_deviation_parameters = t("rotation_start")[0].contiguous()
    six = (t("parser_flux_measured"), t("parser_focal_spots"), t("parser_incident_ray_directions"), t("parser_motor_positions"),
           t("parser_mask", torch.int32), t("parser_target_area_indices", torch.long))
    return scenario, six, torch.tensor([int(v) for v in d["resolution"]])


def synthetic_case(method, heliostats=100, samples=4, rays=10, n_eval=50, resolution=256, sigma=3e-3):
    """The synthetic field with a rigid-body kinematics of ideal actuators; calibration data from the true (zero) deviations."""
    from artist_amd import HeliostatRayTracer, RigidBody
    from artist_amd.scene import build_synthetic_scenario
    scenario = build_synthetic_scenario(heliostats, n_rays=rays, n_cp=(10, 10), n_eval=n_eval, device=DEV)[0]
    group = scenario.heliostat_field.heliostat_groups[0]
    actuators = torch.tensor([[1.0, 1.0], [0.0, 1.0], [0.0, 0.0], [70000.0, 75000.0]], device=DEV).repeat(heliostats, 1, 1)
    group.kinematics = RigidBody(number_of_heliostats=heliostats, heliostat_positions=group.positions,
                                 initial_orientations=torch.tensor([[0.0, -1.0, 0.0, 0.0]], device=DEV).repeat(heliostats, 1),
                                 translation_deviation_parameters=torch.zeros(heliostats, 9, device=DEV),
                                 rotation_deviation_parameters=torch.zeros(heliostats, 4, device=DEV),
                                 actuator_parameters_non_optimizable=actuators, device=DEV)
    n = heliostats * samples
    mask = torch.full((heliostats,), samples, dtype=torch.int32, device=DEV)
    targets = torch.zeros(n, dtype=torch.long, device=DEV)
    incident = torch.nn.functional.normalize(torch.tensor(SUNS[:samples]), dim=1).repeat(heliostats, 1).to(DEV)
    size = torch.tensor([resolution, resolution])
    with torch.no_grad():
        centres = scenario.solar_tower.get_centers_of_target_areas(target_area_indices=targets, device=DEV)
        group.activate_heliostats(active_heliostats_mask=mask, device=DEV)
        group.align_surfaces_with_incident_ray_directions(aim_points=centres, incident_ray_directions=incident,
                                                          active_heliostats_mask=mask, device=DEV)
        motors = group.kinematics.active_motor_positions.clone()
        flux = HeliostatRayTracer(scenario, group, blocking_active=False, random_seed=3, bitmap_resolution=size).trace_rays(
            incident, mask, targets, device=DEV)[0].clone()
    group.kinematics.rotation_deviation_parameters = (sigma * torch.randn(heliostats, 4, generator=torch.Generator().manual_seed(5))).to(DEV)
    return scenario, (flux, centres, incident, motors, mask, targets), size


class Epoch:
    def __init__(self, method, case, epoch_graph=False, parameters=None):
        from artist_amd import CalibrationSamples, FocalSpotLoss
        from artist_amd.optim import AngleLoss, KinematicsReconstructor
        scenario, six, resolution = case
        self.method = method
        self.reconstructor = KinematicsReconstructor(
            ddp_setup=DDP, scenario=scenario, data={"data_parser": CalibrationSamples(six), "heliostat_data_mapping": []},
            optimization_configuration=CONFIGURATION, reconstruction_method=method, bitmap_resolution=resolution, device=DEV,
            **({} if parameters is None else dict(parameters=parameters)))
        self.loss_definition = FocalSpotLoss(scenario=scenario) if method == "raytracing" else AngleLoss()
        self.state = self.reconstructor.prepare(0, DEV)
        self.graph = None
        if epoch_graph:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.graph = self.reconstructor.build_epoch_graph(self.state, self.loss_definition, DEV)
            torch.cuda.synchronize()
            self.build_ms = 1e3 * (time.perf_counter() - t0)

    def step(self, validate=False):
        r, state = self.reconstructor, self.state
        state.optimizer.zero_grad()
        if self.graph is None:
            loss = r.epoch_loss(state, self.loss_definition, DEV)
            loss.total.backward()
            total = loss.total
        else:
            total, _, _ = self.graph.replay()
        if self.method == "alignment":
            for group in state.optimizer.param_groups:
                group["params"][0].grad.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
        state.optimizer.step()
        host = total.item()
        state.scheduler.step()
        if validate:
            r.validate(state, DEV)
        return host


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


def count_calls(fn):
    """The calls through the library handle during ``fn()``, by entry point."""
    from artist_amd import _lib
    handle = _lib.lib()
    calls = collections.Counter()
    real = {name: getattr(handle, name) for name in _lib.SIGNATURES}

    def counting(name):
        def call(*args):
            calls[name] += 1
            return real[name](*args)
        return call

    for name in real:
        setattr(handle, name, counting(name))
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        for name, function in real.items():
            setattr(handle, name, function)
    return dict(sorted(calls.items()))


def learnable(method, case, parameters):
    """``parameters`` without what this mode on this field cannot learn: ``(what is left, {name: why it was left out})``."""
    left_out = {}
    if method == "alignment" and "translation_deviations" in parameters:
        left_out["translation_deviations"] = "do not enter the predicted normal"
    if "actuator_parameters" in parameters and case[0].heliostat_field.heliostat_groups[0].kinematics.actuators.optimizable_parameters.numel() == 0:
        left_out["actuator_parameters"] = "ideal actuators"
    return tuple(name for name in parameters if name not in left_out), left_out


def measure(name, make_case, epochs, blocks, warmup, parameters=None):
    variants, methods, left_out = {}, {}, {}
    for method in METHODS:                               # (each variant on a scenario of its own)
        choices = {method: None}
        if parameters is not None:
            chosen, left_out[method] = learnable(method, make_case(method), parameters)
            choices = {f"{method}, rotation_deviations": ("rotation_deviations",)}
            if chosen:                                   # (nothing left: the rotation deviations alone stand for the variant)
                choices[f"{method}, {' + '.join(chosen)}"] = chosen
        for key, choice in choices.items():
            variants[key] = Epoch(method, make_case(method), parameters=choice)
            variants[f"{key}, epoch_graph"] = Epoch(method, make_case(method), epoch_graph=True, parameters=choice)
            methods[key] = method
    times = {key: [] for key in variants}
    for epoch in variants.values():
        for _ in range(warmup):
            epoch.step()
    for _ in range(blocks):                              # alternating blocks inside one process
        for method, epoch in variants.items():
            torch.cuda.synchronize()
            for _ in range(epochs):
                t0 = time.perf_counter()
                epoch.step()
                torch.cuda.synchronize()
                times[method].append(1e3 * (time.perf_counter() - t0))
    result = {}
    for method, epoch in variants.items():
        calls = count_calls(epoch.step)
        result[method] = summary(times[method]) | dict(
            all_ms=[round(x, 4) for x in times[method]], library_calls=calls, library_calls_total=sum(calls.values()),
            synchronising_calls={"epoch (the loop's read of the loss)": count_syncs(epoch.step),
                                 "epoch + validation": count_syncs(lambda: epoch.step(True)),
                                 "epoch after a validation (re-activation)": count_syncs(epoch.step)})
        v = result[method]
        print(f"[{name}] {method}: median {v['median_ms']:.3f} ms (min {v['min_ms']:.3f}, p10 {v['p10_ms']:.3f}, p90 {v['p90_ms']:.3f}, "
              f"max {v['max_ms']:.3f}); library calls {v['library_calls_total']}: {calls}; synchronising calls {v['synchronising_calls']}",
              flush=True)
    for method in methods:
        e, g = result[method], result[f"{method}, epoch_graph"]
        g["eager_median_ms"], g["eager_over_replayed"] = e["median_ms"], e["median_ms"] / g["median_ms"]
        g["eager_p90_minus_p10_ms"] = e["p90_ms"] - e["p10_ms"]
        g["replay_within_eager_spread"] = g["median_ms"] <= e["median_ms"] + g["eager_p90_minus_p10_ms"]
        g["build_ms"] = variants[f"{method}, epoch_graph"].build_ms
        g["build_in_eager_epochs"] = g["build_ms"] / e["median_ms"]
        print(f"[{name}] {method}, epoch_graph: eager / replayed {g['eager_over_replayed']:.2f}, build {g['build_ms']:.1f} ms = "
              f"{g['build_in_eager_epochs']:.1f} eager epochs, within the eager spread: {g['replay_within_eager_spread']}", flush=True)
    if parameters is not None:
        result["left_out"] = left_out
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="profiles/kinematics_reconstructor_bench.json, with --parameters "
                    "profiles/kinematics_parameters_bench.json")
    ap.add_argument("--parameters", default=None, help="comma-separated KINEMATICS_PARAMETER_NAMES: measure the epoch that learns "
                    "them beside the one that learns the rotation deviations alone")
    ap.add_argument("--epochs", type=int, default=30, help="timed epochs per block and mode")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kinematics_reconstructor_bench.py measures on the GPU; no GPU found")
    parameters = None
    if args.parameters is not None:
        from artist_amd.kinematics_reconstructor import KINEMATICS_PARAMETER_NAMES
        from artist_amd.surface_reconstructor import canonical_parameters
        parameters = canonical_parameters([part.strip() for part in args.parameters.split(",") if part.strip()], KINEMATICS_PARAMETER_NAMES)
    args.out = args.out or str(ROOT / "profiles" / ("kinematics_reconstructor_bench.json" if parameters is None else "kinematics_parameters_bench.json"))
    out = dict(device=torch.cuda.get_device_name(DEV), epochs_per_block=args.epochs, blocks=args.blocks, warmup=args.warmup,
               fixture=measure("fixture: 4 heliostats x 3 training samples, 400 points, 3 rays, 64 x 64", fixture_case, args.epochs,
                               args.blocks, args.warmup, parameters),
               synthetic_100x4=measure("synthetic: 100 heliostats x 3 training samples, 10^4 points, 10 rays, 256 x 256", synthetic_case,
                                       args.epochs, args.blocks, args.warmup, parameters))
    if parameters is not None:
        out["parameters"] = list(parameters)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
