#!/usr/bin/env python3
"""Golden epochs of the reference's ``AimPointOptimizer`` (runs ONLY in the build container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  ONE real run of the reference's ``AimPointOptimizer.optimize``
(artist/optim/aim_point_optimizer.py:724-972, unmodified) on its own scenario file test_blocking.h5, on the CPU, once in fp32
and once in fp64 on the same rays: the field's six heliostats (rigid-body kinematics, linear actuators), 10 x 10 surface points
per facet, 3 rays per point, 64 x 64 bitmaps, the planar target_4 above the cluster of five (every heliostat hits it, three of
them are partly blocked by their neighbours under the chosen sun), the ground truth an outer product of two trapezoids
(the recipe of tutorials/05_motor_positions_optimizer_tutorial.py:200-235), ``KLDivergenceLoss``.  The methods of the instance
are wrapped to record what passes through them; nothing of the reference is changed or copied.

Captured per epoch (three epochs): the parameter and the motor positions at the start, total flux, the three factors,
``flux_loss``, the three constraint terms, the total loss, multipliers and references before and after, the parameter's
gradient, the learning rate, the parameter after ``optimizer.step()``; once: the distortions the reference drew, the ground
truth, the configuration, the initial motor positions and scales, epoch 0 of the fp64 run.  Plus known answers of
``trapezoid_distribution`` (rectangle, cut-off slopes, zero padding) and one ``EarlyStopping`` decision sequence.

Usage:  python tests/golden/generate_aim_point_golden.py            (writes tests/golden/aim_point_optimizer_epochs.npz)
"""
from __future__ import annotations

import json
import os
import pathlib
import sys
import tempfile
import types

OUT_DIR = pathlib.Path(__file__).resolve().parent
REFERENCE = "/root/reference"


def _import_reference():
    """The import recipe of generate_golden.py: empty stand-ins for the packages the reference imports at module scope but
    that are absent here (h5py = artist_amd.h5lite), ``artist.field`` first, a scratch working directory."""
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Fmt:
        def __init__(self, *a, **k):
            pass

    stub("colorlog", ColoredFormatter=_Fmt)
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
    from artist_amd import h5lite
    stub("h5py", File=h5lite.File, Group=h5lite.Group, Dataset=h5lite.Dataset)
    stub("torchvision")
    stub("torchvision.transforms")
    stub("paint")
    stub("paint.util")
    pm = stub("paint.util.paint_mappings")
    pm.__getattr__ = lambda n: n
    sys.path.insert(0, REFERENCE)
    os.chdir(tempfile.mkdtemp(prefix="artist_ref_cwd_"))
    import artist.field  # noqa: F401  (must come first)


_import_reference()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from artist.flux import bitmap  # noqa: E402
from artist.optim import AimPointOptimizer, training  # noqa: E402
from artist.optim.loss import KLDivergenceLoss  # noqa: E402
from artist.scenario.scenario import Scenario  # noqa: E402
from artist.util import constants  # noqa: E402

CPU = torch.device("cpu")

N_EPOCHS = 3
POINTS_PER_FACET = [10, 10]
N_RAYS = 3
RESOLUTION = [64, 64]
TARGET = "target_4"                  # 6 m x 6 m, facing down from 100 m above the cluster: all six heliostats hit it
SUN = [0.0, 0.8, -0.6, 0.0]          # a sun at 37 degrees elevation in the south: heliostats 0, 2 and 4 are partly blocked
DNI = 800.0
TRAPEZOID = dict(slope_width=8, plateau_width=26)            # tutorial 05's 30 / 110 of 256, scaled to 64 pixels
CONFIG = {
    constants.optimization: {constants.initial_learning_rate: 1e-3, constants.tolerance: 0.0, constants.max_epoch: N_EPOCHS - 1,
                             constants.batch_size: 50, constants.log_step: 0, constants.early_stopping_delta: 1e-4,
                             constants.early_stopping_patience: 100, constants.early_stopping_window: 100},
    constants.scheduler: {constants.scheduler_type: constants.exponential, constants.gamma: 0.9, constants.lr_min: 1e-6,
                          constants.lr_max: 1e-3, constants.step_size_up: 500, constants.reduce_factor: 0.3, constants.patience: 100,
                          constants.threshold: 1e-3, constants.cooldown: 10},
    # max_flux_density (W/m^2): 1055 W per pixel, below the 1.3 kW peak of this field's flux, so that the local-flux term is active
    constants.constraints: {constants.rho_flux_integral: 1.0, constants.rho_local_flux: 1.0, constants.rho_intercept: 1.0,
                            constants.max_flux_density: 1.2e5},
}
DDP = dict(device=CPU, is_distributed=False, is_nested=False, rank=0, world_size=1, process_subgroup=None,
           groups_to_ranks_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1, ranks_to_groups_mapping={0: [0]})


def npy(t):
    if isinstance(t, torch.Tensor):
        return t.detach().cpu().numpy().copy()
    return np.asarray(t)


def run(dtype, distortions_f32=None):
    """The reference's run in ``dtype``; returns (per-epoch log, the fp32 distortions drawn, run-wide arrays)."""
    import h5py     # the stand-in installed by _import_reference()
    torch.set_default_dtype(dtype)
    torch.manual_seed(7)
    with h5py.File(pathlib.Path(REFERENCE) / "tests/data/scenarios" / "test_blocking.h5", "r") as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file,
                                                    number_of_surface_points_per_facet=torch.tensor(POINTS_PER_FACET), device=CPU)
    scenario.set_number_of_rays(number_of_rays=N_RAYS)
    group = scenario.heliostat_field.heliostat_groups[0]
    target_area_index = scenario.solar_tower.target_name_to_index[TARGET]
    resolution = torch.tensor(RESOLUTION)
    incident = torch.tensor(SUN, dtype=dtype)

    # the ground truth of tutorial 05: trapezoid x trapezoid, scaled to 75 % of the field's power
    canting_norm = (torch.norm(group.canting[0], dim=1)[0])[:2]
    dimensions = (canting_norm * 4) + 0.02
    target_flux_integral = DNI * dimensions[0] * dimensions[1] * scenario.heliostat_field.number_of_heliostats_per_group.sum() * 0.75
    e_trapezoid = bitmap.trapezoid_distribution(total_width=RESOLUTION[0], device=CPU, **TRAPEZOID)
    u_trapezoid = bitmap.trapezoid_distribution(total_width=RESOLUTION[1], device=CPU, **TRAPEZOID)
    ground_truth = (u_trapezoid.unsqueeze(1) * e_trapezoid.unsqueeze(0)).to(dtype)
    ground_truth = ground_truth / ground_truth.sum() * target_flux_integral

    sun = scenario.light_sources.light_source_list[0]
    drawn = {}
    draw = sun.get_distortions

    def get_distortions(number_of_points, number_of_active_heliostats, random_seed=7):
        if distortions_f32 is not None:                           # the fp64 run traces the fp32 run's rays
            return tuple(torch.from_numpy(a).to(dtype) for a in distortions_f32)
        du, de = draw(number_of_points=number_of_points, number_of_active_heliostats=number_of_active_heliostats,
                      random_seed=random_seed)
        drawn["seed"], drawn["u"], drawn["e"] = random_seed, npy(du), npy(de)
        return du, de

    sun.get_distortions = get_distortions

    opt = AimPointOptimizer(ddp_setup=DDP, scenario=scenario, optimization_configuration=CONFIG, incident_ray_direction=incident,
                            target_area_index=target_area_index, ground_truth=ground_truth, dni=DNI, bitmap_resolution=resolution,
                            device=CPU)
    log = {k: [] for k in ("param_start", "motor_start", "total_flux", "intercept_factors", "on_target_factors", "blocking_factors",
                           "flux_loss", "flux_integral_constraint", "intercept_constraint", "local_flux_constraint", "total_loss",
                           "lambda_before", "lambda_after", "ref_integral_before", "ref_integral_after", "ref_intercept_before",
                           "ref_intercept_after", "grad", "lr", "param_after")}
    once = {}

    init = opt._initialize_group_parameters

    def init_wrapped(**kw):
        out = init(**kw)
        once["scale"], once["initial_motor_positions"] = npy(out[1][0]), npy(out[2][0])
        return out

    opt._initialize_group_parameters = init_wrapped
    align = opt._align_all_groups

    def align_wrapped(**kw):
        log["param_start"].append(npy(kw["optimizer"].param_groups[0]["params"][0]))
        align(**kw)
        log["motor_start"].append(npy(group.kinematics.motor_positions))

    opt._align_all_groups = align_wrapped
    trace = opt._trace_and_accumulate_flux

    def trace_wrapped(**kw):
        out = trace(**kw)
        for key, value in zip(("total_flux", "intercept_factors", "on_target_factors", "blocking_factors"), out):
            log[key].append(npy(value))
        return out

    opt._trace_and_accumulate_flux = trace_wrapped
    constraints = opt._compute_kl_constraints
    H = group.number_of_heliostats

    def constraints_wrapped(**kw):
        log["flux_loss"].append(npy(kw["flux_loss"]))
        log["lambda_before"].append(np.asarray([float(kw[k]) for k in ("lambda_flux_integral", "lambda_intercept", "lambda_local_flux")]))
        log["ref_integral_before"].append(float(kw["flux_integral_reference"]))
        ref = kw["intercept_factors_reference"]
        log["ref_intercept_before"].append(npy(ref) if isinstance(ref, torch.Tensor) else np.zeros(H))
        out = constraints(**kw)
        log["total_loss"].append(npy(out[0]))
        log["flux_integral_constraint"].append(npy(out[1]))
        log["intercept_constraint"].append(npy(out[2]))
        log["local_flux_constraint"].append(npy(out[3]))
        log["ref_integral_after"].append(float(out[4]))
        log["ref_intercept_after"].append(npy(out[5]))
        log["lambda_after"].append(np.asarray([float(out[6]), float(out[7]), float(out[8])]))
        return out

    opt._compute_kl_constraints = constraints_wrapped
    setup = opt._setup_optimizer_scheduler_early_stopping

    def setup_wrapped(**kw):
        optimizer, scheduler, stopper = setup(**kw)
        step = optimizer.step

        def step_wrapped(*a, **k):
            prm = optimizer.param_groups[0]["params"][0]
            log["grad"].append(npy(prm.grad))
            log["lr"].append(float(optimizer.param_groups[0]["lr"]))
            r = step(*a, **k)
            log["param_after"].append(npy(prm))
            return r

        optimizer.step = step_wrapped
        return optimizer, scheduler, stopper

    opt._setup_optimizer_scheduler_early_stopping = setup_wrapped

    final_loss, history, intercept, on_target, blocking = opt.optimize(loss_definition=KLDivergenceLoss(), device=CPU)
    assert len(log["param_after"]) == N_EPOCHS, len(log["param_after"])
    once.update(ground_truth=npy(ground_truth), target_area_index=np.int64(target_area_index), final_loss=npy(final_loss),
                final_motor_positions=npy(group.kinematics.motor_positions),
                motor_limits=npy(group.kinematics.actuators.non_optimizable_parameters[:, 2:4]),
                target_dimensions=npy(scenario.solar_tower.target_areas[0].dimensions[target_area_index]),
                **{f"history_{k}": np.asarray(v, dtype=np.float64) for k, v in history.items()})
    torch.set_default_dtype(torch.float32)
    return {k: np.stack([np.asarray(x) for x in v]) for k, v in log.items()}, drawn, once


def trapezoid_answers():
    """Known answers of the reference's ``trapezoid_distribution``: (total_width, slope_width, plateau_width) -> values."""
    cases = np.asarray([[16, 0, 6],        # no slope: a rectangle
                        [15, 0, 5],        # ... odd width
                        [12, 0, 20],       # ... wider than the bitmap: all ones
                        [16, 4, 4],        # the trapezoid fits: zero padding on both sides
                        [31, 5, 7],        # ... odd width, padded
                        [16, 6, 10],       # 2 * slope + plateau > total: the slopes are cut off
                        [9, 8, 3],         # ... cut off far up the slope
                        [64, 8, 26],       # the ground truth's
                        [1, 3, 0]], dtype=np.int64)
    out = dict(trapezoid_cases=cases)
    for i, (total, slope, plateau) in enumerate(cases):
        out[f"trapezoid_{i}"] = npy(bitmap.trapezoid_distribution(total_width=int(total), slope_width=int(slope),
                                                                 plateau_width=int(plateau), device=CPU)).astype(np.float32)
    return out


def early_stopping_answers():
    """One decision sequence of the reference's ``EarlyStopping`` on a fixed loss list: improving, flat, improving, flat."""
    losses = [1.0, 0.9, 0.8, 0.7, 0.6, 0.6, 0.6, 0.6, 0.6, 0.5, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4, 0.4]
    arguments = dict(window_size=3, patience=4, min_improvement=1e-3, relative=True)
    stopper = training.EarlyStopping(**arguments)
    decisions, counters = [], []
    for loss in losses:
        decisions.append(bool(stopper.step(loss)))
        counters.append(int(stopper.counter))
    assert any(decisions) and not decisions[0]
    absolute = training.EarlyStopping(window_size=2, patience=2, min_improvement=0.05, relative=False)
    return dict(early_stopping_losses=np.asarray(losses), early_stopping_arguments=np.asarray(json.dumps(arguments)),
                early_stopping_decisions=np.asarray(decisions), early_stopping_counters=np.asarray(counters),
                early_stopping_absolute_decisions=np.asarray([bool(absolute.step(loss)) for loss in losses]))


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def main():
    log32, drawn, once32 = run(torch.float32)
    log64, _, once64 = run(torch.float64, distortions_f32=(drawn["u"], drawn["e"]))

    # the conditions on the chosen case
    print("blocking factors, epoch 0:", log32["blocking_factors"][0])
    print("intercept factors, epoch 0:", log32["intercept_factors"][0])
    print("flux loss:", log32["flux_loss"], " total loss:", log32["total_loss"])
    print("local flux term:", log32["local_flux_constraint"], " intercept term:", log32["intercept_constraint"],
          " flux integral term:", log32["flux_integral_constraint"])
    print("lambda after:", log32["lambda_after"])
    print("peak flux per pixel:", log32["total_flux"].max(axis=(1, 2)))
    g32, g64 = log32["grad"][0], log64["grad"][0]
    print("gradient epoch 0, fp32:", g32.ravel(), "\n                  fp64:", g64.ravel())
    print("fp32 vs fp64, epoch 0: flux", rel_l2(log32["total_flux"][0], log64["total_flux"][0]), " gradient", rel_l2(g32, g64),
          " total loss", abs(log32["total_loss"][0].item() - log64["total_loss"][0].item()) / abs(log64["total_loss"][0].item()))
    assert (log32["blocking_factors"][0] > 0).any(), "no heliostat is blocked in epoch 0"
    assert (log32["local_flux_constraint"] != 0).any(), "the local-flux term is zero in every epoch"
    assert (log32["flux_integral_constraint"][1:] != 0).any() or (log32["intercept_constraint"][1:] != 0).any(), \
        "neither the flux-integral nor the intercept violation is active after the first epoch"
    assert (np.sign(g32) == np.sign(g64)).all() and (g64 != 0).all(), "a gradient element changes sign between fp32 and fp64"
    assert (np.abs(g32) >= np.abs(g32 - g64.astype(np.float32))).all(), "a gradient element is smaller than its fp32-vs-fp64 difference"

    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    arrays = dict(points_per_facet=np.asarray(POINTS_PER_FACET), n_rays=np.int64(N_RAYS), resolution=np.asarray(RESOLUTION),
                  target=np.asarray(TARGET), sun=np.asarray(SUN, dtype=np.float32), dni=np.float64(DNI), seed=np.int64(drawn["seed"]),
                  configuration=np.asarray(json.dumps(CONFIG)), epsilon=np.float64(1e-12),
                  distortions_u=drawn["u"], distortions_e=drawn["e"])
    arrays.update({k: f32(v) for k, v in log32.items() if k != "lr"})
    arrays["lr"] = np.asarray(log32["lr"], dtype=np.float64)
    arrays.update({k: (f32(v) if np.asarray(v).dtype.kind == "f" and not k.startswith("history_") else v) for k, v in once32.items()})
    arrays.update({f"{k}_f64_epoch0": np.asarray(v[0], dtype=np.float64) for k, v in log64.items()})
    arrays.update(trapezoid_answers())
    arrays.update(early_stopping_answers())
    path = OUT_DIR / "aim_point_optimizer_epochs.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    largest = max(p.stat().st_size for p in OUT_DIR.glob("*.npz") if p != path)
    print(f"wrote {path.name}: {size / 1024:.1f} KiB, keys={len(arrays)}")
    assert size < largest and size < (1 << 20)


if __name__ == "__main__":
    main()
