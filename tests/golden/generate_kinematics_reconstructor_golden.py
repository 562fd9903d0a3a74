#!/usr/bin/env python3
"""Golden epochs of the reference's ``KinematicsReconstructor`` as a class, in both of its modes (runs ONLY in the build
container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  Per mode ONE real run of the reference's
``KinematicsReconstructor.reconstruct_kinematics`` (artist/optim/kinematics_reconstructor.py:135-1063, unmodified) on its own
scenario file test_blocking.h5, on the CPU, once in fp32 and once in fp64 on the same rays, the same measurements and the same
start: six heliostats (rigid-body kinematics, linear actuators), 10 x 10 surface points per facet, 3 rays per point, 64 x 64
bitmaps on target_3.  Heliostats 0, 2, 4 and 5 have four calibration samples each (the mask is 4 0 4 0 4 4: heliostat_3, which
stands behind the target, and one heliostat between active ones have none), each sample under a sun of its own; the reference's
split makes three training samples and one test sample of them.  The measurements are the reference's own chain with the TRUE
rotation deviations: the motor positions the true kinematics drives to when it aims at the target's centre, the flux it produces
there (tracer seed 3), the target's centre as the focal spot.  The model starts from truth + sigma * randn (generator seed 5):
sigma = 3e-3 in the flux-driven mode (``FocalSpotLoss``), 3e-2 in the alignment-driven mode (``AngleLoss``) - at 3e-3 the
angles are about 5e-3 rad, where ``acos`` in fp32 is quantised and the reference's own fp32 and fp64 runs differ by 31 % per
sample.  Three epochs, an exponential scheduler, validation in every epoch.  The only stand-in is the calibration-data parser
(an object with ``parse_data_for_reconstruction`` that hands out the six tensors).  The methods of the instance are wrapped to
record what passes through them; nothing of the reference is changed or copied.

Usage:  python tests/golden/generate_kinematics_reconstructor_golden.py
        (writes tests/golden/kinematics_reconstructor_class_flux.npz and kinematics_reconstructor_class_alignment.npz)
"""
from __future__ import annotations

import json
import pathlib

import generate_surface_reconstructor_golden as base    # the import recipe of the reference, npy, Samples, rel_l2, DDP

import numpy as np  # noqa: E402
import torch  # noqa: E402
from artist.optim import KinematicsReconstructor  # noqa: E402
from artist.optim.loss import AngleLoss, CosineSimilarityLoss, FocalSpotLoss, VectorLoss  # noqa: E402
from artist.raytracing.heliostat_ray_tracer import HeliostatRayTracer  # noqa: E402
from artist.scenario.scenario import Scenario  # noqa: E402
from artist.util import constants  # noqa: E402

OUT_DIR = pathlib.Path(__file__).resolve().parent
CPU, npy, rel_l2 = base.CPU, base.npy, base.rel_l2

N_EPOCHS = 3
POINTS_PER_FACET = [10, 10]
N_RAYS = 3
RESOLUTION = [64, 64]
TARGET = "target_3"
MASK = [4, 0, 4, 0, 4, 4]            # samples per heliostat: heliostat_3 and one in the middle have none
SUNS = [[0.1, 1.0, -0.2, 0.0], [-0.25, 0.9, -0.35, 0.0], [0.3, 0.8, -0.3, 0.0], [0.0, 1.0, -0.5, 0.0]]    # one per sample of a heliostat
MEASUREMENT_SEED = 3
START_SEED = 5
FLUX, ALIGNMENT = constants.kinematics_reconstruction_raytracing, constants.kinematics_reconstruction_alignment
SIGMA = {FLUX: 3e-3, ALIGNMENT: 3e-2}
CONFIG = {
    constants.optimization: {constants.initial_learning_rate_rotation_deviation: 2e-4, constants.tolerance: 0.0,
                             constants.max_epoch: N_EPOCHS - 1, constants.batch_size: 30, constants.log_step: 1,
                             constants.early_stopping_delta: 1e-9, constants.early_stopping_patience: 100,
                             constants.early_stopping_window: 10},
    constants.scheduler: {constants.scheduler_type: constants.exponential, constants.gamma: 0.9},
}
VALIDATION_KEYS = ("focal_spot_loss", "pixel_loss", "kl_div")


def load(dtype):
    import h5py     # the stand-in installed by the import recipe
    torch.set_default_dtype(dtype)
    torch.manual_seed(7)
    with h5py.File(pathlib.Path(base.REFERENCE) / "tests/data/scenarios" / "test_blocking.h5", "r") as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file,
                                                    number_of_surface_points_per_facet=torch.tensor(POINTS_PER_FACET), device=CPU)
    scenario.set_number_of_rays(number_of_rays=N_RAYS)
    return scenario


def samples_of(scenario, dtype):
    """(mask, target area indices, incident ray directions) of the sixteen samples, a heliostat's four after one another."""
    mask = torch.tensor(MASK, dtype=torch.int32)
    n_active = int((mask > 0).sum())
    targets = torch.full((n_active * len(SUNS),), scenario.solar_tower.target_name_to_index[TARGET], dtype=torch.int64)
    incident = torch.nn.functional.normalize(torch.tensor(SUNS, dtype=torch.float32), dim=1).to(dtype).repeat(n_active, 1)
    return mask, targets, incident


def measure():
    """The calibration data, from the TRUE kinematics in fp32: (flux, focal spots, motor positions, true rotation deviations)."""
    scenario = load(torch.float32)
    group = scenario.heliostat_field.heliostat_groups[0]
    mask, targets, incident = samples_of(scenario, torch.float32)
    with torch.no_grad():
        centres = scenario.solar_tower.get_centers_of_target_areas(target_area_indices=targets, device=CPU)
        group.activate_heliostats(active_heliostats_mask=mask, device=CPU)
        group.align_surfaces_with_incident_ray_directions(aim_points=centres, incident_ray_directions=incident,
                                                          active_heliostats_mask=mask, device=CPU)
        motors = group.kinematics.active_motor_positions.detach().clone()
        tracer = HeliostatRayTracer(scenario=scenario, heliostat_group=group, blocking_active=False, batch_size=100,
                                    random_seed=MEASUREMENT_SEED, bitmap_resolution=torch.tensor(RESOLUTION))
        flux, _, _, _ = tracer.trace_rays(incident_ray_directions=incident, active_heliostats_mask=mask,
                                          target_area_indices=targets, device=CPU)
    return flux.clone(), centres.clone(), motors, group.kinematics.rotation_deviation_parameters.detach().clone()


def run(method, dtype, measured, distortions_f32=None):
    """The reference's run of ``method`` in ``dtype``; returns (per-epoch log, the distortions drawn, run-wide arrays)."""
    flux_measured, focal_spots, motors, true_rotation = measured
    scenario = load(dtype)
    group = scenario.heliostat_field.heliostat_groups[0]
    kinematics = group.kinematics
    mask, targets, incident = samples_of(scenario, dtype)
    generator = torch.Generator().manual_seed(START_SEED)
    start = true_rotation + SIGMA[method] * torch.randn(true_rotation.shape, generator=generator, dtype=torch.float32)
    kinematics.rotation_deviation_parameters = start.to(dtype).clone()
    six = (flux_measured.to(dtype), focal_spots.to(dtype), incident, motors.to(dtype), mask, targets)

    sun = scenario.light_sources.light_source_list[0]
    drawn = {}
    draw = sun.get_distortions

    def get_distortions(number_of_points, number_of_active_heliostats, random_seed=7):
        if distortions_f32 is not None:                           # the fp64 run traces the fp32 run's rays
            assert distortions_f32[number_of_active_heliostats][0] == random_seed
            return tuple(torch.from_numpy(a).to(dtype) for a in distortions_f32[number_of_active_heliostats][1:])
        du, de = draw(number_of_points=number_of_points, number_of_active_heliostats=number_of_active_heliostats,
                      random_seed=random_seed)
        again = drawn.get(number_of_active_heliostats)           # the reference makes a tracer per epoch: the same draw each time
        assert again is None or (again[0] == random_seed and np.array_equal(again[1], npy(du)))
        drawn[number_of_active_heliostats] = (random_seed, npy(du), npy(de))
        return du, de

    sun.get_distortions = get_distortions

    rec = KinematicsReconstructor(ddp_setup=base.DDP, scenario=scenario,
                                  data={constants.data_parser: base.Samples(six), constants.heliostat_data_mapping: []},
                                  optimization_configuration=CONFIG, reconstruction_method=method,
                                  bitmap_resolution=torch.tensor(RESOLUTION))
    log = dict(rotation_start=[], loss_per_sample=[], loss_per_heliostat=[], prediction=[], grad=[], lr=[], rotation_after=[])
    once = dict(validated_epochs=[], **{f"test_{key}": [] for key in VALIDATION_KEYS})
    name = "_compute_raytracing_loss" if method == FLUX else "_compute_alignment_loss"
    epoch_loss = getattr(rec, name)

    def epoch_loss_wrapped(**kw):
        log["rotation_start"].append(npy(kw["heliostat_group"].kinematics.rotation_deviation_parameters))
        split = kw["data_split"]
        once.update(train_indices=npy(split.train_indices), test_indices=npy(split.test_indices),
                    mask_train=npy(split.active_heliostats_mask_train), mask_test=npy(split.active_heliostats_mask_test),
                    split_counts=np.asarray([split.number_of_train_samples, split.number_of_test_samples,
                                             split.number_of_samples_per_heliostat]))
        out = epoch_loss(**kw)
        log["loss_per_heliostat"].append(npy(out[1]))
        return out

    setattr(rec, name, epoch_loss_wrapped)
    measured_normals = rec._compute_measured_normals

    def measured_normals_wrapped(**kw):
        out = measured_normals(**kw)
        once["normals_measured"] = npy(out)
        return out

    rec._compute_measured_normals = measured_normals_wrapped
    setup = rec._setup_optimizer_scheduler_early_stopping

    def setup_wrapped(heliostat_group):
        optimizer, scheduler, stopper = setup(heliostat_group=heliostat_group)
        step = optimizer.step

        def step_wrapped(*a, **k):
            parameter = optimizer.param_groups[0]["params"][0]
            log["grad"].append(npy(parameter.grad))               # (alignment mode: after nan_to_num_)
            log["lr"].append(float(optimizer.param_groups[0]["lr"]))
            r = step(*a, **k)
            log["rotation_after"].append(npy(parameter))
            return r

        optimizer.step = step_wrapped
        return optimizer, scheduler, stopper

    rec._setup_optimizer_scheduler_early_stopping = setup_wrapped
    validate = rec._validate

    def validate_wrapped(**kw):
        out = validate(**kw)
        once["validated_epochs"].append(len(log["rotation_after"]) - 1)
        for key in VALIDATION_KEYS:
            once[f"test_{key}"].append(npy(out[key]))
        return out

    rec._validate = validate_wrapped

    class Recording:
        """The loss the run is given: the reference's, with what passes through it recorded."""

        def __init__(self, loss):
            self.loss = loss

        def __call__(self, *a, **k):
            out = self.loss(*a, **k)
            if out.requires_grad:                                       # (the validation calls run under no_grad)
                log["loss_per_sample"].append(npy(out))
                log["prediction"].append(npy(k["prediction"]))
                once["ground_truth"] = npy(k["ground_truth"])
                once["loss_keywords"] = sorted(k)
            return out

    loss = Recording(FocalSpotLoss(scenario=scenario) if method == FLUX else AngleLoss())
    final_loss, histories = rec.reconstruct_kinematics(loss_definition=loss, device=CPU)
    assert all(len(v) == N_EPOCHS for v in log.values()), {k: len(v) for k, v in log.items()}
    assert len(histories) == 1 and len(histories[0]) == 1
    history = histories[0][0]
    assert not kinematics.rotation_deviation_parameters.requires_grad
    out = {k: np.stack([np.asarray(x) for x in v]) for k, v in log.items()}
    out["total_loss"] = np.asarray(history["total_loss"], dtype=np.float64)
    active = np.nonzero(np.asarray(MASK))[0]
    assert np.allclose(out["loss_per_heliostat"].mean(axis=1), out["total_loss"], rtol=1e-6)
    assert np.array_equal(npy(final_loss)[active], out["loss_per_heliostat"][-1])
    assert np.array_equal(out["rotation_after"][:-1], out["rotation_start"][1:])
    if method == ALIGNMENT:         # the other two losses on vectors, on every epoch's normals (for the CPU tests of the losses)
        assert once["loss_keywords"] == ["ground_truth", "prediction"]
        truth = torch.from_numpy(once["ground_truth"])
        predictions = torch.from_numpy(out["prediction"])
        out["vector_loss_per_sample"] = np.stack([npy(VectorLoss()(p, truth, reduction_dimensions=(1,))) for p in predictions])
        out["cosine_loss_per_sample"] = np.stack([npy(CosineSimilarityLoss()(p, truth)) for p in predictions])
    once = {k: np.stack(v) if isinstance(v, list) and k != "loss_keywords" else v for k, v in once.items()}
    once.pop("loss_keywords")
    once.update(final_loss=npy(final_loss), history_total_loss=np.asarray(history["total_loss"], dtype=np.float64),
                **{f"history_test_{key}": npy(history["test_loss"][key]) for key in VALIDATION_KEYS},
                parser_flux_measured=npy(six[0]), parser_focal_spots=npy(six[1]), parser_incident_ray_directions=npy(six[2]),
                parser_motor_positions=npy(six[3]), parser_mask=npy(mask), parser_target_area_indices=npy(targets),
                true_rotation=npy(true_rotation), heliostat_positions=npy(group.positions))
    torch.set_default_dtype(torch.float32)
    return out, drawn, once


def median_gap(loss_per_sample, n_train):
    """Per epoch and heliostat: the distance from the median training sample's loss to the nearest other sample's."""
    blocks = np.sort(np.asarray(loss_per_sample, dtype=np.float64).reshape(loss_per_sample.shape[0], -1, n_train), axis=2)
    middle = (n_train - 1) // 2                                   # torch.median: the lower of two middle values
    return np.minimum(blocks[..., middle] - blocks[..., middle - 1], blocks[..., middle + 1] - blocks[..., middle])


def write(method, name, measured):
    log32, drawn, once32 = run(method, torch.float32, measured)
    log64, _, once64 = run(method, torch.float64, measured, distortions_f32=drawn)
    mask = np.asarray(MASK)
    active = np.nonzero(mask)[0]
    inactive = np.nonzero(mask == 0)[0]
    n_train, n_test, per_heliostat = (int(v) for v in once32["split_counts"])
    # the conditions the case was chosen for
    assert set(mask.tolist()) == {0, 4} and len(active) == 4 and (n_train, n_test, per_heliostat) == (3, 1, 4)
    assert any(mask[h] == 0 and (active < h).any() and (active > h).any() for h in range(len(mask))), "no inactive heliostat between active ones"
    assert len(once32["validated_epochs"]) > 1, "validation ran in one epoch only"
    assert np.isfinite(log32["grad"]).all() and np.isfinite(log64["grad"]).all(), "a recorded gradient is not finite"
    assert not log32["grad"][:, inactive].any() and (log32["grad"][:, active] != 0).all()
    assert np.isinf(once32["final_loss"][inactive]).all()
    sample_distance = np.abs(log32["loss_per_sample"][0].astype(np.float64) - log64["loss_per_sample"][0])
    print(f"--- {method}\nloss per sample:\n{log32['loss_per_sample']}\ntotal loss: {log32['total_loss']}  lr: {log32['lr']}")
    print("validated in epochs", once32["validated_epochs"], *(f"\n  {key}: {once32['test_' + key].tolist()}" for key in VALIDATION_KEYS))
    print("fp32 vs fp64, epoch 0: loss per sample, largest distance", sample_distance.max(), " relative",
          (sample_distance / np.abs(log64["loss_per_sample"][0])).max(), " prediction", rel_l2(log32["prediction"][0], log64["prediction"][0]),
          " gradient", rel_l2(log32["grad"][0], log64["grad"][0]), " gradient per epoch |g|", np.linalg.norm(log32["grad"], axis=(1, 2)))
    if method == FLUX:
        gap = median_gap(log32["loss_per_sample"], n_train)
        print("gap around each heliostat's median training sample, smallest per epoch:", gap.min(axis=1))
        assert (gap >= 10 * sample_distance.max()).all(), "fp32 and fp64 may pick different median samples"
    else:
        assert (sample_distance / np.abs(log64["loss_per_sample"][0])).max() < 1e-2, "acos is quantised at these angles"

    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    arrays = dict(points_per_facet=np.asarray(POINTS_PER_FACET), n_rays=np.int64(N_RAYS), resolution=np.asarray(RESOLUTION),
                  target=np.asarray(TARGET), suns=np.asarray(SUNS, dtype=np.float32), configuration=np.asarray(json.dumps(CONFIG)),
                  method=np.asarray(method), sigma=np.float64(SIGMA[method]), measurement_seed=np.int64(MEASUREMENT_SEED))
    for kind, count in (("train", len(active) * n_train), ("test", len(active) * n_test)):
        if count in drawn:                                        # (the alignment-driven mode traces for validation only)
            arrays.update({f"seed_{kind}": np.int64(drawn[count][0]), f"distortions_{kind}_u": drawn[count][1],
                           f"distortions_{kind}_e": drawn[count][2]})
    prediction = "flux_predicted" if method == FLUX else "normals_predicted"
    for key, value in log32.items():
        arrays[prediction if key == "prediction" else key] = np.asarray(value, dtype=np.float64) if key in ("lr", "total_loss") else f32(value)
    for key, value in once32.items():
        if key == "ground_truth":
            if method == ALIGNMENT:
                arrays["normals_measured_train"] = f32(value)
        else:
            arrays[key] = f32(value) if np.asarray(value).dtype.kind == "f" and not key.startswith("history_total") else value
    for key in ("prediction", "loss_per_sample", "loss_per_heliostat", "grad", "total_loss"):
        arrays[f"{prediction if key == 'prediction' else key}_f64_epoch0"] = np.asarray(log64[key][0], dtype=np.float64)
    for key in VALIDATION_KEYS:
        arrays[f"test_{key}_f64_epoch0"] = np.asarray(once64[f"test_{key}"][0], dtype=np.float64)
    if method == ALIGNMENT:
        arrays["normals_measured_f64"] = np.asarray(once64["normals_measured"], dtype=np.float64)
    path = OUT_DIR / f"{name}.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    largest = max(p.stat().st_size for p in OUT_DIR.glob("*.npz") if not p.name.startswith("kinematics_reconstructor_class_"))
    print(f"wrote {path.name}: {size / 1024:.1f} KiB (largest other fixture {largest / 1024:.1f} KiB), keys={len(arrays)}")
    assert size < largest and size < (1 << 20)


def main():
    measured = measure()
    assert (npy(measured[0]).sum(axis=(1, 2)) > 0).all(), "a measured bitmap is empty"
    write(FLUX, "kinematics_reconstructor_class_flux", measured)
    write(ALIGNMENT, "kinematics_reconstructor_class_alignment", measured)


if __name__ == "__main__":
    main()
