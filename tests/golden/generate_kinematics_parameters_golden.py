#!/usr/bin/env python3
"""Golden epochs of the reference's ``KinematicsReconstructor`` loop with more leaves: the translation deviations and the
optimisable actuator parameters beside the rotation deviations (runs ONLY in the build container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  The case, the measurements and the run are those of
generate_kinematics_reconstructor_golden.py (imported, unchanged): test_blocking.h5, six heliostats, the mask 4 0 4 0 4 4,
10 x 10 points per facet, 3 rays, 64 x 64 bitmaps, three epochs, an exponential scheduler, validation in every epoch, once in
fp32 and once in fp64 on the fp32 run's rays.  The reference's class learns the rotation deviations alone
(artist/optim/kinematics_reconstructor.py:393-402).  Here the instance's ``_setup_optimizer_scheduler_early_stopping`` is
wrapped: while it runs, the optimiser it constructs is handed one more parameter group per extra tensor -
``kinematics.translation_deviation_parameters`` ``[6, 9]`` and ``kinematics.actuators.optimizable_parameters`` ``[6, 2, 2]``,
as leaves, each at a learning rate of its own - so the scheduler it constructs next scales every group.  Nothing else of the
reference's loop changes: ``activate_heliostats`` repeats the rows of all three tensors with ``repeat_interleave``, which passes
the gradient on.

Two runs.  Flux-driven with ``FocalSpotLoss``: all three tensors.  Alignment-driven with ``AngleLoss``: the rotation deviations
and the actuator parameters - the predicted normal is the third column of the orientation, which the translations do not enter,
so their gradient is identically zero (asserted here in a run of its own, one epoch).

The rotation deviations start as in the imported generator (truth + sigma * randn, seed 5).  The other two start from the file's
values plus ``SIGMA[name] * randn`` (seed 11, drawn in fp32 for all six heliostats): 2 mm on the translations, 1e-3 (rad, m)
on the actuators' initial angles and stroke lengths - of the size of the rotations' 3e-3 rad in their effect on the
orientation, so that the flux stays on the target and every gradient finite.

Usage:  python tests/golden/generate_kinematics_parameters_golden.py
        (writes tests/golden/kinematics_parameters_flux.npz and kinematics_parameters_alignment.npz)
"""
from __future__ import annotations

import copy
import json

import generate_kinematics_reconstructor_golden as k    # the case, the measurements, the run; through it the reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT_DIR = k.OUT_DIR
npy, rel_l2 = k.npy, k.rel_l2
FLUX, ALIGNMENT = k.FLUX, k.ALIGNMENT

NAMES = ("rotation_deviations", "translation_deviations", "actuator_parameters")      # the canonical order
LEARNED = {FLUX: NAMES, ALIGNMENT: ("rotation_deviations", "actuator_parameters")}
RATE_KEYS = {"rotation_deviations": "initial_learning_rate_rotation_deviation",
             "translation_deviations": "initial_learning_rate_translation_deviation",
             "actuator_parameters": "initial_learning_rate_actuator_parameters"}
RATES = {"translation_deviations": 1e-4, "actuator_parameters": 5e-5}       # the rotation deviations keep the case's 2e-4
SIGMA = {"translation_deviations": 2e-3, "actuator_parameters": 1e-3}
PERTURBATION_SEED = 11
CONFIG = copy.deepcopy(k.CONFIG)
CONFIG["optimization"].update({RATE_KEYS[name]: rate for name, rate in RATES.items()})


def slot(kinematics, name):
    """(holder, attribute) of the tensor ``name``."""
    if name == "actuator_parameters":
        return kinematics.actuators, "optimizable_parameters"
    return kinematics, {"rotation_deviations": "rotation_deviation_parameters",
                        "translation_deviations": "translation_deviation_parameters"}[name]


def perturbed_starts():
    """The start of the two extra tensors in fp32: the file's values plus the seeded perturbation."""
    kinematics = k.load(torch.float32).heliostat_field.heliostat_groups[0].kinematics
    generator = torch.Generator().manual_seed(PERTURBATION_SEED)
    starts = {}
    for name in NAMES[1:]:
        holder, attribute = slot(kinematics, name)
        true = getattr(holder, attribute).detach().clone()
        starts[f"true_{name}"] = true
        starts[name] = true + SIGMA[name] * torch.randn(true.shape, generator=generator, dtype=torch.float32)
    return starts


class MoreLeaves:
    """Stands where ``KinematicsReconstructor`` stands in the imported run, for one run: makes the reference's instance on a
    scenario whose extra tensors are at their start, and wraps its ``_setup_optimizer_scheduler_early_stopping``."""

    def __init__(self, learned, starts):
        self.learned, self.starts = learned, starts
        self.log = {f"{what}_{name}": [] for name in learned for what in ("start", "grad", "after")}
        self.log["lr"] = []

    def __call__(self, **kwargs):
        kinematics = kwargs["scenario"].heliostat_field.heliostat_groups[0].kinematics
        dtype = kinematics.rotation_deviation_parameters.dtype
        for name in NAMES[1:]:          # (also a tensor that does not learn starts perturbed: the same model in every run)
            holder, attribute = slot(kinematics, name)
            setattr(holder, attribute, self.starts[name].to(dtype).clone())
        assert kwargs["optimization_configuration"] is k.CONFIG
        kwargs["optimization_configuration"] = CONFIG
        reconstructor = REFERENCE_CLASS(**kwargs)
        setup = reconstructor._setup_optimizer_scheduler_early_stopping
        learned, log = self.learned, self.log

        def setup_with_more_leaves(heliostat_group):
            kinematics = heliostat_group.kinematics
            more = []
            for name in learned[1:]:
                holder, attribute = slot(kinematics, name)
                more.append({"params": getattr(holder, attribute).requires_grad_(), "lr": CONFIG["optimization"][RATE_KEYS[name]]})
            adam = torch.optim.Adam

            def adam_with_more_groups(params, *a, **kw):
                return adam(list(params) + more, *a, **kw)

            torch.optim.Adam = adam_with_more_groups        # the scheduler is made of the optimiser inside ``setup``
            try:
                optimizer, scheduler, stopper = setup(heliostat_group=heliostat_group)
            finally:
                torch.optim.Adam = adam
            assert len(optimizer.param_groups) == len(learned) and learned[0] == NAMES[0]
            step = optimizer.step

            def step_recording(*a, **kw):
                leaves = [group["params"][0] for group in optimizer.param_groups]
                for name, leaf in zip(learned, leaves):
                    assert leaf is getattr(*slot(kinematics, name)), name
                    log[f"start_{name}"].append(npy(leaf))
                    log[f"grad_{name}"].append(npy(leaf.grad))      # as handed to step (the rotations': after nan_to_num_)
                log["lr"].append([float(group["lr"]) for group in optimizer.param_groups])
                out = step(*a, **kw)
                for name, leaf in zip(learned, leaves):
                    log[f"after_{name}"].append(npy(leaf))
                return out

            optimizer.step = step_recording
            return optimizer, scheduler, stopper

        reconstructor._setup_optimizer_scheduler_early_stopping = setup_with_more_leaves
        return reconstructor


REFERENCE_CLASS = k.KinematicsReconstructor


def run(method, dtype, measured, starts, learned, distortions_f32=None):
    """The imported run with more leaves; returns what it returns and the per-tensor log."""
    more = MoreLeaves(learned, starts)
    k.KinematicsReconstructor = more
    try:
        log, drawn, once = k.run(method, dtype, measured, distortions_f32=distortions_f32)
    finally:
        k.KinematicsReconstructor = REFERENCE_CLASS
    per_tensor = {key: np.stack([np.asarray(x) for x in value]) for key, value in more.log.items()}
    assert all(len(value) == k.N_EPOCHS for value in per_tensor.values())
    # the imported run's record of the rotation deviations is this one's
    assert np.array_equal(per_tensor["grad_rotation_deviations"], log["grad"])
    assert np.array_equal(per_tensor["after_rotation_deviations"], log["rotation_after"])
    assert np.array_equal(per_tensor["lr"][:, 0], log["lr"])
    return log, drawn, once, per_tensor


def median_sample(loss_per_sample, n_train):
    """Per heliostat: which of its training samples ``torch.median`` picks (the lower of two middle values)."""
    blocks = np.asarray(loss_per_sample, dtype=np.float64).reshape(-1, n_train)
    return np.argsort(blocks, axis=1, kind="stable")[:, (n_train - 1) // 2]


def write(method, name, measured, starts):
    learned = LEARNED[method]
    log32, drawn, once32, more32 = run(method, torch.float32, measured, starts, learned)
    log64, _, once64, more64 = run(method, torch.float64, measured, starts, learned, distortions_f32=drawn)
    mask = np.asarray(k.MASK)
    active, inactive = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
    n_train, n_test, per_heliostat = (int(v) for v in once32["split_counts"])
    assert (n_train, n_test, per_heliostat) == (3, 1, 4) and len(once32["validated_epochs"]) == k.N_EPOCHS
    assert np.isinf(once32["final_loss"][inactive]).all()
    print(f"--- {method}: learns {learned}\nloss per sample:\n{log32['loss_per_sample']}\ntotal loss: {log32['total_loss']}")
    print("lr per epoch and group:\n", more32["lr"])
    expected = np.asarray([CONFIG["optimization"][RATE_KEYS[n]] for n in learned])[None] * k.CONFIG["scheduler"]["gamma"] ** np.arange(k.N_EPOCHS)[:, None]
    assert np.allclose(more32["lr"], expected, rtol=1e-12) and len(set(more32["lr"][0])) == len(learned)
    for tensor in learned:
        g32, g64 = more32[f"grad_{tensor}"], more64[f"grad_{tensor}"]
        assert np.isfinite(g32).all() and np.isfinite(g64).all(), f"a recorded gradient of {tensor} is not finite"
        assert not g32[:, inactive].any() and not g64[:, inactive].any(), f"{tensor}: a heliostat without samples has a gradient"
        flat = g32[:, active].reshape(k.N_EPOCHS, len(active), -1)
        assert (flat != 0).all(), f"{tensor}: a column of an active heliostat has no gradient"
        f_after = f"after_{tensor}"
        start, after = more32[f"start_{tensor}"], more32[f_after]
        assert np.array_equal(after[:-1], start[1:]) and np.array_equal(after[:, inactive], start[:, inactive])
        assert not np.array_equal(after[-1][active], start[0][active])
        print(f"{tensor}: |g| per epoch {np.linalg.norm(g32.reshape(k.N_EPOCHS, -1), axis=1)}, fp32 vs fp64 at epoch 0: gradient "
              f"{rel_l2(g32[0], g64[0]):.2e}; after the step, per epoch "
              f"{[float(f'{rel_l2(after[e], more64[f_after][e]):.2e}') for e in range(k.N_EPOCHS)]}")
    sample_distance = np.abs(log32["loss_per_sample"][0].astype(np.float64) - log64["loss_per_sample"][0])
    print("fp32 vs fp64, epoch 0: loss per sample, largest distance", sample_distance.max(), " prediction",
          rel_l2(log32["prediction"][0], log64["prediction"][0]))
    if method == FLUX:
        gap = k.median_gap(log32["loss_per_sample"], n_train)
        print("gap around each heliostat's median training sample, smallest per epoch:", gap.min(axis=1))
        assert (gap >= 10 * sample_distance.max()).all(), "fp32 and fp64 may pick different median samples"
        for e in range(k.N_EPOCHS):
            assert np.array_equal(median_sample(log32["loss_per_sample"][e], n_train), median_sample(log64["loss_per_sample"][e], n_train)), \
                f"fp32 and fp64 pick different median samples in epoch {e}"
    else:
        assert (sample_distance / np.abs(log64["loss_per_sample"][0])).max() < 1e-2, "acos is quantised at these angles"

    f32 = lambda a: np.asarray(a, dtype=np.float32)  # noqa: E731
    arrays = dict(points_per_facet=np.asarray(k.POINTS_PER_FACET), n_rays=np.int64(k.N_RAYS), resolution=np.asarray(k.RESOLUTION),
                  target=np.asarray(k.TARGET), suns=np.asarray(k.SUNS, dtype=np.float32), configuration=np.asarray(json.dumps(CONFIG)),
                  method=np.asarray(method), learned=np.asarray(list(learned)), sigma=np.float64(k.SIGMA[method]),
                  perturbation_seed=np.int64(PERTURBATION_SEED), measurement_seed=np.int64(k.MEASUREMENT_SEED))
    for tensor in NAMES[1:]:
        arrays[f"sigma_{tensor}"] = np.float64(SIGMA[tensor])
        arrays[f"true_{tensor}"] = f32(npy(starts[f"true_{tensor}"]))
        arrays[f"initial_{tensor}"] = f32(npy(starts[tensor]))          # (of every run, whether the tensor learns or not)
    for kind, count in (("train", len(active) * n_train), ("test", len(active) * n_test)):
        if count in drawn:                                        # (the alignment-driven mode traces for validation only)
            arrays.update({f"seed_{kind}": np.int64(drawn[count][0]), f"distortions_{kind}_u": drawn[count][1],
                           f"distortions_{kind}_e": drawn[count][2]})
    prediction = "flux_predicted" if method == FLUX else "normals_predicted"
    for key in ("loss_per_sample", "loss_per_heliostat", "prediction"):
        arrays[prediction if key == "prediction" else key] = f32(log32[key])
        arrays[f"{prediction if key == 'prediction' else key}_f64_epoch0"] = np.asarray(log64[key][0], dtype=np.float64)
    arrays["total_loss"] = np.asarray(log32["total_loss"], dtype=np.float64)
    arrays["total_loss_f64_epoch0"] = np.float64(log64["total_loss"][0])
    arrays["rotation_start"] = f32(log32["rotation_start"])        # (the key the scenario's builder of the other fixtures reads)
    arrays["lr"] = np.asarray(more32["lr"], dtype=np.float64)
    for tensor in learned:
        for what in ("start", "grad", "after"):
            arrays[f"{what}_{tensor}"] = f32(more32[f"{what}_{tensor}"])
        arrays[f"grad_{tensor}_f64_epoch0"] = np.asarray(more64[f"grad_{tensor}"][0], dtype=np.float64)
        # the value after the step in EVERY epoch of the fp64 run: the first step of Adam moves every coordinate by its learning
        # rate whatever the gradient's size, so the first epoch's distance says nothing about the later ones
        arrays[f"after_{tensor}_f64"] = np.asarray(more64[f"after_{tensor}"], dtype=np.float64)
    for key, value in once32.items():
        if key == "ground_truth":
            if method == ALIGNMENT:
                arrays["normals_measured_train"] = f32(value)
        else:
            arrays[key] = f32(value) if np.asarray(value).dtype.kind == "f" and not key.startswith("history_total") else value
    for key in k.VALIDATION_KEYS:
        arrays[f"test_{key}_f64_epoch0"] = np.asarray(once64[f"test_{key}"][0], dtype=np.float64)
    if method == ALIGNMENT:
        arrays["normals_measured_f64"] = np.asarray(once64["normals_measured"], dtype=np.float64)
    path = OUT_DIR / f"{name}.npz"
    np.savez_compressed(path, **arrays)
    size = path.stat().st_size
    largest = max(p.stat().st_size for p in OUT_DIR.glob("*.npz") if not p.name.startswith("kinematics_parameters_"))
    print(f"wrote {path.name}: {size / 1024:.1f} KiB (largest other fixture {largest / 1024:.1f} KiB), keys={len(arrays)}")
    assert size < largest and size < (1 << 20)


def translations_have_no_gradient_in_alignment_mode(measured, starts):
    """Why the alignment-driven fixture leaves the translations out: as a leaf there, their gradient is identically zero."""
    _, _, _, more = run(ALIGNMENT, torch.float32, measured, starts, NAMES)
    assert not more["grad_translation_deviations"].any() and more["grad_rotation_deviations"].any()
    assert np.array_equal(more["after_translation_deviations"], more["start_translation_deviations"])
    print("alignment-driven, translations as a leaf: gradient identically zero in every epoch")


def main():
    measured = k.measure()
    assert (npy(measured[0]).sum(axis=(1, 2)) > 0).all(), "a measured bitmap is empty"
    starts = perturbed_starts()
    write(FLUX, "kinematics_parameters_flux", measured, starts)
    write(ALIGNMENT, "kinematics_parameters_alignment", measured, starts)
    translations_have_no_gradient_in_alignment_mode(measured, starts)


if __name__ == "__main__":
    main()
