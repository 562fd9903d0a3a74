"""ARTIST's ``KinematicsReconstructor`` as a class, both modes, reproduced epoch by epoch on the GPU (``-m gpu``).

``tests/golden/kinematics_reconstructor_class_flux.npz`` and ``..._alignment.npz`` hold three epochs each of ONE unmodified run of
the reference's ``KinematicsReconstructor.reconstruct_kinematics`` (artist/optim/kinematics_reconstructor.py:135-1063;
tests/golden/generate_kinematics_reconstructor_golden.py: heliostats 0, 2, 4 and 5 of test_blocking.h5 with four calibration
samples each - three for training, one for testing - flux-driven with ``FocalSpotLoss``, alignment-driven with ``AngleLoss``,
validation in every epoch), and its first epoch in fp64 on the same rays.  ``artist_amd.optim.KinematicsReconstructor`` must land
on the reference's numbers: several samples per row of deviations, inactive heliostats between active ones, validation, the
loop's stop logic, the histories, the final loss.

The yardstick is the reference's own fp32-vs-fp64 distance at the first epoch, stored in the fixture: ``err < 3 x yardstick`` -
the factor covers a different but equally valid fp32 evaluation order.  What is traced - the flux-driven epoch and, in both modes,
the validation - also has the floors tests/test_gpu_optimizer_epoch.py uses for this epoch on this scenario: 2e-5 relative L2 for
flux, 2e-5 m for a focal-spot loss (2e-5 relative for the two bitmap losses of the validation), 5e-4 for the gradient.  The
alignment-driven epoch - normals, angles, their gradient - has no floor.  Losses per sample are compared by their largest absolute
distance, and so is their mean.

Measured on MI355X (yardstick -> error of epochs 0 / 1 / 2): see DESIGN.md 4.13.
"""
import json
import pathlib

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAMES = {"raytracing": "kinematics_reconstructor_class_flux", "alignment": "kinematics_reconstructor_class_alignment"}
METHODS = sorted(NAMES)
DEV = torch.device("cuda:0")
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
FLUX_FLOOR, GRAD_FLOOR, LOSS_FLOOR = 2e-5, 5e-4, 2e-5
VALIDATION_KEYS = ("focal_spot_loss", "pixel_loss", "kl_div")


def t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def abs_max(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))))


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _loss_definition(method, scenario):
    from artist_amd import FocalSpotLoss
    from artist_amd.optim import AngleLoss
    return FocalSpotLoss(scenario=scenario) if method == "raytracing" else AngleLoss()


def _reconstructor(method, d, configuration=None):
    """A freshly loaded scenario at the reference's start and the reconstructor on it, configured as the reference's run was;
    the light source hands out the distortions the reference drew on the CPU (sun.py:224-234) and insists on the seed the
    reference passed - the rank in the group's sub-world for the training tracer, the default 7 for the validation's."""
    from artist_amd import CalibrationSamples
    from artist_amd.optim import KinematicsReconstructor
    from artist_amd.scenario import Scenario, open_scenario_file
    path = pathlib.Path(__file__).resolve().parent / "golden" / "scenarios" / "test_blocking.h5"
    points = torch.tensor([int(v) for v in d["points_per_facet"]])
    with open_scenario_file(path) as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file, number_of_surface_points_per_facet=points, device=DEV)
    scenario.set_number_of_rays(number_of_rays=int(d["n_rays"]))
    recorded = {}
    for kind in ("train", "test"):
        if f"distortions_{kind}_u" in d:                   # (the alignment-driven mode traces for validation only)
            both = torch.stack((torch.from_numpy(d[f"distortions_{kind}_u"]), torch.from_numpy(d[f"distortions_{kind}_e"])), dim=-1).to(DEV)
            recorded[both.shape[0]] = (int(d[f"seed_{kind}"]), both)

    def recorded_distortions(number_of_points, number_of_active_heliostats, random_seed=7):
        seed, both = recorded[number_of_active_heliostats]
        assert random_seed == seed and both.shape[1:3] == (int(d["n_rays"]), number_of_points)
        return both[..., 0], both[..., 1]

    scenario.light_sources.light_source_list[0].get_distortions = recorded_distortions
    kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
    np.testing.assert_allclose(n(kinematics.rotation_deviation_parameters), d["true_rotation"], rtol=1e-6, atol=1e-9)
    kinematics.rotation_deviation_parameters = t(d["rotation_start"][0])
    six = (t(d["parser_flux_measured"]), t(d["parser_focal_spots"]), t(d["parser_incident_ray_directions"]),
           t(d["parser_motor_positions"]), t(d["parser_mask"], torch.int32), t(d["parser_target_area_indices"], torch.long))
    reconstructor = KinematicsReconstructor(
        ddp_setup=DDP, scenario=scenario, data={"data_parser": CalibrationSamples(six), "heliostat_data_mapping": []},
        optimization_configuration=configuration or json.loads(str(d["configuration"])), reconstruction_method=method,
        bitmap_resolution=torch.tensor([int(v) for v in d["resolution"]]), device=DEV)
    return reconstructor, scenario


def _bounds(method, d):
    """The reference's own fp32-vs-fp64 distance at the first epoch -> the bounds: 3 x yardstick, with the floors of the traced
    quantities (module docstring)."""
    flux_driven = method == "raytracing"
    prediction = "flux_predicted" if flux_driven else "normals_predicted"
    yard = dict(prediction=rel_l2(d[prediction][0], d[f"{prediction}_f64_epoch0"]), grad=rel_l2(d["grad"][0], d["grad_f64_epoch0"]),
                loss=abs_max(d["loss_per_sample"][0], d["loss_per_sample_f64_epoch0"]),
                test_focal_spot_loss=abs_max(d["test_focal_spot_loss"][0], d["test_focal_spot_loss_f64_epoch0"]),
                test_pixel_loss=rel_max(d["test_pixel_loss"][0], d["test_pixel_loss_f64_epoch0"]),
                test_kl_div=rel_max(d["test_kl_div"][0], d["test_kl_div_f64_epoch0"]))
    floor = dict(test_focal_spot_loss=LOSS_FLOOR, test_pixel_loss=LOSS_FLOOR, test_kl_div=LOSS_FLOOR)
    if flux_driven:
        floor.update(prediction=FLUX_FLOOR, grad=GRAD_FLOOR, loss=LOSS_FLOOR)
    bound = {k: max(3 * v, floor.get(k, 0.0)) for k, v in yard.items()}
    print(f"{method}: the reference's own fp32-vs-fp64 distance, first epoch: " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    print(f"{method}: bounds: " + ", ".join(f"{k} {v:.2e}" for k, v in bound.items()))
    return bound


def _step(reconstructor, state, loss_definition):
    """What the loop does between its scheduler steps: one epoch's loss, backward, the alignment mode's clean-up, the step."""
    state.optimizer.zero_grad()
    loss = reconstructor.epoch_loss(state, loss_definition, DEV)
    loss.total.backward()
    if reconstructor.reconstruction_method == "alignment":
        state.optimizer.param_groups[0]["params"][0].grad.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
    state.optimizer.step()
    return loss


@pytest.mark.parametrize("method", METHODS)
def test_each_epoch_of_the_reference_run_is_reproduced(golden, method):
    """From the reference's rotation deviations at the start of each epoch: the predicted flux of the twelve training samples
    (flux-driven) or their predicted normals (alignment-driven), the loss per sample and per heliostat, the total loss and
    the gradient w.r.t. the ``[6, 4]`` deviations - three samples summed into each row, exactly nothing for the heliostats
    without samples."""
    d = golden(NAMES[method])
    bound = _bounds(method, d)
    reconstructor, scenario = _reconstructor(method, d)
    loss_definition = _loss_definition(method, scenario)
    prediction_key = "flux_predicted" if method == "raytracing" else "normals_predicted"
    state = reconstructor.prepare(0, DEV)
    parameter = scenario.heliostat_field.heliostat_groups[0].kinematics.rotation_deviation_parameters
    assert parameter.requires_grad and state.optimizer.param_groups[0]["params"][0] is parameter
    active, inactive = np.nonzero(d["parser_mask"])[0], np.nonzero(d["parser_mask"] == 0)[0]
    np.testing.assert_array_equal(n(state.active_rows), active)
    if method == "alignment":
        err = abs_max(n(state.normals_measured), d["normals_measured"])
        print(f"measured normals: largest distance {err:.2e} (the reference's fp32 vs fp64: {abs_max(d['normals_measured'], d['normals_measured_f64']):.2e})")
        assert err <= 4 * float(np.finfo(np.float32).eps)         # two normalisations of differences of fp32 inputs (the CPU test's bound)
        assert torch.equal(state.normals_measured_train, state.normals_measured[t(d["train_indices"], torch.long)])
    missed = []
    for e in range(d["rotation_start"].shape[0]):
        with torch.no_grad():
            parameter.copy_(t(d["rotation_start"][e]))
        parameter.grad = None
        loss = reconstructor.epoch_loss(state, loss_definition, DEV)
        loss.total.backward()
        grad = n(parameter.grad)
        assert loss.prediction.shape == d[prediction_key][e].shape and loss.per_sample.shape == (12,) and loss.per_heliostat.shape == (4,)
        err = dict(prediction=rel_l2(n(loss.prediction), d[prediction_key][e]), grad=rel_l2(grad, d["grad"][e]),
                   loss=abs_max(n(loss.per_sample), d["loss_per_sample"][e]),
                   loss_per_heliostat=abs_max(n(loss.per_heliostat), d["loss_per_heliostat"][e]),
                   total=abs_max(float(loss.total.detach()), d["total_loss"][e]))
        print(f"{method} epoch {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) +
              f"; total loss {float(loss.total.detach()):.7f} (reference {d['total_loss'][e]:.7f})")
        assert np.isfinite(grad).all() and not grad[inactive].any() and grad[active].all()
        missed += [(e, key, value, bound.get(key, bound["loss"])) for key, value in err.items() if not value < bound.get(key, bound["loss"])]
        if e == 0:       # ... and as close to the fp64 run as the reference's own fp32 run is
            err64 = dict(prediction=rel_l2(n(loss.prediction), d[f"{prediction_key}_f64_epoch0"]), grad=rel_l2(grad, d["grad_f64_epoch0"]),
                         loss=abs_max(n(loss.per_sample), d["loss_per_sample_f64_epoch0"]))
            print(f"{method} epoch 0 against the fp64 run: " + ", ".join(f"{k} {v:.2e}" for k, v in err64.items()))
            missed += [(e, key + " (fp64)", value, bound[key]) for key, value in err64.items() if not value < bound[key]]
    assert not missed, missed


_RUNS = {}


def _whole_runs(method, d):
    """``reconstruct_kinematics`` twice, each on a freshly loaded scenario (shared by the tests below): what it returned, the
    gradient before and the deviations after every step, every validation and the last epoch's loss per heliostat."""
    if method not in _RUNS:
        runs = []
        for _ in range(2):
            reconstructor, scenario = _reconstructor(method, d)
            kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
            start = n(kinematics.rotation_deviation_parameters).copy()
            grads, after, validations, last = [], [], [], {}
            prepare, epoch_loss, validate = reconstructor.prepare, reconstructor.epoch_loss, reconstructor.validate

            def prepare_recording(*a, _prepare=prepare, _grads=grads, _after=after, **k):
                state = _prepare(*a, **k)
                step = state.optimizer.step

                def step_recording(*sa, **sk):
                    parameter = state.optimizer.param_groups[0]["params"][0]
                    _grads.append(n(parameter.grad).copy())
                    out = step(*sa, **sk)
                    _after.append(n(parameter).copy())
                    return out

                state.optimizer.step = step_recording
                return state

            def epoch_loss_recording(*a, _epoch_loss=epoch_loss, _last=last, **k):
                _last["loss"] = _epoch_loss(*a, **k)
                return _last["loss"]

            def validate_recording(*a, _validate=validate, _validations=validations, _after=after, **k):
                out = _validate(*a, **k)
                _validations.append((len(_after) - 1, {key: n(value).copy() for key, value in out.items()}))
                return out

            reconstructor.prepare, reconstructor.epoch_loss, reconstructor.validate = prepare_recording, epoch_loss_recording, validate_recording
            final_loss, histories = reconstructor.reconstruct_kinematics(loss_definition=_loss_definition(method, scenario), device=DEV)
            runs.append(dict(final_loss=final_loss, histories=histories, start=start, grads=grads, after=after, validations=validations,
                             kinematics=kinematics, last_per_heliostat=n(last["loss"].per_heliostat)))
        _RUNS[method] = runs
    return _RUNS[method]


@pytest.mark.parametrize("method", METHODS)
def test_the_whole_run_through_reconstruct_kinematics(golden, method):
    """``reconstruct_kinematics()`` for three epochs (``max_epoch=2``, tolerance 0, ``log_step=1``): the history, the rotation
    deviations after every step in units of the learning rate (Adam's first steps move every coordinate by about +-lr whatever
    its gradient's size, so a coordinate whose gradient is almost zero may step the other way), the final loss with its
    ``inf`` pattern, the three losses of every validation."""
    d = golden(NAMES[method])
    bound = _bounds(method, d)
    run = _whole_runs(method, d)[0]
    final_loss, histories = run["final_loss"], run["histories"]
    mask = d["parser_mask"]
    active, inactive = np.nonzero(mask)[0], np.nonzero(mask == 0)[0]
    missed = []
    assert len(histories) == 1 and len(histories[0]) == 1
    history = histories[0][0]
    assert set(history) == {"total_loss", "test_loss"}
    assert len(history["total_loss"]) == len(d["history_total_loss"]) == 3 and all(isinstance(x, float) for x in history["total_loss"])
    print(f"{method}: total loss per epoch {history['total_loss']}, reference {d['history_total_loss'].tolist()}")
    for e in range(3):
        err = abs(history["total_loss"][e] - d["history_total_loss"][e])
        print(f"{method} epoch {e}: total loss differs by {err:.2e} (bound {bound['loss']:.2e})")
        if not err < bound["loss"]:
            missed.append((e, "history", err, bound["loss"]))

    # the rotation deviations after every step
    lrs = d["lr"]
    assert len(run["after"]) == 3
    for e in range(3):
        moved = (run["after"][e] - d["rotation_after"][e]) / lrs[e]
        big = np.abs(d["grad"][e]) > 1e-3 * np.abs(d["grad"][e]).max()
        print(f"{method} epoch {e}: rotation deviations differ from the reference's by at most {np.abs(moved[big]).max():.4f} lr where the "
              f"gradient is sizeable ({int(big.sum())} of {int((d['grad'][e] != 0).sum())}), {np.abs(moved).max():.4f} lr anywhere")
        assert np.abs(moved[big]).max() < 0.05 and np.abs(moved).max() < 2.0 * (e + 1) + 0.1, (e, np.abs(moved[big]).max(), np.abs(moved).max())
        np.testing.assert_array_equal(run["after"][e][inactive], run["start"][inactive])        # no sample, no step
    assert not np.array_equal(run["after"][-1][active], run["start"][active])
    parameter = run["kinematics"].rotation_deviation_parameters
    assert not parameter.requires_grad and parameter.grad_fn is None                            # detached at the end
    np.testing.assert_array_equal(n(parameter), run["after"][-1])

    # the final loss: inf exactly at the heliostats without samples, the last epoch's loss per heliostat elsewhere
    assert final_loss.device.type == "cpu" and final_loss.shape == (6,) and not final_loss.requires_grad
    assert np.isinf(n(final_loss)[inactive]).all() and (n(final_loss)[inactive] > 0).all()
    np.testing.assert_array_equal(n(final_loss)[active], run["last_per_heliostat"])
    assert float(np.mean(n(final_loss)[active].astype(np.float64))) == pytest.approx(history["total_loss"][-1], rel=1e-6)
    err = abs_max(n(final_loss)[active], d["final_loss"][active])
    print(f"{method}: final loss differs by {err:.2e}")
    if not err < bound["loss"]:
        missed.append(("final", "loss", err, bound["loss"]))

    # validation ran after every epoch, the last of them is the history's
    assert d["validated_epochs"].tolist() == [0, 1, 2] and [epoch for epoch, _ in run["validations"]] == [0, 1, 2]
    assert set(history["test_loss"]) == set(VALIDATION_KEYS)
    for v, (_, losses) in enumerate(run["validations"]):
        err = dict(test_focal_spot_loss=abs_max(losses["focal_spot_loss"], d["test_focal_spot_loss"][v]),
                   test_pixel_loss=rel_max(losses["pixel_loss"], d["test_pixel_loss"][v]),
                   test_kl_div=rel_max(losses["kl_div"], d["test_kl_div"][v]))
        print(f"{method} validation {v}: " + ", ".join(f"{k} {x:.2e}" for k, x in err.items()) + f"; focal spot {losses['focal_spot_loss']}, "
              f"pixel {losses['pixel_loss']}, kl {losses['kl_div']}")
        missed += [(v, key, value, bound[key]) for key, value in err.items() if not value < bound[key]]
    for key in VALIDATION_KEYS:
        assert history["test_loss"][key].shape == (4,) and history["test_loss"][key].device.type == "cuda"
        np.testing.assert_array_equal(n(history["test_loss"][key]), run["validations"][-1][1][key])
    assert not missed, missed


@pytest.mark.parametrize("method", METHODS)
def test_a_second_run_gives_the_same_bits(golden, method):
    """Three training samples are summed into every row of the deviations: in a fixed order, so a second run on a freshly loaded
    scenario gives the same gradients, the same deviations after every step and the same history values.  (In the flux-driven
    mode the median passes one sample's gradient on; in the alignment-driven mode all three samples of a heliostat have
    one, so that run is the one that would catch an unordered sum.)"""
    d = golden(NAMES[method])
    first, second = _whole_runs(method, d)
    assert torch.equal(first["final_loss"], second["final_loss"])
    a, b = first["histories"][0][0], second["histories"][0][0]
    assert a["total_loss"] == b["total_loss"]
    for key in VALIDATION_KEYS:
        assert torch.equal(a["test_loss"][key], b["test_loss"][key])
    for x, y in zip(first["grads"] + first["after"], second["grads"] + second["after"]):
        np.testing.assert_array_equal(x, y)
    if method == "alignment":
        assert len(first["grads"]) == 3 and all(g[np.nonzero(d["parser_mask"])[0]].all() for g in first["grads"])


@pytest.mark.parametrize("method", METHODS)
def test_one_epoch_runs_on_the_existing_entry_points(golden, monkeypatch, method):
    """One epoch - prepare, loss, backward, step - through the library handle: every kernel the epoch is made of is called,
    through the signature table every entry point is in, and nothing else - no NURBS evaluation, no crop, nothing of blocking or
    shading; the alignment-driven epoch is the kinematics kernel both ways and the step."""
    from artist_amd import _lib
    d = golden(NAMES[method])
    reconstructor, scenario = _reconstructor(method, d)
    handle = _lib.lib()
    calls = []
    for name in _lib.SIGNATURES:
        if name in ("art_abi_version", "art_last_hip_error", "art_strerror", "art_async_status", "art_blocking_workspace_bytes",
                    "art_trace_bwd_scratch_floats", "art_trace_bwd_scratch_need"):
            continue
        real = getattr(handle, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append(_name)
            return _real(*args)

        monkeypatch.setattr(handle, name, wrapped)
    state = reconstructor.prepare(0, DEV)
    _step(reconstructor, state, _loss_definition(method, scenario))
    torch.cuda.synchronize()
    monkeypatch.undo()
    called = set(calls)
    print(f"{method}: entry points of one epoch: {sorted(called)}")
    kinematics = {"art_rigid_body_fwd", "art_rigid_body_bwd", "art_adam_step"}
    if method == "alignment":
        assert called == kinematics, sorted(called)
    else:
        assert kinematics | {"art_align_fwd", "art_align_bwd", "art_trace_fwd", "art_trace_bwd", "art_flux_center_of_mass",
                             "art_flux_center_of_mass_bwd"} <= called, sorted(called)
        assert not [name for name in called if name.startswith(("art_blocking", "art_shading", "art_nurbs", "art_flux_crop"))]
        assert calls.count("art_trace_fwd") == 1 and calls.count("art_trace_bwd") == 1
    # one evaluation of the kinematics per epoch for all samples, each way
    assert calls.count("art_rigid_body_fwd") == 1 and calls.count("art_rigid_body_bwd") == 1 and calls.count("art_adam_step") == 1


@pytest.mark.parametrize("method", METHODS)
def test_an_epoch_does_not_wait_for_the_device(golden, method):
    """After a warm-up epoch (the first use of a tensor checks it on the host, once), ``epoch_loss`` + ``backward`` + ``step``
    read nothing from the device: the loop's one read per epoch is the loss, after the step has been queued."""
    d = golden(NAMES[method])
    reconstructor, scenario = _reconstructor(method, d)
    loss_definition = _loss_definition(method, scenario)
    state = reconstructor.prepare(0, DEV)
    first = _step(reconstructor, state, loss_definition)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = _step(reconstructor, state, loss_definition)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(second.total.detach()) < float(first.total.detach())                # ... and it was an epoch: the loss went down


@pytest.mark.parametrize("method", METHODS)
def test_the_loop_stops_as_the_reference_does(golden, method):
    """The ways out of the loop (kinematics_reconstructor.py:806-809, 836-860).  ``max_epoch`` 2: three epochs (the whole run
    above).  Early stopping with a window of two epochs, a patience of one and an improvement nobody reaches: the second epoch
    fills the window and stops, validates, and breaks BEFORE its history entry - one entry, while the final loss is the second
    epoch's.  A tolerance above the first epoch's loss: the loop's condition ends the run after that epoch, whose entry is there."""
    d = golden(NAMES[method])
    bound = _bounds(method, d)
    active = d["parser_mask"] > 0
    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"].update(early_stopping_window=2, early_stopping_patience=1, early_stopping_delta=10.0, max_epoch=5)
    reconstructor, scenario = _reconstructor(method, d, configuration)
    validations = []
    validate = reconstructor.validate
    reconstructor.validate = lambda *a, **k: validations.append(1) or validate(*a, **k)
    final_loss, histories = reconstructor.reconstruct_kinematics(loss_definition=_loss_definition(method, scenario), device=DEV)
    history = histories[0][0]
    assert len(history["total_loss"]) == 1 and len(validations) == 2              # epoch 0 and the epoch that stopped
    assert abs(history["total_loss"][0] - d["history_total_loss"][0]) < bound["loss"]
    second = float(np.mean(n(final_loss)[active].astype(np.float64)))               # ... the final loss is the second epoch's
    assert abs(second - d["history_total_loss"][1]) < bound["loss"], (second, d["history_total_loss"][1])

    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"].update(tolerance=1e9, log_step=0)
    reconstructor, scenario = _reconstructor(method, d, configuration)
    final_loss, histories = reconstructor.reconstruct_kinematics(loss_definition=_loss_definition(method, scenario), device=DEV)
    assert len(histories[0][0]["total_loss"]) == 1 and set(histories[0][0]["test_loss"]) == set(VALIDATION_KEYS)   # (0 % max_epoch == 0)
    np.testing.assert_allclose(float(np.mean(n(final_loss)[active].astype(np.float64))), histories[0][0]["total_loss"][0], rtol=1e-6)
