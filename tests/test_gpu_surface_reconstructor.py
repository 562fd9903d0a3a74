"""ARTIST's ``SurfaceReconstructor`` as a class, reproduced epoch by epoch on the GPU (``-m gpu``).

``tests/golden/surface_reconstructor_class_epochs.npz`` holds three epochs of ONE unmodified run of the reference's
``SurfaceReconstructor.reconstruct_surfaces`` (artist/optim/surface_reconstructor.py:842-1160;
tests/golden/generate_surface_reconstructor_golden.py: heliostats 0, 2 and 5 of test_blocking.h5 with four calibration samples
each - three for training, one for testing - on two planar targets, ``PixelLoss``, both regularisers, the flux-integral
constraint active from the first epoch), and its first epoch in fp64 on the same rays.  ``artist_amd.optim.SurfaceReconstructor``
must land on the reference's numbers: several samples per control net, inactive heliostats between active ones, the constraint
and its multiplier, validation, the loop's stop logic, the histories, the final loss, ``update_surfaces``.

The yardstick is the reference's own fp32-vs-fp64 distance at the first epoch: ``err < max(3 x yardstick, floor)`` with the floors
of tests/test_gpu_optimizer_epoch.py (2e-5 relative L2 for cropped flux, 5e-4 for the locked gradient, 2e-5 relative for a loss).
The constraint term is a small difference of large numbers (a sample's flux integral moves by 1e-7 to 2.5e-3 of its reference): its
tolerance is the flux bound carried through the term's formula.

Measured on MI355X (yardstick -> error of epochs 0 / 1 / 2): see DESIGN.md 4.12.
"""
import json
import pathlib

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

NAME = "surface_reconstructor_class_epochs"
DEV = torch.device("cuda:0")
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
FLUX_FLOOR, GRAD_FLOOR, LOSS_FLOOR = 2e-5, 5e-4, 2e-5
CHAINED_LOSS_FLOOR = 1e-4               # tests/test_gpu_optimizer_epoch.py: the total loss of the chained run
HISTORY_KEYS = {"total_loss", "flux_loss", "smoothness_regularizer", "ideal_regularizer", "flux_integral", "flux_integral_constraint",
                "test_loss"}


def t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def rel_max(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))


def _reconstructor(d, configuration=None):
    """A freshly loaded scenario and the reconstructor on it, configured as the reference's run was; the light source hands out
    the distortions the reference drew on the CPU (sun.py:224-234 with the seed the class passes: the group's rank), the
    in-memory parser the reference's six tensors."""
    from artist_amd import CalibrationSamples
    from artist_amd.optim import SurfaceReconstructor
    from artist_amd.scenario import Scenario, open_scenario_file
    path = pathlib.Path(__file__).resolve().parent / "golden" / "scenarios" / "test_blocking.h5"
    points = torch.tensor([int(v) for v in d["points_per_facet"]])
    with open_scenario_file(path) as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file, number_of_surface_points_per_facet=points, device=DEV)
    scenario.set_number_of_rays(number_of_rays=int(d["n_rays"]))
    recorded = {}
    for kind in ("train", "test"):
        both = torch.stack((torch.from_numpy(d[f"distortions_{kind}_u"]), torch.from_numpy(d[f"distortions_{kind}_e"])), dim=-1).to(DEV)
        recorded[both.shape[0]] = (int(d[f"seed_{kind}"]), both)

    def recorded_distortions(number_of_points, number_of_active_heliostats, random_seed=7):
        seed, both = recorded[number_of_active_heliostats]
        assert random_seed == seed and both.shape[1:3] == (int(d["n_rays"]), number_of_points)
        return both[..., 0], both[..., 1]

    scenario.light_sources.light_source_list[0].get_distortions = recorded_distortions
    six = (t(d["parser_flux_measured"]), t(d["parser_focal_spots"]), t(d["parser_incident_ray_directions"]),
           t(d["parser_motor_positions"]), t(d["parser_mask"], torch.int32), t(d["parser_target_area_indices"], torch.long))
    reconstructor = SurfaceReconstructor(
        ddp_setup=DDP, scenario=scenario, data={"data_parser": CalibrationSamples(six), "heliostat_data_mapping": []},
        optimization_configuration=configuration or json.loads(str(d["configuration"])), number_of_surface_points=points,
        bitmap_resolution=torch.tensor([int(v) for v in d["resolution"]]), epsilon=float(d["epsilon"]), device=DEV)
    return reconstructor, scenario


def _control_points_at_start(d, e):
    """The reference's control points at the start of epoch ``e``: the file's nets, with the rows of the heliostats that have
    samples as the step before left them (the fixture stores those rows only)."""
    nets = d["cp_start_epoch0"].copy()
    if e > 0:
        nets[np.nonzero(d["parser_mask"])[0]] = d["cp_after"][e - 1]
    return nets


def _yardsticks(d):
    """The reference's own fp32-vs-fp64 distance at the first epoch -> the bounds ``max(3 x yardstick, floor)``."""
    yard = dict(flux=rel_l2(d["cropped_epoch0"], d["cropped_f64_epoch0"]), sums=rel_l2(d["cropped_sums"][0], d["cropped_sums_f64_epoch0"]),
                grad=rel_l2(d["grad_locked"][0], d["grad_locked_f64_epoch0"]),
                loss_per_sample=rel_max(d["flux_loss_per_sample"][0], d["flux_loss_per_sample_f64_epoch0"]),
                loss_per_heliostat=rel_max(d["flux_loss_per_heliostat"][0], d["flux_loss_per_heliostat_f64_epoch0"]),
                total_per_heliostat=rel_max(d["total_loss_per_heliostat"][0], d["total_loss_per_heliostat_f64_epoch0"]),
                total=rel_max(d["total_loss"][0], d["total_loss_f64_epoch0"]),
                test_pixel=rel_max(d["test_pixel_loss"][0], d["test_pixel_loss_f64_epoch0"]),
                test_kl=rel_max(d["test_kl_div"][0], d["test_kl_div_f64_epoch0"]))
    floor = dict(flux=FLUX_FLOOR, sums=FLUX_FLOOR, grad=GRAD_FLOOR)
    bound = {k: max(3 * v, floor.get(k, LOSS_FLOOR)) for k, v in yard.items()}
    print("the reference's own fp32-vs-fp64 distance, first epoch: " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    print("bounds max(3 x yardstick, floor): " + ", ".join(f"{k} {v:.2e}" for k, v in bound.items()))
    return yard, bound


def test_each_epoch_of_the_reference_run_is_reproduced(golden):
    """From the reference's starting point of each epoch (control points, multiplier, reference integrals): the cropped flux of
    the nine training samples, the losses per sample and per heliostat, the constraint's term, relative differences and
    violation, S, I, alpha, beta, the total loss per heliostat and its mean, the multiplier after the epoch and the locked
    gradient - three samples summed into each control net, nothing for the heliostats without samples."""
    from artist_amd import PixelLoss
    d = golden(NAME)
    _, bound = _yardsticks(d)
    reconstructor, scenario = _reconstructor(d)
    group = scenario.heliostat_field.heliostat_groups[0]
    loaded = n(group.nurbs_control_points)
    print("the loaded nets equal the reference's bit for bit:", np.array_equal(loaded, d["cp_start_epoch0"]))
    np.testing.assert_allclose(loaded, d["cp_start_epoch0"], rtol=1e-6, atol=1e-9)
    state = reconstructor.prepare(0, DEV)
    active = np.nonzero(d["parser_mask"])[0]
    inactive = np.nonzero(d["parser_mask"] == 0)[0]
    np.testing.assert_array_equal(n(state.active_rows), active)
    config = json.loads(str(d["configuration"]))["constraints"]
    rho = config["rho_flux_integral"]
    for e in range(d["cp_after"].shape[0]):
        with torch.no_grad():
            group.nurbs_control_points.copy_(t(_control_points_at_start(d, e)))
        group.nurbs_control_points.grad = None
        state.multiplier = t(d["lambda_before"][e])
        state.reference_integrals = t(d["reference_before"][e]) if e > 0 else None
        cropped = reconstructor.predict_flux(state, DEV)
        loss = reconstructor.epoch_loss(state, cropped, PixelLoss(), DEV)
        loss.total.backward()
        reconstructor.update_multiplier(state, loss.violation)
        locked = n(reconstructor.lock_control_points_on_outer_edges(group.nurbs_control_points.grad))
        sums = n(cropped.sum(dim=(1, 2)))
        err = dict(flux=rel_l2(n(cropped), d["cropped_epoch0"]) if e == 0 else float("nan"), sums=rel_l2(sums, d["cropped_sums"][e]),
                   grad=rel_l2(locked[active], d["grad_locked"][e]),
                   loss_per_sample=rel_max(n(loss.flux_loss_per_sample), d["flux_loss_per_sample"][e]),
                   loss_per_heliostat=rel_max(n(loss.flux_loss_per_heliostat), d["flux_loss_per_heliostat"][e]),
                   total_per_heliostat=rel_max(n(loss.total_per_heliostat), d["total_loss_per_heliostat"][e]),
                   total=rel_max(float(loss.total.detach()), d["total_loss"][e]))
        print(f"epoch {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) +
              f"; total loss {float(loss.total.detach()):.7f} (reference {d['total_loss'][e]:.7f}); constraint {n(loss.constraint)} "
              f"({d['constraint'][e]}); alpha {float(loss.alpha.detach()):.6e} ({float(d['alpha'][e]):.6e}), beta {float(loss.beta.detach()):.6e} "
              f"({float(d['beta'][e]):.6e})")
        assert cropped.shape == (9, 64, 64) and not locked[inactive].any()
        for key, value in err.items():
            assert value < bound[key] or (key == "flux" and e > 0), (e, key, value, bound[key])
        # the regularisers as tests/test_gpu_regularized_epoch.py holds them; both are exactly zero at the start
        np.testing.assert_allclose(n(loss.smoothness), d["smoothness"][e], rtol=1e-5, atol=0)
        np.testing.assert_allclose(n(loss.ideal), d["ideal"][e], rtol=1e-5, atol=0)
        np.testing.assert_allclose(float(loss.alpha.detach()), float(d["alpha"][e]), rtol=max(1e-5, bound["loss_per_heliostat"]))
        np.testing.assert_allclose(float(loss.beta.detach()), float(d["beta"][e]), rtol=max(1e-5, bound["loss_per_heliostat"]))
        # the constraint: every sum may be off by the flux bound, so a relative difference and with it a violation by
        # delta = bound x sum / reference, and the term lambda v + rho / 2 v^2 by (lambda + rho v) delta + rho / 2 delta^2
        reference = d["reference_after"][e].astype(np.float64)
        delta = float(np.max(bound["sums"] * d["cropped_sums"][e] / reference)) if e > 0 else 0.0   # (epoch 0: the sums ARE the reference)
        np.testing.assert_array_equal(n(state.reference_integrals), sums if e == 0 else d["reference_before"][e])
        np.testing.assert_allclose(n(loss.relative_differences), d["relative_differences"][e], rtol=1e-5, atol=delta)
        np.testing.assert_allclose(n(loss.violation), d["violation"][e], rtol=1e-5, atol=delta)
        term_tolerance = np.max((d["lambda_before"][e] + rho * d["violation"][e]) * delta + 0.5 * rho * delta ** 2)
        np.testing.assert_allclose(n(loss.constraint), d["constraint"][e], rtol=1e-5, atol=term_tolerance)
        np.testing.assert_allclose(n(state.multiplier), d["lambda_after"][e], rtol=1e-5, atol=rho * delta)
        assert n(loss.constraint).min() > 0 and n(state.multiplier).min() > 0          # the constraint acts in every epoch
        if e == 0:       # ... and as close to the fp64 run as the reference's own fp32 run is
            assert rel_l2(locked[active], d["grad_locked_f64_epoch0"]) < bound["grad"]
            assert rel_l2(n(cropped), d["cropped_f64_epoch0"]) < bound["flux"]


_RUNS = {}


def _whole_runs(d):
    """``reconstruct_surfaces`` twice, each on a freshly loaded scenario (shared by the tests below): what it returned, the
    control points after every step, the last epoch's loss per heliostat and the field's surface points afterwards."""
    if not _RUNS:
        from artist_amd import PixelLoss
        for run in range(2):
            reconstructor, scenario = _reconstructor(d)
            group = scenario.heliostat_field.heliostat_groups[0]
            start = n(group.nurbs_control_points).copy()
            after, last = [], {}
            prepare, epoch_loss = reconstructor.prepare, reconstructor.epoch_loss

            def prepare_recording(*a, _prepare=prepare, _after=after, **k):
                state = _prepare(*a, **k)
                step = state.optimizer.step

                def step_recording(*sa, **sk):
                    out = step(*sa, **sk)
                    _after.append(n(state.group.nurbs_control_points).copy())
                    return out

                state.optimizer.step = step_recording
                return state

            def epoch_loss_recording(*a, _epoch_loss=epoch_loss, _last=last, **k):
                _last["loss"] = _epoch_loss(*a, **k)
                return _last["loss"]

            reconstructor.prepare, reconstructor.epoch_loss = prepare_recording, epoch_loss_recording
            final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=PixelLoss(), device=DEV)
            _RUNS[run] = dict(final_loss=final_loss, histories=histories, start=start, after=after, group=group,
                              last_total_per_heliostat=n(last["loss"].total_per_heliostat), surface_points=n(group.surface_points),
                              surface_normals=n(group.surface_normals))
    return _RUNS[0], _RUNS[1]


def test_the_whole_run_through_reconstruct_surfaces(golden):
    """``reconstruct_surfaces()`` for three epochs (``max_epoch=2``, tolerance 0): histories, total losses, control points after
    every step in units of the learning rate (Adam's first steps move every coordinate by about +-lr whatever its gradient's
    size, so a coordinate whose gradient is almost zero may step the other way), the outline, the final loss, the last
    validation, the field's surface points after ``update_surfaces``."""
    d = golden(NAME)
    _, bound = _yardsticks(d)
    run, _ = _whole_runs(d)
    final_loss, histories = run["final_loss"], run["histories"]
    mask = d["parser_mask"]
    active = np.nonzero(mask)[0]
    assert len(histories) == 1 and len(histories[0]) == 1
    history = histories[0][0]
    assert set(history) == HISTORY_KEYS
    for key in HISTORY_KEYS - {"test_loss"}:
        assert len(history[key]) == len(d[f"history_{key}"]) == 3 and all(isinstance(x, float) for x in history[key]), key
    print("total loss per epoch:", history["total_loss"], " reference:", d["history_total_loss"])
    loss_bound = max(3 * rel_max(d["total_loss"][0], d["total_loss_f64_epoch0"]), CHAINED_LOSS_FLOOR)
    for e in range(3):
        assert abs(history["total_loss"][e] - d["history_total_loss"][e]) / abs(d["history_total_loss"][e]) < loss_bound
        assert abs(history["flux_loss"][e] - d["history_flux_loss"][e]) / abs(d["history_flux_loss"][e]) < \
            max(bound["loss_per_heliostat"], CHAINED_LOSS_FLOOR)
    assert history["flux_integral"][0] == 0.0 and history["smoothness_regularizer"][0] == 0.0 and history["ideal_regularizer"][0] == 0.0
    np.testing.assert_allclose(history["flux_integral_constraint"][0], d["history_flux_integral_constraint"][0], rtol=1e-5)
    assert history["flux_integral_constraint"][2] > history["flux_integral_constraint"][1] > history["flux_integral_constraint"][0] > 0

    # control points after every step
    lrs = d["lr"]
    assert len(run["after"]) == 3
    for e in range(3):
        moved = (run["after"][e][active] - d["cp_after"][e]) / lrs[e]
        frac_close = float((np.abs(moved) < 0.05).mean())
        print(f"epoch {e}: control points within 0.05 lr of the reference's: {100 * frac_close:.2f} %, largest difference "
              f"{np.abs(moved).max():.3f} lr")
        assert frac_close > 0.97 and np.abs(moved).max() < 2.0 * (e + 1) + 0.1, (e, frac_close, np.abs(moved).max())
    end, start = run["after"][-1], run["start"]
    inactive = np.nonzero(mask == 0)[0]
    np.testing.assert_array_equal(end[inactive], start[inactive])                   # no sample, no step
    for edge in (np.s_[:, :, 0], np.s_[:, :, -1], np.s_[:, :, :, 0], np.s_[:, :, :, -1]):   # the outer control points keep u and v
        np.testing.assert_array_equal(end[edge][..., :2], start[edge][..., :2])
    assert not np.array_equal(end[active][:, :, 0, :, 2], start[active][:, :, 0, :, 2])      # ... and z moved
    np.testing.assert_array_equal(n(run["group"].nurbs_control_points), end)

    # the final loss: inf exactly at the heliostats without samples, the last epoch's total per heliostat elsewhere
    assert final_loss.device.type == "cpu" and final_loss.shape == (6,) and not final_loss.requires_grad
    assert np.isinf(n(final_loss)[mask == 0]).all() and (n(final_loss)[mask == 0] > 0).all()
    np.testing.assert_array_equal(n(final_loss)[active], run["last_total_per_heliostat"])
    assert float(np.mean(n(final_loss)[active].astype(np.float64))) == pytest.approx(history["total_loss"][-1], rel=1e-6)
    assert rel_max(n(final_loss)[active], d["final_loss"][active]) < max(bound["total_per_heliostat"], CHAINED_LOSS_FLOOR)

    # the last validation ran after the second epoch (epoch == max_epoch - 1), none after the third
    assert d["validated_epochs"].tolist() == [0, 1]
    test_loss = history["test_loss"]
    assert set(test_loss) == {"pixel_loss", "kl_div"}
    errs = dict(pixel=rel_max(n(test_loss["pixel_loss"]), d["history_test_pixel_loss"]), kl=rel_max(n(test_loss["kl_div"]), d["history_test_kl_div"]))
    print("test loss after the second epoch:", n(test_loss["pixel_loss"]), n(test_loss["kl_div"]), " reference:",
          d["history_test_pixel_loss"], d["history_test_kl_div"], " relative error:", errs)
    assert errs["pixel"] < max(bound["test_pixel"], CHAINED_LOSS_FLOOR) and errs["kl"] < max(bound["test_kl"], CHAINED_LOSS_FLOOR)

    # update_surfaces: the field's surface points follow the new control points
    h = int(d["recorded_heliostat"])
    err = rel_l2(run["surface_points"][h], d["updated_surface_points"])
    print(f"surface points of heliostat {h} after update_surfaces: relative L2 {err:.2e}")
    assert run["surface_points"].shape == (6, 400, 4) and err < FLUX_FLOOR
    assert not run["group"].surface_points.requires_grad and not run["group"].surface_normals.requires_grad


def test_a_second_run_gives_the_same_bits(golden):
    """Three training samples are summed into every control net: in a fixed order, so a second run on a freshly loaded scenario
    gives the same control points after every step and the same history values."""
    d = golden(NAME)
    first, second = _whole_runs(d)
    assert torch.equal(first["final_loss"], second["final_loss"])
    a, b = first["histories"][0][0], second["histories"][0][0]
    for key in HISTORY_KEYS - {"test_loss"}:
        assert a[key] == b[key], key
    for key in ("pixel_loss", "kl_div"):
        assert torch.equal(a["test_loss"][key], b["test_loss"][key])
    for x, y in zip(first["after"], second["after"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(first["surface_points"], second["surface_points"])
    np.testing.assert_array_equal(first["surface_normals"], second["surface_normals"])


def test_one_epoch_runs_on_the_existing_entry_points(golden, monkeypatch):
    """One epoch - prepare, predict, loss, backward, lock, step - through the library handle: every kernel the epoch is made of
    is called, nothing of blocking or shading, and no backward pass through the kinematics."""
    from artist_amd import PixelLoss, _lib
    d = golden(NAME)
    reconstructor, scenario = _reconstructor(d)
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
    state.optimizer.zero_grad()
    loss = reconstructor.epoch_loss(state, reconstructor.predict_flux(state, DEV), PixelLoss(), DEV)
    loss.total.backward()
    reconstructor.update_multiplier(state, loss.violation)
    reconstructor._synchronize_and_lock_gradients(state.group.nurbs_control_points, DEV)
    state.optimizer.step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    called = set(calls)
    print("entry points of one epoch:", sorted(called))
    assert {"art_nurbs_fwd", "art_nurbs_bwd", "art_rigid_body_fwd", "art_trace_fwd", "art_trace_bwd", "art_flux_crop_fwd",
            "art_flux_crop_bwd", "art_flux_loss", "art_surface_regularizers_fwd", "art_surface_regularizers_bwd",
            "art_adam_step", "art_align_fwd", "art_align_bwd"} <= called, sorted(called)
    assert not [name for name in called if name.startswith(("art_blocking", "art_shading"))] and "art_rigid_body_bwd" not in called
    # one evaluation per epoch for all samples of a heliostat: the NURBS kernels run once each way, not once per sample
    assert calls.count("art_nurbs_fwd") == 1 and calls.count("art_nurbs_bwd") == 1 and calls.count("art_trace_fwd") == 1


def test_the_loop_stops_as_the_reference_does(golden):
    """The two ways out of the loop before ``max_epoch`` (surface_reconstructor.py:967-970, 1079-1097).  Early stopping with a
    window of two epochs, a patience of one and an improvement nobody reaches: the second epoch fills the window and stops,
    validates, and breaks BEFORE its history entry - one entry, while the final loss is the second epoch's.  A tolerance above the
    first epoch's loss: the loop's condition ends the run after that epoch, whose entry is there."""
    from artist_amd import PixelLoss
    d = golden(NAME)
    active = d["parser_mask"] > 0
    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"].update(early_stopping_window=2, early_stopping_patience=1, early_stopping_delta=10.0, max_epoch=5)
    reconstructor, _ = _reconstructor(d, configuration)
    validations = []
    validate = reconstructor.validate
    reconstructor.validate = lambda *a, **k: validations.append(1) or validate(*a, **k)
    final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=PixelLoss(), device=DEV)
    history = histories[0][0]
    assert all(len(history[key]) == 1 for key in HISTORY_KEYS - {"test_loss"}), history
    assert len(validations) == 2                                  # epoch 0 (0 % log_step) and the epoch that stopped
    np.testing.assert_allclose(history["total_loss"][0], d["history_total_loss"][0], rtol=CHAINED_LOSS_FLOOR)
    second = float(np.mean(n(final_loss)[active].astype(np.float64)))          # ... the final loss is the second epoch's
    np.testing.assert_allclose(second, d["history_total_loss"][1], rtol=2 * CHAINED_LOSS_FLOOR)

    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"].update(tolerance=1e9)
    reconstructor, _ = _reconstructor(d, configuration)
    final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=PixelLoss(), device=DEV)
    assert len(histories[0][0]["total_loss"]) == 1
    np.testing.assert_allclose(float(np.mean(n(final_loss)[active].astype(np.float64))), histories[0][0]["total_loss"][0], rtol=1e-6)


def test_kl_divergence_as_the_loss_definition(golden):
    """``KLDivergenceLoss`` as ``loss_definition`` for two epochs: a finite history that does not rise (the loss itself is
    pinned in tests/test_gpu_parity.py and test_gpu_flux_fuzz.py; there is no reference run of this leg)."""
    from artist_amd import KLDivergenceLoss
    d = golden(NAME)
    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"]["max_epoch"] = 1
    reconstructor, _ = _reconstructor(d, configuration)
    final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=KLDivergenceLoss(), device=DEV)
    history = histories[0][0]
    print("KL: total loss per epoch", history["total_loss"], " flux loss", history["flux_loss"])
    assert len(history["total_loss"]) == 2 and all(np.isfinite(v) for key in HISTORY_KEYS - {"test_loss"} for v in history[key])
    assert history["flux_loss"][1] <= history["flux_loss"][0] and history["total_loss"][1] <= history["total_loss"][0]
    assert np.isfinite(n(final_loss)[d["parser_mask"] > 0]).all() and np.isinf(n(final_loss)[d["parser_mask"] == 0]).all()
