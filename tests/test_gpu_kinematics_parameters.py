"""``KinematicsReconstructor(parameters=...)``: translation deviations and actuator parameters learn beside the rotation
deviations, pinned to the reference's own loop with more leaves (``-m gpu``).

``tests/golden/kinematics_parameters_flux.npz`` and ``..._alignment.npz`` (tests/golden/generate_kinematics_parameters_golden.py)
hold three epochs each of the reference's ``KinematicsReconstructor.reconstruct_kinematics`` on the case of
tests/test_gpu_kinematics_reconstructor.py - test_blocking.h5, mask 4 0 4 0 4 4, three training samples and one test sample per
active heliostat - with the extra tensors as leaves in parameter groups of their own: all three tensors flux-driven
(``FocalSpotLoss``), rotation deviations and actuator parameters alignment-driven (``AngleLoss``); learning rates 2e-4, 1e-4 and
5e-5; once in fp32 and once in fp64 on the same rays.  The helpers, the scenario and the recorded distortions are those of
tests/test_gpu_kinematics_reconstructor.py.

Bounds.  Each epoch: ``err < 3 x yardstick``, the yardstick being the reference's own fp32-vs-fp64 distance of that quantity as
stored in the fixture - at the first epoch for the prediction, the loss per sample and every tensor's gradient; for a tensor's
value after the step at the same epoch of the fp64 run (the first step of Adam moves every coordinate by its learning rate
whatever the gradient's size, so the first epoch's distance, fp32 rounding, says nothing about the later epochs).  Flux-driven,
the floors of tests/test_gpu_kinematics_reconstructor.py for what is traced: 2e-5 relative L2 for flux, 2e-5 m for the loss, 5e-4
for a gradient.  Tensors are compared by relative L2, losses by their largest absolute distance.  The whole run: the
tensors after every step in units of their learning rate, the bound of
tests/test_gpu_kinematics_reconstructor.py::test_the_whole_run_through_reconstruct_kinematics (0.05 lr where the gradient is
sizeable: Adam's first steps move a coordinate by about +-lr whatever its gradient's size, so a coordinate whose gradient is
almost zero may step the other way - 2 (e + 1) + 0.1 lr anywhere).  "The same bits" is ``torch.equal``.

Measured on MI355X: see DESIGN.md 4.13, "More kinematic parameters".
"""
import json

import numpy as np
import pytest
import torch

import test_gpu_kinematics_reconstructor as suite
from conftest import rel_l2
from test_gpu_kinematics_reconstructor import FLUX_FLOOR, GRAD_FLOOR, LOSS_FLOOR, VALIDATION_KEYS, abs_max, n, t

pytestmark = pytest.mark.gpu

FIXTURES = {"raytracing": "kinematics_parameters_flux", "alignment": "kinematics_parameters_alignment"}
METHODS = sorted(FIXTURES)
NAMES = ("rotation_deviations", "translation_deviations", "actuator_parameters")
LEARNED = {"raytracing": NAMES, "alignment": ("rotation_deviations", "actuator_parameters")}
DEV = suite.DEV
ABSENT = object()


def _tensor(kinematics, name):
    if name == "actuator_parameters":
        return kinematics.actuators.optimizable_parameters
    return kinematics.rotation_deviation_parameters if name == "rotation_deviations" else kinematics.translation_deviation_parameters


def _reconstructor(method, d, parameters=ABSENT, epoch_graph=False):
    """The scenario of tests/test_gpu_kinematics_reconstructor.py at the fixture's start - the two extra tensors at their
    perturbed values, whether they learn or not - and the reconstructor on it, with ``parameters`` when given."""
    from artist_amd.optim import KinematicsReconstructor
    first, scenario = suite._reconstructor(method, d)
    kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
    for name in NAMES[1:]:
        np.testing.assert_allclose(n(_tensor(kinematics, name)), d[f"true_{name}"], rtol=1e-6, atol=1e-9)
    kinematics.translation_deviation_parameters = t(d["initial_translation_deviations"])
    kinematics.actuators.optimizable_parameters = t(d["initial_actuator_parameters"])
    keyword = {} if parameters is ABSENT else dict(parameters=parameters)
    reconstructor = KinematicsReconstructor(
        ddp_setup=suite.DDP, scenario=scenario, data=first.data, optimization_configuration=json.loads(str(d["configuration"])),
        reconstruction_method=method, bitmap_resolution=first.bitmap_resolution, device=DEV, epoch_graph=epoch_graph, **keyword)
    return reconstructor, scenario


def _bounds(method, d):
    """name -> (yardstick, bound) of what is compared at every epoch against the first epoch's fp32-vs-fp64 distance."""
    flux_driven = method == "raytracing"
    prediction = "flux_predicted" if flux_driven else "normals_predicted"
    yard = dict(prediction=rel_l2(d[prediction][0], d[f"{prediction}_f64_epoch0"]),
                loss=abs_max(d["loss_per_sample"][0], d["loss_per_sample_f64_epoch0"]))
    floor = dict(prediction=FLUX_FLOOR, loss=LOSS_FLOOR) if flux_driven else {}
    for name in LEARNED[method]:
        yard[f"grad_{name}"] = rel_l2(d[f"grad_{name}"][0], d[f"grad_{name}_f64_epoch0"])
        if flux_driven:
            floor[f"grad_{name}"] = GRAD_FLOOR
    return {key: (value, max(3 * value, floor.get(key, 0.0))) for key, value in yard.items()}


def _step(reconstructor, state, loss_definition):
    """What the loop does between its scheduler steps: one epoch's loss, backward, the alignment mode's clean-up, the step."""
    state.optimizer.zero_grad()
    loss = reconstructor.epoch_loss(state, loss_definition, DEV)
    loss.total.backward()
    if reconstructor.reconstruction_method == "alignment":
        for tensor in state.learnables.values():
            tensor.grad.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)
    grads = {name: tensor.grad.clone() for name, tensor in state.learnables.items()}
    state.optimizer.step()
    return loss, grads


@pytest.mark.parametrize("method", METHODS)
def test_each_epoch_reproduces_the_reference_loop_with_more_leaves(golden, method):
    """From the reference's tensors at the start of each epoch: the prediction, the loss per sample, every learned tensor's
    gradient - three samples summed into each row, exactly nothing for the heliostats without samples, no column of an active
    heliostat without one - and its value after the step of a parameter group of its own."""
    d = golden(FIXTURES[method])
    learned = LEARNED[method]
    assert tuple(d["learned"].tolist()) == learned
    bounds = _bounds(method, d)
    reconstructor, scenario = _reconstructor(method, d, parameters=learned[::-1])          # (any order)
    assert reconstructor.parameters == learned
    loss_definition = suite._loss_definition(method, scenario)
    prediction_key = "flux_predicted" if method == "raytracing" else "normals_predicted"
    kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
    state = reconstructor.prepare(0, DEV)
    assert list(state.learnables) == list(learned) and len(state.optimizer.param_groups) == len(learned)
    for name, group in zip(learned, state.optimizer.param_groups):
        assert group["params"][0] is _tensor(kinematics, name) is state.learnables[name] and group["params"][0].requires_grad
    active, inactive = np.nonzero(d["parser_mask"])[0], np.nonzero(d["parser_mask"] == 0)[0]
    missed = []
    for e in range(3):
        with torch.no_grad():
            for name in learned:
                state.learnables[name].copy_(t(d[f"start_{name}"][e]))
        rates = [group["lr"] for group in state.optimizer.param_groups]
        np.testing.assert_allclose(rates, d["lr"][e], rtol=1e-12)
        loss, grads = _step(reconstructor, state, loss_definition)
        state.scheduler.step()
        err = dict(prediction=rel_l2(n(loss.prediction), d[prediction_key][e]), loss=abs_max(n(loss.per_sample), d["loss_per_sample"][e]),
                   loss_per_heliostat=abs_max(n(loss.per_heliostat), d["loss_per_heliostat"][e]),
                   total=abs_max(float(loss.total.detach()), d["total_loss"][e]))
        checks = {key: (value,) + bounds.get(key, bounds["loss"]) for key, value in err.items()}
        for name in learned:
            grad = n(grads[name])
            assert grad.shape == d[f"grad_{name}"][e].shape and np.isfinite(grad).all()
            assert not grad[inactive].any() and grad[active].all(), name
            checks[f"grad_{name}"] = (rel_l2(grad, d[f"grad_{name}"][e]),) + bounds[f"grad_{name}"]
            yard = rel_l2(d[f"after_{name}"][e], d[f"after_{name}_f64"][e])
            after = n(state.learnables[name])
            np.testing.assert_array_equal(after[inactive], d[f"start_{name}"][e][inactive])       # no sample, no step
            checks[f"after_{name}"] = (rel_l2(after, d[f"after_{name}"][e]), yard, 3 * yard)
        print(f"{method} epoch {e} (error, yardstick, bound): " + ", ".join(f"{key} {v[0]:.2e} {v[1]:.2e} {v[2]:.2e}" for key, v in checks.items()))
        missed += [(e, key) + v for key, v in checks.items() if not v[0] < v[2]]
    assert not missed, missed


_RUNS = {}


def _whole_run(method, d, label, parameters=ABSENT, epoch_graph=False):
    """``reconstruct_kinematics`` on a freshly loaded scenario (kept per ``label``, shared by the tests below): what it returned,
    per step the learning rates, the gradients handed to the step and the tensors after it."""
    if (method, label) not in _RUNS:
        reconstructor, scenario = _reconstructor(method, d, parameters=parameters, epoch_graph=epoch_graph)
        kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
        before = {name: _tensor(kinematics, name) for name in NAMES}
        versions = {name: tensor._version for name, tensor in before.items()}
        steps, validations = [], []
        prepare, validate = reconstructor.prepare, reconstructor.validate

        def prepare_recording(*a, **k):
            state = prepare(*a, **k)
            step = state.optimizer.step

            def step_recording(*sa, **sk):
                entry = dict(lr=[group["lr"] for group in state.optimizer.param_groups],
                             grads={name: tensor.grad.clone() for name, tensor in state.learnables.items()})
                out = step(*sa, **sk)
                entry["after"] = {name: tensor.detach().clone() for name, tensor in state.learnables.items()}
                steps.append(entry)
                return out

            state.optimizer.step = step_recording
            return state

        def validate_recording(*a, **k):
            out = validate(*a, **k)
            validations.append({key: value.clone() for key, value in out.items()})
            return out

        reconstructor.prepare, reconstructor.validate = prepare_recording, validate_recording
        final_loss, histories = reconstructor.reconstruct_kinematics(loss_definition=suite._loss_definition(method, scenario), device=DEV)
        _RUNS[(method, label)] = dict(final_loss=final_loss, history=histories[0][0], steps=steps, validations=validations,
                                      kinematics=kinematics, before=before, versions=versions, reconstructor=reconstructor)
    return _RUNS[(method, label)]


def _assert_same_run(a, b, names):
    assert torch.equal(a["final_loss"], b["final_loss"])
    assert a["history"]["total_loss"] == b["history"]["total_loss"] and len(a["steps"]) == len(b["steps"]) == 3
    for key in VALIDATION_KEYS:
        assert torch.equal(a["history"]["test_loss"][key], b["history"]["test_loss"][key])
    assert len(a["validations"]) == len(b["validations"])
    for x, y in zip(a["validations"], b["validations"]):
        assert all(torch.equal(x[key], y[key]) for key in VALIDATION_KEYS)
    for e, (x, y) in enumerate(zip(a["steps"], b["steps"])):
        assert x["lr"] == y["lr"] and list(x["grads"]) == list(y["grads"]) == list(names), e
        for name in names:
            assert torch.equal(x["grads"][name], y["grads"][name]), (e, name)
            assert torch.equal(x["after"][name], y["after"][name]), (e, name)
    for name in NAMES:
        assert torch.equal(_tensor(a["kinematics"], name), _tensor(b["kinematics"], name)), name


@pytest.mark.parametrize("method", METHODS)
def test_the_whole_run_through_reconstruct_kinematics(golden, method):
    """``reconstruct_kinematics()`` for three epochs: the history, every group's learning rate per epoch, the tensors after every
    step and at the end in units of their learning rate, the final loss with its ``inf`` rows; all learned tensors detached."""
    d = golden(FIXTURES[method])
    learned = LEARNED[method]
    loss_bound = _bounds(method, d)["loss"][1]
    run = _whole_run(method, d, "first", parameters=learned)
    history, final_loss = run["history"], n(run["final_loss"])
    active, inactive = np.nonzero(d["parser_mask"])[0], np.nonzero(d["parser_mask"] == 0)[0]
    assert set(history) == {"total_loss", "test_loss"} and len(history["total_loss"]) == 3 and len(run["steps"]) == 3
    missed = []
    for e in range(3):
        err = abs(history["total_loss"][e] - d["history_total_loss"][e])
        print(f"{method} epoch {e}: total loss {history['total_loss'][e]:.7f}, reference {d['history_total_loss'][e]:.7f}, differs by "
              f"{err:.2e} (bound {loss_bound:.2e})")
        if not err < loss_bound:
            missed.append((e, "history", err, loss_bound))
        # every group at its own rate
        np.testing.assert_allclose(run["steps"][e]["lr"], d["lr"][e], rtol=1e-12)
        for g, name in enumerate(learned):
            moved = (n(run["steps"][e]["after"][name]) - d[f"after_{name}"][e]) / d["lr"][e][g]
            big = np.abs(d[f"grad_{name}"][e]) > 1e-3 * np.abs(d[f"grad_{name}"][e]).max()
            print(f"{method} epoch {e}: {name} differs from the reference's by at most {np.abs(moved[big]).max():.4f} lr where the "
                  f"gradient is sizeable ({int(big.sum())} of {int((d[f'grad_{name}'][e] != 0).sum())}), {np.abs(moved).max():.4f} lr anywhere")
            assert np.abs(moved[big]).max() < 0.05 and np.abs(moved).max() < 2.0 * (e + 1) + 0.1, (e, name)
            np.testing.assert_array_equal(n(run["steps"][e]["after"][name])[inactive], d[f"start_{name}"][0][inactive])
    assert len(set(d["lr"][0].tolist())) == len(learned)                          # (a rate of its own each)
    for name in NAMES:
        tensor = _tensor(run["kinematics"], name)
        assert not tensor.requires_grad and tensor.grad_fn is None, name                        # detached at the end
        if name in learned:
            assert torch.equal(tensor, run["steps"][-1]["after"][name])
            assert not np.array_equal(n(tensor)[active], d[f"start_{name}"][0][active])
        else:
            assert tensor is run["before"][name] and tensor._version == run["versions"][name]
    assert final_loss.shape == (6,) and np.isinf(final_loss[inactive]).all() and (final_loss[inactive] > 0).all()
    assert float(np.mean(final_loss[active].astype(np.float64))) == pytest.approx(history["total_loss"][-1], rel=1e-6)
    err = abs_max(final_loss[active], d["final_loss"][active])
    print(f"{method}: final loss differs by {err:.2e}")
    if not err < loss_bound:
        missed.append(("final", "loss", err, loss_bound))
    assert not missed, missed


@pytest.mark.parametrize("method", METHODS)
def test_a_second_run_gives_the_same_bits(golden, method):
    """The sum over a heliostat's samples has a fixed order for every learned tensor: a second run on a freshly loaded scenario
    gives the same gradients, the same tensors after every step and at the end, the same history and validations."""
    d = golden(FIXTURES[method])
    learned = LEARNED[method]
    first = _whole_run(method, d, "first", parameters=learned)
    second = _whole_run(method, d, "second", parameters=list(learned))
    assert first["kinematics"] is not second["kinematics"]
    _assert_same_run(first, second, learned)
    assert all(step["grads"][name].abs().sum() > 0 for step in first["steps"] for name in learned)


@pytest.mark.parametrize("method", METHODS)
def test_the_default_is_unchanged(golden, method):
    """Without the keyword and with ``parameters=("rotation_deviations",)``: the same bits, one parameter group; the other two
    tensors do not become leaves and their storage is not written."""
    d = golden(FIXTURES[method])
    absent = _whole_run(method, d, "absent")
    named = _whole_run(method, d, "rotation alone", parameters=("rotation_deviations",))
    assert absent["reconstructor"].parameters == named["reconstructor"].parameters == ("rotation_deviations",)
    _assert_same_run(absent, named, NAMES[:1])
    rate = json.loads(str(d["configuration"]))["optimization"]["initial_learning_rate_rotation_deviation"]
    for run in (absent, named):
        assert [len(step["lr"]) for step in run["steps"]] == [1, 1, 1] and run["steps"][0]["lr"] == [rate]
        for name in NAMES[1:]:
            tensor = _tensor(run["kinematics"], name)
            assert tensor is run["before"][name] and tensor._version == run["versions"][name], name
            assert not tensor.requires_grad and tensor.grad is None and tensor.grad_fn is None, name
            np.testing.assert_array_equal(n(tensor), d[f"initial_{name}"])
    # ... and it is not the run that learns them all
    assert absent["history"]["total_loss"] != _whole_run(method, d, "first", parameters=LEARNED[method])["history"]["total_loss"]


@pytest.mark.parametrize("method", METHODS)
def test_the_replayed_run_gives_the_eager_bits(golden, method):
    """``epoch_graph=True`` with every learned tensor: the captured step leaves a gradient on each of them; history, validations,
    every gradient, every tensor after every step and at the end are the eager run's bits.  The graph is closed afterwards and
    no autograd graph is left on the kinematics' per-sample tables."""
    d = golden(FIXTURES[method])
    learned = LEARNED[method]
    eager = _whole_run(method, d, "first", parameters=learned)
    replayed = _whole_run(method, d, "replayed", parameters=learned, epoch_graph=True)
    assert replayed["reconstructor"].epoch_graph and not eager["reconstructor"].epoch_graph
    _assert_same_run(eager, replayed, learned)
    kinematics = replayed["kinematics"]
    for active in (kinematics.active_rotation_deviation_parameters, kinematics.active_translation_deviation_parameters,
                   kinematics.actuators.active_optimizable_parameters):
        assert active.grad_fn is None
    from artist_amd import ops
    ops.check_async_errors(DEV)


@pytest.mark.parametrize("method", METHODS)
def test_more_leaves_call_the_same_entry_points(golden, monkeypatch, method):
    """One epoch - prepare, loss, backward, step - that learns every tensor calls the set of library entry points of one that
    learns the rotation deviations alone: ``art_rigid_body_bwd`` writes all three gradients in its one launch.  The kinematics
    kernel runs once each way; the step is one ``art_adam_step`` per learned tensor."""
    from artist_amd import _lib
    d = golden(FIXTURES[method])
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
    per_choice = {}
    for parameters in (NAMES[:1], LEARNED[method]):
        reconstructor, scenario = _reconstructor(method, d, parameters=parameters)
        del calls[:]
        state = reconstructor.prepare(0, DEV)
        _step(reconstructor, state, suite._loss_definition(method, scenario))
        torch.cuda.synchronize()
        per_choice[parameters] = list(calls)
    monkeypatch.undo()
    alone, more = per_choice[NAMES[:1]], per_choice[LEARNED[method]]
    print(f"{method}: entry points of one epoch: {sorted(set(more))}; art_adam_step x {more.count('art_adam_step')}")
    assert set(alone) == set(more) and {"art_rigid_body_fwd", "art_rigid_body_bwd", "art_adam_step"} <= set(more)
    for one in (alone, more):
        assert one.count("art_rigid_body_fwd") == 1 and one.count("art_rigid_body_bwd") == 1
    assert alone.count("art_adam_step") == 1 and more.count("art_adam_step") == len(LEARNED[method])
    strip = lambda names: sorted(name for name in names if name != "art_adam_step")  # noqa: E731
    assert strip(alone) == strip(more)                                         # nothing else is launched, not once more


@pytest.mark.parametrize("method", METHODS)
def test_an_epoch_does_not_wait_for_the_device(golden, method):
    """After a warm-up epoch, ``epoch_loss`` + ``backward`` + ``step`` with every tensor learning read nothing from the device:
    the loop's one read per epoch is the loss, after the step has been queued."""
    d = golden(FIXTURES[method])
    reconstructor, scenario = _reconstructor(method, d, parameters=LEARNED[method])
    loss_definition = suite._loss_definition(method, scenario)
    state = reconstructor.prepare(0, DEV)
    first, _ = _step(reconstructor, state, loss_definition)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second, _ = _step(reconstructor, state, loss_definition)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(second.total.detach()) < float(first.total.detach())                # ... and it was an epoch: the loss went down
