"""``epoch_graph=True``: the reconstructors' epochs replayed from an ``EpochGraph`` give the bits of the eager loop (``-m gpu``).

``SurfaceReconstructor`` and ``KinematicsReconstructor`` (both methods) capture a group's training step once and replay it every
epoch; what follows the step - multiplier, lock, ``nan_to_num_``, ``Adam.step()``, the one host read, scheduler, early stopping,
history, validation - stays eager.  "The same" is ``==`` on float lists and ``torch.equal`` on tensors: every quantity compared here
is bit-reproducible between two eager runs (``test_a_second_run_gives_the_same_bits`` in tests/test_gpu_surface_reconstructor.py and
tests/test_gpu_kinematics_reconstructor.py), so a replay has nothing to differ by and there is no tolerance.  What a wrong replay
looks like: a multiplier that was rebound (the captured constraint keeps epoch 0's), an activation whose memory a validation was
handed (wrong from the first epoch after a validation), a second run that meets the first run's autograd graph.

Fixtures, sizes and ``_reconstructor`` are those of the two eager suites: six heliostats of test_blocking.h5, 10 x 10 points per
facet, 3 rays, 64 x 64.
"""
import json

import numpy as np
import pytest
import torch

import test_gpu_kinematics_reconstructor as kinematics_suite
import test_gpu_surface_reconstructor as surface_suite

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
METHODS = kinematics_suite.METHODS
VARIANTS = ("surfaces", *METHODS)
SURFACE_KEYS = sorted(surface_suite.HISTORY_KEYS - {"test_loss"})
NOT_LAUNCHES = ("art_abi_version", "art_last_hip_error", "art_strerror", "art_async_status", "art_blocking_workspace_bytes",
                "art_trace_bwd_scratch_floats", "art_trace_bwd_scratch_need")


@pytest.fixture(autouse=True)
def nothing_left_on_the_device():
    yield
    from artist_amd import ops
    torch.cuda.set_sync_debug_mode("default")
    ops.check_async_errors(DEV)


def _configuration(d, **optimization):
    configuration = json.loads(str(d["configuration"]))
    configuration["optimization"].update(optimization)
    return configuration


def _make(variant, golden, epoch_graph, **optimization):
    """``(reconstructor, scenario, group, loss_definition, the learnt parameter's getter, d)`` on a freshly loaded scenario;
    ``epoch_graph`` is set on the existing object, as a caller who got the object from elsewhere would."""
    if variant == "surfaces":
        from artist_amd import PixelLoss
        d = golden(surface_suite.NAME)
        reconstructor, scenario = surface_suite._reconstructor(d, _configuration(d, **optimization))
        loss_definition = PixelLoss()
        group = scenario.heliostat_field.heliostat_groups[0]
        parameter = lambda: group.nurbs_control_points                                   # noqa: E731
    else:
        d = golden(kinematics_suite.NAMES[variant])
        reconstructor, scenario = kinematics_suite._reconstructor(variant, d, _configuration(d, **optimization))
        loss_definition = kinematics_suite._loss_definition(variant, scenario)
        group = scenario.heliostat_field.heliostat_groups[0]
        parameter = lambda: group.kinematics.rotation_deviation_parameters             # noqa: E731
    reconstructor.epoch_graph = epoch_graph
    return reconstructor, scenario, group, loss_definition, parameter, d


def _run(variant, made):
    """One ``reconstruct_*()`` with everything a wrong replay would show in: what it returned, the parameter (and the surfaces'
    multiplier) after every step, every validation."""
    reconstructor, scenario, group, loss_definition, parameter, d = made
    after, multipliers, validations = [], [], []
    start = parameter().detach().clone()
    cls = type(reconstructor)

    def prepare(*a, **k):
        state = cls.prepare(reconstructor, *a, **k)
        step = state.optimizer.step

        def step_recording(*sa, **sk):
            out = step(*sa, **sk)
            after.append(parameter().detach().clone())
            if variant == "surfaces":
                multipliers.append(state.multiplier.detach().clone())
            return out

        state.optimizer.step = step_recording
        return state

    def validate(*a, **k):
        out = cls.validate(reconstructor, *a, **k)
        validations.append((len(after) - 1, {key: value.detach().clone() for key, value in out.items()}))
        return out

    reconstructor.prepare, reconstructor.validate = prepare, validate
    reconstruct = reconstructor.reconstruct_surfaces if variant == "surfaces" else reconstructor.reconstruct_kinematics
    final_loss, histories = reconstruct(loss_definition=loss_definition, device=DEV)
    torch.cuda.synchronize()
    assert len(histories) == 1 and len(histories[0]) == 1
    run = dict(final_loss=final_loss, history=histories[0][0], start=start, after=after, multipliers=multipliers, validations=validations,
               end=parameter().detach().clone())
    if variant == "surfaces":
        run.update(surface_points=group.surface_points.clone(), surface_normals=group.surface_normals.clone())
    return run


def _assert_same_run(variant, eager, replayed):
    a, b = eager["history"], replayed["history"]
    assert set(a) == set(b)
    for key in (SURFACE_KEYS if variant == "surfaces" else ["total_loss"]):
        assert a[key] == b[key], (key, a[key], b[key])
    assert set(a["test_loss"]) == set(b["test_loss"])
    for key in a["test_loss"]:
        assert torch.equal(a["test_loss"][key], b["test_loss"][key]), key
    assert torch.equal(eager["final_loss"], replayed["final_loss"]), (eager["final_loss"], replayed["final_loss"])
    assert len(eager["after"]) == len(replayed["after"]) and len(eager["validations"]) == len(replayed["validations"])
    for e, (x, y) in enumerate(zip(eager["after"], replayed["after"])):
        assert torch.equal(x, y), f"the parameter after the step of epoch {e} differs"
    for e, (x, y) in enumerate(zip(eager["multipliers"], replayed["multipliers"])):
        assert torch.equal(x, y), f"the multiplier after epoch {e} differs"
    for (ea, va), (eb, vb) in zip(eager["validations"], replayed["validations"]):
        assert ea == eb and all(torch.equal(va[key], vb[key]) for key in va), f"the validation after epoch {ea} differs"
    assert torch.equal(eager["end"], replayed["end"])
    for key in ("surface_points", "surface_normals"):
        if key in eager:
            assert torch.equal(eager[key], replayed[key]), key


_SURFACES = {}


def _surface_runs(golden):
    """The surfaces' whole run (``max_epoch=5``, ``log_step=2``: six epochs, validations after epochs 0, 2 and 4), eager and
    replayed, each on a fresh scenario; the objects are kept for their second runs."""
    if not _SURFACES:
        for epoch_graph in (False, True):
            made = _make("surfaces", golden, epoch_graph, max_epoch=5, log_step=2)
            _SURFACES[epoch_graph] = dict(made=made, first=_run("surfaces", made))
    return _SURFACES[False], _SURFACES[True]


def test_surfaces_whole_run_replayed_gives_the_eager_bits(golden):
    """Six epochs with the fixture's ``energy_tolerance=-0.01`` (the multiplier changes every epoch) and exponential scheduler (lr
    changes every epoch), training epochs after validations: every history list, the last validation, the final loss per
    heliostat, the control points after every step and at the end, the multiplier after every epoch, every validation, the
    surface points and normals after ``update_surfaces``."""
    eager, replayed = (entry["first"] for entry in _surface_runs(golden))
    history = eager["history"]
    assert all(len(history[key]) == 6 for key in SURFACE_KEYS) and [e for e, _ in eager["validations"]] == [0, 2, 4]
    _assert_same_run("surfaces", eager, replayed)
    # not vacuous: the multiplier is there and changes from epoch to epoch, the constraint acts, the control points moved
    multipliers = eager["multipliers"]
    assert len(multipliers) == 6 and all(float(m.min()) > 0 for m in multipliers)
    assert all(not torch.equal(multipliers[e], multipliers[e + 1]) for e in range(5))
    assert all(value > 0 for value in history["flux_integral_constraint"]) and len(set(history["total_loss"])) == 6
    assert all(not torch.equal(eager["after"][e], eager["after"][e + 1]) for e in range(5)) and not torch.equal(eager["start"], eager["end"])


@pytest.mark.parametrize("method", METHODS)
def test_kinematics_whole_run_replayed_gives_the_eager_bits(golden, method):
    """Five epochs (``max_epoch=4``), a validation after every one (the fixture's ``log_step=1``): the history, every
    validation's three losses, the final loss, the rotation deviations after every step and at the end; the rows of the
    heliostats without samples stay as they were."""
    eager = _run(method, _make(method, golden, False, max_epoch=4))
    replayed = _run(method, _make(method, golden, True, max_epoch=4))
    assert len(eager["history"]["total_loss"]) == 5 and [e for e, _ in eager["validations"]] == [0, 1, 2, 3, 4]
    assert set(eager["history"]["test_loss"]) == set(kinematics_suite.VALIDATION_KEYS)
    _assert_same_run(method, eager, replayed)
    mask = torch.as_tensor(golden(kinematics_suite.NAMES[method])["parser_mask"])
    for run in (eager, replayed):
        start, end = run["start"].cpu(), run["end"].cpu()
        assert torch.equal(end[mask == 0], start[mask == 0]) and (end[mask > 0] != start[mask > 0]).any(dim=1).all()
        assert torch.isinf(run["final_loss"][mask == 0]).all() and torch.isfinite(run["final_loss"][mask > 0]).all()
    assert len(set(eager["history"]["total_loss"])) == 5


@pytest.mark.parametrize("variant", VARIANTS)
def test_an_epoch_after_the_build_is_a_replay(golden, monkeypatch, variant):
    """``max_epoch=5``, ``log_step=3``: validations after epochs 0, 3 and 4.  From ``zero_grad`` to the end of ``optimizer.step()``
    every epoch - the first, the one after a validation, the ones between two validations - calls the library exactly once,
    ``art_adam_step``, activates nothing and runs under ``set_sync_debug_mode("error")``: the step is a replay, its eager tail
    reads nothing.  The captured step itself went through the handle three times (two warm-up runs and the capture) before the
    first epoch."""
    from artist_amd import _lib, graphs
    made = _make(variant, golden, True, max_epoch=5, log_step=3)
    reconstructor, group = made[0], made[2]
    handle = _lib.lib()
    calls, activations, built, epochs, validated = [], [], [], [], []
    for name in _lib.SIGNATURES:
        if name in NOT_LAUNCHES:
            continue
        real = getattr(handle, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append(_name)
            return _real(*args)

        monkeypatch.setattr(handle, name, wrapped)
    activate = group.activate_heliostats
    monkeypatch.setattr(group, "activate_heliostats", lambda *a, **k: activations.append(len(epochs)) or activate(*a, **k))
    epoch_graph = graphs.EpochGraph
    monkeypatch.setattr(graphs, "EpochGraph", lambda *a, **k: built.append(epoch_graph(*a, **k)) or built[-1])
    cls = type(reconstructor)

    def prepare(*a, **k):
        state = cls.prepare(reconstructor, *a, **k)
        zero_grad, step = state.optimizer.zero_grad, state.optimizer.step

        def zero_grad_marking(*za, **zk):
            epochs.append(dict(first_call=len(calls), activations=len(activations)))
            torch.cuda.set_sync_debug_mode("error")
            return zero_grad(*za, **zk)

        def step_marking(*sa, **sk):
            try:
                return step(*sa, **sk)
            finally:
                torch.cuda.set_sync_debug_mode("default")
                epochs[-1].update(calls=calls[epochs[-1]["first_call"]:], activated=len(activations) - epochs[-1]["activations"])

        state.optimizer.zero_grad, state.optimizer.step = zero_grad_marking, step_marking
        return state

    def validate(*a, **k):
        validated.append(len(epochs) - 1)
        return cls.validate(reconstructor, *a, **k)

    reconstructor.prepare, reconstructor.validate = prepare, validate
    reconstruct = reconstructor.reconstruct_surfaces if variant == "surfaces" else reconstructor.reconstruct_kinematics
    try:
        final_loss, histories = reconstruct(loss_definition=made[3], device=DEV)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert len(built) == 1 and len(epochs) == 6 and validated == [0, 3, 4] and len(histories[0][0]["total_loss"]) == 6
    before = calls[:epochs[0]["first_call"]]
    print(f"{variant}: library calls of the build: {sorted(set(before))}; per epoch: {[e['calls'] for e in epochs]}; activations in "
          f"epoch {activations}")
    assert before.count("art_rigid_body_fwd") == 3 and "art_adam_step" not in before
    if variant != "alignment":
        assert before.count("art_trace_fwd") == 3 and before.count("art_trace_bwd") == 3
    for e, epoch in enumerate(epochs):
        assert epoch["calls"] == ["art_adam_step"], (e, epoch["calls"])
        assert epoch["activated"] == 0, f"epoch {e} activated the group"
    # the training activation once, in the build; the test samples' once, in the first validation
    assert activations == [0, 1], activations
    assert torch.isfinite(final_loss[torch.as_tensor(made[5]["parser_mask"]) > 0]).all()


@pytest.mark.parametrize("variant", ("surfaces", "raytracing"))
def test_the_loop_stops_as_the_eager_loop_does(golden, variant):
    """The early-stopping and the tolerance case of ``test_the_loop_stops_as_the_reference_does`` with ``epoch_graph=True``: the
    history lengths, the number of validations and the final loss - the second epoch's after early stopping, which breaks
    before that epoch's history entry - of the eager run of the same configuration."""
    stopping = dict(early_stopping_window=2, early_stopping_patience=1, early_stopping_delta=10.0, max_epoch=5)
    tolerance = dict(tolerance=1e9) if variant == "surfaces" else dict(tolerance=1e9, log_step=0)
    for optimization, entries, validations in ((stopping, 1, 2), (tolerance, 1, 1)):
        eager = _run(variant, _make(variant, golden, False, **optimization))
        replayed = _run(variant, _make(variant, golden, True, **optimization))
        assert len(eager["history"]["total_loss"]) == entries and len(eager["validations"]) == validations, optimization
        assert len(eager["after"]) == validations                       # (early stopping: two steps, one history entry)
        _assert_same_run(variant, eager, replayed)


@pytest.mark.parametrize("variant", VARIANTS)
def test_no_graph_is_open_after_the_run(golden, monkeypatch, variant):
    from artist_amd import ArtistHipError, graphs
    built = []
    epoch_graph = graphs.EpochGraph
    monkeypatch.setattr(graphs, "EpochGraph", lambda *a, **k: built.append(epoch_graph(*a, **k)) or built[-1])
    made = _make(variant, golden, True, max_epoch=1)
    run = _run(variant, made)
    assert len(built) == 1 and len(run["after"]) == 2
    for graph in built:
        with pytest.raises(ArtistHipError, match="closed"):
            graph.replay()
    group = made[2]
    assert group.active_surface_points.grad_fn is None and group.active_surface_normals.grad_fn is None


def test_a_second_run_on_the_same_object_replays_too(golden):
    """``reconstruct_surfaces`` again on the same object and scenario (a new optimiser, multiplier and graph from the control
    points the first run left): the bits of the second of two eager runs on another object."""
    eager, replayed = _surface_runs(golden)
    for entry in (eager, replayed):
        if "second" not in entry:
            entry["second"] = _run("surfaces", entry["made"])
    assert torch.equal(eager["second"]["start"], eager["first"]["end"])
    _assert_same_run("surfaces", eager["second"], replayed["second"])
    assert eager["second"]["history"]["total_loss"] != eager["first"]["history"]["total_loss"]


def test_the_keyword_and_the_eager_pieces_on_such_an_object(golden):
    """Both constructors take ``epoch_graph=True`` (a ``TypeError`` before), keep it as an attribute, and leave ``prepare`` /
    ``predict_flux`` / ``epoch_loss`` / ``validate`` usable eagerly for callers that step themselves: the bits of an object made
    without the keyword."""
    from artist_amd import PixelLoss
    from artist_amd.optim import KinematicsReconstructor, SurfaceReconstructor
    results = {}
    for epoch_graph in (False, True):
        reconstructor, scenario = surface_suite._reconstructor(golden(surface_suite.NAME))
        kwargs = dict(ddp_setup=reconstructor.ddp_setup, scenario=scenario, data=reconstructor.data,
                      optimization_configuration=_configuration(golden(surface_suite.NAME)),
                      number_of_surface_points=reconstructor.number_of_surface_points, bitmap_resolution=reconstructor.bitmap_resolution,
                      epsilon=reconstructor.epsilon, device=DEV)
        reconstructor = SurfaceReconstructor(**kwargs, epoch_graph=True) if epoch_graph else SurfaceReconstructor(**kwargs)
        assert reconstructor.epoch_graph is epoch_graph
        state = reconstructor.prepare(0, DEV)
        loss = reconstructor.epoch_loss(state, reconstructor.predict_flux(state, DEV), PixelLoss(), DEV)
        loss.total.backward()
        reconstructor.update_multiplier(state, loss.violation)
        test_loss = reconstructor.validate(state, DEV)
        assert state.graph is None and not state.static
        results["surfaces", epoch_graph] = [loss.total.detach(), state.group.nurbs_control_points.grad, state.multiplier,
                                            test_loss["pixel_loss"], test_loss["kl_div"]]
        for method in METHODS:
            d = golden(kinematics_suite.NAMES[method])
            reconstructor, scenario = kinematics_suite._reconstructor(method, d)
            kwargs = dict(ddp_setup=reconstructor.ddp_setup, scenario=scenario, data=reconstructor.data,
                          optimization_configuration=_configuration(d), reconstruction_method=method,
                          bitmap_resolution=reconstructor.bitmap_resolution, device=DEV)
            reconstructor = KinematicsReconstructor(**kwargs, epoch_graph=True) if epoch_graph else KinematicsReconstructor(**kwargs)
            assert reconstructor.epoch_graph is epoch_graph
            state = reconstructor.prepare(0, DEV)
            loss = kinematics_suite._step(reconstructor, state, kinematics_suite._loss_definition(method, scenario))
            test_loss = reconstructor.validate(state, DEV)
            assert state.graph is None
            results[method, epoch_graph] = [loss.total.detach(), scenario.heliostat_field.heliostat_groups[0].kinematics.rotation_deviation_parameters.detach(),
                                            *(test_loss[key] for key in kinematics_suite.VALIDATION_KEYS)]
    for variant in VARIANTS:
        for x, y in zip(results[variant, False], results[variant, True]):
            assert torch.isfinite(x).all() or variant == "alignment"
            assert torch.equal(x, y), variant
        assert np.isfinite(float(results[variant, True][0])) and float(results[variant, True][0]) > 0
