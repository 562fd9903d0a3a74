"""``SurfaceReconstructor(parameters=...)``: facet canting and facet translations learn beside the control points (``-m gpu``).

``tests/golden/canting_reconstruction_epochs.npz`` (tests/golden/generate_canting_reconstruction_golden.py) holds two runs of the
reference's own ``SurfaceReconstructor.reconstruct_surfaces`` on the class fixture's small field - heliostats 0, 2 and 5 of
test_blocking.h5 with four calibration samples each, two planar targets, 10 x 10 points per facet, 3 rays, 64 x 64 - extended at
run time by two more leaves, ``heliostat_group.canting`` and ``heliostat_group.facet_translations``, with the gradient of their w
components set to zero.  Both start from one facet of heliostat 2 tilted by 2 mrad.  Run A: three epochs, all three tensors
learn, fp32 and fp64.  Run B: 40 epochs, canting alone, measured flux from the untilted field; the reference recovers the tilt
to 0.16 of its size.

Bounds: ``max(3 x the reference's own fp32-vs-fp64 distance at epoch 0, floor)`` with the floors of
tests/test_gpu_surface_reconstructor.py (2e-5 flux, 5e-4 gradients, 2e-5 losses); the tensors after a step in units of their
group's learning rate with that file's constants (97 % of the elements within 0.05 lr, none further than 2 lr per step + 0.1 lr).

Measured on MI355X: see DESIGN.md 4.12, "Rigid facet parameters".
"""
import json

import numpy as np
import pytest
import torch

import test_gpu_surface_reconstructor as suite
from conftest import rel_l2
from test_gpu_surface_reconstructor import CHAINED_LOSS_FLOOR, FLUX_FLOOR, GRAD_FLOOR, LOSS_FLOOR, n, rel_max, t

pytestmark = pytest.mark.gpu

NAME = "canting_reconstruction_epochs"
DEV = suite.DEV
NAMES = ("nurbs_control_points", "canting", "facet_translations")
KEYS = sorted(suite.HISTORY_KEYS - {"test_loss"})
# tests/test_gpu_surface_reconstructor.py::test_the_whole_run_through_reconstruct_surfaces, control points after every step
# (that file has them inline in its assertion, so they are written again here)
CLOSE, FRACTION_CLOSE, PER_STEP, SLACK = 0.05, 0.97, 2.0, 0.1
NOT_LAUNCHES = ("art_abi_version", "art_last_hip_error", "art_strerror", "art_async_status", "art_blocking_workspace_bytes",
                "art_trace_bwd_scratch_floats", "art_trace_bwd_scratch_need")


def _reconstructor(d, parameters=None, run="a", epoch_graph=False, **optimization):
    """A freshly loaded scenario whose canting starts tilted as the reference's did, and the reconstructor on it: run A's
    measurements and configuration, or run B's.  ``parameters`` None: the keyword is left out."""
    from artist_amd.optim import SurfaceReconstructor
    view = dict(d)
    configuration = json.loads(str(d["configuration" if run == "a" else "b_configuration"]))
    configuration["optimization"].update(optimization)
    if run == "b":
        view["parser_flux_measured"] = d["b_parser_flux_measured"]
    base, scenario = suite._reconstructor(view, configuration)
    kwargs = dict(ddp_setup=base.ddp_setup, scenario=scenario, data=base.data, optimization_configuration=configuration,
                  number_of_surface_points=base.number_of_surface_points, bitmap_resolution=base.bitmap_resolution,
                  epsilon=base.epsilon, device=DEV)
    if epoch_graph:
        kwargs["epoch_graph"] = True
    if parameters is not None:
        kwargs["parameters"] = parameters
    reconstructor = SurfaceReconstructor(**kwargs)
    group = scenario.heliostat_field.heliostat_groups[0]
    np.testing.assert_allclose(n(group.canting), d["canting_true"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(n(group.facet_translations), d["start_facet_translations"], rtol=1e-6, atol=1e-9)
    group.canting = t(d["start_canting"])
    return reconstructor, scenario, group


def _at_start(d, name, e):
    """The reference's tensor ``name`` at the start of epoch ``e`` (the fixture stores the control points' active rows only)."""
    if e == 0:
        return d[f"start_{name}"]
    if name != "nurbs_control_points":
        return d[f"after_{name}"][e - 1]
    nets = d["start_nurbs_control_points"].copy()
    nets[np.nonzero(d["parser_mask"])[0]] = d["after_nurbs_control_points"][e - 1]
    return nets


def _yardsticks(d):
    active = np.nonzero(d["parser_mask"])[0]
    yard = dict(flux=rel_l2(d["cropped"][0], d["cropped_f64_epoch0"]), sums=rel_l2(d["cropped_sums"][0], d["cropped_sums_f64_epoch0"]),
                grad_nurbs_control_points=rel_l2(d["grad_nurbs_control_points"][0], d["grad_nurbs_control_points_f64_epoch0"]),
                grad_canting=rel_l2(d["grad_canting"][0][active], d["grad_canting_f64_epoch0"][active]),
                grad_facet_translations=rel_l2(d["grad_facet_translations"][0][active], d["grad_facet_translations_f64_epoch0"][active]),
                loss_per_sample=rel_max(d["flux_loss_per_sample"][0], d["flux_loss_per_sample_f64_epoch0"]),
                loss_per_heliostat=rel_max(d["flux_loss_per_heliostat"][0], d["flux_loss_per_heliostat_f64_epoch0"]),
                total_per_heliostat=rel_max(d["total_loss_per_heliostat"][0], d["total_loss_per_heliostat_f64_epoch0"]),
                total=rel_max(d["total_loss"][0], d["total_loss_f64_epoch0"]),
                test_pixel=rel_max(d["test_pixel_loss"][0], d["test_pixel_loss_f64_epoch0"]),
                test_kl=rel_max(d["test_kl_div"][0], d["test_kl_div_f64_epoch0"]))
    floor = dict(flux=FLUX_FLOOR, sums=FLUX_FLOOR, grad_nurbs_control_points=GRAD_FLOOR, grad_canting=GRAD_FLOOR,
                 grad_facet_translations=GRAD_FLOOR)
    bound = {k: max(3 * v, floor.get(k, LOSS_FLOOR)) for k, v in yard.items()}
    print("the reference's own fp32-vs-fp64 distance, first epoch: " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    print("bounds max(3 x yardstick, floor): " + ", ".join(f"{k} {v:.2e}" for k, v in bound.items()))
    return yard, bound


def _steps_apart(name, ours, reference, lr, steps, label):
    """``ours`` against ``reference`` in units of the group's learning rate, with the class test's constants."""
    moved = (np.asarray(ours, np.float64) - np.asarray(reference, np.float64)) / lr
    fraction = float((np.abs(moved) < CLOSE).mean())
    print(f"{label}: {name} within {CLOSE} lr of the reference's: {100 * fraction:.2f} %, largest difference {np.abs(moved).max():.3f} lr")
    assert fraction > FRACTION_CLOSE and np.abs(moved).max() < PER_STEP * steps + SLACK, (label, name, fraction, np.abs(moved).max())


def test_each_epoch_of_run_a_is_reproduced(golden):
    """From the reference's state at the start of each epoch - the three tensors, the multiplier, the reference integrals -
    one epoch: cropped flux, losses per sample, per heliostat and in total, the three gradients after the edge lock and the w
    rule, the three tensors after the step.

    Measured on MI355X: DESIGN.md 4.12, "Rigid facet parameters"."""
    from artist_amd import PixelLoss
    d = golden(NAME)
    _, bound = _yardsticks(d)
    reconstructor, scenario, group = _reconstructor(d, parameters=NAMES)
    assert reconstructor.parameters == NAMES
    state = reconstructor.prepare(0, DEV)
    assert list(state.learnables) == list(NAMES) and all(getattr(group, name).requires_grad for name in NAMES)
    assert [g["params"][0] is getattr(group, name) for g, name in zip(state.optimizer.param_groups, NAMES)] == [True] * 3
    active, inactive = np.nonzero(d["parser_mask"])[0], np.nonzero(d["parser_mask"] == 0)[0]
    for e in range(d["lr"].shape[0]):
        with torch.no_grad():
            for name in NAMES:
                getattr(group, name).copy_(t(_at_start(d, name, e)))
        state.optimizer.zero_grad()
        state.multiplier = t(d["lambda_before"][e])
        state.reference_integrals = t(d["reference_before"][e]) if e > 0 else None
        lrs = [g["lr"] for g in state.optimizer.param_groups]
        np.testing.assert_allclose(lrs, d["lr"][e], rtol=1e-12)
        cropped = reconstructor.predict_flux(state, DEV)
        loss = reconstructor.epoch_loss(state, cropped, PixelLoss(), DEV)
        loss.total.backward()
        reconstructor.update_multiplier(state, loss.violation)
        reconstructor._synchronize_and_lock_learnables(state, DEV)
        grads = {name: n(getattr(group, name).grad) for name in NAMES}
        state.optimizer.step()
        state.scheduler.step()
        err = dict(flux=rel_l2(n(cropped), d["cropped"][e]),
                   sums=rel_l2(n(cropped.sum(dim=(1, 2))), d["cropped_sums"][e]),
                   grad_nurbs_control_points=rel_l2(grads["nurbs_control_points"][active], d["grad_nurbs_control_points"][e]),
                   grad_canting=rel_l2(grads["canting"][active], d["grad_canting"][e][active]),
                   grad_facet_translations=rel_l2(grads["facet_translations"][active], d["grad_facet_translations"][e][active]),
                   loss_per_sample=rel_max(n(loss.flux_loss_per_sample), d["flux_loss_per_sample"][e]),
                   loss_per_heliostat=rel_max(n(loss.flux_loss_per_heliostat), d["flux_loss_per_heliostat"][e]),
                   total_per_heliostat=rel_max(n(loss.total_per_heliostat), d["total_loss_per_heliostat"][e]),
                   total=rel_max(float(loss.total.detach()), d["total_loss"][e]))
        print(f"epoch {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) +
              f"; total loss {float(loss.total.detach()):.7f} (reference {d['total_loss'][e]:.7f})")
        assert cropped.shape == (9, 64, 64)
        for name in NAMES:                       # no sample, no gradient; and the w components are no parameters
            assert not grads[name][inactive].any(), name
        assert not grads["canting"][..., 3].any() and not grads["facet_translations"][..., 3].any()
        for key, value in err.items():
            assert value < bound[key], (e, key, value, bound[key])
        if e == 0:       # ... and as close to the fp64 run as the reference's own fp32 run is
            assert rel_l2(n(cropped), d["cropped_f64_epoch0"]) < bound["flux"]
            assert rel_l2(grads["nurbs_control_points"][active], d["grad_nurbs_control_points_f64_epoch0"]) < bound["grad_nurbs_control_points"]
            assert rel_l2(grads["canting"][active], d["grad_canting_f64_epoch0"][active]) < bound["grad_canting"]
            assert rel_l2(grads["facet_translations"][active], d["grad_facet_translations_f64_epoch0"][active]) < bound["grad_facet_translations"]
        for name, lr in zip(NAMES, d["lr"][e]):
            after = n(getattr(group, name))
            reference = d[f"after_{name}"][e]
            _steps_apart(name, after[active], reference if name == "nurbs_control_points" else reference[active], lr, 1, f"epoch {e}")
            np.testing.assert_array_equal(after[inactive], _at_start(d, name, e)[inactive])


_RUNS = {}


def _whole_run(d, key, **made):
    """``reconstruct_surfaces`` on a freshly made reconstructor (``_reconstructor(d, **made)``), once per ``key``: what it
    returned, the three tensors at the start, after every step and at the end, the field's surfaces afterwards."""
    if key not in _RUNS:
        from artist_amd import PixelLoss
        reconstructor, scenario, group = _reconstructor(d, **made)
        start = {name: getattr(group, name).detach().clone() for name in NAMES}
        after = []
        prepare = reconstructor.prepare

        def prepare_recording(*a, **k):
            state = prepare(*a, **k)
            step = state.optimizer.step

            def step_recording(*sa, **sk):
                out = step(*sa, **sk)
                after.append({name: getattr(group, name).detach().clone() for name in NAMES})
                return out

            state.optimizer.step = step_recording
            return state

        reconstructor.prepare = prepare_recording
        final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=PixelLoss(), device=DEV)
        torch.cuda.synchronize()
        assert len(histories) == 1 and len(histories[0]) == 1
        _RUNS[key] = dict(final_loss=final_loss, history=histories[0][0], start=start, after=after, group=group,
                          reconstructor=reconstructor, end={name: getattr(group, name).detach().clone() for name in NAMES},
                          requires_grad={name: getattr(group, name).requires_grad for name in NAMES},
                          surface_points=group.surface_points.clone(), surface_normals=group.surface_normals.clone())
    return _RUNS[key]


def _assert_same_run(a, b):
    for key in KEYS:
        assert a["history"][key] == b["history"][key], key
    for key in ("pixel_loss", "kl_div"):
        assert torch.equal(a["history"]["test_loss"][key], b["history"]["test_loss"][key]), key
    assert torch.equal(a["final_loss"], b["final_loss"]) and len(a["after"]) == len(b["after"])
    for e, (x, y) in enumerate(zip(a["after"], b["after"])):
        for name in NAMES:
            assert torch.equal(x[name], y[name]), f"{name} after the step of epoch {e} differs"
    for name in NAMES:
        assert torch.equal(a["end"][name], b["end"][name]), name
    assert torch.equal(a["surface_points"], b["surface_points"]) and torch.equal(a["surface_normals"], b["surface_normals"])


def test_the_whole_run_with_all_three_parameters(golden):
    """``reconstruct_surfaces()`` for run A's three epochs: the histories and the final loss within the chained-run bounds of
    the class test, the three tensors after every step in units of their learning rates, and ``update_surfaces``: the field's
    surface points and normals are those of a fresh evaluation with the learnt control points, canting and translations."""
    from artist_amd.nurbs import NURBSSurfaces, create_nurbs_evaluation_grid
    d = golden(NAME)
    _, bound = _yardsticks(d)
    run = _whole_run(d, "all", parameters=["facet_translations", "canting", "nurbs_control_points", "canting"])
    assert run["reconstructor"].parameters == NAMES
    history, active = run["history"], np.nonzero(d["parser_mask"])[0]
    assert set(history) == suite.HISTORY_KEYS and all(len(history[key]) == 3 for key in KEYS)
    print("total loss per epoch:", history["total_loss"], " reference:", d["history_total_loss"])
    loss_bound = max(3 * rel_max(d["total_loss"][0], d["total_loss_f64_epoch0"]), CHAINED_LOSS_FLOOR)
    for e in range(3):
        assert abs(history["total_loss"][e] - d["history_total_loss"][e]) / abs(d["history_total_loss"][e]) < loss_bound
        assert abs(history["flux_loss"][e] - d["history_flux_loss"][e]) / abs(d["history_flux_loss"][e]) < \
            max(bound["loss_per_heliostat"], CHAINED_LOSS_FLOOR)
    np.testing.assert_allclose(history["flux_integral_constraint"][0], d["history_flux_integral_constraint"][0], rtol=1e-5)
    assert len(run["after"]) == 3
    for e in range(3):
        for name, lr in zip(NAMES, d["lr"][e]):
            reference = d[f"after_{name}"][e]
            _steps_apart(name, n(run["after"][e][name])[active], reference if name == "nurbs_control_points" else reference[active],
                         lr, e + 1, f"after epoch {e}")
    assert rel_max(n(run["final_loss"])[active], d["final_loss"][active]) < max(bound["total_per_heliostat"], CHAINED_LOSS_FLOOR)
    errs = dict(pixel=rel_max(n(history["test_loss"]["pixel_loss"]), d["history_test_pixel_loss"]),
                kl=rel_max(n(history["test_loss"]["kl_div"]), d["history_test_kl_div"]))
    print("the last validation against the reference's:", errs)
    assert d["validated_epochs"].tolist() == [0, 1] and set(history["test_loss"]) == {"pixel_loss", "kl_div"}
    assert errs["pixel"] < max(bound["test_pixel"], CHAINED_LOSS_FLOOR) and errs["kl"] < max(bound["test_kl"], CHAINED_LOSS_FLOOR)
    # update_surfaces: a fresh evaluation with what was learnt
    group = run["group"]
    for name in NAMES:
        assert torch.equal(getattr(group, name).detach(), run["end"][name]) and not torch.equal(run["end"][name], run["start"][name])
    grid = create_nurbs_evaluation_grid(torch.tensor([10, 10]), device=DEV)
    with torch.no_grad():
        points, normals = NURBSSurfaces(group.nurbs_degrees, run["end"]["nurbs_control_points"], device=DEV).calculate_surface_points_and_normals(
            grid[None, None].expand(6, 4, -1, -1), run["end"]["canting"], run["end"]["facet_translations"])
    assert torch.equal(run["surface_points"], points.reshape(6, -1, 4)) and torch.equal(run["surface_normals"], normals.reshape(6, -1, 4))
    assert not group.surface_points.requires_grad and not group.surface_normals.requires_grad
    h = int(d["recorded_heliostat"])
    err = rel_l2(n(run["surface_points"])[h], d["updated_surface_points"])
    print(f"surface points of heliostat {h} after update_surfaces against the reference's: relative L2 {err:.2e}")
    assert run["surface_points"].shape == (6, 400, 4) and err < FLUX_FLOOR
    # the rigid tensors are constants again for whoever evaluates next
    assert not group.canting.requires_grad and not group.facet_translations.requires_grad


def _facet_normal(canting, d):
    c = np.asarray(canting, dtype=np.float64)[int(d["tilted_heliostat"]), int(d["tilted_facet"])]
    normal = np.cross(c[0, :3], c[1, :3])
    return normal / np.linalg.norm(normal)


def _angle(a, b):
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), np.dot(a, b)))


def test_canting_alone_recovers_the_tilt(golden):
    """Run B: 40 epochs with ``parameters=("canting",)`` against flux measured on the untilted field.  The angle between the
    learnt and the true normal of the tilted facet ends below half of the initial 2 mrad (the reference alone reaches a quarter:
    the generator asserts it), the last epoch's total loss below the first's; the control points and the translations keep
    their bits and do not require grad."""
    d = golden(NAME)
    run = _whole_run(d, "canting", parameters=("canting",), run="b")
    truth = _facet_normal(d["canting_true"], d)
    error = [_angle(_facet_normal(n(x), d), truth) for x in [run["start"]["canting"]] + [a["canting"] for a in run["after"]]]
    history = run["history"]
    print(f"tilt error [mrad]: {np.round(1e3 * np.asarray(error), 4).tolist()}\nthe reference's: {np.round(1e3 * d['b_tilt_error'], 4).tolist()}")
    print("total loss:", history["total_loss"][0], "->", history["total_loss"][-1], " the reference's:", d["b_total_loss"][0], "->", d["b_total_loss"][-1])
    assert len(run["after"]) == len(history["total_loss"]) == len(d["b_total_loss"]) == 40
    assert d["b_tilt_error"][-1] < 0.25 * d["b_tilt_error"][0]
    assert abs(error[0] - float(d["tilt"])) < 1e-3 * float(d["tilt"])
    assert error[-1] < 0.5 * error[0]
    assert history["total_loss"][-1] < history["total_loss"][0]
    for name in ("nurbs_control_points", "facet_translations"):
        assert torch.equal(run["end"][name], run["start"][name]) and not run["requires_grad"][name], name
        assert getattr(run["group"], name).grad is None


def test_a_second_run_gives_the_same_bits_and_the_untouched_keep_theirs(golden):
    """A second run on a freshly loaded scenario: the same histories, final loss and tensors after every step
    (``torch.equal``).  Rows of heliostats without samples and every w component are bit-unchanged."""
    d = golden(NAME)
    first = _whole_run(d, "all", parameters=["facet_translations", "canting", "nurbs_control_points", "canting"])
    second = _whole_run(d, "all again", parameters=NAMES)
    _assert_same_run(first, second)
    inactive = torch.as_tensor(np.nonzero(d["parser_mask"] == 0)[0], device=DEV)
    for run in (first, _whole_run(d, "canting", parameters=("canting",), run="b")):
        for name in NAMES:
            assert torch.equal(run["end"][name][inactive], run["start"][name][inactive]), name
        for name in ("canting", "facet_translations"):
            assert torch.equal(run["end"][name][..., 3], run["start"][name][..., 3]), name
            assert not run["end"][name][..., 3].any()
    assert not torch.equal(first["end"]["facet_translations"][..., :3], first["start"]["facet_translations"][..., :3])


def _count_calls(monkeypatch):
    """Every launch through the library handle, by name, in order."""
    from artist_amd import _lib
    handle, calls = _lib.lib(), []
    for name in _lib.SIGNATURES:
        if name in NOT_LAUNCHES:
            continue
        real = getattr(handle, name)

        def wrapped(*args, _real=real, _name=name):
            calls.append(_name)
            return _real(*args)

        monkeypatch.setattr(handle, name, wrapped)
    return calls


def test_the_default_is_unchanged(golden, monkeypatch):
    """``parameters`` left out and ``("nurbs_control_points",)`` give ``torch.equal`` runs, and neither makes an
    ``art_cant_facets_*`` call: canting and translations stay constants of the one fused launch."""
    d = golden(NAME)
    calls = _count_calls(monkeypatch)
    omitted = _whole_run(d, "default", parameters=None)
    named = _whole_run(d, "named default", parameters=("nurbs_control_points",))
    monkeypatch.undo()
    assert omitted["reconstructor"].parameters == named["reconstructor"].parameters == ("nurbs_control_points",)
    _assert_same_run(omitted, named)
    assert calls.count("art_nurbs_fwd") > 6 and not [name for name in calls if name.startswith("art_cant_facets")], sorted(set(calls))
    for run in (omitted, named):
        for name in ("canting", "facet_translations"):
            assert torch.equal(run["end"][name], run["start"][name]) and not run["requires_grad"][name]
        assert not torch.equal(run["end"]["nurbs_control_points"], run["start"]["nurbs_control_points"])


@pytest.mark.parametrize("parameters", [("canting",), ("facet_translations",), NAMES], ids=["canting", "translations", "all"])
def test_the_staged_route_once_per_training_step(golden, monkeypatch, parameters):
    """With a rigid tensor learning, an epoch's calls hold exactly one ``art_cant_facets_fwd`` and one ``art_cant_facets_bwd``
    - the surfaces are evaluated and canted once per heliostat, not per sample - and the NURBS adjoint only when the control
    points learn; ``validate`` runs under ``no_grad`` and takes the fused launch: no canting call."""
    from artist_amd import PixelLoss
    d = golden(NAME)
    reconstructor, scenario, group = _reconstructor(d, parameters=parameters)
    calls = _count_calls(monkeypatch)
    state = reconstructor.prepare(0, DEV)
    assert not [name for name in calls if name.startswith(("art_cant_facets", "art_nurbs"))]     # prepare only marks the leaves
    state.optimizer.zero_grad()
    loss = reconstructor.epoch_loss(state, reconstructor.predict_flux(state, DEV), PixelLoss(), DEV)
    loss.total.backward()
    reconstructor.update_multiplier(state, loss.violation)
    reconstructor._synchronize_and_lock_learnables(state, DEV)
    state.optimizer.step()
    torch.cuda.synchronize()
    epoch = list(calls)
    reconstructor.validate(state, DEV)
    torch.cuda.synchronize()
    monkeypatch.undo()
    validation = calls[len(epoch):]
    print(f"{parameters}: calls of the epoch {epoch}; of the validation {validation}")
    assert epoch.count("art_cant_facets_fwd") == 1 and epoch.count("art_cant_facets_bwd") == 1
    assert epoch.count("art_nurbs_fwd") == 1 and epoch.count("art_nurbs_bwd") == (1 if "nurbs_control_points" in parameters else 0)
    assert epoch.count("art_adam_step") == len(parameters) and epoch.count("art_trace_fwd") == 1
    assert "art_nurbs_fwd" in validation and not [name for name in validation if name.startswith("art_cant_facets")]
    for name in NAMES:
        assert getattr(group, name).requires_grad == (name in parameters), name
        assert (getattr(group, name).grad is not None) == (name in parameters), name
