"""ARTIST's ``AimPointOptimizer``, reproduced epoch by epoch on the GPU (``-m gpu``).

``tests/golden/aim_point_optimizer_epochs.npz`` holds three epochs of ONE unmodified run of the reference's
``AimPointOptimizer.optimize`` (artist/optim/aim_point_optimizer.py:724-972; tests/golden/generate_aim_point_golden.py: the six
heliostats of test_blocking.h5 on the planar target_4, three of them partly blocked, ``KLDivergenceLoss`` against a trapezoid x
trapezoid distribution, the local-flux constraint active from the first epoch, the other two from the second), and its first epoch
in fp64 on the same rays.  ``artist_amd.optim.AimPointOptimizer`` must land on the reference's numbers - the only optimiser whose
backward pass goes through the soft blocking mask, the motor path of the rigid-body kinematics and the per-target sum together.

The yardstick is the reference's own fp32-vs-fp64 distance at the first epoch: ``err < max(3 x yardstick, floor)`` with the floors
of tests/test_gpu_optimizer_epoch.py (2e-5 relative L2 for flux, 5e-4 for the gradient, 2e-5 relative for a loss).  The three
constraint terms are small differences of large numbers (a flux integral 0.16 % below its reference gives a term of 1e-6): their
tolerance is the flux bound carried through the term's formula (``_term_tolerance``); the intercept term is a function of the
factors alone, which are exact.

Measured on MI355X (yardstick -> error of epochs 0 / 1 / 2): see DESIGN.md 4.11.
"""
import json
import pathlib

import numpy as np
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DDP = dict(rank=0, world_size=1, is_distributed=False, groups_to_ranks_mapping={0: [0]}, ranks_to_groups_mapping={0: [0]},
           heliostat_group_rank=0, heliostat_group_world_size=1)
FLUX_FLOOR, GRAD_FLOOR, LOSS_FLOOR = 2e-5, 5e-4, 2e-5
STEP_BOUND = 0.05                       # of the learning rate (tests/test_gpu_optimizer_epoch.py: "within 0.05 lr of the reference's")


def t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def scalar(x):
    """A one-element array or tensor (the losses are ``[1]``: one bitmap) as a float."""
    return float(n(x).reshape(-1)[0]) if isinstance(x, torch.Tensor) else float(np.asarray(x).reshape(-1)[0])


def _optimizer(d, max_epoch=None):
    """A fresh scenario and the optimiser on it, configured as the reference's run was; the light source hands out the
    distortions the reference drew on the CPU (sun.py:224-234 with the seed the optimiser passes: the group's rank)."""
    from artist_amd.optim import AimPointOptimizer
    from artist_amd.scenario import Scenario, open_scenario_file
    path = pathlib.Path(__file__).resolve().parent / "golden" / "scenarios" / "test_blocking.h5"
    with open_scenario_file(path) as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file,
                                                    number_of_surface_points_per_facet=torch.tensor([int(v) for v in d["points_per_facet"]]),
                                                    device=DEV)
    scenario.set_number_of_rays(number_of_rays=int(d["n_rays"]))
    both = torch.stack((torch.from_numpy(d["distortions_u"]), torch.from_numpy(d["distortions_e"])), dim=-1).to(DEV)

    def recorded_distortions(number_of_points, number_of_active_heliostats, random_seed=7):
        assert random_seed == int(d["seed"]) and both.shape[:3] == (number_of_active_heliostats, int(d["n_rays"]), number_of_points)
        return both[..., 0], both[..., 1]

    scenario.light_sources.light_source_list[0].get_distortions = recorded_distortions
    configuration = json.loads(str(d["configuration"]))
    if max_epoch is not None:
        configuration["optimization"]["max_epoch"] = max_epoch
    optimizer = AimPointOptimizer(ddp_setup=DDP, scenario=scenario, optimization_configuration=configuration,
                                  incident_ray_direction=t(d["sun"]), target_area_index=int(d["target_area_index"]),
                                  ground_truth=t(d["ground_truth"]), dni=scalar(d["dni"]),
                                  bitmap_resolution=torch.tensor([int(v) for v in d["resolution"]]), epsilon=scalar(d["epsilon"]),
                                  device=DEV)
    return optimizer, scenario


def _set_state(optimizer, d, e):
    """The reference's multipliers and references at the start of epoch ``e``."""
    state = optimizer.state
    state.lambda_flux_integral, state.lambda_intercept, state.lambda_local_flux = t(d["lambda_before"][e])
    state.flux_integral_reference = t(d["ref_integral_before"][e]) if e > 0 else None
    state.intercept_factors_reference = t(d["ref_intercept_before"][e]) if e > 0 else None


def _yardsticks(d):
    """The reference's own fp32-vs-fp64 distance at the first epoch -> the bounds ``max(3 x yardstick, floor)``."""
    yard = dict(flux=rel_l2(d["total_flux"][0], d["total_flux_f64_epoch0"]),
                grad=rel_l2(d["grad"][0], d["grad_f64_epoch0"]),
                flux_loss=abs(scalar(d["flux_loss"][0]) - scalar(d["flux_loss_f64_epoch0"])) / abs(scalar(d["flux_loss_f64_epoch0"])),
                total_loss=abs(scalar(d["total_loss"][0]) - scalar(d["total_loss_f64_epoch0"])) / abs(scalar(d["total_loss_f64_epoch0"])))
    bound = dict(flux=max(3 * yard["flux"], FLUX_FLOOR), grad=max(3 * yard["grad"], GRAD_FLOOR),
                 flux_loss=max(3 * yard["flux_loss"], LOSS_FLOOR), total_loss=max(3 * yard["total_loss"], LOSS_FLOOR))
    print("the reference's own fp32-vs-fp64 distance, first epoch: " + ", ".join(f"{k} {v:.2e}" for k, v in yard.items()))
    print("bounds max(3 x yardstick, floor): " + ", ".join(f"{k} {v:.2e}" for k, v in bound.items()))
    return yard, bound


def _term_tolerance(multiplier, rho, violation_of, quantity, relative_error):
    """How far ``lambda v + rho/2 v^2`` (``v`` clamped at 0) moves when the ``quantity`` its violation is formed from - the flux
    integral, the brightest pixel - is off by ``relative_error``, the bound the flux itself is held to."""
    term = lambda q: multiplier * max(violation_of(q), 0.0) + 0.5 * rho * max(violation_of(q), 0.0) ** 2  # noqa: E731
    return max(abs(term(quantity * (1 + s * relative_error)) - term(quantity)) for s in (-1.0, 1.0))


def test_each_epoch_of_the_reference_run_is_reproduced(golden):
    """From the reference's starting point of each epoch (parameter, multipliers, references): total flux, the three factors
    (exact), flux loss, the three constraint terms, total loss and the parameter's gradient - through ``art_flux_loss``,
    ``art_trace_bwd`` with the soft blocking mask, ``art_align_bwd`` and ``art_rigid_body_bwd``'s motor path."""
    from artist_amd import KLDivergenceLoss
    d = golden("aim_point_optimizer_epochs")
    _, bound = _yardsticks(d)
    optimizer, _ = _optimizer(d)
    optimizer.prepare(DEV)
    g = optimizer.groups[0]
    np.testing.assert_allclose(n(g["initial"]), d["initial_motor_positions"], rtol=1e-4)     # (the bound of the kinematics tests)
    np.testing.assert_allclose(n(g["scale"]), d["scale"], rtol=1e-4)
    config = json.loads(str(d["configuration"]))["constraints"]
    allowed = float(np.prod(d["target_dimensions"].astype(np.float64)) / np.prod(d["resolution"]) * config["max_flux_density"])
    np.testing.assert_allclose(float(optimizer.state.max_flux_density_per_pixel), allowed, rtol=1e-6)
    for e in range(d["param_start"].shape[0]):
        with torch.no_grad():
            g["parameter"].copy_(t(d["param_start"][e]))
        g["parameter"].grad = None
        _set_state(optimizer, d, e)
        total, flux_loss, (integral_term, intercept_term, local_term), flux, factors = optimizer.epoch_loss(KLDivergenceLoss(), DEV)
        total.backward()
        err = dict(flux=rel_l2(n(flux), d["total_flux"][e]), grad=rel_l2(n(g["parameter"].grad), d["grad"][e]),
                   flux_loss=abs(scalar(flux_loss) - scalar(d["flux_loss"][e])) / abs(scalar(d["flux_loss"][e])),
                   total_loss=abs(scalar(total) - scalar(d["total_loss"][e])) / abs(scalar(d["total_loss"][e])))
        print(f"epoch {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) +
              f"; total loss {scalar(total):.7f} (reference {scalar(d['total_loss'][e]):.7f}); terms: flux integral "
              f"{scalar(integral_term):.4e} ({scalar(d['flux_integral_constraint'][e]):.4e}), intercept "
              f"{scalar(intercept_term):.4e} ({scalar(d['intercept_constraint'][e]):.4e}), local flux "
              f"{scalar(local_term):.6e} ({scalar(d['local_flux_constraint'][e]):.6e})")
        np.testing.assert_allclose(n(g["group"].kinematics.motor_positions), d["motor_start"][e], rtol=1e-4)
        for got, key in zip(factors, ("intercept_factors", "on_target_factors", "blocking_factors")):
            np.testing.assert_array_equal(n(got), d[key][e], err_msg=key)
        for key in ("flux", "flux_loss", "total_loss", "grad"):
            assert err[key] < bound[key], (e, key, err[key], bound[key])
        # the constraint terms: the flux bound carried through each term's formula
        lam = [float(v) for v in d["lambda_before"][e]]
        ref_flux = d["total_flux"][e].astype(np.float64)
        reference_integral = scalar(d["ref_integral_after"][e])
        tol_integral = _term_tolerance(lam[0], config["rho_flux_integral"], lambda s: (reference_integral - s) / reference_integral,
                                       float(ref_flux.sum()), bound["flux"])
        tol_local = _term_tolerance(lam[2], config["rho_local_flux"], lambda p: (p - allowed) / allowed, float(ref_flux.max()),
                                    bound["flux"])
        np.testing.assert_allclose(scalar(integral_term), scalar(d["flux_integral_constraint"][e]), rtol=1e-5, atol=tol_integral)
        np.testing.assert_allclose(scalar(local_term), scalar(d["local_flux_constraint"][e]), rtol=1e-5, atol=tol_local)
        np.testing.assert_allclose(scalar(intercept_term), scalar(d["intercept_constraint"][e]), rtol=1e-5, atol=0)
        if e == 0:       # ... and as close to the fp64 run as the reference's own fp32 run is
            assert rel_l2(n(g["parameter"].grad), d["grad_f64_epoch0"]) < bound["grad"]
            assert rel_l2(n(flux), d["total_flux_f64_epoch0"]) < bound["flux"]


def test_the_parameter_after_every_step_lands_on_the_reference(golden):
    """The three epochs chained with the optimiser's own ``artist_amd.optim.Adam`` and scheduler.  Adam's first steps move every
    element by about +-lr whatever its gradient's size: compared per element in units of the learning rate.  An element whose
    reference gradient is smaller than the reference's own fp32-vs-fp64 gradient difference may step the other way and is left
    out - at most one of the twelve (the reference's fp32 run leaves out none)."""
    from artist_amd import KLDivergenceLoss
    d = golden("aim_point_optimizer_epochs")
    optimizer, _ = _optimizer(d)
    optimizer.prepare(DEV)
    parameter = optimizer.groups[0]["parameter"]
    uncertain = np.abs(d["grad"][0].astype(np.float64) - d["grad_f64_epoch0"])
    for e in range(d["param_start"].shape[0]):
        lr = optimizer.optimizer.param_groups[0]["lr"]
        np.testing.assert_allclose(lr, d["lr"][e], rtol=1e-12)
        optimizer.optimizer.zero_grad()
        total = optimizer.epoch_loss(KLDivergenceLoss(), DEV)[0]
        total.backward()
        optimizer.optimizer.step()
        optimizer.scheduler.step()
        moved = (n(parameter) - d["param_after"][e]) / lr
        kept = np.abs(d["grad"][e]) >= uncertain
        print(f"epoch {e}: lr {lr:.3e}, total loss {scalar(total):.7f} (reference {scalar(d['total_loss'][e]):.7f}); parameter after "
              f"the step: largest difference {np.abs(moved[kept]).max():.4f} lr over {int(kept.sum())} of {kept.size} elements")
        assert kept.size == 12 and kept.sum() >= 11
        assert np.abs(moved[kept]).max() < STEP_BOUND, (e, moved)


def test_the_whole_run_through_optimize(golden):
    """``optimize()`` for three epochs (``max_epoch=2``, tolerance 0): the histories, the total losses against the reference's,
    motor positions that moved and stayed inside the actuators' limits, and the same bits from a second run on a fresh scenario."""
    from artist_amd import KLDivergenceLoss
    from artist_amd.aim_point_optimizer import HISTORY_KEYS
    d = golden("aim_point_optimizer_epochs")
    _, bound = _yardsticks(d)
    runs = []
    for _ in range(2):
        optimizer, scenario = _optimizer(d, max_epoch=2)
        final_loss, history, intercept, on_target, blocking = optimizer.optimize(loss_definition=KLDivergenceLoss(), device=DEV)
        kinematics = scenario.heliostat_field.heliostat_groups[0].kinematics
        runs.append((final_loss, history, n(kinematics.motor_positions), n(intercept), n(on_target), n(blocking),
                     n(optimizer.groups[0]["parameter"])))
    final_loss, history, motors, intercept, on_target, blocking, parameter = runs[0]
    assert set(history) == set(HISTORY_KEYS) == {"total_loss", "flux_loss", "local_flux_constraint", "intercept_constraint",
                                                 "flux_integral_constraint", "flux_integral"}
    assert all(len(v) == 3 and all(isinstance(x, float) for x in v) for v in history.values())
    print("total loss per epoch:", history["total_loss"], " reference:", d["history_total_loss"])
    for e in range(3):
        assert abs(history["total_loss"][e] - d["history_total_loss"][e]) / abs(d["history_total_loss"][e]) < bound["total_loss"]
        assert abs(history["flux_loss"][e] - d["history_flux_loss"][e]) / abs(d["history_flux_loss"][e]) < bound["flux_loss"]
    assert history["flux_integral"][0] == pytest.approx(100 * 1e-8 / scalar(d["ref_integral_after"][0]), rel=1e-3)
    assert final_loss.device.type == "cpu" and float(final_loss) == history["total_loss"][-1]
    for got in (intercept, on_target, blocking):
        assert got.shape == (6,)
    np.testing.assert_array_equal(blocking, d["blocking_factors"][2])
    # the motor positions are those of the last epoch traced: moved from the start, inside the actuators' limits
    assert np.abs(motors - d["initial_motor_positions"]).min() > 1.0
    np.testing.assert_allclose(motors, d["final_motor_positions"], rtol=1e-4)
    assert (motors >= d["motor_limits"][:, 0]).all() and (motors <= d["motor_limits"][:, 1]).all()
    # ... and a second run gives the same bits
    assert runs[1][1] == history and torch.equal(runs[1][0], final_loss)
    for a, b in zip(runs[0][2:], runs[1][2:]):
        np.testing.assert_array_equal(a, b)


def test_the_gradient_reaches_through_blocking(golden):
    """The partly blocked heliostats' parameter gradient differs from the gradient of the same epoch traced without blocking:
    a silently unblocked path would pass every other comparison of an unblocked case."""
    from artist_amd import KLDivergenceLoss
    d = golden("aim_point_optimizer_epochs")
    blocked = np.nonzero((d["blocking_factors"][0] > 0) & (d["blocking_factors"][0] < 1))[0]
    assert blocked.size > 0
    grads, factors = {}, {}
    for blocking_active in (True, False):
        optimizer, _ = _optimizer(d)
        optimizer.blocking_active = blocking_active
        optimizer.prepare(DEV)
        total, *_, flux, (_, _, blocking_factors) = optimizer.epoch_loss(KLDivergenceLoss(), DEV)
        total.backward()
        grads[blocking_active], factors[blocking_active] = n(optimizer.groups[0]["parameter"].grad), n(blocking_factors)
    np.testing.assert_array_equal(factors[True], d["blocking_factors"][0])
    assert (factors[False] == 1).all()
    difference = np.abs(grads[True] - grads[False])[blocked] / np.abs(grads[True][blocked])
    print("partly blocked heliostats", blocked, ": relative difference of their gradient with / without blocking\n", difference)
    assert rel_l2(grads[True], d["grad"][0]) < rel_l2(grads[False], d["grad"][0])
    for h in blocked:
        assert not np.array_equal(grads[True][h], grads[False][h])
        assert difference[list(blocked).index(h)].max() > 10 * GRAD_FLOOR
