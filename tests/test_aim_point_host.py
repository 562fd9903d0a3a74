"""The host side of the aim-point optimiser (no GPU): ``trapezoid_distribution``, ``artist_amd.training`` and the objective
function against what the reference computed (tests/golden/aim_point_optimizer_epochs.npz, written by
tests/golden/generate_aim_point_golden.py from ONE unmodified run of ARTIST's ``AimPointOptimizer``), and the two errors the
class raises before it touches a device."""
import json
import types

import numpy as np
import pytest
import torch

CPU = torch.device("cpu")


def test_trapezoid_distribution_gives_the_reference_values(golden):
    """Rectangle (no slope), a trapezoid that fits (zero padding), slopes cut off by the axis, the degenerate one-pixel axis."""
    from artist_amd import trapezoid_distribution
    from artist_amd.flux import trapezoid_distribution as from_flux
    assert trapezoid_distribution is from_flux
    d = golden("aim_point_optimizer_epochs")
    kinds = set()
    for i, (total, slope, plateau) in enumerate(d["trapezoid_cases"]):
        got = trapezoid_distribution(total_width=int(total), slope_width=int(slope), plateau_width=int(plateau), device=CPU)
        assert got.shape == (int(total),) and got.dtype == torch.float32 and got.device.type == "cpu"
        np.testing.assert_array_equal(got.numpy(), d[f"trapezoid_{i}"])
        np.testing.assert_array_equal(got.numpy(), got.numpy()[::-1])                            # symmetric
        kinds.add("rectangle" if slope == 0 else "cut off" if 2 * slope + plateau > total else "padded")
    assert kinds == {"rectangle", "cut off", "padded"}
    # a rectangle holds zeros and ones only; a padded trapezoid starts at zero and reaches one; a cut-off one never touches zero
    assert set(np.unique(d["trapezoid_0"])) == {0.0, 1.0}
    padded = trapezoid_distribution(16, 4, 4, device=CPU)
    assert padded[0] == 0 and padded.max() == 1 and trapezoid_distribution(16, 6, 10, device=CPU).min() > 0
    # a tensor for the width, as the tutorial passes it
    assert torch.equal(trapezoid_distribution(torch.tensor([16, 8])[0], 4, 4, device=CPU), padded)


def test_early_stopping_decides_like_the_reference(golden):
    from artist_amd.training import EarlyStopping
    d = golden("aim_point_optimizer_epochs")
    losses = [float(v) for v in d["early_stopping_losses"]]
    stopper = EarlyStopping(**json.loads(str(d["early_stopping_arguments"])))
    decisions, counters = [], []
    for loss in losses:
        decisions.append(stopper.step(loss))
        counters.append(stopper.counter)
    assert decisions == [bool(v) for v in d["early_stopping_decisions"]]
    assert counters == [int(v) for v in d["early_stopping_counters"]]
    assert decisions[:2] == [False, False] and counters[:2] == [0, 0]                 # no decision before the window is full
    absolute = EarlyStopping(window_size=2, patience=2, min_improvement=0.05, relative=False)
    assert [absolute.step(loss) for loss in losses] == [bool(v) for v in d["early_stopping_absolute_decisions"]]
    defaults = EarlyStopping()
    assert (defaults.window_size, defaults.patience, defaults.min_improvement, defaults.relative, defaults.eps) == (10, 20, 1e-4, True, 1e-8)


def test_scheduler_factories_configure_torch_schedulers():
    """``exponential`` / ``cyclic`` / ``reduce_on_plateau`` on ``artist_amd.optim.Adam`` (constructing it needs no GPU)."""
    from artist_amd import training
    from artist_amd.optim import Adam
    parameters = dict(scheduler_type="exponential", gamma=0.9, lr_min=1e-6, lr_max=1e-3, step_size_up=500, reduce_factor=0.3,
                      patience=100, threshold=1e-3, cooldown=10)
    new = lambda: Adam([torch.nn.Parameter(torch.zeros(3))], lr=3e-4)  # noqa: E731
    scheduler = training.exponential(optimizer=new(), parameters=parameters)
    assert type(scheduler) is torch.optim.lr_scheduler.ExponentialLR and scheduler.gamma == 0.9
    optimizer = new()
    scheduler = training.cyclic(optimizer=optimizer, parameters=parameters)
    assert type(scheduler) is torch.optim.lr_scheduler.CyclicLR
    assert scheduler.base_lrs == [1e-6] and scheduler.max_lrs == [1e-3] and scheduler.total_size == 1000.0
    assert optimizer.param_groups[0]["lr"] == 1e-6
    scheduler = training.reduce_on_plateau(optimizer=new(), parameters=parameters)
    assert type(scheduler) is torch.optim.lr_scheduler.ReduceLROnPlateau
    assert (scheduler.factor, scheduler.patience, scheduler.threshold, scheduler.cooldown, scheduler.min_lrs) == (0.3, 100, 1e-3, 10, [1e-6])
    assert getattr(training, parameters["scheduler_type"]) is training.exponential           # (how the optimisers look one up)


def _state(d, e):
    from artist_amd.aim_point_optimizer import ConstraintState
    config = json.loads(str(d["configuration"]))
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    allowed = torch.prod(t(d["target_dimensions"])) / torch.prod(torch.tensor(d["resolution"])) * config["constraints"]["max_flux_density"]
    state = ConstraintState.fresh(config["constraints"], allowed, float(d["epsilon"]))
    state.lambda_flux_integral, state.lambda_intercept, state.lambda_local_flux = t(d["lambda_before"][e])
    if e > 0:
        state.flux_integral_reference, state.intercept_factors_reference = t(d["ref_integral_before"][e]), t(d["ref_intercept_before"][e])
    return state


@pytest.mark.parametrize("epoch", [0, 1, 2])
def test_objective_reproduces_the_reference_terms(golden, epoch):
    """``aim_point_objective`` on the reference's total flux, intercept factors, flux loss and state of each epoch: the three
    terms, the total loss, the multipliers and the references afterwards.  The same torch arithmetic on the same numbers."""
    from artist_amd.aim_point_optimizer import aim_point_objective
    d = golden("aim_point_optimizer_epochs")
    state = _state(d, epoch)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32))  # noqa: E731
    flux = t(d["total_flux"][epoch]).requires_grad_(True)
    total, integral_term, intercept_term, local_term = aim_point_objective(
        t(d["flux_loss"][epoch]), flux, t(d["intercept_factors"][epoch]), state)
    close = lambda got, want: np.testing.assert_allclose(got.detach().numpy().reshape(-1), np.reshape(want, -1), rtol=1e-6, atol=0)  # noqa: E731
    close(total, d["total_loss"][epoch])
    close(integral_term, d["flux_integral_constraint"][epoch])
    close(intercept_term, d["intercept_constraint"][epoch])
    close(local_term, d["local_flux_constraint"][epoch])
    close(torch.stack((state.lambda_flux_integral, state.lambda_intercept, state.lambda_local_flux)), d["lambda_after"][epoch])
    close(state.flux_integral_reference, d["ref_integral_after"][epoch])
    close(state.intercept_factors_reference, d["ref_intercept_after"][epoch])
    assert float(local_term.detach()) > 0                                        # (the case was chosen with the local-flux term active)
    if epoch == 0:                                                      # the references are this epoch's own values: no violation
        assert float(integral_term.detach()) == 0 and float(intercept_term.detach()) == 0
    else:
        assert float(integral_term.detach()) > 0 or float(intercept_term.detach()) > 0
    # the multipliers and references carry no graph, the terms do
    assert not state.lambda_local_flux.requires_grad and not state.flux_integral_reference.requires_grad
    total.sum().backward()
    assert flux.grad is not None and torch.isfinite(flux.grad).all() and float(flux.grad.abs().max()) > 0


def test_fixture_meets_the_conditions_it_was_chosen_for(golden):
    d = golden("aim_point_optimizer_epochs")
    blocking = d["blocking_factors"][0]
    assert ((blocking > 0) & (blocking < 1)).any()                     # a partly blocked heliostat in the first epoch
    assert (d["local_flux_constraint"] != 0).any()
    assert (d["flux_integral_constraint"][1:] != 0).any() or (d["intercept_constraint"][1:] != 0).any()
    g32, g64 = d["grad"][0], d["grad_f64_epoch0"]
    assert g32.size == 12 and (np.sign(g32) == np.sign(g64)).all() and (g32 != 0).all()
    assert (np.abs(g32) >= np.abs(g32 - g64)).all()                    # the reference's own fp32 run leaves no element out


def _configuration():
    return dict(optimization=dict(initial_learning_rate=1e-3, tolerance=0.0, max_epoch=2, batch_size=50, log_step=0,
                                  early_stopping_delta=1e-4, early_stopping_patience=100, early_stopping_window=100),
                scheduler=dict(scheduler_type="exponential", gamma=0.9),
                constraints=dict(rho_flux_integral=1.0, rho_intercept=1.0, rho_local_flux=1.0, max_flux_density=1e5))


DDP = dict(rank=0, world_size=1, is_distributed=False, groups_to_ranks_mapping={0: [0]}, ranks_to_groups_mapping={0: [0]},
           heliostat_group_rank=0, heliostat_group_world_size=1)


def _optimizer(device):
    from artist_amd.optim import AimPointOptimizer
    return AimPointOptimizer(ddp_setup=DDP, scenario=types.SimpleNamespace(), optimization_configuration=_configuration(),
                             incident_ray_direction=torch.tensor([0.0, 1.0, 0.0, 0.0]), target_area_index=0,
                             ground_truth=torch.ones(8, 8), dni=800.0, bitmap_resolution=torch.tensor([8, 8]), device=device)


def test_a_loss_without_a_total_loss_is_a_type_error():
    """Only ``KLDivergenceLoss`` defines the total loss: anything else is refused before the scenario is touched (the empty
    namespace standing in for it would raise an AttributeError at the first use)."""
    from artist_amd import FocalSpotLoss, PixelLoss
    optimizer = _optimizer(torch.device("cuda", 0))
    for loss_definition in (PixelLoss(), FocalSpotLoss(scenario=None), torch.nn.MSELoss()):
        with pytest.raises(TypeError, match="KLDivergenceLoss only"):
            optimizer.optimize(loss_definition=loss_definition, device=torch.device("cuda", 0))


def test_no_cpu_fallback():
    from artist_amd import ArtistHipError, KLDivergenceLoss
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        _optimizer(CPU)
    optimizer = _optimizer(torch.device("cuda", 0))
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        optimizer.optimize(loss_definition=KLDivergenceLoss(), device=CPU)


def test_stand_ins_carry_what_the_optimiser_and_the_tutorial_read():
    from artist_amd.scene import HeliostatField, SolarTower, TowerTargetAreasCylindrical, TowerTargetAreasPlanar
    planar = TowerTargetAreasPlanar(["a", "b"], torch.zeros(2, 4), torch.zeros(2, 4), torch.tensor([[6.0, 5.0], [4.0, 3.0]]))
    cylinders = TowerTargetAreasCylindrical(["c"], torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1, 4), torch.tensor([2.0]),
                                            torch.tensor([7.0]), torch.tensor([1.5]))
    tower = SolarTower([planar, cylinders], device=CPU)
    assert [(areas is planar, row) for areas, row in tower.index_to_target_area] == [(True, 0), (True, 1), (False, 0)]
    assert len(SolarTower([planar], device=CPU).index_to_target_area) == 2
    groups = [types.SimpleNamespace(number_of_heliostats=n) for n in (4, 2)]
    field = HeliostatField(groups, device=CPU)
    assert field.number_of_heliostats_per_group.tolist() == [4, 2]
    # the target's plane dimensions as the optimiser reads them: planar, and arc length x height of a cylinder
    optimizer = _optimizer(torch.device("cuda", 0))
    optimizer.scenario = types.SimpleNamespace(solar_tower=tower)
    optimizer.target_area_index = 1
    assert optimizer._target_plane_dimensions().tolist() == [4.0, 3.0]
    optimizer.target_area_index = 2
    assert optimizer._target_plane_dimensions().tolist() == [3.0, 7.0]
