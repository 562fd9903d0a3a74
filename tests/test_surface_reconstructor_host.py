"""CPU suite: what ``artist_amd.optim.SurfaceReconstructor`` does on the host and in plain torch, against the reference's run.

``tests/golden/surface_reconstructor_class_epochs.npz`` (tests/golden/generate_surface_reconstructor_golden.py) is ONE unmodified
run of the reference's ``SurfaceReconstructor.reconstruct_surfaces``: three of the six heliostats of test_blocking.h5 with four
calibration samples each, three epochs, the flux-integral constraint active.  Checked here, without a GPU: the train/test
split, ``reduce_loss_per_sample``, the constraint term on CPU tensors against every recorded epoch, the multiplier update, the
edge lock, the in-memory parser, the two refusals - and that the fixture is the case it was chosen to be.  The epoch itself
runs in tests/test_gpu_surface_reconstructor.py.
"""
import json
from functools import partial

import numpy as np
import pytest
import torch

NAME = "surface_reconstructor_class_epochs"
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)


def _split(mask, **kw):
    from artist_amd import training
    n = int(sum(mask))
    return training.train_test_split(active_heliostats_mask=torch.tensor(mask, dtype=torch.int32), flux_measured=torch.arange(n).view(n, 1, 1) * torch.ones(n, 2, 2),
                                     focal_spots_measured=torch.zeros(n, 4), incident_ray_directions=torch.arange(n).view(n, 1) * torch.ones(n, 4),
                                     motor_positions=torch.zeros(n, 2), target_area_indices=torch.arange(n), **kw)


def test_train_test_split_gives_the_recorded_split(golden):
    d = golden(NAME)
    split = _split(d["parser_mask"].tolist())
    assert split.train_indices.device.type == "cpu" and split.test_indices.device.type == "cpu"
    np.testing.assert_array_equal(split.train_indices.numpy(), d["train_indices"])
    np.testing.assert_array_equal(split.test_indices.numpy(), d["test_indices"])
    np.testing.assert_array_equal(split.active_heliostats_mask_train.numpy(), d["mask_train"])
    np.testing.assert_array_equal(split.active_heliostats_mask_test.numpy(), d["mask_test"])
    assert (split.number_of_train_samples, split.number_of_test_samples, split.number_of_samples_per_heliostat) == tuple(d["split_counts"])
    # every per-sample tensor is cut by the same indices
    np.testing.assert_array_equal(split.target_area_indices_train.numpy(), d["train_indices"])
    np.testing.assert_array_equal(split.flux_measured_test[:, 0, 0].numpy(), d["test_indices"])
    np.testing.assert_array_equal(split.incident_ray_directions_train[:, 0].numpy(), d["train_indices"])


@pytest.mark.parametrize("mask, train, test, masks", [
    # two samples per heliostat: int(2 * 0.25) = 0 -> at least one test sample; the first is the training sample
    ([2, 0, 2], [0, 2], [1, 3], ([1, 0, 1], [1, 0, 1])),
    # five: int(1.25) = 1 test sample from the end of each block
    ([0, 5, 5, 0], [0, 1, 2, 3, 5, 6, 7, 8], [4, 9], ([0, 4, 4, 0], [0, 1, 1, 0])),
])
def test_train_test_split_on_other_masks(mask, train, test, masks):
    split = _split(mask)
    assert split.train_indices.tolist() == train and split.test_indices.tolist() == test
    assert split.active_heliostats_mask_train.tolist() == masks[0] and split.active_heliostats_mask_test.tolist() == masks[1]
    assert split.number_of_train_samples + split.number_of_test_samples == split.number_of_samples_per_heliostat == max(mask)
    assert split.target_area_indices_test.tolist() == test
    half = _split([4, 4], test_fraction=0.5)                       # another fraction: two from the end
    assert half.test_indices.tolist() == [2, 3, 6, 7] and half.number_of_train_samples == 2


def test_reduce_loss_per_sample():
    from artist_amd.training import reduce_loss_per_sample
    loss = torch.tensor([1.0, 2.0, 6.0, 10.0, 20.0, 60.0, 7.0])
    assert reduce_loss_per_sample(loss, 3, partial(torch.mean, dim=-1)).tolist() == [3.0, 30.0]        # the seventh has no heliostat
    assert reduce_loss_per_sample(loss, 3, partial(torch.median, dim=-1)).tolist() == [2.0, 20.0]      # (values of a named tuple)
    assert reduce_loss_per_sample(loss[:6], 1, partial(torch.mean, dim=-1)).tolist() == loss[:6].tolist()
    grad_in = loss[:6].clone().requires_grad_(True)
    reduce_loss_per_sample(grad_in, 3, partial(torch.mean, dim=-1)).sum().backward()
    assert torch.allclose(grad_in.grad, torch.full((6,), 1 / 3))


def test_flux_integral_constraint_reproduces_every_recorded_epoch(golden):
    from artist_amd import flux_integral_constraint
    d = golden(NAME)
    config = json.loads(str(d["configuration"]))["constraints"]
    rho, tolerance = config["rho_flux_integral"], config["energy_tolerance"]
    samples = int(d["split_counts"][0])
    for e in range(d["cp_after"].shape[0]):
        multiplier = torch.from_numpy(d["lambda_before"][e])
        term, relative, violation = flux_integral_constraint(torch.from_numpy(d["cropped_sums"][e]), torch.from_numpy(d["reference_after"][e]),
                                                             multiplier, rho, tolerance, samples, float(d["epsilon"]))
        np.testing.assert_allclose(term.numpy(), d["constraint"][e], rtol=1e-6, atol=0)
        np.testing.assert_allclose(relative.numpy(), d["relative_differences"][e], rtol=1e-6, atol=0)
        np.testing.assert_allclose(violation.numpy(), d["violation"][e], rtol=1e-6, atol=0)
        after = torch.clamp(multiplier + rho * violation, min=0.0)
        np.testing.assert_allclose(after.numpy(), d["lambda_after"][e], rtol=1e-6, atol=0)
    # a number as the multiplier (the reference starts from 0.0), and a sample that gained flux violates nothing at tolerance 0
    term, relative, violation = flux_integral_constraint(torch.tensor([11.0, 9.0]), torch.tensor([10.0, 10.0]), 0.0, 2.0, 0.0, 1, 1e-12)
    assert violation.tolist() == [0.0, pytest.approx(0.1)] and term.tolist() == [0.0, pytest.approx(0.01)]
    # the term's gradient w.r.t. the sums: -(lambda + rho v) / (reference + eps) / samples, where a sample violates
    sums = torch.tensor([9.0, 9.5, 10.5, 8.0], requires_grad=True)
    term, _, violation = flux_integral_constraint(sums, torch.full((4,), 10.0), torch.tensor([0.5, 0.25]), 2.0, 0.0, 2, 1e-12)
    term.sum().backward()
    want = -(torch.tensor([0.5, 0.25]) + 2.0 * violation.detach()).repeat_interleave(2) / 10.0 / 2 * torch.tensor([1.0, 1.0, 0.0, 1.0])
    assert torch.allclose(sums.grad, want)


def test_the_edge_lock_has_the_recorded_zero_pattern(golden):
    from artist_amd.optim import SurfaceReconstructor
    d = golden(NAME)
    recorded = d["grad_locked"][0]                                 # (the rows of the heliostats that have samples)
    gradients = torch.ones(recorded.shape)
    locked = SurfaceReconstructor.lock_control_points_on_outer_edges(gradients=gradients)
    assert locked is not gradients and bool((gradients == 1).all())                 # a copy
    np.testing.assert_array_equal(locked.numpy() == 0, recorded == 0)
    inner = locked[:, :, 1:-1, 1:-1]
    assert bool((inner == 1).all()) and bool((locked[..., 2] == 1).all()) and not bool(locked[:, :, 0, :, :2].any())


def test_the_in_memory_parser_round_trips(golden):
    from artist_amd import CalibrationSamples
    from artist_amd.scene import HeliostatField, Scenario
    d = golden(NAME)
    six = tuple(torch.from_numpy(d[k]) for k in ("parser_flux_measured", "parser_focal_spots", "parser_incident_ray_directions",
                                                 "parser_motor_positions", "parser_mask", "parser_target_area_indices"))
    groups = [object(), object()]
    field = HeliostatField.__new__(HeliostatField)
    field.heliostat_groups = groups
    scenario = Scenario(None, None, None, field)
    other = tuple(t.clone() + 1 for t in six)
    parser = CalibrationSamples([six, other])
    for group, want in zip(groups, (six, other)):
        got = parser.parse_data_for_reconstruction(heliostat_data_mapping=[], heliostat_group=group, scenario=scenario,
                                                   bitmap_resolution=torch.tensor([64, 64]), device=torch.device("cpu"))
        assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(got, want))
    single = CalibrationSamples(six)                                               # one group: the six tensors themselves
    field.heliostat_groups = groups[:1]
    assert all(torch.equal(a, b) for a, b in zip(single.parse_data_for_reconstruction([], groups[0], scenario), six))
    with pytest.raises(ValueError, match="six tensors"):
        CalibrationSamples(six[:5])


def test_refusals():
    from artist_amd import ArtistHipError
    from artist_amd.optim import SurfaceReconstructor
    configuration = dict(optimization={}, scheduler={}, constraints={})
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        SurfaceReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=configuration, device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="plot"):
        SurfaceReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=configuration, plot_results=True,
                             device=torch.device("cuda", 0))
    reconstructor = SurfaceReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=configuration,
                                         device=torch.device("cuda", 0))           # (nothing here touches the device)
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        reconstructor.reconstruct_surfaces(loss_definition=None, device=torch.device("cpu"))
    # the reference's defaults
    assert reconstructor.number_of_surface_points.tolist() == [50, 50] and reconstructor.bitmap_resolution.tolist() == [256, 256]
    assert reconstructor.epsilon == 1e-12 and reconstructor.dni is None


def test_the_names_are_exported():
    import artist_amd
    from artist_amd import optim, training
    assert optim.SurfaceReconstructor is artist_amd.SurfaceReconstructor and "SurfaceReconstructor" in optim.__all__
    for name in ("TrainTestSplit", "train_test_split", "reduce_loss_per_sample"):
        assert name in training.__all__ and hasattr(training, name)


def test_the_fixture_is_the_case_it_was_chosen_to_be(golden):
    d = golden(NAME)
    mask = d["parser_mask"]
    active = np.nonzero(mask)[0]
    assert set(mask.tolist()) == {0, 4} and len(active) == 3 and len(mask) == 6
    assert tuple(d["split_counts"]) == (3, 1, 4)
    assert any(mask[h] == 0 and (active < h).any() and (active > h).any() for h in range(len(mask)))
    assert d["points_per_facet"].tolist() == [10, 10] and int(d["n_rays"]) == 3 and d["resolution"].tolist() == [64, 64]
    assert (d["parser_flux_measured"].sum(axis=(1, 2)) > 0).all()
    incident = d["parser_incident_ray_directions"].reshape(3, 4, 4)
    assert all(len({tuple(row) for row in incident[h].tolist()}) == 4 for h in range(3))
    assert len(set(d["parser_target_area_indices"][d["train_indices"]].tolist())) >= 2
    config = json.loads(str(d["configuration"]))
    assert config["optimization"]["max_epoch"] == 2 and d["cp_after"].shape[0] == 3
    assert config["scheduler"]["scheduler_type"] == "exponential"
    assert config["constraints"]["weight_smoothness"] == config["constraints"]["weight_ideal_surface"] == 0.005
    np.testing.assert_allclose(d["lr"], config["optimization"]["initial_learning_rate"] * config["scheduler"]["gamma"] ** np.arange(3), rtol=1e-12)
    assert len(d["validated_epochs"]) > 1                                          # validation ran in more than one epoch
    assert (d["constraint"] != 0).any() and (d["lambda_after"] != 0).any()           # the constraint acts, the multiplier moves
    np.testing.assert_array_equal(d["lambda_after"][:-1], d["lambda_before"][1:])
    np.testing.assert_array_equal(d["reference_after"][0], d["cropped_sums"][0])     # the first epoch's sums are the reference
    np.testing.assert_array_equal(d["reference_after"][1:], d["reference_before"][1:])
    # every free element of the locked gradient of the first epoch (stored: the rows of the heliostats that have samples) is
    # larger than its own fp32-vs-fp64 difference
    g32, g64 = d["grad_locked"][0], d["grad_locked_f64_epoch0"]
    assert g32.shape[0] == len(active) and d["cp_after"].shape[1] == len(active) and d["cp_start_epoch0"].shape[0] == len(mask)
    free = np.ones(g32.shape, dtype=bool)
    for edge in (free[:, :, 0], free[:, :, -1], free[:, :, :, 0], free[:, :, :, -1]):
        edge[..., :2] = False
    assert not g32[~free].any() and not g64[~free].any()
    assert (np.abs(g32[free]) > np.abs(g32[free].astype(np.float64) - g64[free])).all()
    # the returned values: inf exactly where no heliostat was reconstructed, histories of three epochs
    assert np.isinf(d["final_loss"][mask == 0]).all() and np.isfinite(d["final_loss"][active]).all()
    np.testing.assert_allclose(d["final_loss"][active], d["total_loss_per_heliostat"][-1], rtol=1e-6)
    for key in ("total_loss", "flux_loss", "smoothness_regularizer", "ideal_regularizer", "flux_integral", "flux_integral_constraint"):
        assert d[f"history_{key}"].shape == (3,)
