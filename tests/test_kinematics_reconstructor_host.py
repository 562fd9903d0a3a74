"""CPU suite: what ``artist_amd.optim.KinematicsReconstructor`` does on the host and in plain torch, against the reference's runs.

``tests/golden/kinematics_reconstructor_class_flux.npz`` and ``..._alignment.npz``
(tests/golden/generate_kinematics_reconstructor_golden.py) are ONE unmodified run each of the reference's
``KinematicsReconstructor.reconstruct_kinematics``, flux-driven with ``FocalSpotLoss`` and alignment-driven with ``AngleLoss``:
four of the six heliostats of test_blocking.h5 with four calibration samples each, three epochs, validation in every epoch.
Checked here, without a GPU: the exports, the refusals and defaults, the three losses on vectors against every recorded epoch, the
measured normals, the split - and that the fixtures are the cases they were chosen to be.  The epochs themselves run in
tests/test_gpu_kinematics_reconstructor.py.
"""
import json
import types

import numpy as np
import pytest
import torch

FLUX, ALIGNMENT = "kinematics_reconstructor_class_flux", "kinematics_reconstructor_class_alignment"
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
CONFIGURATION = dict(optimization={}, scheduler={})
EPS32 = float(np.finfo(np.float32).eps)


def test_the_names_are_exported():
    import artist_amd
    from artist_amd import kinematics_reconstructor, losses, optim
    assert optim.KinematicsReconstructor is artist_amd.KinematicsReconstructor is kinematics_reconstructor.KinematicsReconstructor
    for name in ("KinematicsReconstructor", "VectorLoss", "AngleLoss", "CosineSimilarityLoss"):
        assert name in optim.__all__ and hasattr(optim, name), name
    assert optim.AngleLoss is losses.AngleLoss and optim.VectorLoss is losses.VectorLoss
    assert optim.CosineSimilarityLoss is losses.CosineSimilarityLoss
    assert kinematics_reconstructor.KINEMATICS_RECONSTRUCTION_RAYTRACING == "raytracing"
    assert kinematics_reconstructor.KINEMATICS_RECONSTRUCTION_ALIGNMENT == "alignment"
    for method in ("prepare", "epoch_loss", "validate", "reconstruct_kinematics", "_synchronize_gradients_nested_ddp",
                   "_synchronize_reconstruction_across_ranks", "_compute_measured_normals"):
        assert callable(getattr(optim.KinematicsReconstructor, method)), method


def test_refusals_and_defaults():
    from artist_amd import ArtistHipError
    from artist_amd.optim import KinematicsReconstructor
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        KinematicsReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=CONFIGURATION, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="The kinematics reconstruction method 'flux' is unknown"):
        KinematicsReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=CONFIGURATION,
                                reconstruction_method="flux", device=torch.device("cuda", 0))
    reconstructor = KinematicsReconstructor(ddp_setup=DDP, scenario=None, data={}, optimization_configuration=CONFIGURATION,
                                            device=torch.device("cuda", 0))        # (nothing here touches the device)
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        reconstructor.reconstruct_kinematics(loss_definition=None, device=torch.device("cpu"))
    # the reference's defaults
    assert reconstructor.reconstruction_method == "raytracing" and reconstructor.bitmap_resolution.tolist() == [256, 256]
    assert reconstructor.dni is None
    assert KinematicsReconstructor(DDP, None, {}, CONFIGURATION, 800.0, "alignment", torch.tensor([64, 32]),
                                   device=torch.device("cuda", 0)).bitmap_resolution.tolist() == [64, 32]     # the reference's order
    from artist_amd import FocalSpotLoss, KLDivergenceLoss, PixelLoss
    assert isinstance(reconstructor.validation_loss_focal_spot, FocalSpotLoss) and isinstance(reconstructor.validation_loss_pixel, PixelLoss)
    assert isinstance(reconstructor.validation_loss_kl_div, KLDivergenceLoss)


def test_the_losses_on_vectors_reproduce_every_recorded_epoch(golden):
    """On CPU tensors, from the recorded normals.  The recorded values are fp32 results of the same formulas, so they are met to
    within fp32 rounding: a few ulp for the squared distance and for one minus the cosine (of numbers near one: an absolute
    bound), and for the angle those few ulp of the cosine divided by the sine - ``acos`` magnifies an error of its argument by
    ``1 / sin(angle)``."""
    from artist_amd.optim import AngleLoss, CosineSimilarityLoss, VectorLoss
    d = golden(ALIGNMENT)
    truth = torch.from_numpy(d["normals_measured_train"])
    for e in range(d["normals_predicted"].shape[0]):
        prediction = torch.from_numpy(d["normals_predicted"][e])
        angle = AngleLoss()(prediction=prediction, ground_truth=truth)
        assert angle.shape == (12,) and angle.dtype == torch.float32
        assert (np.abs(angle.numpy() - d["loss_per_sample"][e]) <= 8 * EPS32 / np.sin(d["loss_per_sample"][e])).all()
        cosine = CosineSimilarityLoss()(prediction=prediction, ground_truth=truth)
        np.testing.assert_allclose(cosine.numpy(), d["cosine_loss_per_sample"][e], rtol=0, atol=8 * EPS32)
        vector = VectorLoss()(prediction=prediction, ground_truth=truth, reduction_dimensions=(1,))
        np.testing.assert_allclose(vector.numpy(), d["vector_loss_per_sample"][e], rtol=8 * EPS32, atol=0)
    # the three agree with each other: for unit vectors |a - b|^2 = 2 (1 - cos), and cos(angle) = 1 - (1 - cos)
    # (both sides are differences of numbers near one: 8 ulp of one on the cosine, doubled, and as much for the unit lengths)
    np.testing.assert_allclose(vector.numpy(), 2 * cosine.numpy(), rtol=0, atol=32 * EPS32)
    np.testing.assert_allclose(np.cos(angle.numpy().astype(np.float64)), 1 - cosine.numpy().astype(np.float64), atol=8 * EPS32)
    with pytest.raises(ValueError, match="The vector loss expects 'reduction_dimensions' as keyword argument"):
        VectorLoss()(prediction=prediction, ground_truth=truth)
    # the angle of parallel vectors has no finite derivative: what the reconstructor's nan_to_num_ is there for
    same = truth[:2].clone().requires_grad_(True)
    AngleLoss()(prediction=same, ground_truth=truth[:2] * 3.0).sum().backward()
    assert not torch.isfinite(same.grad[:, :3]).all()
    # fourth components and lengths do not matter to the angle
    longer = prediction * 2.5
    longer[:, 3] = 7.0
    np.testing.assert_allclose(AngleLoss()(longer, truth).numpy(), angle.numpy(), rtol=0, atol=8 * EPS32 / np.sin(d["loss_per_sample"][-1]).min())


def test_the_measured_normals_are_the_recorded_ones(golden):
    from artist_amd.optim import KinematicsReconstructor
    d = golden(ALIGNMENT)
    group = types.SimpleNamespace(positions=torch.from_numpy(d["heliostat_positions"]))
    normals = KinematicsReconstructor._compute_measured_normals(
        group, torch.from_numpy(d["parser_focal_spots"]), torch.from_numpy(d["parser_incident_ray_directions"]),
        torch.from_numpy(d["parser_mask"]), torch.device("cpu"))
    assert normals.shape == (16, 4) and not normals[:, 3].any()
    np.testing.assert_allclose(normals.numpy(), d["normals_measured"], rtol=0, atol=4 * EPS32)
    np.testing.assert_allclose(normals.numpy(), d["normals_measured_f64"], rtol=0, atol=4 * EPS32)
    np.testing.assert_array_equal(d["normals_measured"][d["train_indices"]], d["normals_measured_train"])
    np.testing.assert_allclose(np.linalg.norm(normals.numpy()[:, :3], axis=1), 1.0, atol=4 * EPS32)


@pytest.mark.parametrize("name", [FLUX, ALIGNMENT])
def test_train_test_split_gives_the_recorded_split(golden, name):
    from artist_amd import training
    d = golden(name)
    split = training.train_test_split(*(torch.from_numpy(d[k]) for k in (
        "parser_mask", "parser_flux_measured", "parser_focal_spots", "parser_incident_ray_directions", "parser_motor_positions",
        "parser_target_area_indices")))
    np.testing.assert_array_equal(split.train_indices.numpy(), d["train_indices"])
    np.testing.assert_array_equal(split.test_indices.numpy(), d["test_indices"])
    np.testing.assert_array_equal(split.active_heliostats_mask_train.numpy(), d["mask_train"])
    np.testing.assert_array_equal(split.active_heliostats_mask_test.numpy(), d["mask_test"])
    assert (split.number_of_train_samples, split.number_of_test_samples, split.number_of_samples_per_heliostat) == tuple(d["split_counts"])
    np.testing.assert_array_equal(split.motor_positions_train.numpy(), d["parser_motor_positions"][d["train_indices"]])


@pytest.mark.parametrize("name", [FLUX, ALIGNMENT])
def test_the_fixture_is_the_case_it_was_chosen_to_be(golden, name):
    d = golden(name)
    mask = d["parser_mask"]
    active = np.nonzero(mask)[0]
    inactive = np.nonzero(mask == 0)[0]
    assert set(mask.tolist()) == {0, 4} and len(mask) == 6 and len(active) == 4 and tuple(d["split_counts"]) == (3, 1, 4)
    assert any(mask[h] == 0 and (active < h).any() and (active > h).any() for h in range(len(mask)))      # an inactive one between active ones
    assert d["points_per_facet"].tolist() == [10, 10] and int(d["n_rays"]) == 3 and d["resolution"].tolist() == [64, 64]
    assert str(d["method"]) == ("raytracing" if name == FLUX else "alignment")
    config = json.loads(str(d["configuration"]))
    assert config["optimization"]["max_epoch"] == 2 and config["optimization"]["log_step"] == 1 and config["optimization"]["tolerance"] == 0.0
    epochs = d["rotation_after"].shape[0]
    assert epochs == 3 and d["history_total_loss"].shape == (3,)
    np.testing.assert_allclose(d["lr"], config["optimization"]["initial_learning_rate_rotation_deviation"] * config["scheduler"]["gamma"] ** np.arange(3),
                               rtol=1e-12)
    assert len(d["validated_epochs"]) > 1                                          # more than one validated epoch
    for key in ("test_focal_spot_loss", "test_pixel_loss", "test_kl_div"):
        assert d[key].shape == (len(d["validated_epochs"]), 4) and np.isfinite(d[key]).all()
    assert d["grad"].shape == (3, 6, 4) and np.isfinite(d["grad"]).all() and np.isfinite(d["grad_f64_epoch0"]).all()   # no NaN
    assert not d["grad"][:, inactive].any() and (d["grad"][:, active] != 0).all()
    np.testing.assert_array_equal(d["rotation_after"][:-1], d["rotation_start"][1:])
    np.testing.assert_array_equal(d["rotation_after"][:, inactive], d["rotation_start"][:, inactive])
    assert np.isinf(d["final_loss"][inactive]).all() and np.array_equal(d["final_loss"][active], d["loss_per_heliostat"][-1])
    np.testing.assert_allclose(d["loss_per_heliostat"].astype(np.float64).mean(axis=1), d["total_loss"], rtol=1e-6)
    per_sample = d["loss_per_sample"].astype(np.float64)
    distance = np.abs(per_sample[0] - d["loss_per_sample_f64_epoch0"])
    if name == FLUX:
        # the median sample of every heliostat stands clear of its neighbours: fp32 and fp64 (and another fp32 evaluation
        # order) pick the same one
        assert d["flux_predicted"].shape == (3, 12, 64, 64) and d["distortions_train_u"].shape == (12, 3, 400)
        assert int(d["seed_train"]) == 0 and int(d["seed_test"]) == 7 and d["distortions_test_u"].shape == (4, 3, 400)
        blocks = np.sort(per_sample.reshape(3, 4, 3), axis=2)
        np.testing.assert_array_equal(blocks[..., 1].astype(np.float32), d["loss_per_heliostat"])
        gap = np.minimum(blocks[..., 1] - blocks[..., 0], blocks[..., 2] - blocks[..., 1])
        assert (gap >= 10 * distance.max()).all(), (gap.min(), distance.max())
    else:
        # the angles are large enough for acos in fp32
        assert (distance / np.abs(d["loss_per_sample_f64_epoch0"])).max() < 1e-2
        assert float(d["sigma"]) == 3e-2 and "distortions_train_u" not in d and int(d["seed_test"]) == 7
        np.testing.assert_allclose(per_sample.reshape(3, 4, 3).mean(axis=2), d["loss_per_heliostat"], rtol=1e-6)
        assert d["normals_predicted"].shape == (3, 12, 4) and d["normals_measured"].shape == (16, 4)
