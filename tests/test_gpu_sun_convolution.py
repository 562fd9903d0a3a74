"""The convolved sun on the GPU: one chief ray per point and a Gaussian window per bitmap against the sampled
tracer (the acceptance test), through ``HeliostatRayTracer`` (``Sun.integration = "convolved"``), and inside a captured epoch of
``SurfaceReconstructor``."""
import functools

import pytest
import torch

import artist_amd
from artist_amd import HeliostatRayTracer, ops, optics, scene
from artist_amd.flux import blur_flux

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DDP = dict(rank=0, world_size=1, is_distributed=False, is_nested=False, process_subgroup=None, groups_to_ranks_mapping={0: [0]},
           ranks_to_groups_mapping={0: [0]}, heliostat_group_rank=0, heliostat_group_world_size=1)
VARIANCE = 4.3681e-6


# ---- 4. against the sampled tracer ---------------------------------------------------------------------------------------------
POSITIONS = [(5.0, 60.0, 2.0), (70.0, 50.0, 2.0), (-90.0, 140.0, 2.0)]          # slant ranges of 80, 101 and 175 m
RAYS = 100
SIDE = 100


@functools.lru_cache(maxsize=None)
def sampled_and_convolved():
    """Three flat mirrors of 3.2 m x 2.5 m, 100 x 100 points each, whose point p aims at centre + 0.3 (p - position): two
    independent R = 100 samples, the convolved bitmap, and the convolved bitmap with an isotropic window of the same trace."""
    f64 = torch.float64
    position = torch.tensor(POSITIONS, dtype=f64)
    e, n = torch.meshgrid(torch.linspace(-1.6, 1.6, SIDE, dtype=f64), torch.linspace(-1.25, 1.25, SIDE, dtype=f64), indexing="ij")
    offsets = torch.stack((e.reshape(-1), n.reshape(-1), torch.zeros(SIDE * SIDE, dtype=f64)), dim=-1)
    points = position[:, None, :] + offsets[None]
    centre = torch.tensor([0.0, 0.0, 55.0], dtype=f64)
    incident = torch.nn.functional.normalize(torch.tensor([0.2, 0.5, -0.8], dtype=f64), dim=0)
    aim = centre + 0.3 * offsets[None].expand_as(points)
    normals = torch.nn.functional.normalize(torch.nn.functional.normalize(aim - points, dim=-1) - incident, dim=-1)
    H, P = points.shape[:2]
    points = torch.cat((points, torch.ones(H, P, 1, dtype=f64)), dim=-1).float().to(DEV)
    normals = torch.cat((normals, torch.zeros(H, P, 1, dtype=f64)), dim=-1).float().to(DEV)
    incident = torch.cat((incident, torch.zeros(1, dtype=f64))).float().to(DEV).repeat(H, 1)
    targets = torch.zeros(H, dtype=torch.long, device=DEV)
    tables = (torch.tensor([[0.0, 0.0, 55.0, 1.0]], device=DEV), torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV),
              torch.tensor([[8.0, 8.0]], device=DEV))
    sigma = VARIANCE ** 0.5

    def trace(u, e_, magnitude):
        return artist_amd.trace_rays(points, normals, incident, u, e_, targets, *tables, ray_magnitude=magnitude, extinction=0.0,
                                     reflectivity=1.0, resolution=(256, 256))[0]

    samples = []
    for seed in (101, 202):
        u, e_ = ops.sample_distortions(range(H), RAYS, P, seed, (0.0, 0.0), ((sigma, 0.0), (0.0, sigma)), DEV).permute(3, 0, 1, 2)
        samples.append(trace(u, e_, 1.0).double().cpu())
    zeros = torch.zeros((H, 1, P, 2), device=DEV)
    sharp = trace(zeros[..., 0], zeros[..., 1], float(RAYS))
    covariance = optics.sun_image_covariance(points, normals, incident, targets, *tables,
                                             torch.tensor([VARIANCE, 0.0, VARIANCE], device=DEV), (256, 256))
    half_trace = (covariance[:, 0] + covariance[:, 2]) / 2
    isotropic = torch.stack((half_trace, torch.zeros_like(half_trace), half_trace), dim=1)
    return (samples[0], samples[1], blur_flux(sharp, covariance).double().cpu(), blur_flux(sharp, isotropic).double().cpu(),
            covariance.cpu())


def distance(a, b):
    return (a - b).flatten(1).norm(dim=1)


def test_convolved_sun_against_two_samples():
    """Per heliostat ||conv - MC_i|| <= 0.80 ||MC_1 - MC_2||: a noise-free truth scores 1/sqrt(2) = 0.707 against a noisy sample
    (the oracle gave 0.69 to 0.73 on these inputs, the statistic's own scatter is about 1 %), so 0.80 leaves the method a
    systematic error of at most 0.37 of the sampling noise of 1e6 rays per heliostat.  The totals agree to 1e-4."""
    mc1, mc2, conv, _, covariance = sampled_and_convolved()
    noise = distance(mc1, mc2)
    r1, r2 = distance(conv, mc1) / noise, distance(conv, mc2) / noise
    print("covariances (rr, rc, cc) px^2:", covariance.tolist())
    print("||MC1 - MC2|| / ||MC||:", (noise / mc1.flatten(1).norm(dim=1)).tolist())
    print("||conv - MC1|| / ||MC1 - MC2||:", r1.tolist(), " against MC2:", r2.tolist())
    totals = [(float(conv[h].sum()), float(mc[h].sum())) for h in range(3) for mc in (mc1, mc2)]
    print("totals (conv, MC):", totals)
    assert (r1 <= 0.80).all() and (r2 <= 0.80).all()
    for got, want in totals:
        assert abs(got - want) <= 1e-4 * want


def test_a_window_of_the_wrong_shape_is_caught():
    """The control: the isotropic window of the same trace scores above 2.0 on all three (2.5, 6.8 and 3.2 on the CPU)."""
    mc1, mc2, _, isotropic, _ = sampled_and_convolved()
    noise = distance(mc1, mc2)
    r1, r2 = distance(isotropic, mc1) / noise, distance(isotropic, mc2) / noise
    print("isotropic window: ||conv - MC1|| / ||MC1 - MC2||:", r1.tolist(), " against MC2:", r2.tolist())
    assert (r1 > 2.0).all() and (r2 > 2.0).all()


# ---- 5. through the classes --------------------------------------------------------------------------------------------------
RES = (64, 48)          # (columns, rows)
N_RAYS = 20
TARGETS = dict(target_centers=((0.0, 0.0, 55.0, 1.0), (1.0, 0.0, 47.0, 1.0)), target_normals=((0.0, 1.0, 0.0, 0.0),) * 2,
               target_dims=((8.0, 8.0), (6.0, 5.0)))


def field(optical_errors=None, **kwargs):
    scenario, _ = scene.build_synthetic_scenario(3, n_rays=N_RAYS, n_cp=(6, 6), n_eval=16, device=DEV, **TARGETS, **kwargs)
    group = scenario.heliostat_field.heliostat_groups[0]
    if optical_errors is not None:
        group.optical_errors = optical_errors
    mask = torch.ones(3, dtype=torch.int32, device=DEV)
    group.activate_heliostats(mask)
    targets = torch.tensor([0, 1, 0], dtype=torch.long, device=DEV)
    incident = torch.nn.functional.normalize(torch.tensor([[0.0, 1.0, -0.2, 0.0], [0.2, 0.9, -0.4, 0.0], [-0.1, 0.8, -0.5, 0.0]]),
                                             dim=1).to(DEV)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(targets), incident, mask)
    return scenario, group, mask, targets, incident


def sun_covariance(tril):
    """(C_uu, C_ue, C_ee) of C = L L^T, element by element."""
    return torch.stack((tril[0, 0] * tril[0, 0], tril[0, 0] * tril[1, 0], tril[1, 0] * tril[1, 0] + tril[1, 1] * tril[1, 1]))


def tracer_of(scenario, group):
    return HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=torch.tensor(RES))


def by_hand(scenario, group, tracer, targets, incident, angular):
    planar = scenario.solar_tower.target_areas[0]
    tables = (planar.centers, planar.normals, planar.dimensions)
    points, normals = group.active_surface_points, group.active_surface_normals
    zeros = torch.zeros((3, 1, points.shape[1], 2), device=DEV)
    sharp = artist_amd.trace_rays(points, normals, incident, zeros[..., 0], zeros[..., 1], targets, *tables,
                                  ray_magnitude=float(N_RAYS), extinction=0.0, reflectivity=0.935, resolution=RES,
                                  points_per_facet=tracer._points_per_facet(points))[0]
    return blur_flux(sharp, optics.sun_image_covariance(points, normals, incident, targets, *tables, angular, RES))


def test_the_tracer_assembles_the_ops():
    scenario, group, mask, targets, incident = field()
    sun = scenario.light_sources.light_source_list[0]
    before = tracer_of(scenario, group)
    sampled = before.trace_rays(incident, mask, targets)[0]
    sun.integration = "convolved"
    tracer = tracer_of(scenario, group)
    assert tracer.integration == "convolved" and tracer.distortions_dataset.distortions_u.shape == (3, 1, group.active_surface_points.shape[1])
    assert tracer._max_scatter_angle() == 0.0                  # the cone of a heliostat's rays, for the blocking cull
    flux, intercept, on_target, blocking = tracer.trace_rays(incident, mask, targets)
    angular = torch.tensor([VARIANCE, 0.0, VARIANCE], device=DEV)
    tril = sun.distribution.scale_tril.float()
    sun_c = sun_covariance(tril)
    assert torch.allclose(sun_c, angular, rtol=1e-6, atol=0)
    want = by_hand(scenario, group, tracer, targets, incident, sun_c)
    assert flux.shape == (3, RES[1], RES[0]) and torch.equal(flux, want) and float(flux.sum()) > 0
    assert ops.bitmap_moments(flux) is None
    # the expectation of the sampled bitmap: the same total, up to the sample's own noise and what leaves the target's edge
    print("totals convolved / sampled:", flux.flatten(1).sum(1).tolist(), sampled.flatten(1).sum(1).tolist())
    assert torch.allclose(flux.flatten(1).sum(1), sampled.flatten(1).sum(1), rtol=2e-2)
    # per target: the sum of the heliostats' blurred bitmaps, the same bits
    per_target = tracer.trace_rays_per_target(incident, mask, targets)[0]
    assert per_target.shape == (2, RES[1], RES[0])
    assert torch.equal(per_target, tracer.get_bitmaps_per_target(flux, targets))
    # a gradient reaches the surfaces through the blur
    points = group.active_surface_points.detach().clone().requires_grad_(True)
    group.active_surface_points = points
    weights = torch.linspace(0.5, 1.5, RES[0] * RES[1], device=DEV).reshape(RES[1], RES[0])
    (tracer.trace_rays(incident, mask, targets)[0] * weights).sum().backward()
    assert torch.isfinite(points.grad).all() and float(points.grad.abs().max()) > 0
    group.active_surface_points = points.detach()
    # sampled again: the bits of the tracer that was built before, for the same seed - and those of the op on its sample
    sun.integration = "sampled"
    again = tracer_of(scenario, group)
    assert again.integration == "sampled"
    flux_again = again.trace_rays(incident, mask, targets)[0]
    assert torch.equal(flux_again, sampled)
    planar = scenario.solar_tower.target_areas[0]
    data = again.distortions_dataset
    op = artist_amd.trace_rays(group.active_surface_points, group.active_surface_normals, incident, data.distortions_u,
                               data.distortions_e, targets, planar.centers, planar.normals, planar.dimensions, ray_magnitude=1.0,
                               extinction=0.0, reflectivity=0.935, resolution=RES,
                               points_per_facet=again._points_per_facet(group.active_surface_points))[0]
    assert torch.equal(flux_again, op)


def test_optical_errors_widen_the_window():
    errors = torch.tensor([0.0, 1e-3, 2e-3], device=DEV)
    scenario, group, mask, targets, incident = field(optical_errors=errors)
    scenario.light_sources.light_source_list[0].integration = "convolved"
    tracer = tracer_of(scenario, group)
    flux = tracer.trace_rays(incident, mask, targets)[0]
    tril = scenario.light_sources.light_source_list[0].distribution.scale_tril.float()
    C = sun_covariance(tril)
    variance = errors * errors
    angular = torch.stack((C[0] + variance, C[1].expand_as(variance), C[2] + variance), dim=1)
    assert torch.equal(flux, by_hand(scenario, group, tracer, targets, incident, angular))
    plain = by_hand(scenario, group, tracer, targets, incident, C)
    assert torch.equal(flux[0], plain[0]) and not torch.equal(flux[1], plain[1])
    assert float(flux[2].max()) < float(plain[2].max())


def test_cylindrical_targets_are_refused():
    scenario, group, mask, targets, incident = field()
    tower = scenario.solar_tower
    one = lambda *v: torch.tensor([v], device=DEV)  # noqa: E731
    cylinder = scene.TowerTargetAreasCylindrical(names=["c"], centers=one(0.0, 0.0, 50.0, 1.0), normals=one(0.0, 1.0, 0.0, 0.0),
                                                 axes=one(0.0, 0.0, 1.0, 0.0), radii=torch.tensor([3.0], device=DEV),
                                                 heights=torch.tensor([6.0], device=DEV), opening_angles=torch.tensor([2.0], device=DEV))
    tower.target_areas = [tower.target_areas[0], cylinder]
    scenario.light_sources.light_source_list[0].integration = "convolved"
    tracer = tracer_of(scenario, group)
    assert tracer.trace_rays(incident, mask, targets)[0].shape[0] == 3            # planar targets of such a tower are served
    with pytest.raises(ValueError, match="planar target areas only"):
        tracer.trace_rays(incident, mask, torch.tensor([0, 2, 0], dtype=torch.long, device=DEV))


# ---- 6. a captured epoch -----------------------------------------------------------------------------------------------------
EPOCHS = 3          # the loop runs epochs 0 .. max_epoch inclusive, like the reference's: max_epoch = EPOCHS - 1


def reconstruct(epoch_graph):
    from artist_amd import CalibrationSamples, PixelLoss
    from artist_amd.optim import SurfaceReconstructor
    heliostats, samples = 3, 2
    scenario, _ = scene.build_synthetic_scenario(heliostats, n_rays=N_RAYS, n_cp=(6, 6), n_eval=16, device=DEV)
    scenario.light_sources.light_source_list[0].integration = "convolved"
    n = heliostats * samples
    suns = torch.tensor([[0.0, 0.8, -0.6, 0.0], [0.1, 1.0, -0.2, 0.0]])
    incident = torch.nn.functional.normalize(suns, dim=1).repeat(heliostats, 1).to(DEV)
    measured = (torch.rand((n, 64, 64), generator=torch.Generator().manual_seed(1)) + 0.1).to(DEV)
    six = (measured, torch.zeros(n, 4, device=DEV), incident, torch.zeros(n, 2, device=DEV),
           torch.full((heliostats,), samples, dtype=torch.int32, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV))
    configuration = dict(optimization=dict(initial_learning_rate=1e-6, tolerance=0.0, max_epoch=EPOCHS - 1, batch_size=30, log_step=0,
                                           early_stopping_delta=1e-9, early_stopping_patience=10 ** 6, early_stopping_window=10),
                         scheduler=dict(scheduler_type="exponential", gamma=0.999),
                         constraints=dict(rho_flux_integral=1.0, energy_tolerance=0.01, weight_smoothness=0.005, weight_ideal_surface=0.005))
    reconstructor = SurfaceReconstructor(
        ddp_setup=DDP, scenario=scenario, data={"data_parser": CalibrationSamples(six), "heliostat_data_mapping": []},
        optimization_configuration=configuration, number_of_surface_points=torch.tensor([16, 16]),
        bitmap_resolution=torch.tensor([64, 64]), device=DEV, epoch_graph=epoch_graph)
    group = scenario.heliostat_field.heliostat_groups[0]
    start = group.nurbs_control_points.detach().clone()
    final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=PixelLoss(), device=DEV)
    torch.cuda.synchronize()
    return final_loss, histories[0][0], group.nurbs_control_points.detach().clone(), start


def test_a_convolved_epoch_is_captured_and_replayed():
    loss_e, history_e, points_e, start = reconstruct(False)
    loss_r, history_r, points_r, _ = reconstruct(True)
    print("total loss per epoch:", history_e["total_loss"], " replayed:", history_r["total_loss"])
    for key in ("total_loss", "flux_loss"):
        assert len(history_e[key]) == EPOCHS and history_e[key] == history_r[key], (key, history_e[key], history_r[key])
    assert torch.equal(loss_e, loss_r) and torch.equal(points_e, points_r)
    assert torch.isfinite(points_e).all() and not torch.equal(points_e, start)
