"""Per-heliostat optics, the part that needs no GPU: ``artist_amd.optics`` against closed forms, the group's attributes, every
refusal and its message, the rehearsal of the GPU law test on the restated stream, and that floats and ``None`` reach the
kernel call exactly as they did."""
import math

import numpy as np
import pytest
import torch

import heliostat_optics_ref as ref
from artist_amd import HeliostatRayTracer, _lib, ops, optics, scene
from artist_amd._memo import Memo
from artist_amd.sampling import DistortionsDataset


# ---- optics ------------------------------------------------------------------------------------------------------------------
def test_slant_ranges_and_transmittance_against_closed_forms():
    positions = torch.tensor([[0.0, 100.0, 0.0, 1.0], [300.0, 400.0, 5.0, 1.0], [-1200.0, 900.0, 2.0, 1.0]])
    centres = torch.tensor([[0.0, 0.0, 55.0, 1.0]]).repeat(3, 1)
    d = optics.slant_ranges(positions, centres)
    want = np.linalg.norm(positions.numpy()[:, :3].astype(np.float64) - centres.numpy()[:, :3], axis=1)
    np.testing.assert_allclose(d.numpy(), want, rtol=1e-6)
    np.testing.assert_allclose(optics.atmospheric_transmittance(d, ("exponential", 0.15)).numpy(), np.exp(-0.15 * want / 1e3), rtol=1e-6)
    c = (0.006789, 0.1046, -0.017, 0.002845)
    km = want / 1e3
    np.testing.assert_allclose(optics.atmospheric_transmittance(d, ("polynomial", c)).numpy(),
                               1.0 - np.clip(sum(ck * km ** k for k, ck in enumerate(c)), 0.0, 1.0), rtol=1e-6)
    far = torch.tensor([50_000.0, 0.0])
    assert optics.atmospheric_transmittance(far, ("polynomial", (0.0, 0.1))).tolist() == [0.0, 1.0]      # the loss is clamped to [0, 1]
    assert optics.atmospheric_transmittance(far, ("polynomial", (-0.5,))).tolist() == [1.0, 1.0]
    assert torch.equal(optics.atmospheric_transmittance(d, lambda r: 1.0 / (1.0 + r)), 1.0 / (1.0 + d))
    for bad, message in ((("gaussian", 1.0), "unknown attenuation model"), (("exponential", -1.0), "beta_per_km"),
                         (("polynomial", ()), "at least one coefficient"), (3.0, "an attenuation model is")):
        with pytest.raises(ValueError, match=message):
            optics.atmospheric_transmittance(d, bad)
    with pytest.raises(ValueError, match="must both be"):
        optics.slant_ranges(positions, centres[:2])


def cpu_group(n=3, points=4, mask=None):
    z = torch.zeros
    group = scene.HeliostatGroup(names=[f"h{i}" for i in range(n)], positions=torch.tensor([[10.0 * i, 100.0 + 50.0 * i, 0.0, 1.0] for i in range(n)]),
                                 surface_points=torch.rand(n, points, 4), surface_normals=torch.rand(n, points, 4),
                                 canting=z(n, 4, 2, 4), facet_translations=z(n, 4, 4), nurbs_control_points=z(n, 4, 2, 2, 3),
                                 nurbs_degrees=torch.tensor([1, 1]))
    return group


def cpu_scenario(group, n_rays=2):
    planar = scene.TowerTargetAreasPlanar(names=["a", "b"], centers=torch.tensor([[0.0, 0.0, 55.0, 1.0], [0.0, 0.0, 40.0, 1.0]]),
                                          normals=torch.tensor([[0.0, 1.0, 0.0, 0.0]] * 2), dimensions=torch.tensor([[8.0, 8.0]] * 2))
    return scene.Scenario(torch.zeros(3), scene.SolarTower([planar]), scene.LightSourceArray([scene.Sun(n_rays)]),
                          scene.HeliostatField([group]))


def test_activate_heliostats_expands_both_attributes():
    group = cpu_group()
    assert group.reflectivities is None and group.optical_errors is None
    group.activate_heliostats(torch.tensor([1, 2, 0], dtype=torch.int32))
    assert group.active_reflectivities is None and group.active_optical_errors is None
    group.reflectivities, group.optical_errors = torch.tensor([0.9, 0.8, 0.7]), torch.tensor([1e-3, 2e-3, 3e-3])
    group.activate_heliostats(torch.tensor([1, 2, 0], dtype=torch.int32))                # a heliostat activated twice, one not at all
    assert group.active_reflectivities.tolist() == pytest.approx([0.9, 0.8, 0.8])
    assert group.active_optical_errors.tolist() == pytest.approx([1e-3, 2e-3, 2e-3])
    assert group.active_positions.shape[0] == group.active_reflectivities.shape[0] == 3


def test_heliostat_intensity_factors():
    group = cpu_group()
    scenario = cpu_scenario(group)
    group.activate_heliostats(torch.tensor([1, 2, 0], dtype=torch.int32))
    targets = torch.tensor([0, 1, 0])
    eps, rho = optics.heliostat_intensity_factors(group, scenario.solar_tower, targets, ("exponential", 0.2))
    centres = scenario.solar_tower.target_areas[0].centers.numpy()[targets.numpy(), :3].astype(np.float64)
    want = 1.0 - np.exp(-0.2 * np.linalg.norm(group.active_positions.numpy()[:, :3] - centres, axis=1) / 1e3)
    np.testing.assert_allclose(eps.numpy(), want, rtol=1e-4)
    assert rho == 0.935                                     # no reflectivities: the reference's default, as a float
    group.reflectivities = torch.tensor([0.9, 0.8, 0.7])
    group.activate_heliostats(torch.tensor([1, 2, 0], dtype=torch.int32))
    assert optics.heliostat_intensity_factors(group, scenario.solar_tower, targets, ("exponential", 0.2))[1] is group.active_reflectivities


# ---- refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, position", [("ray_extinction_factor", 0), ("mirror_reflectivity", 1)])
def test_intensity_factor_refusals(name, position):
    def split(value):
        arguments = [0.1, 0.9]
        arguments[position] = value
        return ops.split_intensity_factors(*arguments, 4, torch.device("cpu"), Memo("test", capacity=4))

    good = torch.tensor([0.0, 0.1, 0.2, 1.0])
    assert split(good)[2 + position] is good and split(good)[position] == float(position)     # 0 / 1 for the kernel
    for bad, message in ((torch.zeros(3), rf"{name} must be a float or one value per active heliostat, shape \[4\]"),
                         (torch.zeros(4, 1), rf"{name} must be a float or one value"),
                         (torch.zeros(4, dtype=torch.int64), f"{name} must be a floating-point tensor"),
                         (torch.zeros(4, device="meta"), f"{name} must be on the device that traces"),
                         (torch.tensor([0.1, float("nan"), 0.2, 0.3]), f"{name} must be finite"),
                         (torch.tensor([0.1, float("inf"), 0.2, 0.3]), f"{name} must be finite"),
                         (torch.tensor([0.1, -0.01, 0.2, 0.3]), f"{name} must (lie in|be >= 0)")):
        with pytest.raises(ValueError, match=message):
            split(bad)
    above = torch.tensor([0.1, 1.5, 0.2, 0.3])
    if name == "ray_extinction_factor":
        with pytest.raises(ValueError, match=r"ray_extinction_factor must lie in \[0, 1\]"):
            split(above)
    else:
        assert split(above)[3] is above                     # a reflectivity above 1 is the caller's business


def test_the_value_check_reads_once_per_tensor_and_version(monkeypatch):
    memo = Memo("test", capacity=4)
    reads = []
    real = torch.aminmax
    monkeypatch.setattr(torch, "aminmax", lambda x: (reads.append(1), real(x))[1])
    eps, rho = torch.tensor([0.0, 0.1, 0.2]), torch.tensor([0.9, 0.8, 0.0])
    for _ in range(3):
        assert ops.split_intensity_factors(eps, rho, 3, torch.device("cpu"), memo) == (0.0, 1.0, eps, rho)
    assert len(reads) == 2                                  # one per distinct tensor
    eps.mul_(0.5)                                           # a tracked in-place write: checked anew
    ops.split_intensity_factors(eps, rho, 3, torch.device("cpu"), memo)
    assert len(reads) == 3
    rho[2] = float("nan")
    with pytest.raises(ValueError, match="mirror_reflectivity must be finite"):
        ops.split_intensity_factors(eps, rho, 3, torch.device("cpu"), memo)


def test_floats_and_one_element_tensors_are_floats():
    for value in (0.25, 1, torch.tensor(0.25), torch.tensor([0.25]), np.float32(0.25)):
        e, r, et, rt = ops.split_intensity_factors(value, value, 7, torch.device("cpu"))
        assert isinstance(e, float) and isinstance(r, float) and et is None and rt is None and e == float(value) == r


def test_optical_error_refusals():
    sun = scene.Sun(2)                                      # on the CPU
    errors = torch.tensor([1e-3, 2e-3])
    with pytest.raises(ValueError, match="optical_errors are not supported with a light source on the CPU"):
        sun.get_distortions(4, 2, optical_errors=errors)
    with pytest.raises(ValueError, match="optical_errors are not supported with a light source on the CPU"):
        sun.get_distortions_rows([0, 1], 4, 2, optical_errors=errors)
    sun.sampler = "hip"
    with pytest.raises(ValueError, match="optical_errors are not supported with a light source on the CPU"):
        sun.get_distortions(4, 2, optical_errors=errors)
    for bad, message in ((torch.zeros(3), r"one sigma per requested row, shape \[2\]"), (torch.zeros(2, dtype=torch.int32), "floating-point"),
                         (torch.zeros(2, device="meta"), "on the sun's device"), (torch.tensor([1e-3, -1e-3]), "finite and >= 0"),
                         (torch.tensor([float("nan"), 1e-3]), "finite and >= 0")):
        with pytest.raises(ValueError, match=f"optical_errors must be .*{message}"):
            scene.Sun(2, sampler="torch")._check_optical_errors(bad, 2)
    with pytest.raises(ValueError, match=r"optical_errors must be a tensor with one sigma per active heliostat, shape \[3\]"):
        DistortionsDataset(scene.Sun(2), 4, 3, optical_errors=torch.zeros(2))
    with pytest.raises(ValueError, match="optical_errors"):               # sharded rows of a CPU light source: the reference's one stream
        DistortionsDataset(scene.Sun(2), 4, 3, rows=[0, 2], optical_errors=torch.zeros(3))
    group = cpu_group()
    group.optical_errors = torch.full((3,), 1e-3)
    group.activate_heliostats()
    with pytest.raises(ValueError, match="optical_errors are not supported with a light source on the CPU"):
        HeliostatRayTracer(cpu_scenario(group), group, blocking_active=False)


def test_the_error_stream_differs_from_the_suns():
    assert scene.OPTICAL_ERROR_STREAM == ref.ERROR_STREAM and 0 < scene.OPTICAL_ERROR_STREAM < 1 << 64
    for seed in (0, 7, -5876543210123, (1 << 63) - 1):
        assert scene._error_seed(seed) != seed & 0xFFFFFFFFFFFFFFFF
        z, own = ref.error_rows(seed, [0, 5], 64), ref.philox_ref.gaussian_rows(seed, [0, 5], 64)
        assert abs(np.corrcoef(z.reshape(-1), own.reshape(-1))[0, 1]) < 0.4 and not np.array_equal(z, own)


@pytest.mark.parametrize("kind", ["normal", "pillbox"])
def test_the_law_test_passes_on_the_restated_stream(kind):
    """The GPU law test (tests/test_gpu_heliostat_optics.py) at its fixed seed, rehearsed on the numpy restatement of the
    ``"hip"`` sampler's streams, which the device reproduces to 1e-5: it does not ride on luck."""
    table = scene._radial_table(dict(distribution_type="pillbox", half_angle=ref.DISC)).numpy() if kind == "pillbox" else None
    x = ref.draw_rows(kind, ref.LAW_SEED, list(range(ref.LAW_ROWS)), ref.LAW_R * ref.LAW_P, ref.LAW_SIGMAS, table)
    worst = ref.check_law(x, kind, ref.LAW_SIGMAS)
    print(f"{kind}: largest deviation {worst:.2f} standard errors")
    assert worst < 3.0                                      # a margin for the device's 1e-5
    with pytest.raises(AssertionError):                     # and the test can fail: the sigmas one row off
        ref.check_law(x, kind, ref.LAW_SIGMAS[1:] + ref.LAW_SIGMAS[:1])


# ---- floats and None reach the kernel call as they did ----------------------------------------------------------------------------
def recorded_trace(monkeypatch, group, **factors):
    """The arguments ``TraceRays.apply`` receives from a trace of a CPU scene (the kernel call itself needs the GPU)."""
    seen = []

    def apply(*args):
        seen.append(args)
        H = args[0].shape[0]
        n_maps = 2 if args[14] else H
        return torch.ones(n_maps, args[13], args[12]), torch.ones(3, H), torch.zeros(0)

    monkeypatch.setattr(ops.TraceRays, "apply", apply)
    monkeypatch.setattr(ops, "per_target_sum", lambda flux, idx, n_targets: torch.stack([flux[idx == k].sum(0) for k in range(n_targets)]))
    tracer = HeliostatRayTracer(cpu_scenario(group), group, blocking_active=False, bitmap_resolution=torch.tensor([8, 6]))
    mask = group.active_heliostats_mask
    H = int(group.number_of_active_heliostats)
    inc, tix = torch.tensor([[0.0, 1.0, 0.0, 0.0]]).repeat(H, 1), torch.arange(H) % 2
    out = [tracer.trace_rays(inc, mask, tix, **factors), tracer.trace_rays_per_target(inc, mask, tix, **factors)]
    return seen, out


def test_floats_and_none_reach_the_kernel_call_as_before(monkeypatch):
    group = cpu_group()
    group.activate_heliostats()
    seen, _ = recorded_trace(monkeypatch, group)
    for args, per_target in zip(seen, (False, True)):
        assert args[10:15] == (0.0, 0.935, 8, 6, per_target) and all(isinstance(a, float) for a in args[9:12])
    as_tensors, _ = recorded_trace(monkeypatch, group, ray_extinction_factor=torch.tensor(0.25), mirror_reflectivity=torch.tensor([0.5]))
    as_floats, _ = recorded_trace(monkeypatch, group, ray_extinction_factor=0.25, mirror_reflectivity=0.5)
    for a, b in zip(as_tensors, as_floats):
        assert a[9:15] == b[9:15] and a[10:12] == (0.25, 0.5) and len(a) == len(b)


def test_tensors_run_the_kernel_neutral_and_scale_afterwards(monkeypatch):
    group = cpu_group()
    group.activate_heliostats()
    eps, rho = torch.tensor([0.0, 0.5, 0.2]), torch.tensor([1.0, 0.5, 0.0], requires_grad=True)
    seen, (per_heliostat, per_target) = recorded_trace(monkeypatch, group, ray_extinction_factor=eps, mirror_reflectivity=rho)
    assert [a[10:12] for a in seen] == [(0.0, 1.0)] * 2 and [a[14] for a in seen] == [False, False]     # never the fused mode
    flux, intercept, on_target, blocking = per_heliostat
    assert flux[:, 0, 0].tolist() == pytest.approx([1.0, 0.25, 0.0]) and intercept.tolist() == [1.0, 1.0, 0.0]
    assert on_target.tolist() == [1.0] * 3 and blocking.tolist() == [1.0] * 3
    assert per_target[0][:, 0, 0].tolist() == pytest.approx([1.0, 0.25]) and per_target[0].shape == (2, 6, 8)
    flux.sum().backward()
    assert rho.grad.tolist() == pytest.approx([48.0, 24.0, 38.4])
    seen, _ = recorded_trace(monkeypatch, group, ray_extinction_factor=0.25, mirror_reflectivity=rho)
    assert [a[10:12] for a in seen] == [(0.25, 1.0)] * 2                                              # the float stays in the kernel
    assert ops.bitmap_moments(flux) is None
