"""Per-heliostat optics on the GPU (``-m gpu``): reflectivity and extinction as tensors ``[H]``, the optical error in the sun's
sample, and the attenuation of ``AimPointOptimizer``.

``tests/golden/heliostat_optics.npz`` (tests/golden/generate_heliostat_optics_golden.py) is the reference itself, heliostat by
heliostat: it takes scalars, so tracing the field once per heliostat ``h`` with ``(eps_h, rho_h)`` and keeping row ``h`` is the
expected result of the tensor path.  Two cases, ``off`` (no blocking, two heliostats each activated twice) and ``on`` (the
blocking column of ``small_blocking``); one ``rho_h`` is 0.  Flux, per-target sums and the gradient with respect to the surface
points are held to ``max(3 x yardstick, floor)``, the yardstick the fixture's own fp32-vs-fp64 distance and the floors those of
tests/test_gpu_kinematics_reconstructor.py for traced quantities (2e-5 flux, 5e-4 gradient); the factors are exact.  The second
leg is the CPU restatement (``oracle/``), called once per heliostat with scalars: 1e-6 relative L2, the project's bound for HIP
against the restatement.

Measured on MI355X: see DESIGN.md 4.14.
"""
import json
import math
import pathlib

import numpy as np
import pytest
import torch

import heliostat_optics_ref as ref
import oracle
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FLUX_FLOOR, GRAD_FLOOR = 2e-5, 5e-4
CASES = ["off", "on"]
DDP = dict(rank=0, world_size=1, is_distributed=False, groups_to_ranks_mapping={0: [0]}, ranks_to_groups_mapping={0: [0]},
           heliostat_group_rank=0, heliostat_group_world_size=1)


def t(x, dtype=None):
    out = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return out if dtype is None else out.to(dtype)


def n(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def fixture(golden):
    """name -> the case's arrays without the prefix, plus the field-wide ``extinction`` / ``reflectivity``."""
    d = golden("heliostat_optics")

    def case(name):
        out = {k[len(name) + 1:]: v for k, v in d.items() if k.startswith(name + "_")}
        out.update(extinction=d["extinction"], reflectivity=d["reflectivity"])
        return out
    return case


def trace_inputs(d):
    both = torch.stack((t(d["distortions_u"]), t(d["distortions_e"])), dim=-1).contiguous()
    return dict(origins=t(d["aligned_points"]), normals=t(d["aligned_normals"]), incident=t(d["incident"]),
                dist_u=both[..., 0], dist_e=both[..., 1], target_idx=t(d["target_idx"]), centers=t(d["target_centers"]),
                plane_normals=t(d["target_normals"]), dims=t(d["target_dims"]), ray_magnitude=float(d["ray_magnitude"]),
                resolution=tuple(int(v) for v in d["resolution"]))


def blocking_of(d, points):
    """The rectangles as functions of ``points`` (one group, every heliostat active once: tests/test_gpu_parity.py's way)."""
    from artist_amd.blocking import create_blocking_primitives_rectangles_by_index
    np.testing.assert_array_equal(d["blocking_surfaces"], d["aligned_points"])
    corners, spans, normals = create_blocking_primitives_rectangles_by_index(points)
    H = points.shape[0]
    return dict(corners=corners, spans=spans, normals=normals, owner=torch.arange(H, dtype=torch.int32, device=DEV))


def bounds(d):
    yard = {k: rel_l2(d[k], d[k + "_f64"]) for k in ("flux", "per_target", "grad_aligned_points")}
    floor = dict(flux=FLUX_FLOOR, per_target=FLUX_FLOOR, grad_aligned_points=GRAD_FLOOR)
    return yard, {k: max(3 * v, floor[k]) for k, v in yard.items()}


def traced(d, name, **factors):
    """``(inputs, flux, factors)`` of the functional trace of case ``name`` with the given factors, points in the graph."""
    from artist_amd import trace_rays
    inp = trace_inputs(d)
    inp["origins"].requires_grad_(True)
    blocking = blocking_of(d, inp["origins"]) if name == "on" else None
    flux, fac, *_ = trace_rays(**inp, blocking=blocking, **factors)
    return inp, flux, fac


# ---- 1. tensor factors against the reference, heliostat by heliostat ---------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_tensor_factors_against_the_fixture(fixture, name):
    from artist_amd import per_target_sum
    d = fixture(name)
    yard, bound = bounds(d)
    inp, flux, fac = traced(d, name, extinction=t(d["extinction"]), reflectivity=t(d["reflectivity"]))
    per_target = per_target_sum(flux, inp["target_idx"], 2)
    (flux * t(d["loss_weights"])).sum().backward()
    got = dict(flux=n(flux), per_target=n(per_target), grad_aligned_points=n(inp["origins"].grad))
    for key in ("flux", "per_target", "grad_aligned_points"):
        err = rel_l2(got[key], d[key])
        print(f"{name}: {key}: error {err:.2e}, yardstick {yard[key]:.2e}, bound {bound[key]:.2e}")
    print(f"{name}: factors\n{n(fac)}\nfixture\n{np.stack((d['intercept'], d['on_target'], d['blocking']))}")
    assert all(np.isfinite(v).all() for v in got.values()) and np.isfinite(n(fac)).all()
    zero = int(np.nonzero(d["reflectivity"] == 0)[0][0])
    assert not got["flux"][zero].any() and n(fac)[0, zero] == 0 and n(fac)[1, zero] > 0
    for row, key in enumerate(("intercept", "on_target", "blocking")):
        np.testing.assert_array_equal(n(fac[row]), d[key], err_msg=key)
    for key in ("flux", "per_target", "grad_aligned_points"):
        assert rel_l2(got[key], d[key]) < bound[key], (key, rel_l2(got[key], d[key]), bound[key])


@pytest.mark.parametrize("name", CASES)
def test_rows_against_the_oracle_with_scalars(fixture, name):
    d = fixture(name)
    _, flux, fac = traced(d, name, extinction=t(d["extinction"]), reflectivity=t(d["reflectivity"]))
    H = flux.shape[0]
    blocking = None
    if name == "on":
        blocking = dict(corners=d["prim_corners"], spans=d["prim_spans"], normals=d["prim_normals"], owner=np.arange(H, dtype=np.int32))
    for h in range(H):
        o_flux, o_fac = oracle.trace_fwd(d["aligned_points"], d["aligned_normals"], d["incident"], d["distortions_u"],
                                         d["distortions_e"], d["target_idx"], d["target_centers"], d["target_normals"],
                                         d["target_dims"], d["resolution"], float(d["ray_magnitude"]), float(d["extinction"][h]),
                                         float(d["reflectivity"][h]), blocking=blocking)
        err = rel_l2(n(flux[h]), o_flux[h])
        print(f"{name}: row {h} against the oracle with ({d['extinction'][h]}, {d['reflectivity'][h]}): {err:.2e}")
        assert err <= 1e-6, (h, err)
        np.testing.assert_array_equal(n(fac[:, h]), o_fac[:, h])


@pytest.mark.parametrize("name", CASES)
def test_one_value_in_a_tensor_against_the_float_path(fixture, name, monkeypatch):
    from artist_amd import _lib
    d = fixture(name)
    H = d["aligned_points"].shape[0]
    _, flux_f, fac_f = traced(d, name, extinction=0.07, reflectivity=0.9)
    _, flux_t, fac_t = traced(d, name, extinction=torch.full((H,), 0.07, device=DEV), reflectivity=torch.full((H,), 0.9, device=DEV))
    err = rel_l2(n(flux_t), n(flux_f))                # one rounding per pixel against one per ray
    print(f"{name}: a tensor filled with one value against the float: {err:.2e}")
    assert err <= 1e-6 and torch.equal(fac_t, fac_f)
    # a float handed over as a 0-d (or one-element) tensor IS the float call: same launches, same bits
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name_, *a, **k: (names.append(name_), real(name_, *a, **k))[1])
    _, flux_0, fac_0 = traced(d, name, extinction=torch.tensor(0.07, device=DEV), reflectivity=torch.tensor([0.9]))
    launches_0, names[:] = list(names), []
    _, flux_f2, _ = traced(d, name, extinction=0.07, reflectivity=0.9)
    assert launches_0 == names and "art_trace_fwd" in names
    assert torch.equal(flux_0, flux_f) and torch.equal(fac_0, fac_f) and torch.equal(flux_f2, flux_f)


@pytest.mark.parametrize("name", CASES)
def test_gradient_with_respect_to_the_reflectivities(fixture, name):
    """``d sum(weights * flux) / d rho_h = sum(weights_h * flux_h) / rho_h``, formed from the fixture (for the row with
    ``rho_h = 0``: ``(1 - eps_h)`` times the sum over the fixture's bitmaps with the scalars (0, 1)); the extinctions likewise."""
    d = fixture(name)
    _, bound = bounds(d)
    eps, rho = t(d["extinction"]).requires_grad_(True), t(d["reflectivity"]).requires_grad_(True)
    _, flux, _ = traced(d, name, extinction=eps, reflectivity=rho)
    (flux * t(d["loss_weights"])).sum().backward()
    w64, e64, r64 = d["loss_weights"].astype(np.float64), d["extinction"].astype(np.float64), d["reflectivity"].astype(np.float64)
    share = (w64 * d["flux"]).sum(axis=(1, 2))
    unit = (w64 * d["flux_unit"]).sum(axis=(1, 2))
    want_rho = np.where(r64 > 0, share / np.where(r64 > 0, r64, 1.0), (1.0 - e64) * unit)
    want_eps = -r64 * unit
    for got, want, key in ((rho.grad, want_rho, "reflectivity"), (eps.grad, want_eps, "extinction")):
        err = rel_l2(n(got), want)
        print(f"{name}: gradient w.r.t. {key}: {n(got)} against {want}: {err:.2e}, bound {bound['flux']:.2e}")
        assert np.isfinite(n(got)).all() and err < bound["flux"], (key, err)


# ---- 2. through the ray tracer: per-target route, sharding -----------------------------------------------------------------
def build_field(H, R, sampler="torch", n_eval=8, kind="normal"):
    """A synthetic field with two planar targets, aligned; heliostat ``h`` aims at target ``h % 2``."""
    from artist_amd import scene
    scenario, _ = scene.build_synthetic_scenario(
        H, n_rays=R, n_cp=(6, 6), n_eval=n_eval, device=DEV, target_centers=((0.0, 0.0, 55.0, 1.0), (2.0, 0.0, 47.0, 1.0)),
        target_normals=((0.0, 1.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0)), target_dims=((8.0, 8.0), (6.0, 5.0)))
    if kind != "normal":
        scenario.light_sources = scene.LightSourceArray([scene.Sun(R, dict(distribution_type=kind), device=DEV)])
    scenario.light_sources.light_source_list[0].sampler = sampler
    group = scenario.heliostat_field.heliostat_groups[0]
    return scenario, group


def align(scenario, group):
    H = group.number_of_heliostats
    mask = torch.ones(H, dtype=torch.int32, device=DEV)
    group.activate_heliostats(mask)
    tix = (torch.arange(H, device=DEV) % 2).long()
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
    return mask, tix, inc


def field_factors(H):
    generator = torch.Generator().manual_seed(5)
    eps = (0.3 * torch.rand(H, generator=generator)).to(DEV)
    rho = (0.5 + 0.5 * torch.rand(H, generator=generator)).to(DEV)
    rho[1] = 0.0
    return eps, rho


@pytest.mark.parametrize("which", ["both", "reflectivity only", "extinction only"])
def test_per_target_route_equals_the_sum_of_the_scaled_bitmaps(which):
    from artist_amd import HeliostatRayTracer
    H = 5
    scenario, group = build_field(H, 4)
    mask, tix, inc = align(scenario, group)
    eps, rho = field_factors(H)
    factors = dict(ray_extinction_factor=eps if which != "reflectivity only" else 0.05,
                   mirror_reflectivity=rho if which != "extinction only" else 0.9)
    tracer = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=torch.tensor([64, 48]))
    flux, *fac = tracer.trace_rays(inc, mask, tix, **factors)
    per_target, *fac_t = tracer.trace_rays_per_target(inc, mask, tix, **factors)
    assert per_target.shape == (2, 48, 64) and float(per_target.sum()) > 0
    assert torch.equal(per_target, tracer.get_bitmaps_per_target(flux, tix))
    assert all(torch.equal(a, b) for a, b in zip(fac, fac_t))
    fused, *_ = tracer.trace_rays_per_target(inc, mask, tix)             # floats: still the fused mode, no [H,Hh,W]
    assert fused.shape == per_target.shape and not torch.equal(fused, per_target)


def test_a_rank_takes_its_rows_of_field_wide_tensors():
    from artist_amd import HeliostatRayTracer
    H = 5
    scenario, group = build_field(H, 4)
    mask, tix, inc = align(scenario, group)
    eps, rho = field_factors(H)
    resolution = torch.tensor([64, 48])
    full = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=resolution).trace_rays(
        inc, mask, tix, ray_extinction_factor=eps, mirror_reflectivity=rho)
    total, seen = 0, []
    for rank in range(3):
        tracer = HeliostatRayTracer(scenario, group, blocking_active=False, world_size=3, rank=rank, bitmap_resolution=resolution)
        rows = tracer.get_sampler_indices()
        seen += rows.tolist()
        part = tracer.trace_rays(inc, mask, tix, ray_extinction_factor=eps, mirror_reflectivity=rho)
        for got, want in zip(part, full):
            assert torch.equal(got, want[rows]), rank
        per_target, *_ = tracer.trace_rays_per_target(inc, mask, tix, ray_extinction_factor=eps, mirror_reflectivity=rho)
        assert torch.equal(per_target, tracer.get_bitmaps_per_target(part[0], tix[rows]))
        total = total + per_target.double()
    assert sorted(seen) == list(range(H))
    want = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=resolution).get_bitmaps_per_target(full[0], tix)
    assert rel_l2(n(total), n(want)) <= 1e-6


# ---- 3. optical error -------------------------------------------------------------------------------------------------------
def sun_of(kind, R, sampler="hip"):
    from artist_amd.scene import Sun
    return Sun(R, dict(distribution_type=kind), device=DEV, sampler=sampler)


@pytest.mark.parametrize("R, P", [(3, 667), (2, 1000)])               # R*P odd (a tail ray) and even
def test_optical_error_known_answer(R, P):
    from artist_amd import scene
    assert scene.OPTICAL_ERROR_STREAM == ref.ERROR_STREAM != 0
    rows, seed = [0, 5, (1 << 32) + 3], 7
    sigmas = (2e-3, 0.0, 5e-4)
    sun = sun_of("normal", R)
    u, e = sun.get_distortions_rows(rows, P, 8, seed, optical_errors=torch.tensor(sigmas, device=DEV))
    got = n(torch.stack((u, e), -1)).reshape(3, R * P, 2).astype(np.float64)
    want = ref.draw_rows("normal", seed, rows, R * P, sigmas)
    scale = np.sqrt(ref.COVARIANCE + np.asarray(sigmas) ** 2)[:, None, None]           # in units of each row's standard deviation
    err = np.abs(got - want) / scale / np.maximum(1.0, np.abs(want) / scale)
    print(f"R*P {R * P}: max |hip - restatement| in standard deviations = {err.max():.2e}")
    assert err.max() <= 1e-5, np.unravel_index(err.argmax(), err.shape)
    plain = ref.draw_rows("normal", seed, rows, R * P, (0.0, 0.0, 0.0))
    assert np.abs(want[0] - plain[0]).max() > 1e-3                    # the case is what it says: the error moves row 0


@pytest.mark.parametrize("kind", ["normal", "pillbox"])
@pytest.mark.parametrize("sampler", ["hip", "torch"])
def test_sigma_zero_rows_are_the_plain_draw(kind, sampler):
    rows, P, H = [3, 0, 6, 1], 333, 7
    sun = sun_of(kind, 3, sampler)
    plain = [x.clone() for x in sun.get_distortions_rows(rows, P, H, 11)]
    errors = torch.tensor([0.0, 1e-3, 0.0, 2e-3], device=DEV)
    got = sun.get_distortions_rows(rows, P, H, 11, optical_errors=errors)
    for a, b in zip(got, plain):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
        assert not torch.equal(a[1], b[1]) and not torch.equal(a[3], b[3])
    again = sun.get_distortions_rows(rows, P, H, 11)                  # the shared base sample was not written
    assert all(torch.equal(a, b) for a, b in zip(again, plain))
    full = sun.get_distortions(P, H, 11, optical_errors=torch.full((H,), 1e-3, device=DEV))
    assert torch.equal(full[0][0], got[0][1]) and torch.equal(full[1][0], got[1][1])     # row 0 with sigma 1e-3, either way


@pytest.mark.parametrize("kind", ["normal", "pillbox"])
def test_law_with_optical_errors(kind):
    """Per row: mean and variance within 4 standard errors of ``cov + sigma_row^2`` (tests/heliostat_optics_ref.py; the seed is
    known to pass: tests/test_heliostat_optics_host.py applies the same test to the restated stream)."""
    sun = sun_of(kind, ref.LAW_R)
    u, e = sun.get_distortions(ref.LAW_P, ref.LAW_ROWS, ref.LAW_SEED, optical_errors=torch.tensor(ref.LAW_SIGMAS, device=DEV))
    x = n(torch.stack((u, e), -1).double()).reshape(ref.LAW_ROWS, ref.LAW_R * ref.LAW_P, 2)
    print(f"{kind}: largest deviation {ref.check_law(x, kind, ref.LAW_SIGMAS):.2f} standard errors")


def test_rank_rows_of_a_draw_with_optical_errors():
    from artist_amd import HeliostatRayTracer
    H = 7
    scenario, group = build_field(H, 4, sampler="hip")
    group.optical_errors = torch.linspace(0.0, 3e-3, H, device=DEV)
    align(scenario, group)
    full = HeliostatRayTracer(scenario, group, blocking_active=False).distortions_dataset
    plain = scenario.light_sources.light_source_list[0].get_distortions(full.distortions_u.shape[2], H, 7)[0]
    assert torch.equal(full.distortions_u[0], plain[0]) and not torch.equal(full.distortions_u[1:], plain[1:])
    seen = []
    for rank in range(3):
        tracer = HeliostatRayTracer(scenario, group, blocking_active=False, world_size=3, rank=rank)
        rows = torch.tensor(tracer.distortions_sampler.rank_indices, device=DEV)
        seen += rows.tolist()
        ds = tracer.distortions_dataset
        assert torch.equal(ds.distortions_u, full.distortions_u[rows]) and torch.equal(ds.distortions_e, full.distortions_e[rows]), rank
    assert sorted(seen) == list(range(H))


def test_sample_cache_with_optical_errors(monkeypatch):
    from artist_amd import HeliostatRayTracer, _lib
    H = 5
    scenario, group = build_field(H, 4, sampler="hip")
    sun = scenario.light_sources.light_source_list[0]
    group.optical_errors = torch.full((H,), 1e-3, device=DEV)
    align(scenario, group)
    handle = _lib.lib()
    real = handle.art_sample_distortions
    calls = []
    monkeypatch.setattr(handle, "art_sample_distortions", lambda *args: (calls.append(args[2]), real(*args))[1])
    rt1 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 2                                          # the sun's draw and the error stream
    rt2 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 2                                          # a second tracer on the same group launches nothing
    assert rt2.distortions_dataset.distortions_u.data_ptr() == rt1.distortions_dataset.distortions_u.data_ptr()
    first = rt1.distortions_dataset.distortions_u.clone()
    group.active_optical_errors.mul_(2.0)                           # an in-place write: the sample with errors is made anew
    rt3 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 3 and not torch.equal(rt3.distortions_dataset.distortions_u, first)
    base = sun._cache
    group.active_optical_errors = None                              # None: the plain draw's entry, unchanged and hit
    rt4 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 3 and sun._cache is base and rt4.distortions_dataset.distortions_u.data_ptr() == base[1].data_ptr()
    fresh = sun_of("normal", 4).get_distortions(first.shape[2], H, 7)[0]
    assert torch.equal(rt4.distortions_dataset.distortions_u, fresh)
    third = rt3.distortions_dataset.distortions_u
    assert torch.allclose(third - fresh, 2.0 * (first - fresh), rtol=1e-4, atol=1e-9)        # the same z, twice the sigma


def rms_width(bitmap):
    b = bitmap.double()
    ys, xs = torch.meshgrid(torch.arange(b.shape[0], device=DEV, dtype=torch.float64),
                            torch.arange(b.shape[1], device=DEV, dtype=torch.float64), indexing="ij")
    s = b.sum()
    cy, cx = (b * ys).sum() / s, (b * xs).sum() / s
    return float(torch.sqrt((b * ((ys - cy) ** 2 + (xs - cx) ** 2)).sum() / s))


def test_optical_errors_through_the_ray_tracer(monkeypatch):
    from artist_amd import HeliostatRayTracer, ops
    H, R = 4, 16
    scenario, group = build_field(H, R, sampler="hip", n_eval=16, kind="pillbox")
    group.optical_errors = torch.tensor([0.0, 2e-3, 0.0, 2e-3], device=DEV)
    mask, tix, inc = align(scenario, group)
    planar = scenario.solar_tower.target_areas[0]
    handed = []
    real_views = ops._dist_views
    monkeypatch.setattr(ops, "_dist_views", lambda u, e, shape: (handed.append((u.data_ptr(), e.data_ptr())), real_views(u, e, shape))[1])
    tracer = HeliostatRayTracer(scenario, group, blocking_active=False)
    flux, *_ = tracer.trace_rays(inc, mask, tix)
    du, de = tracer.distortions_dataset.distortions_u, tracer.distortions_dataset.distortions_e
    assert handed == [(du.data_ptr(), de.data_ptr())]               # the sun's views, handed to the kernel as they are
    o_flux, _ = oracle.trace_fwd(n(group.active_surface_points), n(group.active_surface_normals), n(inc), n(du), n(de),
                                 n(tix).astype(np.int32), n(planar.centers), n(planar.normals), n(planar.dimensions), (256, 256))
    err = rel_l2(n(flux), o_flux)
    widths = [rms_width(flux[h]) for h in range(H)]
    print(f"flux against the oracle on the same distortions: {err:.2e}; RMS widths in pixels {widths}")
    assert err < 1e-6
    group.active_optical_errors = None
    sharp, *_ = HeliostatRayTracer(scenario, group, blocking_active=False).trace_rays(inc, mask, tix)
    for h in range(H):
        if h % 2:
            # (the image of a flat 3.2 m mirror on a 6 - 8 m target is mostly the mirror: 2 mrad of error widens it by a percent)
            assert widths[h] > rms_width(sharp[h]), h
        else:
            assert torch.equal(flux[h], sharp[h]), h


# ---- 4. AimPointOptimizer ----------------------------------------------------------------------------------------------------
def aim_point_optimizer(d, **keywords):
    from artist_amd.optim import AimPointOptimizer
    from artist_amd.scenario import Scenario, open_scenario_file
    path = pathlib.Path(__file__).resolve().parent / "golden" / "scenarios" / "test_blocking.h5"
    with open_scenario_file(path) as scenario_file:
        scenario = Scenario.load_scenario_from_hdf5(scenario_file=scenario_file,
                                                    number_of_surface_points_per_facet=torch.tensor([int(v) for v in d["points_per_facet"]]),
                                                    device=DEV)
    scenario.set_number_of_rays(number_of_rays=int(d["n_rays"]))
    optimizer = AimPointOptimizer(ddp_setup=DDP, scenario=scenario, optimization_configuration=json.loads(str(d["configuration"])),
                                  incident_ray_direction=t(d["sun"], torch.float32), target_area_index=int(d["target_area_index"]),
                                  ground_truth=t(d["ground_truth"], torch.float32), dni=float(np.asarray(d["dni"]).reshape(-1)[0]),
                                  bitmap_resolution=torch.tensor([int(v) for v in d["resolution"]]),
                                  epsilon=float(np.asarray(d["epsilon"]).reshape(-1)[0]), device=DEV, **keywords)
    optimizer.prepare(DEV)
    return optimizer, scenario


def test_aim_point_optimizer_with_attenuation(golden, monkeypatch):
    from artist_amd import HeliostatRayTracer, _lib
    d = golden("aim_point_optimizer_epochs")
    optimizer, scenario = aim_point_optimizer(d, attenuation=("exponential", 0.1))
    total_flux, intercept, *_ = optimizer.trace_epoch(DEV)
    total_flux.sum().backward()
    g = optimizer.groups[0]
    grad = g["parameter"].grad
    assert torch.isfinite(grad).all() and float(grad.abs().sum()) > 0
    # the same alignment traced without attenuation, heliostat by heliostat, weighted on the host
    group = g["group"]
    tracer = HeliostatRayTracer(scenario=scenario, heliostat_group=group, blocking_active=True, random_seed=0,
                                bitmap_resolution=optimizer._resolution_cpu, dni=optimizer.dni, batch_size=optimizer.optimizer_dict["batch_size"])
    with torch.no_grad():
        flux, *_ = tracer.trace_rays(g["incident"], g["mask"], g["targets"])
    centre = n(scenario.solar_tower.get_centers_of_target_areas(g["targets"][:1]))[0, :3].astype(np.float64)
    distance = np.linalg.norm(n(group.active_positions)[:, :3].astype(np.float64) - centre, axis=1)
    tau = np.exp(-0.1 * distance / 1000.0)
    assert distance.min() > 10 and tau.max() < 0.9999 and len(set(np.round(tau, 6))) > 1
    want = (tau[:, None, None] * n(flux).astype(np.float64)).sum(axis=0)
    err = rel_l2(n(total_flux), want)
    print(f"total flux against the transmittance-weighted sum of the un-attenuated bitmaps: {err:.2e}; tau {tau}")
    assert err <= 1e-6
    np.testing.assert_allclose(n(g["extinction"]), 1.0 - tau, rtol=0, atol=2e-7)
    # without the keyword: the epoch it was - the fused per-target mode, no scale pass, the same bits
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name_, *a, **k: (names.append(name_), real(name_, *a, **k))[1])
    plain, _ = aim_point_optimizer(d)
    names[:] = []
    flux_plain, *factors_plain = plain.trace_epoch(DEV)
    launches_plain, names[:] = list(names), []
    none, _ = aim_point_optimizer(d, attenuation=None)
    names[:] = []
    flux_none, *factors_none = none.trace_epoch(DEV)
    assert names == launches_plain and "art_per_target_sum" not in names and "art_trace_fwd" in names
    assert torch.equal(flux_none, flux_plain) and all(torch.equal(a, b) for a, b in zip(factors_none, factors_plain))
    assert plain.groups[0]["extinction"] is None and not torch.equal(flux_plain, total_flux.detach())
