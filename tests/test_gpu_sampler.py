"""The HIP distortion sampler on the GPU (``-m gpu``): ``art_sample_distortions`` against the numpy restatement of its stream
(tests/philox_ref.py), the law of its draws, the rank-sharding invariant, ``Sun(sampler="hip")`` through the ray tracer
against the oracle, and the per-sun sample cache."""
import math

import numpy as np
import pytest
import torch

import oracle
import philox_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EYE = ((1.0, 0.0), (0.0, 1.0))


def n(x):
    return x.detach().cpu().numpy()


def build_field(H, R, n_cp=6, n_eval=16, sampler="hip"):
    """The synthetic field the way tests/test_gpu_configs.py builds it, its sun switched to ``sampler`` after loading."""
    from artist_amd import scene
    scenario, _ = scene.build_synthetic_scenario(H, n_rays=R, n_cp=(n_cp, n_cp), n_eval=n_eval, device=DEV)
    scenario.light_sources.light_source_list[0].sampler = sampler
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=DEV)
    group.activate_heliostats(mask)
    tix = torch.zeros(H, dtype=torch.long, device=DEV)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
    return scenario, group, mask, tix, inc


# ---- 1. known answer -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [7, -5876543210123])
@pytest.mark.parametrize("R, P", [(3, 66667), (2, 100000)])          # R*P odd (a tail ray) and even (float4 stores only)
def test_known_answer_against_the_restated_stream(seed, R, P):
    from artist_amd import ops
    rows = [0, 5, (1 << 32) + 3]
    out = ops.sample_distortions(rows, R, P, seed, (0.0, 0.0), EYE, DEV)
    assert out.shape == (3, R, P, 2) and out.dtype == torch.float32 and out.is_contiguous()
    got = n(out).reshape(3, R * P, 2).astype(np.float64)
    ref = philox_ref.gaussian_rows(seed, rows, R * P)
    assert ref.shape[1] == R * P and (R * P) // 2 >= 100000
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print(f"seed {seed}, R*P {R * P}: max |hip - restatement| / max(1, |z|) = {err.max():.2e}")
    assert err.max() <= 1e-5, np.unravel_index(err.argmax(), err.shape)
    # the law: loc + scale_tril @ z, element-wise (u from z0, e from both)
    loc, tril = (1e-3, -2e-3), ((2.0, 0.0), (0.5, 3.0))
    got = n(ops.sample_distortions(rows[1:2], R, P, seed, loc, tril, DEV)).reshape(1, R * P, 2)
    want = philox_ref.apply_law(ref[1:2], loc, tril)
    assert np.abs(got - want).max() <= 4e-5 * max(1.0, np.abs(want).max())


# ---- 2. law ------------------------------------------------------------------------------------------------------------
def _check_law(x, mu, cov, rows, R, P):
    """x [rows, R, P, 2] fp32 draws of N(mu, cov): moments, tail fractions of the whitened components, correlations."""
    x = x.double()
    mu, cov = torch.tensor(mu, dtype=torch.float64, device=DEV), torch.tensor(cov, dtype=torch.float64, device=DEV)
    flat = x.reshape(-1, 2)
    N = flat.shape[0]
    m = flat.mean(0)
    d = flat - m
    c = d.T @ d / (N - 1)
    mean_sigma = torch.sqrt(torch.diagonal(cov) / N)
    assert ((m - mu).abs() <= 4 * mean_sigma).all(), (m, mu, mean_sigma)
    cov_sigma = torch.sqrt((torch.outer(torch.diagonal(cov), torch.diagonal(cov)) + cov * cov) / N)
    assert ((c - cov).abs() <= 4 * cov_sigma).all(), (c, cov, cov_sigma)
    w = torch.linalg.solve_triangular(torch.linalg.cholesky(cov), (x - mu).reshape(-1, 2).T, upper=False).T
    for k in (1, 2, 3):
        p = math.erfc(k / math.sqrt(2.0))                            # 2 (1 - Phi(k))
        frac = (w.abs() > k).double().mean(0)
        assert ((frac - p).abs() <= 4 * math.sqrt(p * (1 - p) / N)).all(), (k, frac, p)
    w = w.reshape(rows, R * P, 2)

    def corr(a, b):
        a, b = a - a.mean(), b - b.mean()
        return float((a * b).sum() / torch.sqrt((a * a).sum() * (b * b).sum())), a.numel()

    for comp in (0, 1):
        r, cnt = corr(w[:, :-1, comp].reshape(-1), w[:, 1:, comp].reshape(-1))    # neighbouring rays (inside and across pairs)
        assert abs(r) <= 4 / math.sqrt(cnt), ("rays", comp, r)
        r, cnt = corr(w[0, :, comp], w[1, :, comp])                                 # rows 0 and 1
        assert abs(r) <= 4 / math.sqrt(cnt), ("rows", comp, r)
    r, cnt = corr(w[..., 0].reshape(-1), w[..., 1].reshape(-1))                     # the two components of a ray
    assert abs(r) <= 4 / math.sqrt(cnt), ("components", r)


def test_law_of_the_default_diagonal_sun():
    from artist_amd.scene import Sun
    rows, R, P = 10, 10, 100000                                      # 1e7 draws
    sun = Sun(R, device=DEV, sampler="hip")
    u, e = sun.get_distortions(number_of_points=P, number_of_active_heliostats=rows)
    var = sun.distribution_parameters["covariance"]
    _check_law(torch.stack((u, e), -1), (0.0, 0.0), ((var, 0.0), (0.0, var)), rows, R, P)


def test_law_of_a_correlated_sun_with_a_mean():
    from artist_amd.scene import Sun
    rows, R, P = 10, 10, 100000
    sun = Sun(R, device=DEV, sampler="hip")
    mu, cov = (1e-3, -2e-3), ((4e-6, 1.5e-6), (1.5e-6, 2e-6))
    sun.distribution = torch.distributions.MultivariateNormal(torch.tensor(mu, device=DEV), torch.tensor(cov, device=DEV))
    u, e = sun.get_distortions(number_of_points=P, number_of_active_heliostats=rows)
    _check_law(torch.stack((u, e), -1), mu, cov, rows, R, P)


# ---- 3. sharding -------------------------------------------------------------------------------------------------------
def test_rank_rows_are_the_rows_of_the_full_draw():
    from artist_amd import HeliostatRayTracer, ops
    H, R = 7, 4
    scenario, group, mask, tix, inc = build_field(H, R, n_eval=8)
    sun = scenario.light_sources.light_source_list[0]
    full = HeliostatRayTracer(scenario, group, blocking_active=False).distortions_dataset
    fu, fe = full.distortions_u, full.distortions_e
    P = fu.shape[2]
    seen = []
    for rank in range(3):
        rtr = HeliostatRayTracer(scenario, group, blocking_active=False, world_size=3, rank=rank)
        rows = rtr.distortions_sampler.rank_indices
        seen += rows
        ds = rtr.distortions_dataset
        assert ds.distortions_u.shape[0] == len(rows)               # owned rows only
        sel = torch.tensor(rows, device=DEV)
        assert torch.equal(ds.distortions_u, fu[sel]) and torch.equal(ds.distortions_e, fe[sel]), rank
    assert sorted(seen) == list(range(H))
    perm = [5, 2, 6, 0]
    pu, pe = sun.get_distortions_rows(perm, number_of_points=P, number_of_active_heliostats=H)
    sel = torch.tensor(perm, device=DEV)
    assert torch.equal(pu, fu[sel]) and torch.equal(pe, fe[sel])
    law = sun._host_law()
    a = ops.sample_distortions(list(range(H)), R, P, 7, *law, DEV)
    b = ops.sample_distortions(torch.arange(H, device=DEV), R, P, 7, *law, DEV)
    assert torch.equal(a, b) and torch.equal(a[..., 0], fu) and torch.equal(a[..., 1], fe)


# ---- 4. through the tracer ---------------------------------------------------------------------------------------------
def test_hip_sampled_flux_through_the_ray_tracer(monkeypatch):
    from artist_amd import HeliostatRayTracer, ops
    H, R = 6, 16
    scenario, group, mask, tix, inc = build_field(H, R)
    sun = scenario.light_sources.light_source_list[0]
    planar = scenario.solar_tower.target_areas[0]
    strides = []
    real_views = ops._dist_views

    def spy(u, e, shape):
        strides.append((u.stride(), e.stride(), e.data_ptr() - u.data_ptr()))
        return real_views(u, e, shape)

    monkeypatch.setattr(ops, "_dist_views", spy)

    def trace(sampler, seed):
        sun.sampler = sampler
        rt = HeliostatRayTracer(scenario, group, blocking_active=False, random_seed=seed)
        flux, *_ = rt.trace_rays(inc, mask, tix)
        return rt, flux.detach()

    rt, flux_hip = trace("hip", 7)
    P = group.active_surface_points.shape[1]
    assert strides == [((2 * R * P, 2 * P, 2), (2 * R * P, 2 * P, 2), 4)]   # the interleaved views, passed as they are
    du, de = rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e
    o_flux, _ = oracle.trace_fwd(n(group.active_surface_points), n(group.active_surface_normals), n(inc), n(du), n(de),
                                 n(tix).astype(np.int32), n(planar.centers), n(planar.normals), n(planar.dimensions), (256, 256))
    err = rel_l2(n(flux_hip), o_flux)
    print(f"hip-sampled flux vs oracle on the same distortions: rel L2 {err:.2e}")
    assert err < 1e-6
    _, flux_t7 = trace("torch", 7)
    _, flux_t8 = trace("torch", 8)
    d_hip, d_seeds = rel_l2(n(flux_hip), n(flux_t7)), rel_l2(n(flux_t8), n(flux_t7))
    print(f"rel L2: hip vs torch seed 7 {d_hip:.3e}, torch seed 8 vs seed 7 {d_seeds:.3e}")
    assert 0 < d_hip <= 1.5 * d_seeds


# ---- 5. cache ----------------------------------------------------------------------------------------------------------
def test_sample_cache(monkeypatch):
    from artist_amd import HeliostatRayTracer, _lib
    H, R = 5, 4
    scenario, group, mask, tix, inc = build_field(H, R, n_eval=8)
    sun = scenario.light_sources.light_source_list[0]
    P = group.active_surface_points.shape[1]
    handle = _lib.lib()
    real = handle.art_sample_distortions
    calls = []

    def counted(*args):
        calls.append(args[2])
        return real(*args)

    monkeypatch.setattr(handle, "art_sample_distortions", counted)
    rt1 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 1
    rt2 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert len(calls) == 1                                          # a hit: no launch
    assert rt2.distortions_dataset.distortions_u.data_ptr() == rt1.distortions_dataset.distortions_u.data_ptr()
    first = rt1.distortions_dataset.distortions_u.clone()
    del rt1, rt2

    draw = lambda seed=7, rows=range(H): sun.get_distortions_rows(rows, number_of_points=P, number_of_active_heliostats=H,  # noqa: E731
                                                                  random_seed=seed)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)

    def settled():
        """Bytes allocated beyond ``base``: one sample is 40 KB, a new law's own tensors a few hundred bytes."""
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated(DEV) - base

    torch.cuda.set_sync_debug_mode("error")                         # (the comparisons wait for the device: made after)
    try:
        hit = draw()[0]                                             # hit
        n_hit = len(calls)
        u, e = draw(seed=8)                                         # miss with the law known: still no synchronisation
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert n_hit == 1 and len(calls) == 2
    assert torch.equal(hit, first) and not torch.equal(u, first)    # the kept seed-7 sample, then a seed-8 one
    del hit, u, e
    assert settled() <= 2048

    u = draw(seed=8, rows=[4, 3, 2, 1, 0])[0]                       # new rows
    assert len(calls) == 3 and torch.equal(u[4], draw(seed=8, rows=[0])[0][0])
    assert len(calls) == 4                                          # (which replaced the entry: rows [0] drawn anew)
    del u
    assert settled() <= 2048

    sun.number_of_rays = R - 1                                      # (Scenario.set_number_of_rays) fewer rays: drawn anew
    u = draw()[0]
    assert len(calls) == 5 and u.shape == (H, R - 1, P)
    del u
    assert settled() <= 2048
    sun.number_of_rays = R

    sun.distribution = torch.distributions.MultivariateNormal(torch.zeros(2, device=DEV), 4.0 * torch.eye(2, device=DEV))
    u = draw()[0]                                                   # a new law
    assert len(calls) == 6 and torch.allclose(u, 2.0 * first / math.sqrt(sun.distribution_parameters["covariance"]),
                                              rtol=1e-5, atol=1e-6)
    u2 = draw()[0]
    assert len(calls) == 6 and u2.data_ptr() == u.data_ptr()
    del u, u2
    assert settled() <= 2048

    u = draw()[0]
    u.add_(1.0)                                                     # a caller wrote into the shared sample
    u2 = draw()[0]
    assert len(calls) == 7 and torch.allclose(u2 + 1.0, u)
    sun.clear_distortion_cache()
    del u, u2
    u = draw()[0]
    assert len(calls) == 8
