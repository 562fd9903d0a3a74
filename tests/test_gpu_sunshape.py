"""The radial sun shapes on the GPU (``-m gpu``): ``art_sample_radial_distortions`` against the numpy restatement of its recipe
(tests/sunshape_ref.py), the law of its draws, the rank-sharding invariant, the per-sun sample cache keyed by the table, and a
pillbox sun through the ray tracer against the oracle."""
import math

import numpy as np
import pytest
import torch

import oracle
import sunshape_ref
from conftest import rel_l2
from sunshape_ref import DISC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def n(x):
    return x.detach().cpu().numpy()


def radial_sun(kind, rays, **params):
    from artist_amd.scene import Sun
    return Sun(rays, dict(distribution_type=kind, **params), device=DEV, sampler="hip")


def build_field(H, R, sun=None, n_cp=6, n_eval=8):
    """The synthetic field of tests/test_gpu_sampler.py; ``sun`` replaces its light source (default: its normal sun on "hip")."""
    from artist_amd import scene
    scenario, _ = scene.build_synthetic_scenario(H, n_rays=R, n_cp=(n_cp, n_cp), n_eval=n_eval, device=DEV)
    if sun is None:
        scenario.light_sources.light_source_list[0].sampler = "hip"
    else:
        scenario.light_sources.light_source_list[0] = sun
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=DEV)
    group.activate_heliostats(mask)
    tix = torch.zeros(H, dtype=torch.long, device=DEV)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
    return scenario, group, mask, tix, inc


@pytest.fixture(scope="module")
def tables():
    """name -> the fp32 quantile table on the device: Buie at chi = 0.05 (K = 1024) and the pillbox (K = 1)."""
    return {"buie": radial_sun("buie", 1).quantile_table, "pillbox": radial_sun("pillbox", 1).quantile_table}


# ---- 1. known answer -------------------------------------------------------------------------------------------------
ROWS = [0, 5, (1 << 32) + 3]
# A lone tail ray; an odd R*P (the float2 stores); and, with three rows, a grid of ceil(8192 / 3) = 2731 workgroups of 256
# lanes per row, 699136 lanes: 750000 pairs make every lane's loop over the pairs wrap.
SIZES = [(1, 1), (3, 667), (3, 500000)]


@pytest.mark.parametrize("seed", [7, -5876543210123])
@pytest.mark.parametrize("R, P", SIZES)
def test_known_answer_against_the_restated_rule(seed, R, P, tables):
    from artist_amd import ops
    assert (SIZES[2][0] * SIZES[2][1] + 1) // 2 > -(-8192 // len(ROWS)) * 256
    for name in ("buie", "pillbox"):                                # the pillbox right after Buie: a stale table would show
        table = tables[name]
        out = ops.sample_radial_distortions(ROWS, R, P, seed, (0.0, 0.0), table, DEV)
        assert out.shape == (3, R, P, 2) and out.dtype == torch.float32 and out.is_contiguous()
        got = n(out).reshape(3, R * P, 2).astype(np.float64)
        ref = sunshape_ref.radial_rows(seed, ROWS, R * P, n(table))
        bound = 1e-5 * math.sqrt(float(table[-1]))
        err = np.abs(got - ref)
        print(f"{name}, seed {seed}, R*P {R * P}: max |hip - restatement| = {err.max():.2e} (bound {bound:.2e})")
        assert err.max() <= bound, np.unravel_index(err.argmax(), err.shape)


def test_known_answer_with_a_centre(tables):
    from artist_amd import ops
    loc, R, P = (1e-3, -2e-3), 3, 667
    for name in ("buie", "pillbox"):
        table = tables[name]
        got = n(ops.sample_radial_distortions(ROWS[1:], R, P, 7, loc, table, DEV)).reshape(2, R * P, 2).astype(np.float64)
        ref = sunshape_ref.radial_rows(7, ROWS[1:], R * P, n(table), loc)
        assert np.abs(got - ref).max() <= 1e-5 * math.sqrt(float(table[-1]))


# ---- 2. law ------------------------------------------------------------------------------------------------------------
LAWS = {"buie": (dict(circumsolar_ratio=0.05), lambda: sunshape_ref.buie_law(0.05),
                 (1e-3, 2e-3, 3e-3, 4e-3, 4.6e-3, 5e-3, 7e-3, 10e-3, 20e-3, 40e-3)),
        "pillbox": (dict(), lambda: sunshape_ref.PillboxLaw(DISC),
                    tuple(f * DISC for f in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.97)))}


@pytest.mark.parametrize("kind", ["buie", "pillbox"])
def test_law_of_the_hip_draws(kind):
    params, law, radii = LAWS[kind]
    rows, R, P = 10, 10, 100000                                      # 1e7 draws
    sun = radial_sun(kind, R, **params)
    u, e = sun.get_distortions(number_of_points=P, number_of_active_heliostats=rows)
    assert u.shape == (rows, R, P) and e.data_ptr() == u.data_ptr() + 4
    theta = sunshape_ref.check_radial_law(u, e, (0.0, 0.0), law(), radii, sun.quantile_table.shape[0] - 1)
    if kind == "pillbox":
        assert float(theta.max()) <= DISC * (1 + 1e-6)
    w = torch.stack((u, e), -1).double().reshape(rows, R * P, 2)
    for comp in (0, 1):                                              # as tests/test_gpu_sampler.py::_check_law
        a, b = w[:, :-1, comp].reshape(-1), w[:, 1:, comp].reshape(-1)          # neighbouring rays (inside and across pairs)
        r = sunshape_ref.correlation(a, b)
        assert abs(r) <= 4 / math.sqrt(a.numel()), ("rays", comp, r)
        r = sunshape_ref.correlation(w[0, :, comp], w[1, :, comp])              # rows 0 and 1
        assert abs(r) <= 4 / math.sqrt(R * P), ("rows", comp, r)


# ---- 3. sharding -------------------------------------------------------------------------------------------------------
def test_rank_rows_of_a_buie_sun_are_the_rows_of_the_full_draw():
    from artist_amd import HeliostatRayTracer, ops
    H, R = 7, 4
    sun = radial_sun("buie", R)
    scenario, group, mask, tix, inc = build_field(H, R, sun)
    full = HeliostatRayTracer(scenario, group, blocking_active=False).distortions_dataset
    fu, fe = full.distortions_u, full.distortions_e
    P = fu.shape[2]
    assert float(torch.sqrt(fu * fu + fe * fe).max()) > DISC         # a Buie sample: some ray lies in the aureole
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
    a = ops.sample_radial_distortions(list(range(H)), R, P, 7, (0.0, 0.0), sun.quantile_table, DEV)
    b = ops.sample_radial_distortions(torch.arange(H, device=DEV), R, P, 7, (0.0, 0.0), sun.quantile_table, DEV)
    assert torch.equal(a, b) and torch.equal(a[..., 0], fu) and torch.equal(a[..., 1], fe)


def test_torch_sampler_rows_of_a_radial_sun_on_the_device():
    """The "torch" sampler of a radial sun on the GPU: per-row streams (a row's bits whatever the other rows), the same law."""
    sun = radial_sun("pillbox", 8)
    sun.sampler = "torch"
    u, e = sun.get_distortions(number_of_points=5000, number_of_active_heliostats=5)
    pu, pe = sun.get_distortions_rows([3, 0], number_of_points=5000, number_of_active_heliostats=5)
    assert torch.equal(pu, u[[3, 0]]) and torch.equal(pe, e[[3, 0]]) and pe.data_ptr() == pu.data_ptr() + 4
    sunshape_ref.check_radial_law(u, e, (0.0, 0.0), sunshape_ref.PillboxLaw(DISC), LAWS["pillbox"][2], 1)


# ---- 4. cache ----------------------------------------------------------------------------------------------------------
def test_sample_cache_tells_two_tables_apart(monkeypatch):
    from artist_amd import HeliostatRayTracer, _lib
    H, R = 5, 4
    sun = radial_sun("buie", R)
    scenario, group, mask, tix, inc = build_field(H, R, sun)
    P = group.active_surface_points.shape[1]
    handle = _lib.lib()
    real = handle.art_sample_radial_distortions
    calls = []

    def counted(*args):
        calls.append(args[8])                                        # K
        return real(*args)

    monkeypatch.setattr(handle, "art_sample_radial_distortions", counted)
    rt1 = HeliostatRayTracer(scenario, group, blocking_active=False)
    rt2 = HeliostatRayTracer(scenario, group, blocking_active=False)
    assert calls == [1024]                                          # the second tracer: a hit, no launch
    assert rt2.distortions_dataset.distortions_u.data_ptr() == rt1.distortions_dataset.distortions_u.data_ptr()
    first = rt1.distortions_dataset.distortions_u.clone()
    del rt1, rt2
    draw = lambda seed=7: sun.get_distortions_rows(range(H), number_of_points=P, number_of_active_heliostats=H,  # noqa: E731
                                                   random_seed=seed)[0]
    torch.cuda.set_sync_debug_mode("error")                         # neither a hit nor a miss waits for the device
    try:
        hit = draw()
        other_seed = draw(seed=8)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(calls) == 2 and torch.equal(hit, first) and not torch.equal(other_seed, first)
    del hit, other_seed

    assert torch.equal(draw(), first) and len(calls) == 3
    sun.quantile_table.mul_(4.0)                                    # an in-place write: drawn anew, every radius doubled
    doubled = draw()
    assert len(calls) == 4 and torch.allclose(doubled, 2.0 * first, rtol=1e-5, atol=1e-9)
    assert draw().data_ptr() == doubled.data_ptr() and len(calls) == 4
    del doubled

    sun.quantile_table = radial_sun("pillbox", R).quantile_table    # another table: drawn anew, with K = 1
    disc = draw()
    assert calls[4:] == [1] and float(torch.abs(disc).max()) <= DISC * (1 + 1e-6)
    same_values = sun.quantile_table.clone()                        # equal values in a new tensor: a new table all the same
    sun.quantile_table = same_values
    again = draw()
    assert len(calls) == 6 and torch.equal(again, disc)


# ---- 5. through the tracer ---------------------------------------------------------------------------------------------
def test_pillbox_flux_through_the_ray_tracer_and_nothing_left_behind():
    from artist_amd import HeliostatRayTracer
    H, R = 2, 4
    scenario, group, mask, tix, inc = build_field(H, R)
    sources = scenario.light_sources.light_source_list
    normal, pillbox = sources[0], radial_sun("pillbox", R)
    planar = scenario.solar_tower.target_areas[0]

    def trace(sun):
        sources[0] = sun
        rt = HeliostatRayTracer(scenario, group, blocking_active=False)
        flux, *_ = rt.trace_rays(inc, mask, tix)
        return rt, flux.detach().clone()

    _, before = trace(normal)
    rt, flux = trace(pillbox)
    du, de = rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e
    assert float(torch.sqrt(du * du + de * de).max()) <= DISC * (1 + 1e-6)
    o_flux, _ = oracle.trace_fwd(n(group.active_surface_points), n(group.active_surface_normals), n(inc), n(du), n(de),
                                 n(tix).astype(np.int32), n(planar.centers), n(planar.normals), n(planar.dimensions), (256, 256))
    err = rel_l2(n(flux), o_flux)
    print(f"pillbox flux vs oracle on the same distortions: rel L2 {err:.2e}")
    assert err < 1e-6
    normal.clear_distortion_cache()                                 # the normal sun draws again after the radial launch
    _, after = trace(normal)
    assert torch.equal(before, after) and not torch.equal(before, flux)
