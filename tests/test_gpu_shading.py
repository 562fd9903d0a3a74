"""Heliostat shading on the GPU (``-m gpu``): the cull, the sheared tables and their adjoint against tests/shading_ref.py, the
shaded flux against first principles (sunward rays, no shear) and against the CPU restatement of the trace given the GPU's
own virtual rows, and what the feature must leave alone: defaults, overflow reporting, no waiting, sharding.

The field: six flat heliostats in two rows behind one another along the sun's azimuth, sun elevation 15 degrees, four facets
of 8 x 8 points, a 64 x 64 bitmap.  The surfaces are built in NumPy (tests/shading_ref.py: field) and handed to the group, so
that the conditions the tests rest on - who is shaded, how far everything is from a threshold or a shadow edge - are checked
from the same numbers in fp64.
"""
import numpy as np
import pytest
import torch

import oracle
import shading_ref as ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RES = (64, 64)
AIM = (0.0, 0.0, 40.0)
LOW_SUN = np.array([0.0, np.cos(np.radians(15.0)), -np.sin(np.radians(15.0)), 0.0])
HIGH_SUN = np.array([0.0, np.cos(np.radians(70.0)), -np.sin(np.radians(70.0)), 0.0])
POSITIONS = np.array([[-6.0, 100.0, 0.0], [0.0, 100.0, 0.0], [6.0, 100.0, 0.0],
                      [-5.66, 105.26, 0.0], [0.34, 105.26, 0.0], [6.56, 105.26, 0.0]])
# the same field with the back row where the front row's upper shadow edge runs along a row of surface points (2 to 4 mm off): rays cross it
ON_EDGE = np.array([[-6.0, 100.0, 0.0], [0.0, 100.0, 0.0], [6.0, 100.0, 0.0], [-5.66, 105.6, 0.0], [0.34, 105.6, 0.0], [6.56, 105.6, 0.0]])
CROWDED = np.array([[-1.7, 100.0, 0.0], [1.7, 100.0, 0.0], [0.0, 105.26, 0.0], [9.0, 100.0, 0.0]])    # heliostat 2 has two shaders


def n(x):
    return x.detach().cpu().numpy()


def t(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def make_field(positions=POSITIONS, sun=LOW_SUN, rays=4):
    """``(scenario, group, mask, tix, incident, points64, normals64)``: the scenario stand-in with the NumPy-built surfaces as
    the group's aligned surfaces (every heliostat active, one planar target)."""
    from artist_amd.scene import build_synthetic_scenario
    H = len(positions)
    points, normals = ref.field(positions, sun, AIM)
    scenario, _ = build_synthetic_scenario(H, rays, n_eval=8, z_noise=0.0, device=DEV, target_centers=((*AIM, 1.0),))
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=DEV)
    group.activate_heliostats(mask, DEV)
    group.positions = t(np.concatenate([positions, np.ones((H, 1))], 1))
    group.active_surface_points, group.active_surface_normals = t(points), t(normals)
    tix = torch.zeros(H, dtype=torch.long, device=DEV)
    incident = t(np.tile(sun, (H, 1)))
    return scenario, group, mask, tix, incident, points, normals


def tracer(scenario, group, **kw):
    from artist_amd import HeliostatRayTracer
    rt = HeliostatRayTracer(scenario, group, bitmap_resolution=torch.tensor(RES), **kw)
    rt.lbvh_compat = False
    return rt


@pytest.fixture(scope="module")
def scene():
    """The field, its fp64 reference quantities (computed once, never modified) and the conditions every test relies on."""
    scenario, group, mask, tix, incident, points, normals = make_field()
    corners32 = n(ref_corners(group))
    owner = np.arange(len(POSITIONS))
    inc = np.tile(LOW_SUN, (len(POSITIONS), 1))
    rt = tracer(scenario, group, shading_active=True)
    scatter = rt._max_scatter_angle()
    listed, margin = ref.cull(corners32.astype(np.float64), owner, inc.astype(np.float32).astype(np.float64), scatter)
    assert margin[np.isfinite(margin)].min() > 1e-4, margin            # no rectangle within 1e-4 (relative) of the cull threshold
    tau = ref.direct_transmittance(n(group.active_surface_points).astype(np.float64), owner, inc, corners32.astype(np.float64))
    shaded = 1.0 - tau.mean(1)
    assert (shaded[:3] < 1e-9).all() and ((shaded[3:] > 0.2) & (shaded[3:] < 0.8)).all(), shaded   # a free row, a partly shaded one
    return dict(scenario=scenario, group=group, mask=mask, tix=tix, incident=incident, corners=corners32, owner=owner, inc=inc,
                listed=listed, scatter=scatter, tau=tau, rt=rt)


def ref_corners(group):
    from artist_amd.blocking import create_blocking_primitives_rectangles_by_index
    return create_blocking_primitives_rectangles_by_index(group.active_surface_points)[0]


def gpu_tables(sc, slots=8):
    from artist_amd.blocking import create_shading_primitives
    return create_shading_primitives(t(sc["corners"]), torch.arange(len(sc["owner"]), dtype=torch.int32, device=DEV), sc["incident"],
                                     sc["scatter"], slots)


def test_cull_lists_equal_the_reference_rule(scene):
    from artist_amd.blocking import shading_cull
    for slots in (8, 1):
        idx, count = shading_cull(t(scene["corners"]), torch.arange(6, dtype=torch.int32, device=DEV), scene["incident"],
                                  scene["scatter"], slots)
        want_idx, want_count = ref.cull_lists(scene["listed"], slots)
        np.testing.assert_array_equal(n(idx), want_idx)
        np.testing.assert_array_equal(n(count), want_count)
    assert want_count.tolist() == [0, 0, 0, 1, 1, 1]
    # a field in which the lists are longer than one entry, and longer than the slots
    scenario, group, mask, tix, incident, _, _ = make_field(CROWDED)
    corners = n(ref_corners(group))
    listed, margin = ref.cull(corners.astype(np.float64), np.arange(4), np.tile(LOW_SUN, (4, 1)).astype(np.float32).astype(np.float64), 0.01)
    assert margin[np.isfinite(margin)].min() > 1e-4
    for slots in (8, 1):
        idx, count = shading_cull(t(corners), torch.arange(4, dtype=torch.int32, device=DEV), incident, 0.01, slots)
        want_idx, want_count = ref.cull_lists(listed, slots)
        np.testing.assert_array_equal(n(idx), want_idx)
        np.testing.assert_array_equal(n(count), want_count)
    assert want_count[2] == 2
    # a sun in the mirror's plane: no shaders, whatever lies around
    grazing = scene["incident"].clone()
    normal = np.cross(scene["corners"][4, 1, :3] - scene["corners"][4, 0, :3], scene["corners"][4, 3, :3] - scene["corners"][4, 0, :3])
    along = np.cross(normal, [1.0, 0.0, 0.0])
    grazing[4, :3] = t(along / np.linalg.norm(along))
    idx, count = shading_cull(t(scene["corners"]), torch.arange(6, dtype=torch.int32, device=DEV), grazing, scene["scatter"], 8)
    assert int(count[4]) == 0 and (n(idx[4]) == -1).all() and int(count[3]) == 1


def test_tables_equal_the_fp64_reference(scene):
    """The bound: 8 times the distance between the reference evaluated in fp32 and in fp64 on this scene (largest absolute
    difference), floor 1e-5 m.  Measured on MI355X: see DESIGN.md 4.9."""
    tabs = gpu_tables(scene)
    idx = n(tabs["shader_idx"])
    inc32 = n(scene["incident"])
    want = ref.shear_tables(scene["corners"].astype(np.float64), scene["owner"], inc32.astype(np.float64), idx)
    in32 = ref.shear_tables(scene["corners"], scene["owner"], inc32, idx, np.float32)
    for name, got, w64, w32 in zip(("corners", "spans", "normals"), (tabs["corners"], tabs["spans"], tabs["normals"]), want, in32):
        yard = float(np.abs(w32.astype(np.float64) - w64).max())
        err = float(np.abs(n(got).astype(np.float64) - w64).max())
        print(f"shading tables, {name}: GPU - fp64 {err:.2e}, reference fp32 - fp64 {yard:.2e}")
        assert err <= max(8.0 * yard, 1e-5), (name, err, yard)
    empty = (idx.reshape(-1) < 0)
    assert empty.any() and not n(tabs["corners"])[empty].any() and not n(tabs["spans"])[empty].any() and not n(tabs["normals"])[empty].any()


def test_shaded_flux_equals_first_principles(scene):
    """Flat mirrors, an all-zero distortion sample, R = 1, shading only: the bitmap is the CPU restatement's unblocked per-ray
    intensities times the DIRECT per-point transmittance (sunward rays against the real rectangles), splatted.  This leg
    never touches the sheared tables.  Bound: test_blocking_forward's 2e-6 plus the relative L2 that the reference's own
    fp32-vs-fp64 transmittances produce in that product."""
    scenario, group, mask, tix, incident, points, normals = make_field(rays=1)
    rt = tracer(scenario, group, blocking_active=False, shading_active=True)
    P = group.active_surface_points.shape[1]
    zeros = torch.zeros((6, 1, P), device=DEV)
    rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e = zeros, zeros.clone()
    flux, intercept, on_target, unshaded = rt.trace_rays(incident, mask, tix)
    pts32 = n(group.active_surface_points)
    edge = ref.shadow_edge_distance(pts32, scene["owner"], scene["inc"], scene["corners"])
    assert edge.min() > 0.05, edge.min()                       # no surface point within 5 cm of a shadow edge
    planar = scenario.solar_tower.target_areas[0]
    _, _, dbg = oracle.trace_fwd(pts32, n(group.active_surface_normals), n(incident), n(zeros), n(zeros), n(tix), n(planar.centers),
                                 n(planar.normals), n(planar.dimensions), RES, debug=True)
    tau64 = ref.direct_transmittance(pts32.astype(np.float64), scene["owner"], n(incident).astype(np.float64), scene["corners"].astype(np.float64))
    tau32 = ref.direct_transmittance(pts32, scene["owner"], n(incident), scene["corners"], np.float32)
    inten = dbg["intensities"][:, 0].astype(np.float64) * np.float64(np.float32(0.935))

    def bitmaps(tau):
        return np.stack([oracle.splat(dbg["e_px"][h, 0].astype(np.float64), dbg["u_px"][h, 0].astype(np.float64), inten[h] * tau[h], RES)
                         for h in range(6)])
    want = bitmaps(tau64)
    yard = rel_l2(bitmaps(tau32.astype(np.float64)), want)
    err = rel_l2(n(flux).astype(np.float64), want)
    print(f"shaded flux against first principles: {err:.2e} (reference fp32 - fp64 in the product: {yard:.2e})")
    assert err < 2e-6 + yard, (err, yard)
    rays = P
    np.testing.assert_allclose(n(unshaded), (1.0 - tau64 < 1e-3).mean(1), rtol=0, atol=1.5 / rays)      # (free = blocked < 1e-3)
    assert float(unshaded[:3].min()) == 1.0 and 0.2 < float(unshaded[3:].max()) < 0.8
    assert float(flux[4].sum()) < 0.8 * float(flux[1].sum())


def test_flux_and_gradients_against_the_cpu_restatement(scene):
    """Blocking and shading both on, random distortions.  For each heliostat separately (H = 1, no tree compatibility) the
    fp32 CPU restatement traces with the real tables plus the GPU's own virtual rows of that heliostat, forward and backward:
    flux within 2e-6, gradients of points, normals and the three tables within 2e-5 (test_blocking_forward / _backward).
    The back row stands where a shadow edge runs along a row of surface points, so that the scattered rays cross it and the
    virtual rows receive gradients worth comparing (away from an edge they are the sigmoids' e^-30 tails, which the kernels
    skip)."""
    from artist_amd import ops
    from artist_amd.blocking import create_blocking_primitives_rectangles_by_index
    scenario, group, mask, tix, incident, _, _ = make_field(ON_EDGE)
    rt = tracer(scenario, group, shading_active=True)
    corners32 = n(ref_corners(group))
    edge = ref.shadow_edge_distance(n(group.active_surface_points), np.arange(6), np.tile(LOW_SUN, (6, 1)), corners32)
    assert ((edge < 0.006).sum(1) >= 8).tolist() == [False] * 3 + [True] * 3              # a row of points within 6 mm of an edge
    scene = dict(scenario=scenario, group=group, tix=tix, incident=incident, corners=corners32, owner=np.arange(6),
                 scatter=rt._max_scatter_angle())
    _, margin = ref.cull(corners32.astype(np.float64), scene["owner"], n(incident).astype(np.float64), scene["scatter"])
    assert margin[np.isfinite(margin)].min() > 1e-4
    H, S = 6, 8
    points = group.active_surface_points.detach().clone().requires_grad_(True)
    normals = group.active_surface_normals.detach().clone().requires_grad_(True)
    corners, spans, pnormals = (x.detach().requires_grad_(True) for x in create_blocking_primitives_rectangles_by_index(points))
    tabs = gpu_tables(scene)
    shade = dict(tabs, **{k: tabs[k].detach().requires_grad_(True) for k in ("corners", "spans", "normals")})
    du, de = rt.distortions_dataset.distortions_u, rt.distortions_dataset.distortions_e
    planar = scene["scenario"].solar_tower.target_areas[0]
    owner = torch.arange(H, dtype=torch.int32, device=DEV)
    flux, factors, _ = ops.trace_rays(points, normals, scene["incident"], du, de, scene["tix"], planar.centers, planar.normals,
                                      planar.dimensions, resolution=RES,
                                      blocking=dict(corners=corners, spans=spans, normals=pnormals, owner=owner,
                                                    max_scatter_angle=scene["scatter"], lbvh_compat=False), shading=shade)
    w = torch.rand(flux.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    (flux * w).sum().backward()
    assert float(factors[2, 3:].max()) < 0.8 and float(factors[2, :3].min()) > 0.8
    idx = n(tabs["shader_idx"])
    real = [np.zeros_like(n(x)) for x in (corners, spans, pnormals)]
    worst = {}
    for h in range(H):
        rows = [h * S + k for k in range(S) if idx[h, k] >= 0]
        blk = dict(corners=np.concatenate([n(corners), n(shade["corners"])[rows]]), spans=np.concatenate([n(spans), n(shade["spans"])[rows]]),
                   normals=np.concatenate([n(pnormals), n(shade["normals"])[rows]]), owner=np.array([h], np.int32), lbvh_compat=False)
        common = (n(points)[h:h + 1], n(normals)[h:h + 1], n(scene["incident"])[h:h + 1], n(du)[h:h + 1], n(de)[h:h + 1], n(scene["tix"])[h:h + 1],
                  n(planar.centers), n(planar.normals), n(planar.dimensions), RES)
        o_flux, o_fac = oracle.trace_fwd(*common, blocking=blk)
        go, gn, gpc, gps, gpn = oracle.trace_bwd(*common, n(w)[h:h + 1], blocking=blk)
        pairs = [("flux", n(flux)[h], o_flux[0]), ("points", n(points.grad)[h], go[0]), ("normals", n(normals.grad)[h], gn[0])]
        if rows:
            pairs += [("shade corners", n(shade["corners"].grad)[rows], gpc[H:]), ("shade spans", n(shade["spans"].grad)[rows], gps[H:]),
                      ("shade normals", n(shade["normals"].grad)[rows], gpn[H:])]
        for name, got, want in pairs:
            if np.linalg.norm(want) == 0:
                assert not got.any(), (h, name)
                continue
            if name.startswith("shade"):                        # rays do cross the edge: these are not the sigmoids' tails
                assert np.linalg.norm(want) > 1e-6 * np.linalg.norm(go), (h, name, np.linalg.norm(want), np.linalg.norm(go))
            worst[name] = max(worst.get(name, 0.0), rel_l2(got, want))
        for acc, g in zip(real, (gpc, gps, gpn)):
            acc += g[:H]
        np.testing.assert_allclose(n(factors)[:, h], o_fac[:, 0], rtol=0, atol=1.5 / (du.shape[1] * du.shape[2]))
    for name, got, want in (("corners", corners.grad, real[0]), ("spans", spans.grad, real[1]), ("rectangle normals", pnormals.grad, real[2])):
        worst[name] = rel_l2(n(got), want)
    print("against the CPU restatement: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert set(worst) >= {"flux", "points", "normals", "shade corners", "shade spans", "shade normals", "corners", "spans", "rectangle normals"}
    for name, err in worst.items():
        assert err < (2e-6 if name == "flux" else 2e-5), (name, err)


def test_adjoint_of_the_tables(scene):
    """``art_shading_prims_bwd`` against autograd through the fp64 reference in torch on the CPU: relative L2 within 4 times
    that reference's own fp32-vs-fp64 distance; two runs give the same bits."""
    from artist_amd.blocking import ShadingTables
    scenario, group, mask, tix, incident, _, _ = make_field(CROWDED)          # (both paths, and a rectangle that shades two)
    H, S = 4, 8
    corners0 = n(ref_corners(group))
    from artist_amd.blocking import shading_cull
    owner = torch.arange(H, dtype=torch.int32, device=DEV)
    idx, count = shading_cull(t(corners0), owner, incident, 0.01, S)
    assert n(count).tolist()[2] == 2
    gen = torch.Generator().manual_seed(5)
    weights = [torch.rand((H * S, 4, 3), generator=gen, dtype=torch.float64), torch.rand((H * S, 2, 3), generator=gen, dtype=torch.float64),
               torch.rand((H * S, 3), generator=gen, dtype=torch.float64)]

    def gpu():
        c = t(corners0).requires_grad_(True)
        tabs = ShadingTables.apply(c, owner, incident, idx)
        sum((x[..., :3] * wt.to(DEV, torch.float32)).sum() for x, wt in zip(tabs, weights)).backward()
        return c.grad

    def cpu(dtype):
        c = torch.from_numpy(corners0).to(dtype).requires_grad_(True)
        tabs = ref.shear_tables_torch(c, n(owner), n(incident), n(idx))
        sum((x * wt.to(dtype)).sum() for x, wt in zip(tabs, weights)).backward()
        return c.grad.numpy().astype(np.float64)

    first, second = gpu(), gpu()
    assert torch.equal(first, second)
    g64, g32 = cpu(torch.float64), cpu(torch.float32)
    yard, err = rel_l2(g32, g64), rel_l2(n(first).astype(np.float64), g64)
    print(f"adjoint of the shading tables: GPU - fp64 {err:.2e}, reference fp32 - fp64 {yard:.2e}")
    assert np.abs(g64[:3, :, :3]).sum(axis=(1, 2)).min() > 0 and not n(first)[..., 3].any()   # shaders and shaded get some, w none
    assert not n(first)[3].any() and not g64[3].any()                                         # the bystander is written too: zeros
    assert err <= 4.0 * yard, (err, yard)


def test_default_is_unchanged_and_a_high_sun_shades_nothing(scene):
    from artist_amd import HeliostatRayTracer
    scenario, group, mask, tix, incident = (scene[k] for k in ("scenario", "group", "mask", "tix", "incident"))
    plain = HeliostatRayTracer(scenario, group, bitmap_resolution=torch.tensor(RES))
    off = HeliostatRayTracer(scenario, group, bitmap_resolution=torch.tensor(RES), shading_active=False)
    for a, b in zip(plain.trace_rays(incident, mask, tix), off.trace_rays(incident, mask, tix)):
        assert torch.equal(a, b)
    on = tracer(scenario, group, shading_active=True).trace_rays(incident, mask, tix)
    assert not torch.equal(on[0], tracer(scenario, group).trace_rays(incident, mask, tix)[0])       # (here shading does matter)
    scenario, group, mask, tix, incident, _, _ = make_field(sun=HIGH_SUN)
    for blocking in (True, False):
        with_shading = tracer(scenario, group, blocking_active=blocking, shading_active=True)
        res_on = with_shading.trace_rays(incident, mask, tix)
        res_off = tracer(scenario, group, blocking_active=blocking).trace_rays(incident, mask, tix)
        assert int(with_shading._shading[1].sum()) == 0
        for a, b in zip(res_on, res_off):
            assert torch.equal(a, b)
    assert float(res_on[0].sum()) > 0


def test_more_shaders_than_slots_is_reported_as_nan(scene, monkeypatch):
    from artist_amd import ops
    scenario, group, mask, tix, incident, _, _ = make_field(CROWDED)
    good = tracer(scenario, group, shading_active=True).trace_rays(incident, mask, tix)
    assert all(bool(torch.isfinite(x).all()) for x in good)
    monkeypatch.setattr(ops, "SHADING_SLOTS", 1)
    rt = tracer(scenario, group, shading_active=True)
    flux, *factors = rt.trace_rays(incident, mask, tix)
    assert n(rt._shading[1]).tolist()[2] == 2
    assert bool(torch.isnan(flux[2]).all()) and all(bool(torch.isnan(f[2])) for f in factors)
    for h in (0, 1, 3):
        assert torch.equal(flux[h], good[0][h]) and all(torch.equal(f[h], g[h]) for f, g in zip(factors, good[1:]))
    ops.check_async_errors(DEV)                                 # the report is the NaN: the device status stays clear


@pytest.mark.parametrize("blocking", [False, True])
def test_shaded_trace_does_not_wait_for_the_device(scene, blocking):
    """``test_trace_rays_does_not_wait_for_the_device`` with shading on: the cull, the tables, their adjoint and the append
    queue behind one another; no count is read back."""
    scenario, group, mask, tix, incident = (scene[k] for k in ("scenario", "group", "mask", "tix", "incident"))
    saved = group.active_surface_points
    points = saved.detach().clone().requires_grad_(True)
    group.active_surface_points = points
    try:
        rt = tracer(scenario, group, blocking_active=blocking, shading_active=True)
        weights = torch.rand((6, *RES), device=DEV)

        def epoch():
            flux, intercept, on_target, unblocked = rt.trace_rays(incident, mask, tix)
            points.grad = None
            (flux * weights).sum().backward(retain_graph=True)      # (the rectangles hang off the constructor's graph)
            return rt.get_bitmaps_per_target(flux.detach(), tix)

        epoch()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            per_target = epoch()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert float(per_target.sum()) > 0 and float(points.grad.abs().sum()) > 0
    finally:
        group.active_surface_points = saved


def test_sharded_shading_equals_single_rank(scene):
    """A 3-rank split: every rank gets exactly its rows of the unsharded result."""
    scenario, group, mask, tix, incident = (scene[k] for k in ("scenario", "group", "mask", "tix", "incident"))
    for blocking in (True, False):
        whole = tracer(scenario, group, blocking_active=blocking, shading_active=True).trace_rays(incident, mask, tix)
        assert float(whole[3].min()) < 0.8
        seen = []
        for rank in range(3):
            part = tracer(scenario, group, blocking_active=blocking, shading_active=True, world_size=3, rank=rank)
            rows = part.get_sampler_indices()
            seen += rows.tolist()
            for got, want in zip(part.trace_rays(incident, mask, tix), whole):
                assert torch.equal(got, want[rows])
        assert sorted(seen) == list(range(6))
