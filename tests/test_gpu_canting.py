"""The facet canting on the GPU (``-m gpu``): ``artist_amd.perform_canting`` / ``ops.CantFacets`` and the route
``NURBSSurfaces`` takes when the canting vectors or the facet translations learn - bit identity with the fused evaluation,
gradients against the reference's own (tests/golden/canting.npz, generate_canting_golden.py) and against the fp64 restatement
(tests/canting_ref.py) at the workload's shape, reproducibility, launch counts, and one descent step end to end."""
import numpy as np
import pytest
import torch

import canting_ref as ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def bound(yard):
    return max(3 * yard, 1e-5)


def _group(c):
    """The case's leaves in a ``scene.HeliostatGroup``, activated with the case's mask: ``active_canting`` and its kin come
    from ``repeat_interleave``, which keeps the graph (a heliostat listed twice collects both replicas' gradients)."""
    from artist_amd.scene import HeliostatGroup
    Hb = c["canting"].shape[0]
    cant, tr, cp = (t(c[k]).requires_grad_(True) for k in ("canting", "translations", "cp"))
    group = HeliostatGroup(names=[f"h{i}" for i in range(Hb)], positions=torch.zeros(Hb, 4, device=DEV),
                           surface_points=torch.zeros(Hb, 1, 4, device=DEV), surface_normals=torch.zeros(Hb, 1, 4, device=DEV),
                           canting=cant, facet_translations=tr, nurbs_control_points=cp, nurbs_degrees=torch.tensor(c["degrees"]),
                           device=DEV)
    group.activate_heliostats(t(c["mask"], torch.int32))
    return group, cant, tr, cp


def _surfaces(group, c, orientations=None, detach=False):
    from artist_amd import NURBSSurfaces
    d = (lambda x: x.detach()) if detach else (lambda x: x)
    return NURBSSurfaces(group.nurbs_degrees, group.active_nurbs_control_points, device=DEV).calculate_surface_points_and_normals(
        t(c["uv"]), d(group.active_canting), d(group.active_facet_translations), orientations=orientations)


def _orientations(H, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.eye(4).repeat(H, 1, 1) + 0.3 * torch.randn(H, 4, 4, generator=g)).to(DEV)


# ---- 1. bit identity ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ref.CASES)
def test_two_stage_route_equals_the_fused_evaluation_on_every_fixture_case(golden, name):
    c = ref.fixture_case(golden("canting"), name)
    group, *_ = _group(c)
    H = int(c["mask"].sum())
    for ori in (None, _orientations(H)):
        fused = _surfaces(group, c, ori, detach=True)
        staged = _surfaces(group, c, ori)
        assert staged[0].requires_grad and staged[1].requires_grad
        assert torch.equal(fused[0], staged[0].detach()) and torch.equal(fused[1], staged[1].detach())
    pts, nrm = _surfaces(group, c)
    assert rel_l2(n(pts), c["points"]) < 1e-6 and rel_l2(n(nrm), c["normals"]) < 1e-6


@pytest.mark.parametrize("M", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("H, F", [(1, 1), (1, 2), (3, 4)])
def test_two_stage_route_equals_the_fused_evaluation_at_every_size(M, H, F):
    """Scattered evaluation points (M need not be a grid), random nets, cantings whose n is not orthogonal to e."""
    from artist_amd import ops
    g = torch.Generator().manual_seed(100 * M + 10 * H + F)
    cp = torch.randn(H, F, 5, 6, 3, generator=g).to(DEV)
    uv = (0.02 + 0.96 * torch.rand(H, F, M, 2, generator=g)).to(DEV)
    cant = torch.randn(H, F, 2, 4, generator=g).to(DEV)
    tr = torch.randn(H, F, 4, generator=g).to(DEV)
    knots = [torch.cat([torch.zeros(3), torch.linspace(0, 1, k - 2), torch.ones(3)]).to(DEV) for k in (5, 6)]
    for ori in (None, _orientations(H)):
        fused = ops.nurbs_surface_points_and_normals(cp, uv, knots[0], knots[1], (3, 3), cant, tr, orientation=ori)
        for learns in ((True, False), (False, True), (True, True)):
            c2, t2 = cant.clone().requires_grad_(learns[0]), tr.clone().requires_grad_(learns[1])
            staged = ops.nurbs_surface_points_and_normals(cp, uv, knots[0], knots[1], (3, 3), c2, t2, orientation=ori)
            assert staged[0].requires_grad
            assert torch.equal(fused[0], staged[0].detach()) and torch.equal(fused[1], staged[1].detach())


@pytest.mark.parametrize("name", ref.CASES)
def test_perform_canting_against_the_reference_and_there_and_back(golden, name):
    from artist_amd import perform_canting
    c = ref.fixture_case(golden("canting"), name)
    cant, data = t(c["canting"]), t(c["pc_data"])
    fwd, inv = perform_canting(cant, data), perform_canting(cant, data, inverse=True)
    assert fwd.shape == data.shape and fwd.dtype == torch.float32
    yard = max(rel_l2(c["pc_fwd"], c["pc_fwd_f64"]), rel_l2(c["pc_inv"], c["pc_inv_f64"]))
    assert rel_l2(n(fwd), c["pc_fwd"]) < bound(yard) and rel_l2(n(inv), c["pc_inv"]) < bound(yard)
    assert torch.equal(fwd[..., 3], data[..., 3]) and torch.equal(inv[..., 3], data[..., 3])      # w passes through
    back = perform_canting(cant, fwd, inverse=True, device=DEV)
    keep = slice(0, 1) if name == "e" else slice(None)          # (e)'s second facet has no basis to come back through
    err = rel_l2(n(back)[:, keep], c["pc_data"][:, keep])
    print(f"case {name}: there and back {err:.2e}, yard {yard:.2e}")
    assert err < bound(yard)
    # the inverse's gradients
    c2, d2 = cant.clone().requires_grad_(True), data.clone().requires_grad_(True)
    (perform_canting(c2, d2, inverse=True) * t(c["pc_w"])).sum().backward()
    for got, key in ((c2.grad, "pc_inv_grad_canting"), (d2.grad, "pc_inv_grad_data")):
        yard = rel_l2(c[key], c[key + "_f64"])
        assert rel_l2(n(got), c[key]) < bound(yard), key


# ---- 2. gradients against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ref.CASES)
def test_gradients_reach_canting_translations_and_control_points(golden, name):
    """Through ``NURBSSurfaces`` on the group's activated tensors: each gradient within max(3 x the reference's own fp32-vs-fp64
    distance, 1e-5) of the reference's fp32 gradient.  (On the parent commit canting.grad and translations.grad are None.)"""
    c = ref.fixture_case(golden("canting"), name)
    group, cant, tr, cp = _group(c)
    pts, nrm = _surfaces(group, c)
    ((pts * t(c["wp"])).sum() + (nrm * t(c["wn"])).sum()).backward()
    assert cant.grad is not None and tr.grad is not None and cp.grad is not None
    assert cant.grad.shape == cant.shape and tr.grad.shape == tr.shape
    if not int(c["grads_finite"]):
        return                                                   # the fixture marks the case forward-only
    assert not cant.grad[..., 3].any()
    for got, key in ((cant.grad, "grad_canting"), (tr.grad, "grad_translations"), (cp.grad, "grad_cp")):
        yard = rel_l2(c[key], c[key + "_f64"])
        err = rel_l2(n(got), c[key])
        print(f"case {name} {key}: err {err:.2e}, yard {yard:.2e}")
        assert np.isfinite(n(got)).all() and err < bound(yard), (key, err, yard)


class _Spy:
    """Records the calls into the library (name, arguments)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


@pytest.mark.parametrize("name", ["b", "d"])
def test_subsets_of_gradients_ask_for_nothing_more(golden, name, monkeypatch):
    """Only canting, only translations, only data, translations=None: the gradients asked for are the reference's, the others
    stay None, and the one backward call passes NULL for every output nobody asked for."""
    from artist_amd import _lib, ops
    c = ref.fixture_case(golden("canting"), name)
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    mask = c["mask"]
    cant_np, tr_np = ref.activate(c["canting"], mask), ref.activate(c["translations"], mask)
    wp, wn = t(c["wp"]), t(c["wn"])

    def run(learn, with_tr=True):
        leaves = dict(cant=t(cant_np), tr=t(tr_np) if with_tr else None, p0=t(c["points0"]), n0=t(c["normals0"]))
        for key in learn:
            leaves[key].requires_grad_(True)
        spy.calls.clear()
        pts, nrm = ops.CantFacets.apply(leaves["cant"], leaves["tr"], leaves["p0"], leaves["n0"], False)
        ((pts * wp).sum() + (nrm * wn).sum()).backward()
        assert [call[0] for call in spy.calls] == ["art_cant_facets_fwd", "art_cant_facets_bwd"]
        outs = spy.calls[1][1][8:12]                  # grad_data_points, grad_data_normals, grad_canting, grad_translations
        return leaves, [o is not None for o in outs]

    def check(got, want32, want64, key):
        yard = rel_l2(want32, want64)
        assert rel_l2(n(got), want32) < bound(yard), (key, rel_l2(n(got), want32), yard)

    pairs =lambda sfx: [(c["points0" + sfx], c["wp"], True), (c["normals0" + sfx], c["wn"], False)]  # noqa: E731
    r32 = ref.gradients(cant_np, pairs(""), with_translations=True, dtype=np.float32)
    r64 = ref.gradients(cant_np, pairs("_f64"), with_translations=True)
    g_c, g_t, g_d = zip(r32, r64)

    leaves, asked = run(["cant"])
    assert asked == [False, False, True, False] and leaves["tr"].grad is None and leaves["p0"].grad is None
    check(leaves["cant"].grad, g_c[0], g_c[1], "canting alone")
    # against the fixture too: the replicas' rows added up are the reference's gradient of the base tensor
    yard = rel_l2(c["grad_canting"], c["grad_canting_f64"])
    assert rel_l2(ref.to_base(n(leaves["cant"].grad), mask), c["grad_canting"]) < bound(yard)

    leaves, asked = run(["tr"])
    assert asked == [False, False, False, True] and leaves["cant"].grad is None
    check(leaves["tr"].grad, g_t[0], g_t[1], "translations alone")
    assert spy.calls[1][1][1] is None and spy.calls[1][1][2] is None          # ... and no data is read for it

    leaves, asked = run(["p0", "n0"])
    assert asked == [True, True, False, False] and leaves["cant"].grad is None and leaves["tr"].grad is None
    check(leaves["p0"].grad, g_d[0][0], g_d[1][0], "points alone")
    check(leaves["n0"].grad, g_d[0][1], g_d[1][1], "normals alone")

    leaves, asked = run(["cant", "p0"], with_tr=False)
    assert asked == [True, False, True, False]
    assert spy.calls[0][1][1] is None                                         # no translation in the forward either
    check(leaves["cant"].grad, g_c[0], g_c[1], "canting without translations")      # (the translation does not enter it)
    check(leaves["p0"].grad, g_d[0][0], g_d[1][0], "points without translations")


# ---- 3. the workload's shape against the restatement -----------------------------------------------------------------------------

def _field(H=8, F=4, n_eval=50, seed=5):
    """Un-canted surfaces of H heliostats x F facets on an n_eval^2 grid (the fused kernel without canting), cantings with
    mrad-scale tilts, translations and upstream weights."""
    from artist_amd import NURBSSurfaces, create_nurbs_evaluation_grid
    from artist_amd.scene import synthetic_control_points
    g = torch.Generator().manual_seed(seed)
    cp, cant, tr = synthetic_control_points(H, (6, 6), 1e-3, device=DEV)
    cant = cant + (3e-3 * torch.randn(cant.shape, generator=g)).to(DEV) * torch.tensor([1.0, 1.0, 1.0, 0.0], device=DEV)
    uv = create_nurbs_evaluation_grid(torch.tensor([n_eval, n_eval]), device=DEV)[None, None].expand(H, F, -1, -1)
    with torch.no_grad():
        p0, n0 = NURBSSurfaces(torch.tensor([3, 3]), cp, device=DEV).calculate_surface_points_and_normals(uv, None, None)
    wp = (torch.rand(p0.shape, generator=g) - 0.5).to(DEV)
    wn = (torch.rand(p0.shape, generator=g) - 0.5).to(DEV)
    return cant, tr, p0, n0, wp, wn


def _cant_grads(cant, tr, p0, n0, wp, wn):
    from artist_amd import ops
    leaves = [x.detach().clone().requires_grad_(True) for x in (cant, tr, p0, n0)]
    pts, nrm = ops.CantFacets.apply(*leaves, False)
    ((pts * wp).sum() + (nrm * wn).sum()).backward()
    return [x.grad for x in leaves]


def test_workload_shape_against_the_restatement():
    """8 heliostats x 4 facets x 2500 points: all four gradients against the fp64 restatement on the downloaded un-canted
    surfaces, within max(3 x the restatement's own fp32-vs-fp64 distance, 1e-5)."""
    cant, tr, p0, n0, wp, wn = _field()
    got = _cant_grads(cant, tr, p0, n0, wp, wn)
    pairs = [(n(p0), n(wp), True), (n(n0), n(wn), False)]
    want = {}
    for dtype in (np.float64, np.float32):
        g_c, g_t, g_d = ref.gradients(n(cant), pairs, with_translations=True, dtype=dtype)
        want[dtype] = [g_c, g_t, g_d[0], g_d[1]]
    for key, g, w64, w32 in zip(("canting", "translations", "points", "normals"), got, want[np.float64], want[np.float32]):
        yard, err = rel_l2(w32, w64), rel_l2(n(g), w64)
        print(f"workload shape, grad {key}: err {err:.2e}, yard {yard:.2e}")
        assert np.isfinite(n(g)).all() and err < bound(yard), (key, err, yard)


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits_and_a_heliostat_does_not_see_its_batch():
    cant, tr, p0, n0, wp, wn = _field(H=5, n_eval=23)             # 529 points: an odd count, three passes of the workgroup
    full = _cant_grads(cant, tr, p0, n0, wp, wn)
    again = _cant_grads(cant, tr, p0, n0, wp, wn)
    for a, b in zip(full, again):
        assert torch.equal(a, b)
    for h in range(5):
        rows = slice(h, h + 1)
        alone = _cant_grads(*(x[rows] for x in (cant, tr, p0, n0, wp, wn)))
        for a, b in zip(full, alone):
            assert torch.equal(a[rows], b), h
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)               # the same heliostats at other positions of the batch
    moved = _cant_grads(*(x[perm] for x in (cant, tr, p0, n0, wp, wn)))
    for a, b in zip(full, moved):
        assert torch.equal(a[perm], b)
    assert float(full[0].abs().max()) > 0 and float(full[1].abs().max()) > 0


# ---- 5. no extra launches ------------------------------------------------------------------------------------------------------------

def test_constants_take_the_one_fused_launch(golden, monkeypatch):
    from artist_amd import _lib
    c = ref.fixture_case(golden("canting"), "b")
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    group, cant, tr, cp = _group(c)
    pts, nrm = _surfaces(group, c, detach=True)                    # the control points learn, canting and translations do not
    (pts.sum() + nrm.sum()).backward()
    assert [call[0] for call in spy.calls] == ["art_nurbs_fwd", "art_nurbs_bwd"]
    assert spy.calls[0][1][6] is not None and cp.grad is not None and cant.grad is None
    spy.calls.clear()
    with torch.no_grad():                                          # nothing records: the tensors' flags do not matter
        _surfaces(group, c)
    assert [call[0] for call in spy.calls] == ["art_nurbs_fwd"]
    group, cant, tr, cp = _group(c)                                # (a fresh graph: the first one has been walked)
    spy.calls.clear()
    pts, nrm = _surfaces(group, c, _orientations(3))               # they learn: evaluation, canting, alignment - and back
    (pts.sum() + nrm.sum()).backward()
    assert [call[0] for call in spy.calls] == ["art_nurbs_fwd", "art_cant_facets_fwd", "art_align_fwd",
                                               "art_align_bwd", "art_cant_facets_bwd", "art_nurbs_bwd"]
    assert spy.calls[0][1][6] is None and spy.calls[0][1][18] is None          # stage one: no canting, no orientation


def test_empty_batches():
    from artist_amd import ops, perform_canting
    assert perform_canting(torch.zeros(0, 4, 2, 4, device=DEV), torch.zeros(0, 4, 9, 4, device=DEV)).shape == (0, 4, 9, 4)
    cant = torch.randn(2, 3, 2, 4, device=DEV, requires_grad=True)
    tr = torch.randn(2, 3, 4, device=DEV, requires_grad=True)
    pts, _ = ops.CantFacets.apply(cant, tr, torch.zeros(2, 3, 0, 4, device=DEV), None, False)
    assert pts.shape == (2, 3, 0, 4)
    g_c, g_t = torch.autograd.grad(pts.sum(), (cant, tr))
    assert not g_c.any() and not g_t.any()                        # no points: zeros, written in full


# ---- 6. end to end: one descent step ------------------------------------------------------------------------------------------------

def test_one_descent_step_on_a_tilted_facet_lowers_the_flux_loss_as_predicted(golden):
    """smoke()'s field (2 heliostats, 8 rays, 6 x 6 nets, 16 x 16 points per facet, 64 x 64 bitmaps); the target flux is the
    unperturbed field's.  One facet's n is tilted by 2 mrad, the canting goes through NURBS -> alignment -> trace_rays -> squared
    pixel loss, and moves by -eta grad with eta such that the first-order prediction is the fixture's fraction of the loss (1 %
    unless the reference's own pipeline was outside 0.8 .. 1.2 there: generate_canting_golden.py).  The measured decrease is
    between 0.5 and 1.5 times the prediction."""
    from artist_amd import HeliostatRayTracer, NURBSSurfaces
    from artist_amd.scene import build_synthetic_scenario
    d = golden("canting")
    fraction, (h, f) = float(d["descent_fraction"]), d["descent_facet"].tolist()
    scenario, uv = build_synthetic_scenario(2, n_rays=8, n_cp=(6, 6), n_eval=16, device=DEV)
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(2, dtype=torch.int32, device=DEV)
    tix = torch.zeros(2, dtype=torch.long, device=DEV)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(2, 1)
    aim = scenario.solar_tower.get_centers_of_target_areas(tix)
    base = group.canting.clone()
    group.activate_heliostats(mask)
    rt = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=torch.tensor([64, 64]))

    def flux_of(canting):
        group.canting = canting
        group.activate_heliostats(mask)                            # active_canting = canting.repeat_interleave(mask): in the graph
        pts, nrm = NURBSSurfaces(group.nurbs_degrees, group.active_nurbs_control_points, device=DEV).calculate_surface_points_and_normals(
            uv, group.active_canting, group.active_facet_translations)
        group.active_surface_points, group.active_surface_normals = pts.reshape(2, -1, 4), nrm.reshape(2, -1, 4)
        group.align_surfaces_with_incident_ray_directions(aim, inc, mask)
        return rt.trace_rays(inc, mask, tix)[0]

    with torch.no_grad():
        target = flux_of(base)
    tilted = base.clone()
    tilted[h, f, 1, 2] += float(d["descent_tilt"]) * float(torch.linalg.norm(base[h, f, 1]))
    tilted.requires_grad_(True)
    loss = ((flux_of(tilted) - target) ** 2).sum()
    grad, = torch.autograd.grad(loss, tilted)
    loss = loss.detach()
    assert float(loss) > 0 and torch.isfinite(grad).all() and float(grad[h, f, 1, 2].abs()) > 0
    eta = fraction * float(loss) / float((grad * grad).sum())
    with torch.no_grad():
        stepped = ((flux_of(tilted.detach() - eta * grad) - target) ** 2).sum()
    ratio = float(loss - stepped) / (fraction * float(loss))
    print(f"descent: fraction {fraction:g}, eta {eta:.3e}, loss {float(loss):.6e} -> {float(stepped):.6e}, ratio {ratio:.4f} "
          f"(reference {float(d['descent_ref_ratio']):.4f})")
    assert 0.5 <= ratio <= 1.5, ratio
