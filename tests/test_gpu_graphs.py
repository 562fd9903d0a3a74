"""An epoch captured into a HIP graph and replayed gives the bits of the eager epoch (``-m gpu``).

``artist_amd.EpochGraph`` warms ``step_fn`` up on a stream of its own, captures it there with ``torch.cuda.graph`` and replays
it; the optimiser step stays eager.  "The same bits" is ``torch.equal``: the flux and every gradient of the epoch are
bit-reproducible from run to run (README.md), so a replay has nothing to differ by.  The cases stay off the two documented
exceptions (candidate lists beyond 32, the scattered NURBS scheme of ``fit_nurbs``).  Sizes are the smallest that reach every
launch of a path: 3 heliostats x 4 facets x 16^2 points, 64 x 64 bitmaps."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPOCHS = 3
RES = 64


class _Epoch:
    """NURBS (control points as the leaf, fused alignment) -> trace -> crop + loss -> backward on a synthetic field, and the
    Adam step that follows it.  Everything ``step`` reads lives at a fixed address."""

    def __init__(self, H=3, R=8, per_target=False, loss="pixel", cylinder=False, seed=0):
        from artist_amd import HeliostatRayTracer, scene
        from artist_amd.optim import Adam
        self.H, self.per_target, self.loss_kind = H, per_target, loss
        scenario, self.uv = scene.build_synthetic_scenario(H, n_rays=R, n_cp=(6, 6), n_eval=16, device=DEV)
        self.tix = torch.zeros(H, dtype=torch.long, device=DEV)
        if cylinder:        # one planar and one cylindrical area, heliostats aiming at both: the other split call
            cyl = scene.TowerTargetAreasCylindrical(
                names=["cyl"], centers=torch.tensor([[0.0, -12.0, 55.0, 1.0]], device=DEV),
                normals=torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV), axes=torch.tensor([[0.0, 0.0, 1.0, 0.0]], device=DEV),
                radii=torch.tensor([12.0], device=DEV), heights=torch.tensor([30.0], device=DEV),
                opening_angles=torch.tensor([2.0], device=DEV))
            scenario.solar_tower = scene.SolarTower([scenario.solar_tower.target_areas[0], cyl], device=DEV)
            self.tix = (torch.arange(H, device=DEV) % 2).long()
        self.tower = scenario.solar_tower
        self.group = group = scenario.heliostat_field.heliostat_groups[0]
        self.mask = torch.ones(H, dtype=torch.int32, device=DEV)
        self.inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
        group.activate_heliostats(self.mask, DEV)
        self.orientation = scene.ideal_orientations(group.active_positions, self.tower.get_centers_of_target_areas(self.tix), self.inc)
        self.tracer = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=torch.tensor([RES, RES]))
        n_maps = 1 if per_target else H
        self.loss_tix = torch.zeros(1, dtype=torch.long, device=DEV) if per_target else self.tix
        self.truth = torch.rand((n_maps, RES, RES), generator=torch.Generator().manual_seed(seed + 1)).to(DEV) + 0.1
        self.cp = group.active_nurbs_control_points.clone().requires_grad_(True)
        self.optimizer = Adam([self.cp], lr=2e-4)
        torch.cuda.synchronize()

    @property
    def leaf(self):
        return self.cp

    def step(self):
        from artist_amd import NURBSSurfaces, crop_and_kl_loss, crop_and_pixel_loss
        group, H = self.group, self.H
        pts, nrm = NURBSSurfaces(group.nurbs_degrees, self.cp, device=DEV).calculate_surface_points_and_normals(
            self.uv, group.active_canting, group.active_facet_translations, orientations=self.orientation)
        group.active_surface_points, group.active_surface_normals = pts.reshape(H, -1, 4), nrm.reshape(H, -1, 4)
        trace = self.tracer.trace_rays_per_target if self.per_target else self.tracer.trace_rays
        flux, intercept, on_target, unblocked = trace(self.inc, self.mask, self.tix)
        crop_and_loss = crop_and_kl_loss if self.loss_kind == "kl" else crop_and_pixel_loss
        loss = crop_and_loss(flux, self.tower, self.loss_tix, self.truth).sum()
        loss.backward()
        return flux, intercept, on_target, unblocked, loss


def _eager_epochs(epoch, epochs=EPOCHS):
    """``epochs`` x (step, Adam) eagerly: per epoch (flux, three factors, loss, gradient), and the leaf at the end."""
    records = []
    for _ in range(epochs):
        epoch.optimizer.zero_grad(set_to_none=True)
        outputs = epoch.step()
        records.append([x.detach().clone() for x in (*outputs, epoch.leaf.grad)])
        epoch.optimizer.step()
    torch.cuda.synchronize()
    return records, epoch.leaf.detach().clone()


def _replayed_epochs(epoch, epochs=EPOCHS):
    """The same from the same start, the step replayed from an ``EpochGraph`` and the Adam step eager."""
    from artist_amd import EpochGraph
    graph = EpochGraph(epoch.step, warmup=2)
    records = []
    for _ in range(epochs):
        outputs = graph.replay()
        records.append([x.detach().clone() for x in (*outputs, epoch.leaf.grad)])
        epoch.optimizer.step()
    torch.cuda.synchronize()
    return records, epoch.leaf.detach().clone(), graph


NAMES = ("flux", "intercept factor", "on-target factor", "unblocked factor", "loss", "gradient")


def _assert_same_epochs(eager, replayed):
    (records_e, leaf_e), (records_r, leaf_r) = eager, replayed
    assert len(records_e) == len(records_r) == EPOCHS
    for e, (rec_e, rec_r) in enumerate(zip(records_e, records_r)):
        for name, a, b in zip(NAMES, rec_e, rec_r):
            assert a.shape == b.shape and torch.equal(a, b), f"epoch {e}: {name} of the replayed step differs from the eager one"
    assert torch.equal(leaf_e, leaf_r), "the parameters after the last step differ"
    # the case is not vacuous: light arrived, the gradient is there and moved the parameters from epoch to epoch
    assert float(records_e[0][0].sum()) > 0 and float(records_e[0][5].abs().sum()) > 0
    assert torch.isfinite(records_e[-1][5]).all() and not torch.equal(records_e[0][5], records_e[-1][5])


CASES = {
    "lean planar": dict(),
    "per target, field groups": dict(R=4, per_target=True),
    "kl loss": dict(loss="kl"),
}


@pytest.mark.parametrize("case", CASES)
def test_replayed_epochs_equal_eager_epochs(case, monkeypatch, capfd):
    """Three epochs of NURBS -> trace -> crop + loss -> backward -> Adam: eagerly, then from the same start with the step
    replayed.  Per epoch the flux, the three factors, the loss and the control points' gradient are the same bits, and so are
    the control points after the third step.  Cases: the lean planar launch; ``trace_rays_per_target`` with four rays, whose
    forward is the field-group launch (a field of three is too small to be grouped by the cost model: the launch geometry is
    forced to whole heliostats per item and groups of two, and the library's own geometry print shows that it was taken); the
    KL loss in place of the pixel loss."""
    kwargs = CASES[case]
    grouped = kwargs.get("per_target", False)
    if grouped:
        for knob, value in (("ARTIST_HIP_FWD_BLOCKS", "1"), ("ARTIST_HIP_FIELD_GROUP", "2"), ("ARTIST_HIP_PRINT_GEOMETRY", "1")):
            monkeypatch.setenv(knob, value)
    capfd.readouterr()
    eager = _eager_epochs(_Epoch(**kwargs))
    if grouped:
        groups = [int(g) for g in re.findall(r"art_trace_fwd:.* group (\d+)", capfd.readouterr().err)]
        assert groups and min(groups) > 1, f"the field-group launch was not taken: {groups}"
    records, leaf, graph = _replayed_epochs(_Epoch(**kwargs))
    _assert_same_epochs(eager, (records, leaf))
    from artist_amd import ops
    ops.check_async_errors(DEV)


def test_mixed_tower_epoch_replays():
    """One planar and one cylindrical target area, heliostats aiming at both: the planes' lean launch and the cylinder
    launch - the other split call.  Same equality."""
    from artist_amd import ops
    eager = _eager_epochs(_Epoch(H=4, cylinder=True))
    records, leaf, graph = _replayed_epochs(_Epoch(H=4, cylinder=True))
    _assert_same_epochs(eager, (records, leaf))
    for rec in eager[0]:                                                  # light on both receivers
        assert float(rec[0][0].sum()) > 0 and float(rec[0][1].sum()) > 0
    ops.check_async_errors(DEV)


def _plain_trace(H, seed):
    """A functional ``ops.trace_rays`` call on ``H`` synthetic heliostats: (arguments, keyword arguments)."""
    from artist_amd import scene
    scenario, _ = scene.build_synthetic_scenario(H, n_rays=8, n_cp=(6, 6), n_eval=16, device=DEV)
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(H, dtype=torch.int32, device=DEV)
    tix = torch.zeros(H, dtype=torch.long, device=DEV)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV).repeat(H, 1)
    group.activate_heliostats(mask, DEV)
    group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask, DEV)
    P = group.active_surface_points.shape[1]
    du, de = scenario.light_sources.light_source_list[0].get_distortions(P, H, random_seed=seed)
    planar = scenario.solar_tower.target_areas[0]
    args = (group.active_surface_points.detach(), group.active_surface_normals.detach(), inc, du, de, tix, planar.centers, planar.normals,
            planar.dimensions)
    return args, dict(resolution=(RES, RES))


def test_two_graphs_and_eager_work_do_not_share_state():
    """Two graphs of different fields replayed alternately, an eager trace on the default stream between the replays: every
    result is the one the same work gives eagerly and alone - the graphs' streams, counters, tables, scratch and accumulators
    are their own - and the device has nothing to report afterwards."""
    from artist_amd import EpochGraph, ops
    alone = [_eager_epochs(_Epoch(H=3, seed=0), epochs=1)[0][0], _eager_epochs(_Epoch(H=2, R=12, seed=5), epochs=1)[0][0]]
    args, kwargs = _plain_trace(5, seed=11)
    eager_alone = [x.clone() for x in ops.trace_rays(*args, **kwargs)]
    torch.cuda.synchronize()

    epochs = [_Epoch(H=3, seed=0), _Epoch(H=2, R=12, seed=5)]
    graphs = [EpochGraph(ep.step, warmup=1) for ep in epochs]
    for round_ in range(3):
        for k in (0, 1):
            outputs = graphs[k].replay()
            between = ops.trace_rays(*args, **kwargs)                    # queued behind the replay, no synchronisation
            got = [x.clone() for x in (*outputs, epochs[k].leaf.grad)]
            for name, a, b in zip(NAMES, alone[k], got):
                assert torch.equal(a, b), f"round {round_}, graph {k}: {name} differs from the eager epoch run alone"
            for a, b in zip(eager_alone, between):
                assert torch.equal(a, b), f"round {round_}: the eager trace between the replays differs from the same trace alone"
    ops.check_async_errors(DEV)
    assert graphs[0]._stream.cuda_stream != graphs[1]._stream.cuda_stream
    for g in graphs:
        g.close()
        with pytest.raises(Exception, match="closed"):
            g.replay()


def test_capture_without_warm_up_is_refused_and_harmless():
    """A hand-rolled ``torch.cuda.graph`` around a trace on a stream that has never traced: refused, by the Python layer
    (the stream has no pixel accumulators, and a captured ``zeros`` is not zero) and, with accumulators provided, by the
    library itself (the stream has no work counters, and an allocation under capture would fail and invalidate the
    capture: none is attempted).  Nothing is broken afterwards: an eager trace gives the bits it gave before, and the device
    has nothing to report."""
    from artist_amd import ArtistHipError, ops
    args, kwargs = _plain_trace(3, seed=2)
    before = [x.clone() for x in ops.trace_rays(*args, **kwargs)]
    torch.cuda.synchronize()

    # (torch hands streams out of a pool of 32 per priority, round robin: a high-priority one has not been handed to any other
    #  test of the suite, so it has never traced)
    stream = torch.cuda.Stream(device=DEV, priority=-1)
    with pytest.raises(ArtistHipError, match="before capturing"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
            ops.trace_rays(*args, **kwargs)
    # ... and the library's own guard: the accumulators exist (made eagerly, zero), the stream's work counters do not
    key = (DEV.index, stream.cuda_stream)
    assert key not in ops._ACCUM
    ops._ACCUM[key] = torch.zeros((3 * RES * RES,), dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    try:
        with pytest.raises(ArtistHipError, match="art_trace_fwd: first use on this stream.*before capturing"):
            with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
                ops.trace_rays(*args, **kwargs)
    finally:
        del ops._ACCUM[key]
    torch.cuda.synchronize()
    after = ops.trace_rays(*args, **kwargs)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    ops.check_async_errors(DEV)
    # the refused stream is as good as new: warmed up, it captures and replays
    with torch.cuda.stream(stream):
        ops.trace_rays(*args, **kwargs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = ops.trace_rays(*args, **kwargs)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(before, captured):
        assert torch.equal(a, b)
    ops.check_async_errors(DEV)


def test_blocking_under_capture_is_refused():
    """Blocking is not captured: a trace with the rectangle tables under capture is an error before anything
    is enqueued, on a stream that is warmed up as well, and the same trace runs eagerly afterwards."""
    from artist_amd import ArtistHipError, ops
    from artist_amd.blocking import create_blocking_primitives_rectangles_by_index
    args, kwargs = _plain_trace(3, seed=4)
    corners, spans, normals = create_blocking_primitives_rectangles_by_index(args[0])
    blocking = dict(corners=corners, spans=spans, normals=normals, owner=torch.arange(3, dtype=torch.int32, device=DEV),
                    max_scatter_angle=0.05, lbvh_compat=False)
    before = [x.clone() for x in ops.trace_rays(*args, blocking=blocking, **kwargs)]
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        ops.trace_rays(*args, blocking=blocking, **kwargs)
    torch.cuda.synchronize()
    with pytest.raises(ArtistHipError, match="blocking / shading under graph capture is not supported"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
            ops.trace_rays(*args, blocking=blocking, **kwargs)
    torch.cuda.synchronize()
    for a, b in zip(before, ops.trace_rays(*args, blocking=blocking, **kwargs)):
        assert torch.equal(a, b)
    ops.check_async_errors(DEV)


def test_adam_step_refuses_capture():
    """``art_adam_step`` takes the step number by value: a replay would repeat it.  ``Adam.step()`` under capture is an error
    that names the pattern, and it leaves the parameter, the state and the capture alone."""
    from artist_amd import ArtistHipError
    from artist_amd.optim import Adam
    p = torch.ones(64, device=DEV, requires_grad=True)
    p.grad = torch.full_like(p, 0.5)
    optimizer = Adam([p], lr=1e-2)
    optimizer.step()                                                      # (eagerly: fine)
    torch.cuda.synchronize()
    value = p.detach().clone()
    stream = torch.cuda.Stream(device=DEV)
    with pytest.raises(ArtistHipError, match=r"replay\(\); optimizer\.step\(\)"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=stream):
            optimizer.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), value) and optimizer.state[p]["step"] == 1
