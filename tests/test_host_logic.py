"""CPU suite: host-side logic of the drop-in classes (no kernels): sampler partition, knot vectors and span
search of the NURBS mirror, helper constructors, the distortion recipe, tracer bookkeeping and error behaviour."""
import pathlib

import numpy as np
import pytest
import torch

from conftest import sun_distortions

CPU = torch.device("cpu")


def test_sampler_matches_reference_table(golden):
    from artist_amd import RestrictedDistributedSampler
    for row in golden("known_answers")["sampler_table"]:       # tests/raytracing/test_sampling.py:8-15
        ns, nh, ws, rank = (int(v) for v in row[:4])
        assert list(RestrictedDistributedSampler(ns, nh, ws, rank)) == [int(v) for v in row[4:] if v >= 0]


def test_owned_heliostats_partition():
    from artist_amd.distributed import owned_heliostats
    for n, world in ((1000, 8), (10, 3), (2, 4), (1, 1)):
        rows = [owned_heliostats(n, world, r) for r in range(world)]
        assert sorted(sum(rows, [])) == list(range(n))
        assert all(r == list(range(i, n, min(n, world))) for i, r in enumerate(rows) if i < min(n, world))
        assert all(r == [] for r in rows[min(n, world):])


def test_nurbs_mirror_knots_and_spans(golden):
    from artist_amd import NURBSSurfaces
    ka = golden("known_answers")
    for name in ("small_deg3", "small_deg2_tilted"):
        d = golden(name)
        surf = NURBSSurfaces(torch.from_numpy(d["degrees"]), torch.from_numpy(d["control_points"]), device=CPU)
        assert np.array_equal(surf.knot_vectors_u[0, 0].numpy(), d["knots_u"])
        assert np.array_equal(surf.knot_vectors_v[0, 0].numpy(), d["knots_v"])
        assert tuple(surf.knot_vectors_u.shape[:2]) == d["control_points"].shape[:2]
        n, p = d["control_points"].shape[2], int(d["degrees"][0])
        assert surf._unique_counts()[0] == n - p + 1 == torch.unique(surf.knot_vectors_u, dim=2).shape[2]
    # tests/nurbs/test_surfaces.py:150-199
    x, y = torch.meshgrid(torch.linspace(1e-2, 1 - 1e-2, 6), torch.linspace(1e-2, 1 - 1e-2, 6), indexing="ij")
    ev = torch.from_numpy(ka["span_eval"])[None, None]
    knots = torch.from_numpy(ka["span_knots"])[None, None]
    surf = NURBSSurfaces(torch.tensor([3, 3]), torch.stack([x, y], -1)[None, None], device=CPU)
    assert surf.find_spans(0, ev, knots).flatten().tolist() == ka["span_expected"].tolist()
    surf.uniform = False
    assert surf.find_spans(0, ev, knots).flatten().tolist() == ka["span_nonuniform_reference"].tolist()
    # swapping the knot tensors triggers a recount of the distinct knots (surfaces.py:199 semantics)
    surf.knot_vectors_u = knots
    assert surf._unique_counts()[0] == 4


def test_helper_constructors_match_reference(golden):
    from artist_amd import create_nurbs_evaluation_grid, create_planar_nurbs_control_points
    from artist_amd.scene import CANTING
    d = golden("config1")                                  # planar control points (z-noise 0), 50x50 grid
    canting = torch.tensor(CANTING).unsqueeze(0).repeat(4, 1, 1)
    cp = create_planar_nurbs_control_points(torch.tensor([10, 10]), canting, device=CPU)
    assert np.array_equal(cp.numpy(), d["control_points"][0])
    uv = create_nurbs_evaluation_grid(torch.tensor([50, 50]), device=CPU)
    assert np.array_equal(uv.numpy(), d["eval_points_grid"])


def test_sun_stand_in_matches_reference_recipe(golden):
    from artist_amd.scene import Sun
    ka = golden("known_answers")
    du, de = Sun(3, device=CPU).get_distortions(number_of_points=5, number_of_active_heliostats=2, random_seed=7)
    assert np.array_equal(du.numpy(), ka["sun_u"]) and np.array_equal(de.numpy(), ka["sun_e"])
    assert list(du.stride()) == [30, 10, 2] and de.data_ptr() == du.data_ptr() + 4     # one interleaved buffer
    ref_u, ref_e = sun_distortions(2, 3, 5)
    assert torch.equal(du, ref_u) and torch.equal(de, ref_e)
    with pytest.raises(ValueError, match="Unknown sunlight distribution type."):      # artist/scene/sun.py:82-86
        Sun(3, dict(distribution_type="uniform"))


def test_ideal_orientation_is_a_rigid_transform_that_hits_the_aim_point(golden):
    from artist_amd.scene import ideal_orientations
    d = golden("mid_256")
    ori_ref = torch.from_numpy(d["orientation"])
    pos = ori_ref[:, :, 3].clone()
    aim, inc = torch.from_numpy(d["aim_points"]), torch.from_numpy(d["incident"])
    ori = ideal_orientations(pos, aim, inc)
    r = ori[:, :3, :3]
    torch.testing.assert_close(r @ r.transpose(1, 2), torch.eye(3).expand_as(r), atol=1e-6, rtol=0)
    torch.testing.assert_close(torch.linalg.det(r), torch.ones(r.shape[0]), atol=1e-6, rtol=0)
    # the mirror normal (local +z) bisects -incident and the aim direction, like the reference's kinematics
    torch.testing.assert_close(ori[:, :3, 2], ori_ref[:, :3, 2], atol=2e-4, rtol=0)
    torch.testing.assert_close(ori[:, :, 3], ori_ref[:, :, 3])


class _Stub:
    pass


def _tiny_scene(n_heliostats=4, n_rays=3, n_points=8):
    from artist_amd.scene import (HeliostatField, HeliostatGroup, LightSourceArray, Scenario, SolarTower, Sun,
                                  TowerTargetAreasPlanar)
    g = HeliostatGroup(
        names=[f"h{i}" for i in range(n_heliostats)], positions=torch.zeros(n_heliostats, 4),
        surface_points=torch.zeros(n_heliostats, n_points, 4), surface_normals=torch.zeros(n_heliostats, n_points, 4),
        canting=torch.ones(n_heliostats, 4, 2, 4), facet_translations=torch.zeros(n_heliostats, 4, 4),
        nurbs_control_points=torch.zeros(n_heliostats, 4, 6, 6, 3), nurbs_degrees=torch.tensor([3, 3]), device=CPU)
    planar = TowerTargetAreasPlanar(["r"], torch.tensor([[0.0, 0.0, 10.0, 1.0]]), torch.tensor([[0.0, 1.0, 0.0, 0.0]]),
                                    torch.tensor([[2.0, 2.0]]))
    sc = Scenario(torch.zeros(3), SolarTower([planar], device=CPU), LightSourceArray([Sun(n_rays, device=CPU)]),
                  HeliostatField([g]))
    return sc, g


def test_tracer_bookkeeping_and_errors():
    from artist_amd import HeliostatRayTracer
    sc, g = _tiny_scene()
    g.activate_heliostats(torch.tensor([2, 0, 1, 1], dtype=torch.int32))
    assert g.number_of_active_heliostats == 4 and g.active_surface_points.shape[0] == 4
    with pytest.raises(Exception):                                       # replicas + blocking: the reference's
        HeliostatRayTracer(sc, g)                                        # surfaces[mask] = active points fails too
    # reference default is blocking_active=True: heliostat_ray_tracer.py:159-183 (aligned rows where active,
    # surface + position elsewhere)
    g.positions = torch.arange(16, dtype=torch.float32).reshape(4, 4)
    g.activate_heliostats(torch.tensor([1, 0, 1, 1], dtype=torch.int32))
    g.active_surface_points = g.active_surface_points + 5.0
    rtb = HeliostatRayTracer(sc, g)
    assert rtb.blocking_active and rtb.blocking_heliostat_surfaces_active.shape == (4, 8, 4)
    assert torch.equal(rtb.blocking_heliostat_surfaces_active[1], g.surface_points[1] + g.positions[1])
    assert torch.equal(rtb.blocking_heliostat_surfaces_active[[0, 2, 3]], g.active_surface_points)
    assert rtb._max_scatter_angle() == float(max(rtb.distortions_dataset.distortions_u.abs().max(),
                                               rtb.distortions_dataset.distortions_e.abs().max()))
    g.activate_heliostats(torch.tensor([2, 0, 1, 1], dtype=torch.int32))
    # heliostat_ray_tracer.py:185-203: ray magnitude from dni
    rt = HeliostatRayTracer(sc, g, blocking_active=False, dni=800.0, bitmap_resolution=torch.tensor([32, 16]))
    dims = torch.norm(g.canting[0], dim=1)[0][:2] * 4 + 0.02
    assert float(rt.ray_magnitude) == pytest.approx(float(800.0 * dims[0] * dims[1] / (8 * 3)))
    assert rt._resolution_host == (32, 16)
    assert rt.distortions_dataset.distortions_u.shape == (4, 3, 8) and len(rt.distortions_dataset) == 4
    # 3 distinct active heliostats over 2 ranks... the reference's sampler needs uniform replica counts
    g.activate_heliostats(torch.tensor([2, 2, 0, 0], dtype=torch.int32))
    idx = [HeliostatRayTracer(sc, g, blocking_active=False, world_size=2, rank=r).get_sampler_indices().tolist()
           for r in range(2)]
    assert idx == [[0, 1], [2, 3]]
    rt = HeliostatRayTracer(sc, g, blocking_active=False)
    with pytest.raises(AssertionError, match="Some heliostats were not aligned and cannot be raytraced."):
        rt.trace_rays(torch.zeros(4, 4), torch.tensor([1, 1, 1, 1], dtype=torch.int32), torch.zeros(4, dtype=torch.long))


def test_interop_record_with_the_reference_objects():
    """tests/golden/generate_golden.py::save_interop_check built ``artist_amd.HeliostatRayTracer`` on ARTIST's own
    ``Scenario`` / ``HeliostatGroupRigidBody`` (loaded from its test_blocking.h5) next to ARTIST's ray tracer and
    recorded what agreed; this pins the record (the reference itself is not importable on the GPU box)."""
    import json
    import pathlib
    rec = json.loads((pathlib.Path(__file__).parent / "golden" / "interop_check.json").read_text())
    assert rec["blocking_surfaces_equal"] and rec["distortions_equal"] and rec["sampler_indices_equal"]
    assert rec["ray_magnitude_equal"] and rec["primitives_max_abs_diff"] == 0.0
    assert rec["planar_tables"] == [[5, 4], [5, 4], [5, 2]] and rec["cylinder_tables"][3:] == [[6], [6], [6]]
    assert rec["owner"] == [0, 1, 2, 3, 4, 5] and "no CPU fallback" in rec["cpu_trace"]
    # radius x opening angle and height for the cylindrical areas (artist/flux/bitmap.py:183-216)
    assert rec["target_dimensions"][2] == pytest.approx([4.14 * 1.0471976, 5.2291923], rel=1e-6)


# ---------------------------------------------------------------- scenario files
SCENARIOS = pathlib.Path(__file__).resolve().parent / "golden" / "scenarios"
SCENARIO_CASES = {"real_blocking": "test_blocking.h5", "real_paint_mixed": "test_scenario_paint_four_heliostats.h5"}


@pytest.mark.parametrize("fixture", SCENARIO_CASES)
def test_scenario_tables_equal_the_reference_loader(golden, fixture):
    """The reference's own scenario files, read by artist_amd (built-in HDF5 reader): every table equals, bit for
    bit, what ARTIST's loader produced when the fixture was generated (target areas, kinematic deviations, actuator
    tables incl. the initial-angle offset, positions, fitted control points)."""
    from artist_amd import scenario
    d = golden(fixture)
    with scenario.open_scenario_file(SCENARIOS / SCENARIO_CASES[fixture]) as f:
        tables = scenario.read_scenario_tables(f)
    assert float(tables["version"]) == 1.0 and tables["power_plant_position"].shape == (3,)
    for ours, key in (("centers", "target_centers"), ("normals", "target_normals"), ("dimensions", "target_dims")):
        np.testing.assert_array_equal(tables["planar"][ours], d[key])
    for ours, key in (("centers", "cyl_centers"), ("normals", "cyl_normals"), ("axes", "cyl_axes"), ("radii", "cyl_radii"),
                      ("heights", "cyl_heights"), ("opening_angles", "cyl_opening")):
        np.testing.assert_array_equal(tables["cylindrical"][ours], d[key])
    assert tables["light_sources"][0]["number_of_rays"] == 10
    assert tables["light_sources"][0]["distribution_parameters"] == dict(distribution_type="normal", mean=0.0, covariance=4.3681e-06)
    first = tables["heliostats"][0]["actuators"]["type"]               # the fixture holds the FIRST group
    members = [h for h in tables["heliostats"] if h["actuators"]["type"] == first]
    stack = lambda f_: np.stack([f_(h) for h in members])  # noqa: E731
    np.testing.assert_array_equal(stack(lambda h: h["position"]), d["kin_positions"])
    np.testing.assert_array_equal(stack(lambda h: h["kinematics"]["translation"]), d["kin_trans_dev"])
    np.testing.assert_array_equal(stack(lambda h: h["kinematics"]["rotation"]), d["kin_rot_dev"])
    np.testing.assert_array_equal(stack(lambda h: h["actuators"]["non_optimizable"]), d["kin_act_nonopt"])
    np.testing.assert_array_equal(stack(lambda h: h["actuators"]["optimizable"]).reshape(d["kin_act_opt"].shape), d["kin_act_opt"])
    np.testing.assert_array_equal(stack(lambda h: h["surface"]["control_points"]), d["control_points"])


def test_index_mapping_and_aim_points(golden):
    """Scenario.index_mapping (scenario.py:261-418) and SolarTower.get_centers_of_target_areas (solar_tower.py:129-188,
    cylinder aim point = centre + radius * normal) on CPU tensors against the reference's results in the fixture."""
    from artist_amd import scene, scenario
    d = golden("real_paint_mixed")
    t = torch.from_numpy
    tower = scene.SolarTower([scene.TowerTargetAreasPlanar(["multi_focus_tower", "solar_tower_juelich_lower", "solar_tower_juelich_upper"],
                                                           t(d["target_centers"]), t(d["target_normals"]), t(d["target_dims"])),
                              scene.TowerTargetAreasCylindrical(["receiver"], t(d["cyl_centers"]), t(d["cyl_normals"]), t(d["cyl_axes"]),
                                                                t(d["cyl_radii"]), t(d["cyl_heights"]), t(d["cyl_opening"]))])
    sc = scenario.Scenario(power_plant_position=None, solar_tower=tower, light_sources=None, heliostat_field=None)

    class Group:                                             # the fixture's group: the two heliostats with ideal actuators
        names = ["AA28", "AC43"]
        positions = torch.zeros((2, 4))

    sun = torch.nn.functional.normalize(torch.tensor([0.3, 0.8, -0.52, 0.0]), dim=0)
    mapping = [("AA28", "receiver", sun), ("AA31", "multi_focus_tower", sun), ("AA39", "receiver", sun),
               ("AC43", "solar_tower_juelich_upper", sun)]
    mask, targets, incident = sc.index_mapping(Group, mapping, device="cpu")
    np.testing.assert_array_equal(mask.numpy(), d["active_mask"])
    np.testing.assert_array_equal(targets.numpy(), d["target_idx"])
    np.testing.assert_array_equal(incident.numpy(), d["incident"])
    np.testing.assert_array_equal(tower.get_centers_of_target_areas(targets).numpy(), d["aim_points"])
    # repeats stay adjacent in group order; other groups' heliostats are ignored
    mask, targets, incident = sc.index_mapping(Group, [("AC43", "receiver", sun), ("AA28", "multi_focus_tower", sun),
                                                       ("AC43", "multi_focus_tower", sun)], device="cpu")
    assert mask.tolist() == [1, 2] and targets.tolist() == [0, 3, 0]
    with pytest.raises(ValueError, match="Invalid target 'nowhere'"):
        sc.index_mapping(Group, [("AA28", "nowhere", sun)], device="cpu")
    with pytest.raises(ValueError, match="Invalid incident ray direction"):
        sc.index_mapping(Group, [("AA28", "receiver", 2 * sun)], device="cpu")
    mask, targets, incident = sc.index_mapping(Group, device="cpu", single_target_area_index=2)
    assert mask.tolist() == [1, 1] and targets.tolist() == [2, 2] and incident.tolist() == [[0.0, 1.0, 0.0, 0.0]] * 2
    with pytest.raises(ValueError, match="single target area index is invalid"):
        sc.index_mapping(Group, device="cpu", single_target_area_index=4)


def test_h5lite_reads_groups_datasets_and_attributes():
    from artist_amd import h5lite
    with h5lite.File(SCENARIOS / "test_scenario_stral_single_heliostat.h5") as f:
        assert float(f.attrs["version"]) == 1.0
        assert "heliostats" in f and "nothing" not in f and f.get("nothing") is None
        assert f["power_plant/position"][()].shape == (3,) and f["power_plant"]["position"].dtype in (np.float32, np.float64)
        assert f["lightsources/sun_1/type"][()] == b"sun"
        names = list(f["heliostats"].keys())
        assert len(names) == 1 and f["heliostats"][names[0]]["position"].shape == (4,)
    with pytest.raises(OSError):
        h5lite.File(pathlib.Path(__file__), "r")


@pytest.mark.parametrize("name", ["small_deg3", "small_deg2_tilted", "small_offtarget", "mid_256"])
def test_torch_eager_baseline_equals_reference_fixtures(golden, name):
    """tools/torch_eager_baseline.py (the reference-shaped CPU baseline that bench.py times) against what the imported
    reference produced on the same inputs: flux, the two ray-count factors and the autograd gradients."""
    import sys
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent / "tools"))
    import torch_eager_baseline as teb

    d = golden(name)
    tt = lambda k: torch.from_numpy(np.ascontiguousarray(d[k]))  # noqa: E731
    pts, nrm = tt("aligned_points").requires_grad_(True), tt("aligned_normals").requires_grad_(True)
    for batch in (1, 100):
        flux, intercept, on_target = teb.trace_rays(
            pts, nrm, tt("incident"), tt("distortions_u"), tt("distortions_e"), tt("target_idx"), tt("target_centers"),
            tt("target_normals"), tt("target_dims"), tuple(int(v) for v in d["resolution"]), float(d["ray_magnitude"]),
            float(d["extinction"]), float(d["reflectivity"]), batch_size=batch)
        ref = d["flux"].astype(np.float64)
        err = np.linalg.norm(flux.detach().numpy() - ref) / max(np.linalg.norm(ref), 1e-30)
        assert err < 1e-6, (name, batch, err)          # same ATen ops; scatter_add_ order is the only freedom
        assert np.array_equal(intercept.numpy(), d["intercept"]) and np.array_equal(on_target.numpy(), d["on_target"])
    (flux * tt("loss_weights")).sum().backward()
    for got, key in ((pts.grad, "grad_aligned_points"), (nrm.grad, "grad_aligned_normals")):
        ref = d[key].astype(np.float64)
        assert np.linalg.norm(got.numpy() - ref) / np.linalg.norm(ref) < 1e-5, (name, key)


def test_distortions_dataset_keeps_owned_rows_of_the_same_seeded_stream():
    """A rank's DistortionsDataset holds its own rows only, and they are the rows of the unsharded seed-7 tensor
    (reference recipe: artist/scene/sun.py:224-233; partition: artist/raytracing/sampling.py:129-146)."""
    from artist_amd.sampling import DistortionsDataset, RestrictedDistributedSampler
    from artist_amd.scene import Sun

    for (H, R, P) in [(5, 4, 64), (7, 3, 63)]:            # 2RP a multiple of 16 (stream slicing) / not (sample + slice)
        sun = Sun(R, device=torch.device("cpu"))
        full = DistortionsDataset(sun, P, H, random_seed=7)
        ref_u, ref_e = sun_distortions(H, R, P)
        assert torch.equal(full.distortions_u, ref_u) and torch.equal(full.distortions_e, ref_e)
        seen = []
        for rank in range(3):
            rows = RestrictedDistributedSampler(H, H, world_size=3, rank=rank).rank_indices
            part = DistortionsDataset(sun, P, H, random_seed=7, rows=rows)
            assert len(part) == len(rows) and part.distortions_u.shape == (len(rows), R, P)
            assert torch.equal(part.distortions_u, ref_u[rows]) and torch.equal(part.distortions_e, ref_e[rows])
            # still the two stride-2 views of one interleaved buffer (one 8-byte load per ray in the kernel)
            assert part.distortions_u.stride() == part.distortions_e.stride() and part.distortions_u.stride(-1) == 2
            seen += rows
        assert sorted(seen) == list(range(H))


def test_idle_rank_constructs_an_empty_dataset_and_tracer():
    """More ranks than active heliostats: the surplus ranks are idle (artist/raytracing/sampling.py:107-157,
    ``number_of_active_ranks``) - their sampler is empty, their DistortionsDataset holds zero rows (for ARTIST's own
    CPU ``Sun`` recipe as well as for any other light source) and ``HeliostatRayTracer`` can be constructed for them."""
    from artist_amd import HeliostatRayTracer
    from artist_amd.sampling import DistortionsDataset, RestrictedDistributedSampler
    from artist_amd.scene import Sun

    sampler = RestrictedDistributedSampler(2, 2, 4, 3)
    assert list(sampler) == [] and len(sampler) == 0
    for (R, P) in [(4, 64), (3, 63)]:                        # both branches of the owned-rows recipe
        sun = Sun(R, device=torch.device("cpu"))
        empty = DistortionsDataset(sun, P, 2, random_seed=7, rows=[])
        assert len(empty) == 0
        assert tuple(empty.distortions_u.shape) == (0, R, P) and tuple(empty.distortions_e.shape) == (0, R, P)
    scenario, group = _tiny_scene(n_heliostats=2, n_rays=4, n_points=8)
    group.activate_heliostats(torch.tensor([1, 1], dtype=torch.int32))
    for rank in range(4):
        rt = HeliostatRayTracer(scenario, group, blocking_active=False, world_size=4, rank=rank)
        owned = rt.get_sampler_indices().tolist()
        assert owned == ([rank] if rank < 2 else [])
        assert len(rt.distortions_dataset) == len(owned)


@pytest.mark.parametrize("name", ["test_blocking.h5", "test_scenario_paint_four_heliostats.h5", "test_scenario_stral_single_heliostat.h5"])
def test_h5lite_is_pinned_by_an_independent_scan_of_the_raw_bytes(name):
    """h5py is absent, so h5lite reads the reference's scenario files for the fixture generator AND for the product: a
    reader bug would cancel.  tests/h5_dumb_scan.py shares nothing with it (no traversal by name: signature grep of
    SNOD / TREE / HEAP + minimal version-1 header decoding) and yields (leaf name, sha256 of the raw bytes, shape, item
    size) for every fixed-size dataset; the committed table tests/golden/scenarios/h5_index.json is that scan's output.
    Every fixed-size dataset h5lite returns must be in both, bit for bit, and nothing of the table may be missing from
    what h5lite finds (variable-length strings - 'sun', 'linear', ... - live in a global heap the scan does not decode;
    their values are asserted as text in the loader tests)."""
    import hashlib
    import json

    import h5_dumb_scan
    from artist_amd import h5lite
    path = SCENARIOS / name
    scanned = h5_dumb_scan.scan(path)
    table = {(d["name"], d["sha256"], tuple(d["shape"]), d["itemsize"]) for d in json.loads((SCENARIOS / "h5_index.json").read_text())[name]}
    assert scanned == table                                   # the committed pin is what the scan says today
    seen, strings = set(), 0

    def walk(group):
        nonlocal strings
        for key in group.keys():
            child = group[key]
            if isinstance(child, h5lite.Group):
                walk(child)
                continue
            value = np.asarray(child[()])
            if value.dtype.kind in "OSU":
                strings += 1
                continue
            seen.add((key, hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest(), tuple(value.shape), value.dtype.itemsize))

    with h5lite.File(path) as f:
        walk(f)
    assert seen == table, (sorted(seen - table)[:3], sorted(table - seen)[:3])
    assert len(table) >= 35 and 3 <= strings <= 40


def test_trace_bwd_never_rejects_a_buffer_of_the_reported_scratch_size():
    """Round-3 advisor finding: `art_trace_bwd_scratch_floats` sized the rectangle-gradient slabs from the generic launch geometry
    while a planar tower with blocking takes the lean one (facet-sized items: more of them), so `art_trace_bwd` rejected a buffer
    of exactly the reported size (H=100, R=100, P=10000, facet 2500, Cmax=8: 67200 reported).  The two now share one geometry
    routine; this sweeps sizes, facets, capacities and receiver configurations through the host arithmetic
    (`art_trace_bwd_scratch_need` = what the call takes for one configuration) ..."""
    from artist_amd import _lib
    lib = _lib.lib()
    worst = 0
    for R, P, facet in ((100, 10000, 2500), (180, 3600, 900), (1, 10000, 2500), (4, 400, 100), (100, 10000, 0), (7, 1024, 256)):
        for Cmax in (0, 1, 8, 16, 32, 33, 256):        # (beyond 32: rows wider than the kernels' tables - fp64 rows for the rest)
            for H in list(range(1, 600, 7)) + [1000, 4096]:
                reported = lib.art_trace_bwd_scratch_floats(H, R, P, facet, Cmax)
                for T, Tc in ((1, 0), (0, 1), (2, 1)):
                    need = lib.art_trace_bwd_scratch_need(H, R, P, facet, T, Tc, Cmax)
                    assert need <= reported, (H, R, P, facet, Cmax, T, Tc, need, reported)
                    worst = max(worst, need)
                assert Cmax == 0 or reported >= H * min(Cmax, 32) * 12 + (H * (Cmax - 31) * 24 if Cmax > 32 else 0)
    assert worst > 0
    assert lib.art_trace_bwd_scratch_floats(100, 100, 10000, 2500, 8) > 67200      # the advisor's case


@pytest.mark.skipif(torch.cuda.is_available(), reason="host arithmetic with placeholder pointers: only where no kernel can be launched")
def test_trace_bwd_accepts_the_reported_scratch_size_on_the_host():
    """... and, where there is no GPU to launch on, through `art_trace_bwd` itself: with placeholder pointers (the host code never
    dereferences device memory) the call must get PAST its argument checks with a buffer of the reported size - it then fails
    at the first HIP call (ART_ELAUNCH), never with ART_EINVAL - and must fail WITH ART_EINVAL when blocking is on and the
    buffer is one float short."""
    import ctypes

    from artist_amd import _lib
    lib = _lib.lib()
    fake = ctypes.c_void_p(0x1000)       # 16-byte aligned, never dereferenced
    null = ctypes.c_void_p(0)

    def call(H, R, P, facet, T, Tc, Cmax, scratch_floats):
        planar = [fake if T else null] * 3
        cyl = [fake if Tc else null] * 6
        prim = [fake if Cmax else null] * 5
        return lib.art_trace_bwd(fake, fake, fake, fake, fake, 2 * R * P, 2 * P, 2, fake, *planar, *cyl, *prim, Cmax, max(Cmax, 1) * 4, 0.01,
                                 1.0, 1.0, 0.935, H, R, P, facet, T, Tc, 256, 256, 0, fake, fake, fake,
                                 *([fake if Cmax else null] * 3), fake, scratch_floats, null)

    for R, P, facet in ((100, 10000, 2500), (180, 3600, 900)):
        for Cmax in (0, 8, 16, 100):
            for H in (1, 3, 60, 100, 101, 313, 599):
                reported = lib.art_trace_bwd_scratch_floats(H, R, P, facet, Cmax)
                for T, Tc in ((1, 0), (0, 1), (1, 1)):
                    rc = call(H, R, P, facet, T, Tc, Cmax, reported)
                    assert rc != _lib.ART_EINVAL and rc != 0, (H, R, P, facet, Cmax, T, Tc, rc)
                    if Cmax:
                        need = lib.art_trace_bwd_scratch_need(H, R, P, facet, T, Tc, Cmax)
                        whole = H * min(Cmax, 32) * 12 + (H * (Cmax - 31) * 24 if Cmax > 32 else 0)     # the least any geometry needs
                        assert call(H, R, P, facet, T, Tc, Cmax, min(need, whole) - 1) == _lib.ART_EINVAL


def test_diagnostic_switches_live_in_one_header_only():
    """The shipped sources carry no build-time variants: no `.hip` under artist_amd/csrc has a preprocessor conditional,
    trace_diag.hpp is the only header there with a conditional on an ART_ macro (the diagnostic hooks, empty in the product), and
    a plain `make` defines none of the switches."""
    import re
    import subprocess
    csrc = pathlib.Path(__file__).resolve().parent.parent / "artist_amd" / "csrc"
    hips = sorted(csrc.glob("*.hip"))
    assert hips
    for f in hips:
        assert [ln for ln in f.read_text().splitlines() if ln.startswith("#if")] == [], f.name
    conditional = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b.*\bART_", re.M)
    assert [f.name for f in sorted(csrc.glob("*.hpp")) if conditional.search(f.read_text())] == ["trace_diag.hpp"]
    # -B: every recipe is printed whatever has been built already; -n: nothing runs
    recipes = subprocess.run(["make", "-n", "-B"], cwd=csrc, check=True, capture_output=True, text=True).stdout
    assert "hipcc" in recipes and "-DART_" not in recipes
