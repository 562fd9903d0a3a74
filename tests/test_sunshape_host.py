"""Host side of the radial sun shapes (pillbox, Buie, tabulated): their quantile tables, the law of ``Sun(sampler="torch")`` on
the CPU, parameter validation, the argument checks of ``art_sample_radial_distortions`` and the light-source reader."""
import ctypes

import numpy as np
import pytest
import torch

import sunshape_ref
from sunshape_ref import DISC, EXTENT

K = 1024


def sun(kind, sampler="torch", rays=4, **params):
    from artist_amd.scene import Sun
    return Sun(rays, dict(distribution_type=kind, **params), device="cpu", sampler=sampler)


@pytest.fixture(scope="module")
def buie_tables():
    return {chi: sun("buie", circumsolar_ratio=chi).quantile_table for chi in (0.05, 0.3)}


@pytest.fixture(scope="module")
def buie_laws():
    return {chi: sunshape_ref.buie_law(chi) for chi in (0.05, 0.3)}


@pytest.mark.parametrize("params, half_angle", [({}, 4.65e-3), (dict(half_angle=2.5e-3), 2.5e-3)])
def test_pillbox_table_is_the_disc_itself(params, half_angle):
    s = sun("pillbox", **params)
    table = s.quantile_table
    assert table.dtype == torch.float32 and table.device.type == "cpu" and table is s.distribution.quantile_table
    assert table.tolist() == [0.0, float(np.float32(half_angle ** 2))]
    assert s.distribution_parameters["half_angle"] == half_angle and s.distribution.loc.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("chi", [0.05, 0.3])
def test_buie_table(chi, buie_tables, buie_laws):
    table = buie_tables[chi]
    assert table.dtype == torch.float32 and tuple(table.shape) == (K + 1,)
    t2 = table.numpy().astype(np.float64)
    assert t2[0] == 0.0 and (np.diff(t2) >= 0).all()
    assert abs(t2[K] - EXTENT ** 2) <= EXTENT ** 2 * 2.0 ** -24    # fp32 rounding
    share, want = sunshape_ref.table_share_beyond(t2, DISC), 1.0 - buie_laws[chi].cdf(DISC)
    print(f"chi {chi}: share beyond the disc, table {share:.6f}, formulas {want:.6f}")
    assert abs(share - want) <= 1.0 / K
    assert abs(want - chi) < 0.03 and want != chi                  # chi goes in uncorrected: the share is near it, not it


def test_tabulated_buie_profile_gives_the_buie_table(buie_tables):
    # 2000 angles, two of them 1e-9 rad either side of the disc's edge: a piecewise-linear profile has no jump, and without
    # them the ramp between the two samples around 4.65 mrad (22 urad apart) moves the nodes next to the limb by 1.24 annuli
    angles = np.sort(np.concatenate((np.linspace(0.0, EXTENT, 1998), [DISC - 1e-9, DISC + 1e-9])))
    assert angles.shape == (2000,) and (np.diff(angles) > 0).all()
    tab = sun("tabulated", profile_angles=angles, profile_radiance=sunshape_ref.buie_radiance(angles, 0.05))
    ref = buie_tables[0.05].numpy().astype(np.float64)
    got = tab.quantile_table.numpy().astype(np.float64)
    assert got.shape == ref.shape
    annulus = np.maximum(np.diff(ref, append=ref[-1]), np.diff(ref, prepend=ref[0]))
    excess = np.abs(got - ref) - annulus
    print(f"largest |t2_tab - t2_buie| / annulus: {(np.abs(got - ref) / np.maximum(annulus, 1e-300)).max():.3f} at node "
          f"{int(excess.argmax())}")
    assert (excess <= 0).all(), int(excess.argmax())


BUIE_RADII = (1e-3, 2e-3, 3e-3, 4e-3, 4.6e-3, 5e-3, 7e-3, 10e-3, 20e-3, 40e-3)
PILLBOX_RADII = tuple(f * DISC for f in (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.97))


@pytest.mark.parametrize("kind", ["pillbox", "buie"])
def test_law_of_the_torch_sampler_on_the_cpu(kind, buie_laws):
    H, R, P = 10, 10, 10000                                         # 1e6 rays
    s = sun(kind, rays=R, mean=1e-3)
    law, radii = (sunshape_ref.PillboxLaw(DISC), PILLBOX_RADII) if kind == "pillbox" else (buie_laws[0.05], BUIE_RADII)
    u, e = s.get_distortions(number_of_points=P, number_of_active_heliostats=H)
    assert u.shape == e.shape == (H, R, P) and e.data_ptr() == u.data_ptr() + 4     # one interleaved buffer
    theta = sunshape_ref.check_radial_law(u, e, (1e-3, 1e-3), law, radii, s.quantile_table.shape[0] - 1)
    if kind == "pillbox":
        # u - loc is rounded in fp32 at |u| ~ 1e-3 + theta: an absolute 6e-11 on theta, inside 1e-6 half_angle = 4.65e-9
        assert float(theta.max()) <= DISC * (1 + 1e-6)
    u2, _ = s.get_distortions(number_of_points=P, number_of_active_heliostats=H)
    assert torch.equal(u, u2)                                       # one seeded stream
    assert not torch.equal(u, s.get_distortions(number_of_points=P, number_of_active_heliostats=H, random_seed=8)[0])
    assert s.get_distortions_rows([1], number_of_points=P, number_of_active_heliostats=H) is None   # CPU: the caller slices


def test_a_cpu_tracer_dataset_slices_the_one_stream():
    from artist_amd.sampling import DistortionsDataset
    s = sun("buie", rays=3)
    full = DistortionsDataset(s, 5, 4)
    part = DistortionsDataset(s, 5, 4, rows=[3, 1])
    assert torch.equal(part.distortions_u, full.distortions_u[[3, 1]]) and torch.equal(part.distortions_e, full.distortions_e[[3, 1]])


@pytest.mark.parametrize("kind, params, match", [
    ("pillbox", dict(half_angle=0.0), "half_angle"),
    ("pillbox", dict(half_angle=-1e-3), "half_angle"),
    ("pillbox", dict(half_angle=float("nan")), "half_angle"),
    ("buie", dict(circumsolar_ratio=0.0), "circumsolar_ratio"),
    ("buie", dict(circumsolar_ratio=1.0), "circumsolar_ratio"),
    ("buie", dict(circumsolar_ratio=-0.1), "circumsolar_ratio"),
    ("tabulated", dict(), "profile_angles"),
    ("tabulated", dict(profile_angles=[0.0, 1e-3]), "profile_radiance"),
    ("tabulated", dict(profile_angles=[1e-3], profile_radiance=[1.0]), "profile_angles"),
    ("tabulated", dict(profile_angles=[-1e-3, 1e-3], profile_radiance=[1.0, 1.0]), "profile_angles"),
    ("tabulated", dict(profile_angles=[0.0, 2e-3, 2e-3], profile_radiance=[1.0, 1.0, 1.0]), "profile_angles"),
    ("tabulated", dict(profile_angles=[0.0, 2e-3, 1e-3], profile_radiance=[1.0, 1.0, 1.0]), "profile_angles"),
    ("tabulated", dict(profile_angles=[0.0, 1e-3, 2e-3], profile_radiance=[1.0, 1.0]), "profile_radiance"),
    ("tabulated", dict(profile_angles=[0.0, 1e-3, 2e-3], profile_radiance=[1.0, -1.0, 1.0]), "profile_radiance"),
    ("tabulated", dict(profile_angles=[0.0, 1e-3, 2e-3], profile_radiance=[0.0, 0.0, 0.0]), "profile_radiance"),
])
def test_bad_parameters_are_value_errors_that_name_the_parameter(kind, params, match):
    with pytest.raises(ValueError, match=match):
        sun(kind, **params)


def test_unknown_types_and_the_normal_sun_are_as_before():
    from artist_amd.scene import Sun
    for kind in ("uniform", "Pillbox", "gaussian", ""):
        with pytest.raises(ValueError, match=r"^Unknown sunlight distribution type\.$"):
            Sun(3, dict(distribution_type=kind))
    normal = Sun(3, device="cpu")
    assert normal.quantile_table is None and isinstance(normal.distribution, torch.distributions.MultivariateNormal)
    assert normal.distribution_parameters == dict(distribution_type="normal", mean=0.0, covariance=4.3681e-06)
    with pytest.raises(ValueError, match="quantile table"):
        normal.quantile_table = torch.zeros(2)


def test_a_tabulated_sun_with_a_dark_centre_and_a_dark_rim():
    """Radiance only between 2 and 3 mrad: every radius of the table lies there, whatever the zeros around it."""
    s = sun("tabulated", profile_angles=[1e-3, 2e-3, 2.5e-3, 3e-3, 4e-3], profile_radiance=[0.0, 0.0, 1.0, 0.0, 0.0])
    t2 = s.quantile_table.numpy().astype(np.float64)
    assert (np.diff(t2) >= 0).all() and abs(t2[0] - 4e-6) <= 1e-12 and abs(t2[-1] - 9e-6) <= 1e-12
    assert abs(np.sqrt(t2[K // 2]) - 2.5e-3) < 2e-5                # the triangle's median, sin(theta) tilting it outwards


def test_quantile_table_builder_takes_a_callable_and_a_sampled_profile():
    from artist_amd.scene import radial_quantile_table
    flat = radial_quantile_table(lambda theta: np.ones_like(theta), 8, theta_max=2e-3)
    assert flat.dtype == torch.float32 and tuple(flat.shape) == (9,)
    np.testing.assert_allclose(flat.numpy(), np.arange(9) / 8 * 4e-6, rtol=1e-5, atol=1e-13)   # a disc: theta^2 uniform
    sampled = radial_quantile_table(([0.0, 2e-3], [1.0, 1.0]), 8)
    np.testing.assert_allclose(sampled.numpy(), flat.numpy(), rtol=1e-5, atol=1e-13)
    step = radial_quantile_table(lambda theta: np.where(theta <= 1e-3, 3.0, 1.0), 2, theta_max=2e-3, breaks=(1e-3,))
    np.testing.assert_allclose(step.numpy(), [0.0, 1e-6, 4e-6], rtol=1e-5)                      # half the energy on either side
    for bad in (dict(K=0, theta_max=1e-3), dict(K=4), dict(K=4, theta_max=0.0)):
        with pytest.raises(ValueError, match="K|theta_max"):
            radial_quantile_table(lambda theta: np.ones_like(theta), **bad)
    with pytest.raises(ValueError, match="positive integral"):
        radial_quantile_table(lambda theta: np.zeros_like(theta), 4, theta_max=1e-3)


def test_restated_rule_on_a_pillbox_and_at_the_ends_of_the_table():
    ue = sunshape_ref.radial_rows(-3, [0, 1 << 40], 20001, np.float32([0.0, 4.0]))
    assert ue.shape == (2, 20001, 2) and np.isfinite(ue).all() and not np.array_equal(ue[0], ue[1])
    r2 = (ue ** 2).sum(-1)
    assert r2.max() <= 4.0 * (1 + 1e-12) and abs(r2.mean() - 2.0) < 0.03          # theta^2 uniform on [0, 4]
    shifted = sunshape_ref.radial_rows(-3, [0], 20001, np.float32([0.0, 4.0]), loc=(1.0, -2.0))
    np.testing.assert_allclose(shifted[0] - ue[0], np.broadcast_to([1.0, -2.0], (20001, 2)), atol=1e-12)


def test_hip_sampler_on_a_cpu_radial_sun_has_no_fallback():
    from artist_amd import _lib, ops
    s = sun("pillbox", sampler="hip")
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        s.get_distortions(number_of_points=3, number_of_active_heliostats=2)
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        ops.sample_radial_distortions([0], 2, 3, 7, (0.0, 0.0), s.quantile_table, "cpu")


def test_radial_sampler_argument_checks_need_no_device():
    from artist_amd import _lib
    f = _lib.lib().art_sample_radial_distortions
    loc = (0.0, 0.0)
    assert f(7, None, 0, 3, 5, *loc, None, 1, None, None) == 0     # nothing to draw: no launch, no pointer needed
    assert f(7, None, 4, 0, 5, *loc, None, 4096, None, None) == 0
    assert f(7, None, -1, 3, 5, *loc, None, 1, None, None) == _lib.ART_EINVAL
    assert f(7, None, 2, 3, -5, *loc, None, 1, None, None) == _lib.ART_EINVAL
    for bad_k in (0, -1, 4097, 1 << 40):                            # K out of range, with and without work to do
        assert f(7, None, 0, 3, 5, *loc, None, bad_k, None, None) == _lib.ART_EINVAL
        assert f(7, None, 2, 3, 5, *loc, None, bad_k, None, None) == _lib.ART_EINVAL
    assert f(7, None, 2, 3, 5, *loc, None, 1, None, None) == _lib.ART_EINVAL       # null pointers with work to do
    rows, out = (ctypes.c_int64 * 2)(), (ctypes.c_float * 64)()              # (never reached: the null table returns first)
    assert f(7, ctypes.addressof(rows), 2, 3, 5, *loc, None, 1, ctypes.addressof(out), None) == _lib.ART_EINVAL


class Leaf:
    """An HDF5 dataset stand-in: ``leaf[()]`` is its value."""

    def __init__(self, value):
        self.value = value

    def __getitem__(self, key):
        assert key == ()
        return self.value


def light_source(kind, **params):
    dp = {"distribution_type": Leaf(kind.encode())}
    dp.update({k: Leaf(v) for k, v in params.items()})
    return {"type": Leaf(b"sun"), "number_of_rays": Leaf(np.int64(6)), "distribution_parameters": dp}


def test_reader_round_trips_the_new_keys():
    from artist_amd import scenario
    from artist_amd.scene import LightSourceArray, Sun
    angles, radiance = np.linspace(0.0, 5e-3, 7), np.linspace(1.0, 0.5, 7)
    cfg = {"lightsources": {
        "a_pillbox": light_source("pillbox", half_angle=np.float64(3e-3)),
        "b_buie": light_source("buie", circumsolar_ratio=np.float64(0.2)),
        "c_table": light_source("tabulated", profile_angles=angles, profile_radiance=radiance),
        "d_normal": light_source("normal", mean=np.float64(0.0), covariance=np.float64(4.3681e-06))}}
    pill, buie, table, normal = scenario.read_light_sources(cfg)
    assert pill == dict(name="a_pillbox", number_of_rays=6, distribution_parameters=dict(distribution_type="pillbox", half_angle=3e-3))
    assert buie["distribution_parameters"] == dict(distribution_type="buie", circumsolar_ratio=0.2)
    assert sorted(table["distribution_parameters"]) == ["distribution_type", "profile_angles", "profile_radiance"]
    np.testing.assert_array_equal(table["distribution_parameters"]["profile_angles"], angles)
    np.testing.assert_array_equal(table["distribution_parameters"]["profile_radiance"], radiance)
    assert normal["distribution_parameters"] == dict(distribution_type="normal", mean=0.0, covariance=4.3681e-06)   # as before
    suns = LightSourceArray.from_hdf5(cfg, device="cpu").light_source_list
    assert [s.distribution_parameters["distribution_type"] for s in suns] == ["pillbox", "buie", "tabulated", "normal"]
    assert suns[0].quantile_table.tolist() == [0.0, float(np.float32(9e-6))] and suns[3].quantile_table is None
    assert torch.equal(suns[2].quantile_table, Sun(6, table["distribution_parameters"], device="cpu").quantile_table)
    one = Sun.from_hdf5(cfg["lightsources"]["b_buie"], "b_buie", device="cpu")
    assert one.number_of_rays == 6 and tuple(one.quantile_table.shape) == (K + 1,)
