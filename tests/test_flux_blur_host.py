"""The convolved sun, the part that needs no GPU: the fp64 reference operator's own properties, the Jacobian of
``optics.sun_image_covariance`` against the reference's ``rotate_distortions`` + ``line_plane_intersections`` (a stored
finite-difference fixture), and every refusal with its message."""
import pathlib

import numpy as np
import pytest
import torch

import flux_blur_ref as ref
from artist_amd import HeliostatRayTracer, _lib, flux, optics, scene

GOLDEN = pathlib.Path(__file__).parent / "golden" / "sun_convolution.npz"

# the covariances of the GPU operator test (tests/test_gpu_flux_blur.py): every branch of the definition
COVARIANCES = [(0.64, 0.0, 0.64), (9.0, 3.0, 4.0), (4.0, -5.0, 9.0), (9.0, 6.0, 4.00001), (1e-5, 0.0, 6.0), (30.0, 0.0, 30.0)]


# ---- the reference operator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("covariance", COVARIANCES + [(118.86, 54.12, 178.89)])
def test_reference_operator_is_self_adjoint(covariance):
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((2, 48, 40))
    fx, fy = ref.blur_one(x, covariance), ref.blur_one(y, covariance)
    assert abs((fx * y).sum() - (x * fy).sum()) <= 1e-12 * np.linalg.norm(x) * np.linalg.norm(y)


@pytest.mark.parametrize("covariance", COVARIANCES[:5])
def test_reference_operator_keeps_the_sum_of_an_interior_delta(covariance):
    x = np.zeros((96, 80))
    x[48, 40] = 1.0                       # the widest of these windows reaches 12 rows and 17 columns
    z = ref.blur_one(x, covariance)
    assert abs(z.sum() - 1.0) <= 1e-12
    assert z.min() >= 0.0


def test_reference_operator_has_the_covariance_it_is_given():
    """The second moments of a delta's image are the covariance, up to the truncation at 4 sigma, the lattice and the
    linear interpolation's own variance f (1 - f) <= 1/4 per tap: within 2 % + 0.3 px^2."""
    for covariance in [(9.0, 3.0, 4.0), (4.0, -5.0, 9.0), (50.7, -3.3, 16.3)]:
        n = 129
        x = np.zeros((n, n))
        x[n // 2, n // 2] = 1.0
        z = ref.blur_one(x, covariance)
        r, c = np.mgrid[:n, :n] - n // 2
        got = ((z * r * r).sum(), (z * r * c).sum(), (z * c * c).sum())
        for g, want in zip(got, covariance):
            assert abs(g - want) <= 0.02 * max(covariance[0], covariance[2]) + 0.3, (covariance, got)


def test_reference_operator_marks_what_it_cannot_blur():
    x = np.ones((4, 5))
    for bad in [(4.0, 5.0, 4.0), (-1.0, 0.0, 1.0), (1.0, 0.0, -1.0), (float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0),
                (256.5, 0.0, 1.0), (1.0, 0.0, 300.0)]:
        assert np.isnan(ref.blur_one(x, bad)).all(), bad
    assert np.array_equal(ref.blur_one(x, (0.0, 0.0, 0.0)), x)              # both passes the identity
    assert np.isfinite(ref.blur_one(x, (256.0, 0.0, 256.0))).all()          # the limit itself: 4 sqrt(256) = 64


# ---- the Jacobian ------------------------------------------------------------------------------------------------------------
ANGULAR = [(4.3681e-6, 0.0, 4.3681e-6), (4.3681e-6, 1.5e-6, 9.0e-6), (1.0e-6, -0.8e-6, 2.5e-6)]


def test_sun_image_covariance_against_the_reference_jacobian():
    """``J C J^T`` with the fixture's fp64 finite-difference ``J`` of the reference's own two functions: every entry within 1e-4
    relative.  Both sides start from the same fp32 inputs; the rounding of the fp32 result is ~1e-7 and the central
    difference's own error ~1e-9 of the matrix's scale; a wrong sign, a swapped axis or a missing flip is an error of order 1."""
    d = np.load(GOLDEN)
    t = lambda k: torch.from_numpy(d[k])  # noqa: E731
    G = d["points"].shape[0]
    assert G >= 8 and len({tuple(r) for r in d["resolution"]}) >= 4
    for angular in ANGULAR:
        for per_heliostat in (False, True):
            a = torch.tensor(angular, dtype=torch.float32)
            for g in range(G):
                got = optics.sun_image_covariance(
                    t("points")[g:g + 1], t("normals")[g:g + 1], t("incident")[g:g + 1], t("target_idx")[g:g + 1], t("centers"),
                    t("plane_normals"), t("dimensions"), a.repeat(1, 1) if per_heliostat else a, tuple(d["resolution"][g]))
                assert got.shape == (1, 3) and got.dtype == torch.float32 and not got.requires_grad
                J = d["jacobian"][g]
                want = J @ np.array([[float(a[0]), float(a[1])], [float(a[1]), float(a[2])]], np.float64) @ J.T
                want = np.array([want[0, 0], want[0, 1], want[1, 1]])
                assert (np.abs(got[0].double().numpy() - want) <= 1e-4 * np.abs(want)).all(), (g, angular, got, want)
    # all heliostats in one call: the rows of the calls above
    res = tuple(d["resolution"][0])
    same = [g for g in range(G) if tuple(d["resolution"][g]) == res]
    batch = optics.sun_image_covariance(t("points")[same], t("normals")[same], t("incident")[same], t("target_idx")[same],
                                        t("centers"), t("plane_normals"), t("dimensions"), torch.tensor(ANGULAR[1]), res)
    for k, g in enumerate(same):
        one = optics.sun_image_covariance(t("points")[g:g + 1], t("normals")[g:g + 1], t("incident")[g:g + 1],
                                          t("target_idx")[g:g + 1], t("centers"), t("plane_normals"), t("dimensions"),
                                          torch.tensor(ANGULAR[1]), res)
        assert torch.equal(batch[k], one[0])
    with pytest.raises(ValueError, match="angular_covariance must be"):
        optics.sun_image_covariance(t("points")[:1], t("normals")[:1], t("incident")[:1], t("target_idx")[:1], t("centers"),
                                    t("plane_normals"), t("dimensions"), torch.zeros(2), res)


def test_table_rows_from_the_fixture():
    """The first three geometries are the issue's table: sigma^2 = 4.3681e-6 gives its covariances (to the digits it prints)."""
    d = np.load(GOLDEN)
    table = [(50.7, -3.3, 16.3), (74.5, -83.7, 121.7), (118.9, 54.1, 178.9)]
    for g, want in enumerate(table):
        got = optics.sun_image_covariance(*(torch.from_numpy(d[k][g:g + 1]) for k in ("points", "normals", "incident", "target_idx")),
                                          *(torch.from_numpy(d[k]) for k in ("centers", "plane_normals", "dimensions")),
                                          torch.tensor([4.3681e-6, 0.0, 4.3681e-6]), (256, 256))
        assert np.abs(got[0].numpy() - np.array(want)).max() <= 0.06, (got, want)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def cpu_group(n=3, points=4):
    z = torch.zeros
    return scene.HeliostatGroup(names=[f"h{i}" for i in range(n)],
                                positions=torch.tensor([[10.0 * i, 100.0 + 50.0 * i, 0.0, 1.0] for i in range(n)]),
                                surface_points=torch.rand(n, points, 4), surface_normals=torch.rand(n, points, 4),
                                canting=z(n, 4, 2, 4), facet_translations=z(n, 4, 4), nurbs_control_points=z(n, 4, 2, 2, 3),
                                nurbs_degrees=torch.tensor([1, 1]))


def cpu_scenario(group, sun):
    planar = scene.TowerTargetAreasPlanar(names=["a"], centers=torch.tensor([[0.0, 0.0, 55.0, 1.0]]),
                                          normals=torch.tensor([[0.0, 1.0, 0.0, 0.0]]), dimensions=torch.tensor([[8.0, 8.0]]))
    return scene.Scenario(torch.zeros(3), scene.SolarTower([planar]), scene.LightSourceArray([sun]), scene.HeliostatField([group]))


def test_integration_is_a_checked_property():
    sun = scene.Sun(4)
    assert sun.integration == "sampled" and scene.INTEGRATIONS == ("sampled", "convolved")
    sun.integration = "convolved"
    assert sun.integration == "convolved"
    with pytest.raises(ValueError, match="Unknown sun integration 'analytic'"):
        sun.integration = "analytic"
    assert sun.integration == "convolved"
    sun.integration = "sampled"
    assert sun.integration == "sampled"


def tracer_of(sun, group=None):
    group = cpu_group() if group is None else group
    group.activate_heliostats(torch.ones(3, dtype=torch.int32))
    return HeliostatRayTracer(cpu_scenario(group, sun), group, blocking_active=False)


@pytest.mark.parametrize("kind", scene.RADIAL_TYPES)
def test_a_radial_sun_cannot_be_convolved(kind):
    params = dict(distribution_type=kind)
    if kind == "tabulated":
        params.update(profile_angles=[0.0, 4e-3, 5e-3], profile_radiance=[1.0, 0.8, 0.0])
    sun = scene.Sun(4, params)
    sun.integration = "convolved"
    with pytest.raises(ValueError, match="needs a Gaussian sun"):
        tracer_of(sun)


def test_a_sun_off_centre_cannot_be_convolved():
    sun = scene.Sun(4, dict(mean=1e-3))
    sun.integration = "convolved"
    with pytest.raises(ValueError, match="needs a sun centred on 0"):
        tracer_of(sun)


def test_learned_optical_errors_cannot_be_convolved():
    sun = scene.Sun(4)
    sun.integration = "convolved"
    group = cpu_group()
    group.optical_errors = torch.tensor([1e-3, 2e-3, 3e-3], requires_grad=True)
    with pytest.raises(ValueError, match="optical_errors.requires_grad must be False"):
        tracer_of(sun, group)


def test_a_sun_on_the_cpu_has_no_fallback():
    sun = scene.Sun(4)
    sun.integration = "convolved"
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        tracer_of(sun)
    sun.integration = "sampled"                     # ... and sampled, the same sun builds its tracer as before
    assert tracer_of(sun).integration == "sampled"


def test_blur_flux_refusals():
    x, cov = torch.zeros(2, 4, 5), torch.ones(2, 3)
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        flux.blur_flux(x, cov)
    with pytest.raises(ValueError, match="covariance of blur_flux is a constant"):
        flux.blur_flux(x, cov.clone().requires_grad_(True))


def test_the_c_abi_is_untouched():
    """The blur is a mode of an existing entry point: no export, no signature and no header was added."""
    assert "art_flux_crop_fwd" in _lib.SIGNATURES and not any("blur" in name for name in _lib.SIGNATURES)
    assert _lib.ABI_VERSION == 13
