"""The gradient of the convolved sun's window, the part that needs no GPU: the fp64 reference
(tests/flux_blur_grad_ref.py) against difference quotients of ``flux_blur_ref.blur``, its rules for identity passes and invalid
covariances, ``optics.sun_image_covariance(differentiable=True)``, ``Sun.window_gradient`` and the refusals that stay, the case
table against the kernel's named branches, and the sigma recovery of the GPU test in numpy."""
import math
import pathlib

import numpy as np
import pytest
import torch

import flux_blur_grad_ref as gref
import flux_blur_ref as ref
import test_flux_blur_host as host
from artist_amd import _lib, flux, optics, scene

GOLDEN = pathlib.Path(__file__).parent / "golden" / "sun_convolution.npz"
Hh, W = 48, 40


def inputs():
    """A sparse bitmap and a white-noise upstream gradient."""
    rng = np.random.default_rng(3)
    x = (rng.random((Hh, W)) < 0.2) * rng.random((Hh, W))
    return x, rng.standard_normal((Hh, W))


def loss(x, g, covariance):
    return float((g * ref.blur_one(x, covariance)).sum())


# ---- the definition against difference quotients -----------------------------------------------------------------------------------
@pytest.mark.parametrize("covariance", [(0.64, 0.1, 0.64), (1.5, 0.4, 1.0), (4.1, -5.0, 9.0), (4.1, 0.3, 3.3)])
def test_reference_against_central_differences(covariance):
    x, g = inputs()
    S = np.array(covariance, np.float64)
    step = 1e-5 * np.maximum(1.0, np.abs(S))
    assert gref.crossings(S, step) == []            # no radius threshold and no integer s k inside the step: the quotient is valid
    got = gref.covariance_gradient(x, g, S)
    quotient = np.array([(loss(x, g, S + e) - loss(x, g, S - e)) / (2.0 * e[i]) for i, e in enumerate(np.diag(step))])
    error = np.abs(got - quotient).max() / np.abs(got).max()
    print(covariance, "gradient", got, "central differences", quotient, "error / largest component", error)
    assert error <= 1e-6


def test_crossings_are_noticed():
    assert gref.crossings((4.0, 0.0, 4.0), (1e-5,) * 3) == ["integer s k", "radius"]         # K = ceil(4 sqrt(4)) jumps, and s = 0
    assert gref.crossings((4.1, 2.05, 3.3), (1e-5,) * 3) == ["integer s k"]                  # s = 1/2: every second tap
    assert gref.crossings((4.1, 0.3, 3.3), (1e-5,) * 3) == []


def test_integer_positions_take_the_mean_of_the_one_sided_slopes():
    """At ``S_rc = 0`` every tap sits on a pixel and ``L`` has a kink in ``S_rc``: the definition's value is the mean of the left
    and the right difference quotient (which differ by far more than the bound)."""
    x, g = inputs()
    S, h = np.array((3.3, 0.0, 2.2)), 1e-5
    e = np.array((0.0, h, 0.0))
    right, left = (loss(x, g, S + e) - loss(x, g, S)) / h, (loss(x, g, S) - loss(x, g, S - e)) / h
    got = gref.covariance_gradient(x, g, S)
    print("dL/dS_rc", got[1], "right", right, "left", left)
    assert abs(right - left) > 0.1 * abs(got).max()
    assert abs(got[1] - 0.5 * (left + right)) <= 1e-6 * np.abs(got).max()


def test_identity_passes_and_invalid_covariances():
    x, g = inputs()
    row_identity = gref.covariance_gradient(x, g, (1e-5, 0.0, 6.0))
    assert row_identity[0] == 0.0 and row_identity[1] == 0.0 and row_identity[2] != 0.0
    h = 1e-5                                    # ... and D_a is the derivative with respect to S_cc
    quotient = (loss(x, g, (1e-5, 0.0, 6.0 + h)) - loss(x, g, (1e-5, 0.0, 6.0 - h))) / (2 * h)
    assert abs(row_identity[2] - quotient) <= 1e-6 * abs(quotient)
    column_identity = gref.covariance_gradient(x, g, (6.0, 0.0, 1e-5))
    assert column_identity[2] == 0.0 and column_identity[0] != 0.0
    assert not gref.covariance_gradient(x, g, (1e-5, 0.0, 1e-5)).any()
    assert abs(gref.derivative_tap(2.5, 7, np.float64).sum()) <= 1e-15 and not gref.derivative_tap(1e-5, 0, np.float64).any()
    for bad in [(4.0, 5.0, 4.0), (-1.0, 0.0, 1.0), (float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0), (256.5, 0.0, 1.0)]:
        assert np.isnan(gref.covariance_gradient(x, g, bad)).all(), bad
        assert np.isnan(gref.covariance_gradient(x, g, bad, np.float32)).all(), bad
    assert np.isfinite(gref.covariance_gradient(x, g, (256.0, 0.0, 256.0))).all()


def test_yardstick_is_small():
    """The fp32 evaluation is within 1e-4 of the scale of the sum: it measures rounding, not another operator."""
    x, g = inputs()
    for covariance in gref.OPERATOR_COVARIANCES:
        low, want = (gref.covariance_gradient(x, g, covariance, dt) for dt in (np.float32, np.float64))
        assert (np.abs(low - want) <= 1e-4 * gref.magnitude(x, g, covariance) + 1e-30).all(), covariance


# ---- the window's covariance in the graph -----------------------------------------------------------------------------------------
def jacobian(d, k):
    """``J [(row, column), (u, e)]`` of fixture geometry ``k`` in numpy fp64: the formulas of ``optics.sun_image_covariance``."""
    o = d["points"][k, :, :3].astype(np.float64).mean(axis=0)
    n = d["normals"][k, :, :3].astype(np.float64).mean(axis=0)
    n /= np.linalg.norm(n)
    i = d["incident"][k, :3].astype(np.float64)
    ray = i - 2.0 * (i @ n) * n
    t_idx = int(d["target_idx"][k])
    c, m, size = (d[key][t_idx].astype(np.float64) for key in ("centers", "plane_normals", "dimensions"))
    c, m = c[:3], m[:3]
    dm = ray @ m
    t = ((c - o) @ m) / dm
    axes = np.array([(-ray[1], ray[0], 0.0), (0.0, -ray[2], ray[1])])               # a_u = z x d, a_e = x x d
    shift = t * (axes - ray[None] * ((axes @ m) / dm)[:, None])                     # [(u, e), (E, N, U)]
    columns, rows = (float(v) for v in d["resolution"][k])
    return -np.stack((shift[:, 2] * (rows - 1.0) / size[1], shift[:, 0] * (columns - 1.0) / size[0]))


def test_differentiable_sun_image_covariance():
    """The same bits as the default call, and the autograd gradient of ``sum(w S)`` with respect to ``(C_uu, C_ue, C_ee)`` against
    the closed form from ``J`` (``S`` is linear in ``C``) to 1e-12 relative - ``J`` restated in numpy fp64 from the fixture's
    geometries and held to the fixture's own finite-difference Jacobians first."""
    d = np.load(GOLDEN)
    t = lambda key, k: torch.from_numpy(d[key][k:k + 1])  # noqa: E731
    tables = tuple(torch.from_numpy(d[key]) for key in ("centers", "plane_normals", "dimensions"))
    w = np.array([0.75, -1.25, 0.5])                # exact in fp32: S is fp32, and so is the gradient that enters its cast
    for k in range(d["points"].shape[0]):
        J = jacobian(d, k)
        assert np.abs(J - d["jacobian"][k]).max() <= 1e-4 * np.abs(d["jacobian"][k]).max()
        for angular, per_heliostat in (((4.3681e-6, 1.5e-6, 9.0e-6), False), ((1.0e-6, -0.8e-6, 2.5e-6), True)):
            C = torch.tensor([angular] if per_heliostat else angular, dtype=torch.float64, requires_grad=True)
            args = (t("points", k), t("normals", k), t("incident", k), t("target_idx", k), *tables)
            resolution = tuple(d["resolution"][k])
            S = optics.sun_image_covariance(*args, C, resolution, differentiable=True)
            plain = optics.sun_image_covariance(*args, C.detach(), resolution)
            assert S.requires_grad and not plain.requires_grad and S.dtype == torch.float32 and torch.equal(S.detach(), plain)
            assert not optics.sun_image_covariance(*args, C, resolution).requires_grad              # the default call: a constant
            (S[0].double() * torch.from_numpy(w)).sum().backward()
            (r_u, r_e), (c_u, c_e) = J
            dS = np.array([[r_u * r_u, 2 * r_u * r_e, r_e * r_e],                       # S_rr
                           [r_u * c_u, r_u * c_e + r_e * c_u, r_e * c_e],               # S_rc
                           [c_u * c_u, 2 * c_u * c_e, c_e * c_e]])                      # S_cc, each by (C_uu, C_ue, C_ee)
            want = w @ dS
            got = C.grad.reshape(3).numpy()
            assert (np.abs(got - want) <= 1e-12 * np.abs(want).max()).all(), (k, got, want)


# ---- the switch and the refusals that stay ------------------------------------------------------------------------------------------
def test_window_gradient_is_a_checked_property():
    sun = scene.Sun(4)
    assert sun.window_gradient is False
    sun.window_gradient = True
    assert sun.window_gradient is True
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="window_gradient must be True or False"):
            sun.window_gradient = bad
    assert sun.window_gradient is True
    sun.window_gradient = False
    assert sun.window_gradient is False


def learned_group():
    group = host.cpu_group()
    group.optical_errors = torch.tensor([1e-3, 2e-3, 3e-3], requires_grad=True)
    return group


@pytest.mark.parametrize("window", scene.WINDOWS)
def test_without_the_switch_the_refusals_are_unchanged(window):
    sun = scene.Sun(4)
    sun.integration, sun.window = "convolved", window
    with pytest.raises(ValueError, match="optical_errors.requires_grad must be False"):
        host.tracer_of(sun, learned_group())
    x, cov = torch.zeros(2, 4, 5), torch.ones(2, 3)
    with pytest.raises(ValueError, match="covariance of blur_flux is a constant"):
        flux.blur_flux(x, cov.clone().requires_grad_(True))


def test_with_the_switch_learned_optical_errors_pass_the_check():
    """... and the next check is the device: no CPU fallback, for the tracer and for the operator."""
    sun = scene.Sun(4)
    sun.integration, sun.window_gradient = "convolved", True
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        host.tracer_of(sun, learned_group())
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        flux.differentiable_blur_flux(torch.zeros(2, 4, 5), torch.ones(2, 3, requires_grad=True))
    import artist_amd
    assert artist_amd.differentiable_blur_flux is flux.differentiable_blur_flux


def test_the_c_abi_is_untouched():
    assert _lib.ABI_VERSION == 13 and not any("blur" in name for name in _lib.SIGNATURES)


# ---- the kernel's branches -----------------------------------------------------------------------------------------------------------
def test_the_case_table_covers_every_branch():
    seen = set()
    for covariance, shape in gref.CASES:
        plan = gref.tiling(covariance, *shape)
        assert plan is not None, (covariance, shape)
        assert plan["TR"] <= gref.TILE_ROWS and plan["TR"] + 2 * plan["Kr"] <= gref.TILE_ROWS + 2 * ref.MAX_RADIUS
        seen |= plan["branches"]
    assert seen == gref.BRANCHES, gref.BRANCHES - seen
    for bad in [(4.0, 5.0, 4.0), (300.0, 0.0, 9.0), (float("nan"), 0.0, 1.0)]:
        assert gref.tiling(bad, 48, 40) is None


def test_claimed_branches():
    claims = [((256.0, 0.0, 256.0), (300, 130), {"row_taps==129", "column_taps==129", "tile_rows>1", "tile_columns>1", "whole_taps"}),
              ((256.0, 200.0, 256.0), (257, 66), {"row_taps==129", "column_taps<=128", "fraction_taps", "clamped_rows"}),
              ((0.03125, 2.0078125, 160.0), (300, 130), {"shear10", "corner_tiles", "tile_rows>1"}),
              ((0.01, 0.9, 100.0), (7, 3), {"shear10", "Hh<TR", "idle_waves"}),
              ((1e-5, 0.0, 256.0), (129, 70), {"row_identity", "column_taps==129"}),
              ((256.0, 0.0, 1e-5), (129, 70), {"column_identity"}),
              ((100.0, 30.0, 100.0), (300, 130), {"row_taps<=128", "column_taps<=128", "shear16"})]
    for covariance, shape, names in claims:
        assert names <= gref.tiling(covariance, *shape)["branches"], (covariance, shape)


# ---- a sigma that learns ---------------------------------------------------------------------------------------------------------------
def test_sigma_recovery_in_fp64():
    """The GPU test's recovery (tests/test_gpu_flux_blur_grad.py) with the fp64 reference as the operator: 1.4929e-3."""
    x = gref.sparse_spot(np.random.default_rng(0)).astype(np.float64)
    M = gref.RECOVERY_METRIC
    target = ref.blur_one(x, M * gref.RECOVERY["truth"] ** 2)

    def loss_gradient(sigma):
        S = M * sigma * sigma
        residual = ref.blur_one(x, S) - target
        return float((gref.covariance_gradient(x, residual, S) * M).sum() * 2.0 * sigma)

    sigma = gref.adam_recovery(loss_gradient)
    print("sigma after", gref.RECOVERY["steps"], "steps:", sigma)
    assert abs(sigma - gref.RECOVERY["truth"]) <= gref.RECOVERY["bound"] * gref.RECOVERY["truth"]
    assert math.isclose(sigma, 1.4929e-3, rel_tol=1e-4)
