"""Numpy fp64 restatement of the slope-error tilt (artist_amd.optics.tilt_normals) and of its sample zeta on
tests/philox_ref.py, and the law test of the reflected direction.  Test infrastructure."""
import math

import numpy as np

import philox_ref

SLOPE_STREAM = 0xBF58476D1CE4E5B9           # written down here independently of artist_amd.optics.SLOPE_ERROR_STREAM
OPTICAL_STREAM = 0x9E3779B97F4A7C15         # artist_amd.scene.OPTICAL_ERROR_STREAM
LAW_SEED, LAW_N = 7, 200_000
LAW_SIGMA = 1.5e-3
LAW_ANGLES = (0.0, math.radians(40.0))

# roundings on the way from (n, a, b) to a component of n' (each at most one unit roundoff u = eps / 2, relative to a vector of
# length about 1): x.n * n and the subtraction (2), normalize t1 = squares, sum, sqrt, divide (5), the cross product (3),
# a t1, b t2 and the two additions (4), the last normalize (5)
TILT_OPERATIONS = 19


def _normalize(v, eps=1e-12):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), eps)


def tilt(normals, slopes):
    """``normals [..., 4]``, ``slopes [..., 2]`` -> tilted normals ``[..., 4]`` (float64)."""
    normals, slopes = np.asarray(normals, dtype=np.float64), np.asarray(slopes, dtype=np.float64)
    n = normals[..., :3]
    x = np.zeros_like(n)
    x[..., 0] = 1.0
    t1 = _normalize(x - n[..., :1] * n)
    t2 = np.cross(n, t1)
    tilted = _normalize(n + slopes[..., :1] * t1 + slopes[..., 1:] * t2)
    return np.concatenate((tilted, normals[..., 3:]), axis=-1)


def zeta_rows(seed, rows, n_points):
    """The standard normal pairs ``zeta[k, p, 0:2]`` of heliostats ``rows``: the sampler's stream, one ray per point, with the
    seed XOR the slope stream's constant."""
    return philox_ref.gaussian_rows((int(seed) & 0xFFFFFFFFFFFFFFFF) ^ SLOPE_STREAM, rows, n_points)


def reflect(incident, normals):
    return incident - 2.0 * np.sum(incident * normals, axis=-1, keepdims=True) * normals


def check_law(theta, sigma=LAW_SIGMA, seed=LAW_SEED, n=LAW_N):
    """A flat mirror (normal z) under a ray at incidence ``theta`` in the x-z plane, its normal tilted by ``sigma * zeta`` for
    ``n`` restated pairs: the reflected direction's deviation from the specular one has the variance ``(2 sigma)^2`` in the plane
    of incidence and ``(2 sigma cos theta)^2`` across it, each within 4 standard errors ``var * sqrt(2 / n)``.  Returns the two
    deviations in standard errors."""
    zeta = zeta_rows(seed, [0], n)[0]
    normals = np.zeros((n, 4))
    normals[:, 2] = 1.0
    incident = np.array([math.sin(theta), 0.0, -math.cos(theta), 0.0])
    reflected = reflect(incident[None], tilt(normals, sigma * zeta))[:, :3]
    specular = np.array([math.sin(theta), 0.0, math.cos(theta)])
    in_plane = np.array([math.cos(theta), 0.0, -math.sin(theta)])          # perpendicular to the specular ray, in the x-z plane
    across = np.array([0.0, 1.0, 0.0])
    deviation = reflected - specular
    out = []
    for axis, want in ((in_plane, (2.0 * sigma) ** 2), (across, (2.0 * sigma * math.cos(theta)) ** 2)):
        got = float(np.var(deviation @ axis, ddof=1))
        errors = abs(got - want) / (want * math.sqrt(2.0 / n))
        assert errors <= 4.0, (theta, axis, got, want, errors)
        out.append(errors)
    return out
