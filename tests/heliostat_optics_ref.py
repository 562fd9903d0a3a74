"""Numpy restatement of a draw with optical errors (artist_amd.scene.Sun) on tests/philox_ref.py and
tests/sunshape_ref.py, and the law test both the GPU test and its CPU rehearsal apply.  Test infrastructure."""
import math

import numpy as np

import philox_ref
import sunshape_ref

ERROR_STREAM = 0x9E3779B97F4A7C15           # written down here independently of artist_amd.scene.OPTICAL_ERROR_STREAM
DISC = 4.65e-3
COVARIANCE = 4.3681e-06
LAW_SEED, LAW_ROWS, LAW_R, LAW_P = 7, 4, 4, 50_000
LAW_SIGMAS = (0.0, 1e-3, 2e-3, 3.5e-3)


def error_rows(seed, rows, n_rays_per_row):
    """The standard normal pairs ``z[k, i, 0:2]`` of the error stream: the sampler's stream with the seed XOR the constant."""
    return philox_ref.gaussian_rows((int(seed) & 0xFFFFFFFFFFFFFFFF) ^ ERROR_STREAM, rows, n_rays_per_row)


def draw_rows(kind, seed, rows, n_rays_per_row, sigmas, table=None):
    """``[len(rows), n, 2]`` float64: the sun's rows (``"normal"``: the default diagonal Gaussian; ``"pillbox"``: ``table``)
    plus ``sigma_row * z``."""
    if kind == "normal":
        s = math.sqrt(COVARIANCE)
        base = philox_ref.apply_law(philox_ref.gaussian_rows(seed, rows, n_rays_per_row), (0.0, 0.0), ((s, 0.0), (0.0, s)))
    else:
        base = sunshape_ref.radial_rows(seed, rows, n_rays_per_row, table)
    return base + np.asarray(sigmas, dtype=np.float64)[:, None, None] * error_rows(seed, rows, n_rays_per_row)


def sun_moments(kind):
    """(variance, fourth moment) of one component of the sun's law alone."""
    if kind == "normal":
        return COVARIANCE, 3.0 * COVARIANCE ** 2
    return DISC ** 2 / 4.0, DISC ** 4 / 8.0          # a uniform disc of radius a: E[x^2] = a^2/4, E[x^4] = a^4/8


def check_law(x, kind, sigmas):
    """``x [rows, n, 2]`` (float64 numpy): per row and component, mean and variance within 4 standard errors of 0 and
    ``var_sun + sigma_row^2``.  Returns the largest deviation in standard errors."""
    var_sun, m4_sun = sun_moments(kind)
    worst = 0.0
    for row, sigma in enumerate(sigmas):
        n = x.shape[1]
        var = var_sun + sigma ** 2
        m4 = m4_sun + 6.0 * var_sun * sigma ** 2 + 3.0 * sigma ** 4
        se_mean, se_var = math.sqrt(var / n), math.sqrt((m4 - var ** 2) / n)
        for comp in (0, 1):
            mean_dev = abs(x[row, :, comp].mean()) / se_mean
            var_dev = abs(x[row, :, comp].var(ddof=1) - var) / se_var
            assert mean_dev <= 4 and var_dev <= 4, (kind, row, comp, mean_dev, var_dev)
            worst = max(worst, mean_dev, var_dev)
    return worst
