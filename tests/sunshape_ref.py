"""numpy restatement of ``art_sample_radial_distortions`` (include/artist_hip_sampler.h): the Philox stream of
``tests/philox_ref.py``, then the quantile-table rule with fp32 ``q``, ``b``, ``t`` and float64 for the rest.  Also what the
law tests of the radial sun shapes share: Buie's formulas written down a second time, the moments and the CDF of a profile
on a fine float64 grid of their own, and the conditions a sample of the law has to meet."""
import math

import numpy as np

from philox_ref import MASK32, philox4x32_10

DISC, EXTENT = 4.65e-3, 43.6e-3                                   # rad: the solar disc's edge, the end of Buie's aureole


def radial_rows(seed, rows, n_rays_per_row, table, loc=(0.0, 0.0)):
    """``(u, e)[k, i, 0:2]`` of the ``n_rays_per_row`` rays of heliostat rows ``rows`` for the fp32 ``table`` [K+1], float64."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (s & 0xFFFFFFFF, s >> 32)
    t2 = np.asarray(table, dtype=np.float32).astype(np.float64)
    K = t2.shape[0] - 1
    n_pairs = (n_rays_per_row + 1) // 2
    j = np.arange(n_pairs, dtype=np.uint64)
    out = []
    for row in rows:
        r = int(row) & 0xFFFFFFFFFFFFFFFF
        x = philox4x32_10((j & MASK32, j >> np.uint64(32), np.uint64(r & 0xFFFFFFFF), np.uint64(r >> 32)), key)
        ue = np.empty((n_pairs, 2, 2))
        for half, (xe, xo) in enumerate(((x[0], x[1]), (x[2], x[3]))):
            q = xe.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)
            b = xo.astype(np.float32) * np.float32(2.0 ** -32)
            t = q * np.float32(K)
            assert q.dtype == b.dtype == t.dtype == np.float32
            i = np.minimum(t.astype(np.int64), K - 1)
            f = t.astype(np.float64) - i
            theta = np.sqrt(t2[i] + f * (t2[i + 1] - t2[i]))
            ue[:, half, 0] = loc[0] + theta * np.cos(2.0 * np.pi * b.astype(np.float64))
            ue[:, half, 1] = loc[1] + theta * np.sin(2.0 * np.pi * b.astype(np.float64))
        out.append(ue.reshape(2 * n_pairs, 2)[:n_rays_per_row])
    return np.stack(out)


def buie_radiance(theta, chi):
    """Buie, Monger and Dey (2003), ``theta`` in rad: the formulas written down independently of ``artist_amd.scene``."""
    mrad = np.asarray(theta, dtype=np.float64) * 1e3
    kappa = 0.9 * math.log(13.5 * chi) * chi ** -0.3
    gamma = 2.2 * math.log(0.52 * chi) * chi ** 0.43 - 0.1
    out = np.zeros_like(mrad)
    disc, aureole = mrad <= 4.65, (mrad > 4.65) & (mrad <= 43.6)
    out[disc] = np.cos(0.326 * mrad[disc]) / np.cos(0.308 * mrad[disc])
    out[aureole] = math.exp(kappa) * mrad[aureole] ** gamma
    return out


class Law:
    """A radial law on a fine grid: ``cdf(theta)``, ``m2 = E[theta^2]``, ``m4 = E[theta^4]``, for density ~ B sin(theta)."""

    def __init__(self, grid, radiance):
        w = radiance * np.sin(grid)
        cell = 0.5 * np.diff(grid)
        mass = np.concatenate(([0.0], np.cumsum(cell * (w[1:] + w[:-1]))))
        self.grid, self.mass, self.total = grid, mass / mass[-1], mass[-1]
        self.m2 = float(np.sum(cell * ((w * grid ** 2)[1:] + (w * grid ** 2)[:-1])) / mass[-1])
        self.m4 = float(np.sum(cell * ((w * grid ** 4)[1:] + (w * grid ** 4)[:-1])) / mass[-1])

    def cdf(self, theta):
        return float(np.interp(theta, self.grid, self.mass))


def buie_law(chi, points=500_001):
    """Buie's formulas integrated piece by piece, a grid point on either side of the jump at the disc's edge."""
    grid = np.concatenate((np.linspace(0.0, DISC, points), np.linspace(np.nextafter(DISC, 1.0), EXTENT, points)))
    return Law(grid, buie_radiance(grid, chi))


class PillboxLaw:
    """The uniform disc in the small-angle reading the sampler makes: ``theta^2`` uniform on ``[0, half_angle^2]``."""

    def __init__(self, half_angle):
        self.half_angle, self.m2, self.m4 = half_angle, half_angle ** 2 / 2.0, half_angle ** 4 / 3.0

    def cdf(self, theta):
        return min(1.0, (theta / self.half_angle) ** 2)


def table_share_beyond(table, theta):
    """The energy share a quantile table puts beyond ``theta`` (linear in ``theta^2`` inside an annulus)."""
    t2 = np.asarray(table, dtype=np.float64)
    K = t2.shape[0] - 1
    i = min(int(np.searchsorted(t2, theta * theta, side="right")) - 1, K - 1)
    return 1.0 - (i + (theta * theta - t2[i]) / (t2[i + 1] - t2[i])) / K


def check_radial_law(u, e, loc, law, radii, K):
    """``u``, ``e``: torch tensors of draws (any shape, any device) of the radial ``law`` centred on ``loc``, from a table of
    ``K`` annuli.  The empirical CDF of theta at ``radii`` within 4 sigma of binomial noise plus half an annulus (nothing for
    K = 1, where the table is the law itself); means, second moments and the correlation of u and e within 4 sigma."""
    import torch
    u, e = u.reshape(-1).double(), e.reshape(-1).double()
    N = u.numel()
    du, de = u - loc[0], e - loc[1]
    theta = torch.sqrt(du * du + de * de)
    half_annulus = 0.0 if K == 1 else 0.5 / K
    for r in radii:
        p = law.cdf(r)
        got = float((theta <= r).double().mean())
        tol = 4.0 * math.sqrt(p * (1.0 - p) / N) + half_annulus
        print(f"  cdf({r * 1e3:.3f} mrad): sample {got:.6f}, law {p:.6f}, tolerance {tol:.2e}")
        assert abs(got - p) <= tol, (r, got, p, tol)
    mean_sigma = math.sqrt(law.m2 / 2.0 / N)
    square_sigma = math.sqrt((0.375 * law.m4 - (law.m2 / 2.0) ** 2) / N)       # E[cos^4] = 3/8
    for name, d in (("u", du), ("e", de)):
        m, s = float(d.mean()), float((d * d).mean())
        print(f"  {name}: mean - loc {m:.3e} (sigma {mean_sigma:.2e}), E[{name}^2] {s:.6e} vs {law.m2 / 2.0:.6e} (sigma {square_sigma:.2e})")
        assert abs(m) <= 4.0 * mean_sigma, (name, m, mean_sigma)
        assert abs(s - law.m2 / 2.0) <= 4.0 * square_sigma, (name, s, law.m2 / 2.0, square_sigma)
    r = correlation(du, de)
    print(f"  corr(u, e) {r:.3e} (bound {4.0 / math.sqrt(N):.2e})")
    assert abs(r) <= 4.0 / math.sqrt(N), r
    return theta


def correlation(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / (a * a).sum().sqrt() / (b * b).sum().sqrt())
