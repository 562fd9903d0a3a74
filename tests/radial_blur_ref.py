"""The radial window of ``art_flux_crop_fwd`` (``artist_amd.flux.radial_blur_flux``) in numpy: the definition of
include/artist_hip.h restated, in fp64 by default.  TEST INFRASTRUCTURE - not part of the product.

The stencil is formed in fp64 in both evaluations.  ``dtype=np.float32`` rounds the weights to fp32 once and convolves with every
product and sum in fp32; its distance from the fp64 evaluation (fp64 weights, fp64 sums) is the yardstick of the GPU tests - what
rounding alone does to this operator on these inputs.  ``sample`` is the table rule of ``RadialSunShape.transform_``."""
from __future__ import annotations

import math

import numpy as np

MAX_RADIUS = 64
MIN_DET = 1e-6
SUB = (np.arange(4) * 2 - 3) / 8.0          # the 4 x 4 sub-lattice: -3/8, -1/8, 1/8, 3/8


def table_ok(t2) -> bool:
    t2 = np.asarray(t2, np.float64)
    return bool(np.isfinite(t2).all() and t2[0] >= 0.0 and (np.diff(t2) >= 0.0).all())


def k_star(metric, t2):
    """The largest node whose two half extents are both <= 64 pixels, or None where the bitmap is NaN."""
    m_rr, m_rc, m_cc = (float(np.float32(v)) for v in metric)
    t2 = np.asarray(t2, np.float32).astype(np.float64)
    if not table_ok(t2) or not all(math.isfinite(v) for v in (m_rr, m_rc, m_cc)):
        return None
    if m_rr <= 0.0 or m_cc <= 0.0 or not (m_rr * m_cc - m_rc * m_rc > MIN_DET * (m_rr * m_cc)):
        return None
    fits = (t2 * m_rr <= MAX_RADIUS ** 2) & (t2 * m_cc <= MAX_RADIUS ** 2)        # = sqrt(t2[k] M) <= 64, exact in fp64
    k = int(fits.sum()) - 1
    return k if k >= 1 else None


def kept_fraction(metric, t2) -> float:
    k = k_star(metric, t2)
    return float("nan") if k is None else k / (len(t2) - 1)


def stencil(metric, t2):
    """``w [129,129]`` in fp64, ``w[64 + dr, 64 + dc]``, or None where the bitmap is NaN."""
    k = k_star(metric, t2)
    if k is None:
        return None
    m_rr, m_rc, m_cc = (float(np.float32(v)) for v in metric)
    t2 = np.asarray(t2, np.float32).astype(np.float64)
    K = len(t2) - 1
    det = m_rr * m_cc - m_rc * m_rc
    taps = np.arange(-MAX_RADIUS, MAX_RADIUS + 1, dtype=np.float64)
    raw = np.zeros((taps.size, taps.size))
    nodes = t2[:k + 1]
    width = np.diff(nodes)

    def density(i, j):
        pr, pc = (taps + SUB[i])[:, None], (taps + SUB[j])[None, :]
        q = (m_cc * pr * pr - 2.0 * m_rc * pr * pc + m_rr * pc * pc) / det
        node = np.searchsorted(nodes, q, side="right") - 1              # the largest node with t2[node] <= q
        inside = (node >= 0) & (node < k)
        w = width[np.clip(node, 0, k - 1)]
        return np.where(inside & (w > 0), 1.0 / np.where(w > 0, w, 1.0), 0.0)

    for i in range(2):          # eight pairs of opposite points: the mirrored tap sums the same pairs in the same order
        for j in range(4):
            raw += density(i, j) + density(3 - i, 3 - j)
    raw /= 16.0
    total = raw.sum()
    if total == 0.0:            # far below a pixel, or a table of zeros: one tap
        w = np.zeros_like(raw)
        w[MAX_RADIUS, MAX_RADIUS] = k / K
        return w
    return raw * (k / K) / total


def convolve(x: np.ndarray, w: np.ndarray, dtype) -> np.ndarray:
    """z[r, c] = sum over dr, then dc, ascending, of the non-zero taps w[dr, dc] x[r - dr, c - dc]; x zero outside the image."""
    dtype = np.dtype(dtype).type
    Hh, W = x.shape
    x = x.astype(dtype)
    w = w.astype(dtype)
    z = np.zeros((Hh, W), dtype)
    R = MAX_RADIUS
    for a, b in zip(*np.nonzero(w)):
        dr, dc = int(a) - R, int(b) - R
        r_lo, r_hi = max(0, dr), min(Hh, Hh + dr)
        c_lo, c_hi = max(0, dc), min(W, W + dc)
        if r_lo < r_hi and c_lo < c_hi:
            z[r_lo:r_hi, c_lo:c_hi] += w[a, b] * x[r_lo - dr:r_hi - dr, c_lo - dc:c_hi - dc]
    return z


def blur_one(x: np.ndarray, metric, t2, dtype=np.float64) -> np.ndarray:
    w = stencil(metric, t2)
    if w is None:
        return np.full(x.shape, np.nan, np.dtype(dtype).type)
    return convolve(x, w, dtype)


def blur(x: np.ndarray, metric: np.ndarray, t2, dtype=np.float64) -> np.ndarray:
    """``x [B,Hh,W]``, ``metric [B,3]``, ``t2 [K+1]`` -> ``[B,Hh,W]``."""
    return np.stack([blur_one(x[b], metric[b], t2, dtype) for b in range(x.shape[0])])


def yardstick(x: np.ndarray, metric: np.ndarray, t2):
    """``(the fp64 result, per bitmap max |fp32 evaluation - fp64 evaluation|)`` (0 for a bitmap that is NaN in both)."""
    ref = blur(x, metric, t2, np.float64)
    low = blur(x, metric, t2, np.float32).astype(np.float64)
    gap = np.abs(low - ref).reshape(x.shape[0], -1)
    return ref, np.where(np.isnan(gap), 0.0, gap).max(axis=1)


POSITIONS = [(5.0, 60.0, 2.0), (70.0, 50.0, 2.0), (-90.0, 140.0, 2.0)]          # slant ranges of 80, 101 and 175 m


def acceptance_geometry(side: int = 100):
    """The geometry of the acceptance tests (that of tests/test_gpu_sun_convolution.py) as fp32 torch tensors on the CPU: three
    flat mirrors of 3.2 m x 2.5 m, ``side`` x ``side`` points each, whose point p aims at centre + 0.3 (p - position), one 8 m x
    8 m target.  ``dict(points, normals, incident, targets, tables=(centers, plane normals, dimensions))``."""
    import torch
    f64 = torch.float64
    position = torch.tensor(POSITIONS, dtype=f64)
    e, n = torch.meshgrid(torch.linspace(-1.6, 1.6, side, dtype=f64), torch.linspace(-1.25, 1.25, side, dtype=f64), indexing="ij")
    offsets = torch.stack((e.reshape(-1), n.reshape(-1), torch.zeros(side * side, dtype=f64)), dim=-1)
    points = position[:, None, :] + offsets[None]
    centre = torch.tensor([0.0, 0.0, 55.0], dtype=f64)
    incident = torch.nn.functional.normalize(torch.tensor([0.2, 0.5, -0.8], dtype=f64), dim=0)
    aim = centre + 0.3 * offsets[None].expand_as(points)
    normals = torch.nn.functional.normalize(torch.nn.functional.normalize(aim - points, dim=-1) - incident, dim=-1)
    H, P = points.shape[:2]
    return dict(points=torch.cat((points, torch.ones(H, P, 1, dtype=f64)), dim=-1).float(),
                normals=torch.cat((normals, torch.zeros(H, P, 1, dtype=f64)), dim=-1).float(),
                incident=torch.cat((incident, torch.zeros(1, dtype=f64))).float().repeat(H, 1),
                targets=torch.zeros(H, dtype=torch.long),
                tables=(torch.tensor([[0.0, 0.0, 55.0, 1.0]]), torch.tensor([[0.0, 1.0, 0.0, 0.0]]), torch.tensor([[8.0, 8.0]])))


def sample(t2, n: int, rng: np.random.Generator) -> np.ndarray:
    """``[n,2]`` draws ``(u, e)`` by the table rule: a uniform quantile picks theta^2 between two nodes, a uniform azimuth turns."""
    t2 = np.asarray(t2, np.float64)
    K = len(t2) - 1
    t = rng.random(n) * K
    i = np.minimum(t.astype(np.int64), K - 1)
    theta = np.sqrt(t2[i] + (t - i) * (t2[i + 1] - t2[i]))
    phi = rng.random(n) * (2.0 * math.pi)
    return np.stack((theta * np.cos(phi), theta * np.sin(phi)), axis=-1)
