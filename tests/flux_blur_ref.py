"""The blur of ``art_flux_crop_fwd``'s blur mode (``artist_amd.flux.blur_flux``) in numpy: the definition of include/artist_hip.h
restated, in fp64 by default.  TEST INFRASTRUCTURE - not part of the product.

``dtype=np.float32`` evaluates the same formulas with every weight, fraction, product and sum in fp32 (the radii and the validity
of a covariance are decided in fp64 from the covariance's values in both): its distance from the fp64 evaluation is the yardstick
of the GPU tests - what rounding alone does to this operator on these inputs."""
from __future__ import annotations

import math

import numpy as np

MIN_VARIANCE = 1e-4
MAX_RADIUS = 64
PSD_SLACK = 1e-5


def plan(covariance):
    """``(Kr, s, a, Ka)`` of a covariance ``(S_rr, S_rc, S_cc)``, or None for one whose bitmap is NaN: not finite, not positive
    semi-definite, or wider than the operator's window."""
    s_rr, s_rc, s_cc = (float(v) for v in covariance)
    if not all(math.isfinite(v) for v in (s_rr, s_rc, s_cc)):
        return None
    if s_rr < 0.0 or s_cc < 0.0 or s_rc * s_rc > s_rr * s_cc * (1.0 + PSD_SLACK):
        return None
    if s_rr > MAX_RADIUS ** 2 / 16.0 or s_cc > MAX_RADIUS ** 2 / 16.0:
        return None
    kr, s, a = 0, 0.0, s_cc
    if s_rr >= MIN_VARIANCE:
        kr = int(math.ceil(4.0 * math.sqrt(s_rr)))
        s = s_rc / s_rr
        a = s_cc - s_rc * s_rc / s_rr
    ka = int(math.ceil(4.0 * math.sqrt(a))) if a >= MIN_VARIANCE else 0
    if kr > MAX_RADIUS or ka > MAX_RADIUS:
        return None
    return kr, s, a, ka


def tap(v: float, K: int, dtype) -> np.ndarray:
    """Weights of the taps k = -K..K: exp(-k^2 / (2 v)) over their sum; the single tap 1 for K = 0."""
    if K == 0:
        return np.ones(1, dtype)
    k = np.arange(-K, K + 1).astype(dtype)
    w = np.exp(-(k * k) / (dtype(2.0) * dtype(v)))
    return (w / w.sum(dtype=dtype)).astype(dtype)


def blur_one(x: np.ndarray, covariance, dtype=np.float64) -> np.ndarray:
    """One bitmap ``x [Hh,W]`` under one covariance."""
    dtype = np.dtype(dtype).type
    Hh, W = x.shape
    p = plan(covariance)
    if p is None:
        return np.full((Hh, W), np.nan, dtype)
    kr, s, a, ka = p
    x = x.astype(dtype)
    g_a, g_r = tap(a, ka, dtype), tap(float(covariance[0]), kr, dtype)
    s = dtype(s)
    E = int(math.ceil(abs(float(s)) * kr)) + 2                  # how far beyond the image's edges the row pass reads y
    # column pass on the extended domain: columns -E .. W-1+E of y (rows beyond the image are zero: x is)
    xp = np.zeros((Hh, W + 2 * E + 2 * ka), dtype)
    xp[:, E + ka:E + ka + W] = x
    y = np.zeros((Hh, W + 2 * E), dtype)
    for t, k in enumerate(range(-ka, ka + 1)):                  # ascending k; y column j is image column j - E
        y += g_a[t] * xp[:, ka - k:ka - k + W + 2 * E]
    z = np.zeros((Hh, W), dtype)
    for t, k in enumerate(range(-kr, kr + 1)):
        pos = -s * dtype(k)
        o = math.floor(float(pos))
        f = dtype(pos - dtype(o))
        lo, hi = max(0, k), min(Hh, Hh + k)                     # output rows r with 0 <= r - k < Hh
        if lo >= hi:
            continue
        src = y[lo - k:hi - k]
        v0, v1 = src[:, E + o:E + o + W], src[:, E + o + 1:E + o + 1 + W]
        z[lo:hi] += g_r[t] * (v0 + f * (v1 - v0))
    return z


def blur(x: np.ndarray, covariance: np.ndarray, dtype=np.float64) -> np.ndarray:
    """``x [B,Hh,W]``, ``covariance [B,3]`` -> ``[B,Hh,W]``."""
    return np.stack([blur_one(x[b], covariance[b], dtype) for b in range(x.shape[0])])


def yardstick(x: np.ndarray, covariance: np.ndarray):
    """``(the fp64 result, per bitmap max |fp32 evaluation - fp64 evaluation|)``."""
    ref = blur(x, covariance, np.float64)
    low = blur(x, covariance, np.float32).astype(np.float64)
    return ref, np.abs(low - ref).reshape(x.shape[0], -1).max(axis=1)
