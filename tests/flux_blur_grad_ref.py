"""The gradient of the blur with respect to its covariance - the blur mode of ``art_flux_crop_bwd``
(``artist_amd.flux.differentiable_blur_flux``) - in numpy: the definition of include/artist_hip.h restated, in fp64 by default.
TEST INFRASTRUCTURE - not part of the product.

For one bitmap ``L = sum g z``, ``z = flux_blur_ref.blur_one(x, S)`` with the radii held fixed.  ``dtype=np.float32`` evaluates the
tap products and the per-pixel sums in fp32 (weights ``w`` as ``flux_blur_ref.tap`` forms them in that dtype, ``w'`` rounded from
fp64; the sums over pixels and the chain rule in fp64 either way, as the kernel has them): its distance from the fp64 evaluation
is the yardstick of the GPU tests."""
from __future__ import annotations

import math

import numpy as np

import flux_blur_ref as ref


def derivative_tap(u: float, K: int, dtype) -> np.ndarray:
    """``w'_k = w_k (k^2 - m2) / (2 u^2)``, ``m2 = sum_j w_j j^2``, k = -K..K: the derivative of ``flux_blur_ref.tap`` with respect
    to the variance at a fixed radius, formed in fp64; the single 0 for an identity pass."""
    if K == 0:
        return np.zeros(1, dtype)
    k = np.arange(-K, K + 1).astype(np.float64)
    w = ref.tap(u, K, np.float64)
    m2 = (w * k * k).sum()
    return (w * (k * k - m2) / (2.0 * u * u)).astype(dtype)


def partials(x: np.ndarray, covariance, dtype=np.float64):
    """``(p_v, p_s, p_a)``, each ``[Hh,W]``: per pixel the derivative of ``z`` with respect to ``v = S_rr``, ``s = S_rc / S_rr`` and
    ``a = S_cc - S_rc^2 / S_rr``; None for a covariance whose bitmap is NaN."""
    dtype = np.dtype(dtype).type
    Hh, W = x.shape
    p = ref.plan(covariance)
    if p is None:
        return None
    kr, s, a, ka = p
    x = x.astype(dtype)
    v = float(covariance[0])
    w_a, d_a = ref.tap(a, ka, dtype), derivative_tap(a, ka, dtype)
    w_r, d_r = ref.tap(v, kr, dtype), derivative_tap(v, kr, dtype)
    s = dtype(s)
    E = int(math.ceil(abs(float(s)) * kr)) + 2
    xp = np.zeros((Hh, W + 2 * E + 2 * ka), dtype)
    xp[:, E + ka:E + ka + W] = x
    y = np.zeros((Hh, W + 2 * E), dtype)
    yd = np.zeros((Hh, W + 2 * E), dtype)
    for t, k in enumerate(range(-ka, ka + 1)):                  # ascending k, as the forward
        y += w_a[t] * xp[:, ka - k:ka - k + W + 2 * E]
        yd += d_a[t] * xp[:, ka - k:ka - k + W + 2 * E]
    p_v, p_s, p_a = (np.zeros((Hh, W), dtype) for _ in range(3))
    for t, k in enumerate(range(-kr, kr + 1)):
        pos = -s * dtype(k)
        o = math.floor(float(pos))
        f = dtype(pos - dtype(o))
        lo, hi = max(0, k), min(Hh, Hh + k)
        if lo >= hi:
            continue
        cut = lambda image, shift: image[lo - k:hi - k, E + o + shift:E + o + shift + W]  # noqa: E731
        v0, v1, u0, u1 = cut(y, 0), cut(y, 1), cut(yd, 0), cut(yd, 1)
        p_v[lo:hi] += d_r[t] * (v0 + f * (v1 - v0))
        p_a[lo:hi] += w_r[t] * (u0 + f * (u1 - u0))
        slope = (v1 - v0) if f != 0 else dtype(0.5) * (v1 - cut(y, -1))      # f == 0: the mean of the two one-sided slopes
        p_s[lo:hi] += (w_r[t] * dtype(-k)) * slope
    return p_v, p_s, p_a


def chain(D_v, D_s, D_a, covariance):
    """``(d/dS_rr, d/dS_rc, d/dS_cc)`` from the derivatives with respect to ``(v, s, a)`` (numbers or images), in fp64."""
    v = float(covariance[0])
    if v < ref.MIN_VARIANCE:                    # the row pass is the identity: a = S_cc
        return np.stack((np.zeros_like(D_a), np.zeros_like(D_a), D_a))
    s = float(covariance[1]) / v
    return np.stack((D_v - (s / v) * D_s + s * s * D_a, D_s / v - 2.0 * s * D_a, D_a))


def covariance_gradient(x: np.ndarray, g: np.ndarray, covariance, dtype=np.float64) -> np.ndarray:
    """``[3]`` (fp64) = ``dL/d(S_rr, S_rc, S_cc)`` of one bitmap ``x [Hh,W]`` under the upstream gradient ``g [Hh,W]``; NaN for a
    covariance whose bitmap the forward marks NaN."""
    dtype = np.dtype(dtype).type
    parts = partials(x, covariance, dtype)
    if parts is None:
        return np.full(3, np.nan)
    g = g.astype(dtype)
    D = [(g * part).astype(np.float64).sum() for part in parts]              # products in dtype, sums over pixels in fp64
    return chain(np.float64(D[0]), np.float64(D[1]), np.float64(D[2]), covariance)


def magnitude(x: np.ndarray, g: np.ndarray, covariance) -> np.ndarray:
    """``[3]``: ``sum |g| |dz/dS_i|`` in fp64 - the scale of the sum that ``covariance_gradient`` is."""
    parts = partials(x, covariance, np.float64)
    if parts is None:
        return np.full(3, np.nan)
    dz = chain(*parts, covariance)
    return (np.abs(g.astype(np.float64))[None] * np.abs(dz)).reshape(3, -1).sum(axis=1)


def yardstick(x: np.ndarray, g: np.ndarray, covariance: np.ndarray):
    """For a batch ``x, g [B,Hh,W]``, ``covariance [B,3]``: ``(the fp64 gradients [B,3], the bound [B,3])`` with the bound
    ``max(4 |fp32 evaluation - fp64 evaluation|, 1e-6 sum |g| |dz/dS_i|)`` per component."""
    want = np.stack([covariance_gradient(x[b], g[b], covariance[b]) for b in range(x.shape[0])])
    low = np.stack([covariance_gradient(x[b], g[b], covariance[b], np.float32) for b in range(x.shape[0])])
    scale = np.stack([magnitude(x[b], g[b], covariance[b]) for b in range(x.shape[0])])
    return want, np.maximum(4.0 * np.abs(low - want), 1e-6 * scale)


def crossings(covariance, step) -> list:
    """Why a central difference over ``[S - step, S + step]`` (``step [3]``) is not valid for the fixed-radius derivative: the
    names of what the eight corners of the box do not share with the centre - a radius, or the integer part of a tap's ``s k``."""
    centre = ref.plan(covariance)
    found = set()
    for signs in np.ndindex(2, 2, 2):
        p = ref.plan(tuple(float(c) + (2 * sg - 1) * float(h) for c, sg, h in zip(covariance, signs, step)))
        if p is None or p[0] != centre[0] or p[3] != centre[3]:
            found.add("radius")
            continue
        for k in range(1, centre[0] + 1):
            if math.floor(p[1] * k) != math.floor(centre[1] * k) or math.floor(-p[1] * k) != math.floor(-centre[1] * k):
                found.add("integer s k")
    return sorted(found)


# ---- the kernel's launch decisions, restated (flux_blur_grad_kernel, artist_amd/csrc/flux_blur_kernels.hip) --------------------------
TILE_ROWS = 64                      # two images of y in LDS: a quarter of the forward's tile
ROWS_PER_WAVE = TILE_ROWS // ref.WAVES

BRANCHES = frozenset({
    "tile_rows>1", "tile_columns>1", "Hh<TR",
    "row_taps<=64", "row_taps<=128", "row_taps==129", "column_taps<=64", "column_taps<=128", "column_taps==129",
    "row_identity", "column_identity", "shear16", "shear10", "corner_tiles", "empty_run", "idle_waves", "clamped_rows",
    "whole_taps", "fraction_taps"})


def tiling(covariance, Hh: int, W: int):
    """The plan of ``flux_blur_grad_kernel`` for one bitmap, or None for one whose gradient is NaN: ``Kr``, ``Ka``, ``TR``, ``grid``
    = (tile rows, tile columns), ``skipped`` corner tiles, ``runs`` and ``branches`` - a subset of ``BRANCHES``."""
    covariance = tuple(float(np.float32(v)) for v in covariance)
    p = ref.plan(covariance)
    if p is None or abs(p[1]) > 4096.0:
        return None
    kr, s, _, ka = p
    TR = ref.MIN_TILE_ROWS
    while TR < TILE_ROWS and TR < Hh:
        TR <<= 1
    bits = 16 if abs(s) <= 64.0 else 10
    sfix = int(round(s * (1 << bits)))

    def sh(d):
        return (sfix * d) >> bits

    last = sh(TR - 1)
    smin, smax = min(0, last), max(0, last)
    tiles_x = (W + (smax - smin) + ref.TILE_COLS - 1) // ref.TILE_COLS
    tiles_y = (Hh + TR - 1) // TR
    names = {ref._taps_name("row", kr), ref._taps_name("column", ka), "shear16" if bits == 16 else "shear10"}
    if kr == 0:
        names.add("row_identity")
    if ka == 0:
        names.add("column_identity")
    if tiles_y > 1:
        names.add("tile_rows>1")
    if tiles_x > 1:
        names.add("tile_columns>1")
    if Hh < TR:
        names.add("Hh<TR")
    for k in range(-kr, kr + 1):
        pos = -s * k
        names.add("whole_taps" if pos == math.floor(pos) else "fraction_taps")
    skipped, runs = [], {}
    for tile in range(tiles_x * tiles_y):
        ty, tx = divmod(tile, tiles_x)
        r0, c0 = ty * TR, tx * ref.TILE_COLS - smax
        rows = min(TR, Hh - r0)
        a0, a1 = c0 + sh(0), c0 + sh(rows - 1)
        if max(a0, a1) + ref.TILE_COLS <= 0 or min(a0, a1) >= W:
            skipped.append((ty, tx))
            continue
        meets = [i for i in range(TR) if r0 + i < Hh and c0 + sh(i) + ref.TILE_COLS > 0 and c0 + sh(i) < W]
        if not meets:
            runs[(ty, tx)] = (TR, 0)
            names.add("empty_run")
            continue
        ia, iz = meets[0], meets[-1] + 1
        assert meets == list(range(ia, iz))
        runs[(ty, tx)] = (ia, iz)
        for wave in range(ref.WAVES):
            i0 = ia + ROWS_PER_WAVE * wave
            if i0 >= iz:
                names.add("idle_waves")
            elif i0 + ROWS_PER_WAVE > iz:
                names.add("clamped_rows")
    if skipped:
        names.add("corner_tiles")
    assert names <= BRANCHES
    return dict(Kr=kr, Ka=ka, s=s, TR=TR, shear_bits=bits, smin=smin, smax=smax, grid=(tiles_y, tiles_x), skipped=skipped, runs=runs,
                branches=names)


# ---- the case table of the GPU test (tests/test_gpu_flux_blur_grad.py; held to BRANCHES by tests/test_flux_blur_grad_host.py) -----
OPERATOR_COVARIANCES = [(0.64, 0.0, 0.64), (9.0, 3.0, 4.0), (4.0, -5.0, 9.0), (9.0, 6.0, 4.00001), (1e-5, 0.0, 6.0), (30.0, 0.0, 30.0)]
OPERATOR_SHAPE = (48, 40)
BATCH_SHAPES = [(1, 1), (7, 3), (9, 65), (129, 70), (257, 66), (300, 130)]          # each under flux_blur_ref.COVARIANCES as the batch
SPOT = ((118.86, 54.12, 178.89), (256, 256))
CASES = [(c, OPERATOR_SHAPE) for c in OPERATOR_COVARIANCES] + \
    [(tuple(float(v) for v in c), shape) for shape in BATCH_SHAPES for c in ref.COVARIANCES] + [SPOT]


def sparse_spot(rng, Hh: int = 48, W: int = 40) -> np.ndarray:
    """The sharp bitmap of the sigma recovery: a Gaussian spot under a sparse random mask (the mask drawn first)."""
    r, c = np.mgrid[:Hh, :W].astype(np.float64)
    mask = rng.random((Hh, W)) < 0.3
    return (np.exp(-((r - 22.0) ** 2 / 30.0 + (c - 18.0) ** 2 / 18.0)) * mask * rng.random((Hh, W))).astype(np.float32)


RECOVERY_METRIC = np.array([4e6, 1e6, 3e6])
RECOVERY = dict(truth=1.5e-3, start=0.8e-3, lr=5e-5, steps=80, bound=0.03)


def adam_recovery(loss_gradient) -> float:
    """Adam (default betas, eps 1e-8) on sigma alone for ``RECOVERY['steps']`` steps; ``loss_gradient(sigma) -> dL/dsigma``."""
    sigma, m, v = RECOVERY["start"], 0.0, 0.0
    for step in range(1, RECOVERY["steps"] + 1):
        grad = float(loss_gradient(sigma))
        m = 0.9 * m + 0.1 * grad
        v = 0.999 * v + 0.001 * grad * grad
        sigma -= RECOVERY["lr"] * (m / (1.0 - 0.9 ** step)) / (math.sqrt(v / (1.0 - 0.999 ** step)) + 1e-8)
    return sigma
