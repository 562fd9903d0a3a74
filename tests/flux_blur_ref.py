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


# ---- the kernel's launch decisions, restated (artist_amd/csrc/flux_blur_kernels.hip) -------------------------------------------
# The kernel cannot be asked which branch it took: ``tiling`` restates its plan from the same inputs, in the words of the kernel's
# own comments and constants, and tests/test_blur_shapes_host.py holds ``CASES`` to the full list of branches.
TILE_COLS = 64                      # a tile row is the wave
MIN_TILE_ROWS, MAX_TILE_ROWS = 8, 256
WAVES = 16
ROWS_PER_WAVE = 8                   # consecutive output rows per wave in a block of 128 tile rows
BLOCK_ROWS = WAVES * ROWS_PER_WAVE
ROUND = 2                           # rows of y per wave and round of the column pass
IMAGE_COLS = TILE_COLS + 4          # columns of a row of y in LDS
MAX_GROUPS = 65535

BRANCHES = frozenset({
    "tile_rows>1", "Hh<TR", "Hh==TR",
    "row_taps<=64", "row_taps<=128", "row_taps==129", "column_taps<=64", "column_taps<=128", "column_taps==129",
    "row_identity", "column_identity", "shear16", "shear10", "corner_tiles", "tiles>groups", "run>128", "clamped_block",
    "clamped_behind_full_block", "full_block_tap_blocks"})


def _taps_name(which: str, K: int) -> str:
    taps = 2 * K + 1                # three table segments of 64 taps: the third holds the single tap 128
    return f"{which}_taps<=64" if taps <= 64 else f"{which}_taps<=128" if taps <= 128 else f"{which}_taps==129"


def tiling(covariance, Hh: int, W: int):
    """The plan of ``flux_blur_kernel`` for one bitmap ``[Hh,W]`` under ``covariance``, or None for a bitmap that is NaN: ``Kr``,
    ``Ka``, ``s``, the tile height ``TR``, ``shear_bits``, ``lean`` (s rounded to them: the tiles' slope), ``smin``/``smax`` (the
    range of the lean ``sh(i)`` over a tile's rows), ``grid`` = (tile rows, tile columns), ``groups`` (the workgroups the launcher
    asks for), ``skipped`` (the tiles that are corners of the leaning grid), ``runs`` (per tile that is not skipped, the rows
    ``ia..iz`` that meet the image; (TR, 0) where none does) and ``branches``, a subset of ``BRANCHES``.
    ``full_block_tap_blocks`` is decided for an input without zeros."""
    covariance = tuple(float(np.float32(v)) for v in covariance)        # the kernel reads fp32 and decides in fp64
    p = plan(covariance)
    if p is None or abs(p[1]) > 4096.0:
        return None
    kr, s, _, ka = p
    TR = MIN_TILE_ROWS
    while TR < MAX_TILE_ROWS and TR < Hh:
        TR <<= 1
    bits = 16 if abs(s) <= 64.0 else 10
    sfix = int(round(s * (1 << bits)))          # llrint: half to even, as round()

    def sh(d):                                   # how far row r0 + d of a tile leans (an arithmetic shift: floor)
        return (sfix * d) >> bits

    last = sh(TR - 1)
    smin, smax = min(0, last), max(0, last)
    tiles_x = (W + (smax - smin) + TILE_COLS - 1) // TILE_COLS
    tiles_y = (Hh + TR - 1) // TR
    lean = min(Hh, MAX_TILE_ROWS) // 2
    groups = min(((Hh + MAX_TILE_ROWS - 1) // MAX_TILE_ROWS) * ((W + lean + TILE_COLS - 1) // TILE_COLS), MAX_GROUPS)
    rows_y, Wx = TR + 2 * kr, IMAGE_COLS + 2 * ka
    names = {_taps_name("row", kr), _taps_name("column", ka), "shear16" if bits == 16 else "shear10"}
    if kr == 0:
        names.add("row_identity")
    if ka == 0:
        names.add("column_identity")
    if tiles_y > 1:
        names.add("tile_rows>1")
    if Hh < TR:
        names.add("Hh<TR")
    if Hh == TR:
        names.add("Hh==TR")
    if tiles_x * tiles_y > groups:
        names.add("tiles>groups")
    skipped, runs = [], {}
    for tile in range(tiles_x * tiles_y):
        ty, tx = divmod(tile, tiles_x)
        r0, c0 = ty * TR, tx * TILE_COLS - smax
        rows = min(TR, Hh - r0)
        a0, a1 = c0 + sh(0), c0 + sh(rows - 1)
        if max(a0, a1) + TILE_COLS <= 0 or min(a0, a1) >= W:
            skipped.append((ty, tx))
            continue
        meets = [i for i in range(TR) if r0 + i < Hh and c0 + sh(i) + TILE_COLS > 0 and c0 + sh(i) < W]
        if not meets:               # a steep lean steps over a narrow image between two rows: the tile is walked and writes nothing
            runs[(ty, tx)] = (TR, 0)
            continue
        ia, iz = meets[0], meets[-1] + 1
        assert meets == list(range(ia, iz))              # the lean is monotone: one run
        runs[(ty, tx)] = (ia, iz)
        if iz - ia > BLOCK_ROWS:
            names.add("run>128")
        # the rows of y that hold anything when no input is zero, in whole rounds of the column pass
        live = [j // ROUND for j in range(rows_y)
                if 0 <= r0 + j - kr < Hh and c0 + sh(j - kr) - 2 - ka < W and c0 + sh(j - kr) - 2 - ka + Wx > 0]
        j_lo, j_hi = (ROUND * live[0], ROUND * (live[-1] + 1)) if live else (rows_y, 0)
        for ib in range(ia, iz, BLOCK_ROWS):
            for i0 in range(ib, min(ib + BLOCK_ROWS, iz), ROWS_PER_WAVE):
                if i0 + ROWS_PER_WAVE > iz:
                    names.add("clamped_block")
                    if ib > ia:
                        names.add("clamped_behind_full_block")
                    continue
                t_lo = max(0, i0 + 2 * kr - (j_hi - 1))
                t_hi = min(2 * kr, i0 + ROWS_PER_WAVE - 1 + 2 * kr - j_lo)
                for g in range(3):
                    if max(64 * g, t_lo) + ROWS_PER_WAVE <= min(64 * g + 64, t_hi + 1):
                        names.add("full_block_tap_blocks")
    if skipped:
        names.add("corner_tiles")
    assert names <= BRANCHES
    return dict(Kr=kr, Ka=ka, s=s, TR=TR, shear_bits=bits, lean=sfix / (1 << bits), smin=smin, smax=smax, grid=(tiles_y, tiles_x), groups=groups,
                skipped=skipped, runs=runs, branches=names)


# ---- the case table of the shape tests (tests/test_blur_shapes_host.py, tests/test_gpu_flux_blur_shapes.py) ----------------------
# Every covariance is exactly representable in fp32 wherever a threshold matters.
COVARIANCES = np.array([
    (0.64, 0.0, 0.64),              # 0: below one pixel
    (256.0, 0.0, 256.0),            # 1: THE limit, Kr = Ka = 64: 129 taps per pass, a third table segment of one tap
    (256.0, 200.0, 256.0),          # 2: the limit, sheared: Kr = 64, Ka = 40, s = 0.78
    (256.0, -200.0, 256.0),         # 3: ... s = -0.78
    (4.0, -5.0, 9.0),               # 4: s = -1.25
    (0.03125, 2.0, 160.0),          # 5: s = 64 exactly: the last 16-bit shear, 258 tile columns at W = 130
    (0.03125, 2.0078125, 160.0),    # 6: s = 64.25: the first 10-bit one
    (0.01, 0.9, 100.0),             # 7: s = 90
    (0.02, -1.4, 120.0),            # 8: s = -70
    (1e-5, 0.0, 1e-5),              # 9: both passes are the identity
    (256.0, 0.0, 1e-5),             # 10: the column pass is the identity
    (1e-5, 0.0, 256.0),             # 11: the row pass is the identity
    (100.0, 30.0, 100.0),           # 12: Kr = 40, Ka = 39: both passes end in the second table segment
], np.float32)
SHAPES = [(1, 1), (1, 130), (7, 3), (8, 64), (9, 65), (129, 70), (257, 66), (300, 130), (513, 40)]
INPUTS = ("dense", "seams", "bands")
CASES = [(shape, name) for shape in SHAPES for name in INPUTS]           # every covariance is the batch of every case
# (covariance, shape) -> the branches its comment above claims (held by tests/test_blur_shapes_host.py)
CLAIMS = [
    (1, (300, 130), {"row_taps==129", "column_taps==129", "tile_rows>1", "run>128", "full_block_tap_blocks"}),
    (2, (257, 66), {"row_taps==129", "column_taps<=128", "shear16", "tile_rows>1", "clamped_block"}),
    (3, (257, 66), {"row_taps==129", "column_taps<=128", "shear16", "tile_rows>1", "clamped_block"}),
    (4, (9, 65), {"row_taps<=64", "column_taps<=64", "Hh<TR"}),
    (5, (300, 130), {"shear16", "corner_tiles", "tiles>groups", "tile_rows>1"}),
    (6, (300, 130), {"shear10", "corner_tiles", "tiles>groups"}),
    (7, (257, 66), {"shear10", "corner_tiles", "tiles>groups"}),
    (8, (513, 40), {"shear10", "corner_tiles", "tiles>groups", "tile_rows>1"}),
    (9, (8, 64), {"row_identity", "column_identity", "Hh==TR"}),
    (10, (129, 70), {"column_identity", "row_taps==129", "run>128", "clamped_behind_full_block"}),
    (11, (129, 70), {"row_identity", "column_taps==129", "run>128", "clamped_behind_full_block"}),
    (0, (1, 1), {"Hh<TR", "clamped_block", "row_taps<=64", "column_taps<=64"}),
    (1, (7, 3), {"Hh<TR", "clamped_block", "row_taps==129"}),
    (12, (300, 130), {"row_taps<=128", "column_taps<=128", "shear16", "full_block_tap_blocks"}),
]
SEAM_ROWS, SEAM_COLS = (0, 127, 128, 255, 256), (0, 63, 64)


def case_input(shape, name: str) -> np.ndarray:
    """The fp32 input ``[Hh,W]`` of a case: ``dense`` a seeded standard normal (signed: the backward pass feeds the operator
    gradients); ``seams`` single pixels of distinct values on the rows and columns where tiles, blocks of rows and the image end;
    ``bands`` zero but for three rows from ``Hh // 3`` and the right half of the last row (the rounds of zeros that the column
    pass skips, and the window of taps that the row pass walks)."""
    Hh, W = shape
    rng = np.random.default_rng(1000 * Hh + W)
    if name == "dense":
        return rng.standard_normal((Hh, W)).astype(np.float32)
    x = np.zeros((Hh, W), np.float32)
    if name == "seams":
        rows = sorted({r for r in SEAM_ROWS + (Hh - 1,) if r < Hh})
        cols = sorted({c for c in SEAM_COLS + (W - 1,) if c < W})
        for i, r in enumerate(rows):
            for j, c in enumerate(cols):
                x[r, c] = (1.0 + 0.25 * i + 0.0625 * j) * (-1.0 if (i + j) % 3 == 2 else 1.0)
        return x
    if name == "bands":
        x[Hh // 3:Hh // 3 + 3] = rng.standard_normal(x[Hh // 3:Hh // 3 + 3].shape).astype(np.float32)
        x[Hh - 1, W // 2:] = rng.standard_normal(W - W // 2).astype(np.float32)
        return x
    raise KeyError(name)
