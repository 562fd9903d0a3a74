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


# ---- the kernel's launch decisions, restated (artist_amd/csrc/radial_blur_kernels.hip) -----------------------------------------
# The kernel cannot be asked which branch it took: ``tiling`` restates its plan from the same inputs, in the words of the kernel's
# own comments and constants, and tests/test_blur_shapes_host.py holds the case table below to the full list of branches.
WAVES = 16
COLS_PER_LANE = 8
LDS_FLOATS = 38912                  # table, half stencil, tile
TABLE_CHUNK = 1024                  # table entries per round of the k* count
TILE_SHAPES = [(2, 8, 64), (1, 8, 64), (1, 4, 64), (1, 2, 64), (1, 1, 64), (1, 1, 32)]          # (WR, WC, RW)
MAX_GROUPS = 65535
GROUP_BUDGET = 2048                 # workgroups of a launch, shared by its bitmaps

BRANCHES = frozenset({f"shape{shape}" for shape in TILE_SHAPES} | {
    "Rr==64", "Rc==64", "table_chunks>1", "kstar<K", "ragged_rows", "ragged_cols", "tiles>groups", "share<tiles"})


def tile_stride(cols: int) -> int:
    """Floats per tile row of ``cols`` columns: four more, then up to the next 4 (mod 8)."""
    s = cols + 4
    return s + ((12 - (s & 7)) & 7)


def tiling(metric, t2, Hh: int, W: int, B: int, x=None):
    """The plan of ``flux_radial_blur_kernel`` for one bitmap ``[Hh,W]`` of a batch of ``B``, or None for a bitmap that is NaN:
    ``kstar``, ``Rr``, ``Rc``, ``shape`` = (WR, WC, RW) by the kernel's LDS budget, ``grid`` = (tile rows, tile columns),
    ``share`` = ceil(2048 / B), ``launch_tiles`` (the bitmap's tiles at the largest shape, what the launcher counts), ``groups``
    (workgroups per bitmap), ``row64_taps`` (the non-zero taps of stencil row 64, the one that is read from LDS), ``table_chunks``
    and ``branches``, a subset of ``BRANCHES``.  With the bitmap ``x`` also ``zero_tiles`` (the tiles whose inputs are all zero
    under their halo), ``zero_ragged_tiles`` (those of them that the image cuts) and ``late_stencil`` (some workgroup meets a
    zero tile before its first tile that is not: it builds its stencil late)."""
    k = k_star(metric, t2)
    if k is None:
        return None
    m_rr, _, m_cc = (float(np.float32(v)) for v in metric)
    table = np.asarray(t2, np.float32).astype(np.float64)
    K = len(table) - 1
    T = float(table[k])
    Rr = min(MAX_RADIUS, int(math.floor(math.sqrt(T * m_rr) + 0.375)))
    Rc = min(MAX_RADIUS, int(math.floor(math.sqrt(T * m_cc) + 0.375)))
    table_floats = (K + 1 + 3) & ~3
    stencil_floats = ((Rr + 1) * (2 * Rc + 1) + 3) & ~3
    halo = 2 * Rc + COLS_PER_LANE - 1
    room = LDS_FLOATS - table_floats - stencil_floats
    shape = TILE_SHAPES[-1]
    for WR, WC, RW in reversed(TILE_SHAPES):             # the first shape whose tile and halo fit
        if (WR * RW + 2 * Rr) * tile_stride(WC * COLS_PER_LANE + halo) <= room:
            shape = (WR, WC, RW)
    WR, WC, RW = shape
    TR, TC = WR * RW, WC * COLS_PER_LANE
    tiles_y, tiles_x = (Hh + TR - 1) // TR, (W + TC - 1) // TC
    tiles = tiles_y * tiles_x
    launch_tiles = ((Hh + 127) // 128) * ((W + 63) // 64)
    share = (GROUP_BUDGET + B - 1) // B
    groups = min(launch_tiles, share, MAX_GROUPS)
    row64 = int(np.count_nonzero(stencil(metric, t2)[2 * MAX_RADIUS])) if Rr == MAX_RADIUS else 0
    chunks = K // TABLE_CHUNK + 1                       # rounds of `for (base = 0; base <= K; base += 1024)`
    names = {f"shape{shape}"}
    for name, holds in (("Rr==64", Rr == MAX_RADIUS), ("Rc==64", Rc == MAX_RADIUS), ("table_chunks>1", chunks > 1),
                        ("kstar<K", k < K), ("ragged_rows", Hh % TR != 0), ("ragged_cols", W % TC != 0),
                        ("tiles>groups", tiles > groups), ("share<tiles", share < launch_tiles)):
        if holds:
            names.add(name)
    assert names <= BRANCHES
    out = dict(kstar=k, Rr=Rr, Rc=Rc, shape=shape, grid=(tiles_y, tiles_x), share=share, launch_tiles=launch_tiles, groups=groups,
               row64_taps=row64, table_chunks=chunks, branches=names)
    if x is not None:
        x = np.asarray(x)
        zero = []
        for t in range(tiles):
            r0, c0 = (t // tiles_x) * TR, (t % tiles_x) * TC
            under = x[max(0, r0 - Rr):min(Hh, r0 + TR + Rr), max(0, c0 - Rc - (COLS_PER_LANE - 1)):min(W, c0 + TC + Rc)]
            zero.append(not np.any(under != 0))           # (a NaN is non-zero)
        out["zero_tiles"] = [divmod(t, tiles_x) for t in range(tiles) if zero[t]]
        out["zero_ragged_tiles"] = [(ty, tx) for ty, tx in out["zero_tiles"] if (ty + 1) * TR > Hh or (tx + 1) * TC > W]
        late = False
        for g in range(groups):
            walk = [zero[t] for t in range(g, tiles, groups)]
            late |= (False in walk) and walk[0]
        out["late_stencil"] = late
    return out


# ---- the case table of the shape tests (tests/test_blur_shapes_host.py, tests/test_gpu_radial_blur_shapes.py) --------------------
def disc(radius_px: float) -> float:
    """The metric entry at which the pillbox's edge lies ``radius_px`` pixels out."""
    from artist_amd import scene
    return (radius_px / scene.SOLAR_DISC_HALF_ANGLE) ** 2


def _uniform_disc(K: int) -> np.ndarray:
    from artist_amd import scene
    return (np.arange(K + 1, dtype=np.float64) / K * float(np.float32(scene.SOLAR_DISC_HALF_ANGLE)) ** 2).astype(np.float32)


_TABLES: dict = {}


def tables() -> dict:
    """name -> (table [K+1] fp32, metrics [n,3] fp32, per metric the branches its line claims at ``CLAIM_SHAPE`` with the table's
    metrics as the batch).  Built on first use (the solar disc's half angle and the Buie table are the package's own)."""
    if _TABLES:
        return _TABLES
    from artist_amd import scene
    theta = scene.SOLAR_DISC_HALF_ANGLE
    d = disc
    wide, narrow = d(63.8), d(20.0)
    cross = 0.99 * math.sqrt(wide * narrow)
    pillbox = np.array([0.0, np.float32(theta) ** 2], np.float32)
    pillbox_metrics = np.array([
        (d(5.0), 0.0, d(5.0)),              # 0: shape (2,8,64)
        (d(50.0), 0.0, d(50.0)),            # 1: shape (1,8,64)
        (d(60.0), 0.0, d(60.0)),            # 2: shape (1,4,64)
        (d(63.8), 0.0, d(63.8)),            # 3: shape (1,2,64), Rr = Rc = 64, 11 non-zero taps in stencil row 64
        (wide, cross, narrow),              # 4: Rr = 64, Rc = 20
        (narrow, -cross, wide),             # 5: Rr = 20, Rc = 64
    ], np.float32)
    pillbox_claims = [{"shape(2, 8, 64)"}, {"shape(1, 8, 64)"}, {"shape(1, 4, 64)"}, {"shape(1, 2, 64)", "Rr==64", "Rc==64"},
                      {"Rr==64"}, {"Rc==64"}]
    buie = scene.Sun(4, dict(distribution_type="buie")).quantile_table.numpy().astype(np.float32)
    _TABLES.update({
        "pillbox": (pillbox, pillbox_metrics, pillbox_claims),
        # a uniform disc in K annuli of equal area: the table alone fills LDS
        "uniform1024": (_uniform_disc(1024), np.array([(d(63.8), 0.0, d(63.8))], np.float32),
                        [{"shape(1, 1, 64)", "Rr==64", "Rc==64", "table_chunks>1"}]),
        # ... of which 64 px hold k* = 2621 nodes of 4096: five table chunks, the wave's upper half repeats row 31
        "uniform4096": (_uniform_disc(4096), np.array([(d(80.0), 0.0, d(80.0))], np.float32),
                        [{"shape(1, 1, 32)", "Rr==64", "Rc==64", "table_chunks>1", "kstar<K"}]),
        # the K = 1024 Buie table at the metric of tests/test_gpu_radial_blur.py's bench-size case
        "buie": (buie, np.array([(2.7213e7, 1.2391e7, 4.0957e7)], np.float32), [{"table_chunks>1", "kstar<K"}]),
    })
    for entry in _TABLES.values():
        for a in entry[:2]:
            a.setflags(write=False)
    return _TABLES


SHAPES = [(1, 1), (5, 3), (33, 9), (65, 17), (130, 70)]
SPOT_SHAPE = (200, 150)             # with the `spot` input and the first two pillbox metrics only
INPUTS = ("dense", "seams")
CLAIM_SHAPE = (130, 70)
CASES = [(table, shape, name) for table in ("pillbox", "uniform1024", "uniform4096", "buie") for shape in SHAPES for name in INPUTS]
# same bits whatever the batch: (table, shape, batch sizes).  At (40, 20) the launcher counts one tile and one workgroup serves
# the bitmap at every B; at (130, 70) it counts four, and B = 1025 and B = 2049 cut the grid to `share` = 2 and 1.
BATCH_CASES = [("uniform4096", (40, 20), (1, 1025, 2049)), ("uniform4096", (130, 70), (1, 1025, 2049))]
SEAM_ROWS, SEAM_COLS = (31, 32, 63, 64, 127, 128), (7, 8, 63, 64)


def case_input(shape, name: str) -> np.ndarray:
    """The fp32 input ``[Hh,W]`` of a case: ``dense`` a seeded standard normal (signed: the backward pass feeds the operator
    gradients); ``seams`` the four corners and single pixels of distinct values on both sides of the rows and columns where
    tiles of any shape end; ``spot`` zero but for ``x[190:193, 140:142]``."""
    Hh, W = shape
    rng = np.random.default_rng(1000 * Hh + W + 7)
    if name == "dense":
        return rng.standard_normal((Hh, W)).astype(np.float32)
    x = np.zeros((Hh, W), np.float32)
    if name == "seams":
        rows = sorted({r for r in (0, Hh - 1) + SEAM_ROWS if r < Hh})
        cols = sorted({c for c in (0, W - 1) + SEAM_COLS if c < W})
        for i, r in enumerate(rows):
            for j, c in enumerate(cols):
                if r in (0, Hh - 1) and c in (0, W - 1) or r in SEAM_ROWS and c in SEAM_COLS:
                    x[r, c] = (1.0 + 0.25 * i + 0.0625 * j) * (-1.0 if (i + j) % 3 == 2 else 1.0)
        return x
    if name == "spot":
        x[190:193, 140:142] = rng.random((3, 2), dtype=np.float32) + 0.5
        return x
    raise KeyError(name)
