"""torch fp64 (CPU) restatement of the flux epilogue - the crop around the centre of mass (artist/flux/bitmap.py:121-246), PixelLoss
and KLDivergenceLoss with ``reduction_dimensions=(1, 2)`` (artist/optim/loss.py:251-410) and ``get_center_of_mass``
(bitmap.py:12-71) - written from the formulas with ``affine_grid`` / ``grid_sample`` and differentiated by autograd, plus the case
table and the input generator that tests/test_flux_reference_host.py and tests/test_gpu_flux_fuzz.py share.

The host test pins the C oracle's fp64 chain to this restatement; the GPU test then measures the HIP kernels against that chain.
Nothing here knows about the kernels except the NOTES of the case table, which say which path of
artist_amd/csrc/flux_kernels.hip a shape was chosen to reach."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
CROP_W, CROP_H = 6.0, 5.0          # metres; a case's target dimensions are (CROP_W / scale_x, CROP_H / scale_y)
KINK_PX = 1e-3                     # no in-frame sampling coordinate of a non-empty bitmap may be this close to an integer
_KINK_MARGIN_PX = 2e-3             # what the generator asks of the bitmaps it accepts

Case = collections.namedtuple("Case", "B Hh W scale_x scale_y note")

# flux_crop_bwd_tiled_kernel: tiles of 64 x 32 input pixels, at most four taps per axis, 64 staged rows
TILED_BACKWARD = [
    Case(3, 33, 65, 0.75, 0.62, "3 and 4 taps; a second tile column and row one pixel deep"),
    Case(3, 40, 70, 0.55, 0.9, "four taps on x at the most (a column turns wide below scale 0.502), three on y: tiled"),
    Case(3, 40, 70, 0.45, 0.9, "x wide, y not: per-pixel form, gather_rows<4> and <8>"),
    Case(3, 70, 40, 0.9, 0.52, "four taps on y; a tile's rows sample fewer than 64 output rows: tiled"),
    Case(3, 70, 40, 0.9, 0.505, "not wide, but a tile's rows sample 64 or more output rows: per-pixel form"),
    Case(3, 36, 68, 0.3, 0.3, "gather_rows<8>"),
    Case(3, 20, 24, 0.1, 0.15, "the general loop of the per-pixel form"),
    Case(3, 48, 64, 2.0, 2.0, "zoom-out: one or two taps per axis, weights down to 0"),
    Case(3, 9, 300, 1.0, 0.77, "scale exactly 1 on one axis, off-centre spot; the forward crop's second x-block"),
    Case(3, 5, 3, 0.8, 0.7, "W < 4: the horizontal pass without the 16-byte tap load"),
    Case(3, 2, 2, 0.6, 1.3, "W < 4, the smallest bitmap"),
    Case(3, 4, 2, 1.5, 0.75, "W < 4, zoom-out on x"),
]
# the centre-of-mass loops (1024 threads; four pixels per load when W % 4 == 0)
CENTRE_LOOPS = [
    Case(2, 3, 1025, 0.75, 0.8, "scalar loop, W > block size"),
    Case(2, 2, 4100, 0.75, 0.5, "W / 4 > block size"),
    Case(3, 7, 12, 0.7, 0.85, "W / 4 = 3 does not divide 1024"),
]
# art_flux_crop_pixel_loss_fwd: rows staged in LDS (one workgroup per bitmap, W divides 1024), parts, scratch slots
FUSED_FORWARD = [
    Case(3, 5, 4, 0.8, 0.75, "staged rows, the narrowest staged width"),
    Case(3, 16, 64, 0.75, 0.8, "staged rows"),
    Case(3, 64, 64, 2.0, 2.0, "staging refused per part: the part samples more rows than were staged"),
    Case(2, 128, 512, 0.75, 0.5, "73 728 B of dynamic LDS: the launch above 48 KB"),
    Case(2, 160, 512, 0.75, 0.75, "above 76 KB: no staging"),
    Case(2, 64, 1024, 0.5, 0.75, "above 76 KB: no staging, widest column owner"),
    Case(2, 56, 1024, 0.75, 0.625, "staged at the widest column-owner width"),
    Case(2, 33, 17, 0.8, 0.9, "no column owner; npix % 4 != 0"),
    Case(3, 60, 100, 0.75, 0.6, "no column owner"),
    Case(3, 2, 8, 0.8, 0.9, "Hh = 2: two of the four parts are empty"),
    Case(3, 3, 6, 0.9, 0.8, "Hh = 3: one empty part, no column owner"),
    Case(129, 8, 8, 0.75, 0.8, "one workgroup per bitmap by the CU rule (no knob)"),
    Case(512, 8, 8, 0.8, 0.75, "the last scratch slot when four workgroups share a bitmap"),
    Case(513, 8, 8, 0.75, 0.75, "more bitmaps than the part scratch holds"),
]
CASES = TILED_BACKWARD + CENTRE_LOOPS + FUSED_FORWARD
assert len(set(c[:5] for c in CASES)) == len(CASES)


def case_id(case):
    return f"{case.B}x{case.Hh}x{case.W}-sx{case.scale_x:g}-sy{case.scale_y:g}"


# ------------------------------------------------------------------------------------------------
# the operations, torch fp64
# ------------------------------------------------------------------------------------------------
def _t(a):
    return a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def crop_grid(flux, dims, crop_width=CROP_W, crop_height=CROP_H):
    """The sampling grid [B,Hh,W,2] of the crop of ``flux`` [B,Hh,W] (bitmap.py:165-232): normalised centre of mass ->
    affine_grid (align_corners=True) with the crop's share of the target area as the scale."""
    B, Hh, W = flux.shape
    normalized = flux / (flux.sum(dim=(1, 2), keepdim=True) + 1e-8)
    x_center = (torch.linspace(-1, 1, W, dtype=F64)[None, None, :] * normalized).sum(dim=(1, 2))
    y_center = (torch.linspace(-1, 1, Hh, dtype=F64)[None, :, None] * normalized).sum(dim=(1, 2))
    theta = torch.zeros((B, 2, 3), dtype=F64)
    theta[:, 0, 0] = crop_width / dims[:, 0].clamp_min(1e-8)
    theta[:, 1, 1] = crop_height / dims[:, 1].clamp_min(1e-8)
    theta[:, 0, 2] = x_center
    theta[:, 1, 2] = y_center
    return F.affine_grid(theta, (B, 1, Hh, W), align_corners=True)


def crop(flux, dims, crop_width=CROP_W, crop_height=CROP_H):
    grid = crop_grid(flux, dims, crop_width, crop_height)
    return F.grid_sample(flux[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[:, 0]


def pixel_loss(prediction, truth):
    """loss.py:312-318 with reduction_dimensions=(1, 2)."""
    return ((prediction - truth) ** 2).sum(dim=(1, 2)) / truth.sum(dim=(1, 2))


def kl_loss(prediction, truth, eps=1e-12):
    """loss.py:385-410: both bitmaps L1-normalised (clamped norm), KL(truth || prediction) of log(. + eps), summed per sample."""
    p = prediction / prediction.abs().sum(dim=(1, 2), keepdim=True).clamp_min(eps)
    g = truth / truth.abs().sum(dim=(1, 2), keepdim=True).clamp_min(eps)
    t, q = torch.log(g + eps), torch.log(p + eps)
    return (torch.exp(t) * (t - q)).sum(dim=(1, 2))


def center_of_mass(bitmaps):
    """bitmap.py:46-71: [B,2] = (e pixel, u pixel)."""
    B, Hh, W = bitmaps.shape
    normalized = bitmaps / (bitmaps.sum(dim=(1, 2), keepdim=True) + 1e-8)
    e = (torch.arange(W, dtype=F64)[None, None, :] * normalized).sum(dim=(1, 2))
    u = (torch.arange(Hh, dtype=F64)[None, :, None] * normalized).sum(dim=(1, 2))
    return torch.stack((e, u), dim=1)


def integer_distance(flux, dims, crop_width=CROP_W, crop_height=CROP_H):
    """[B] = the smallest distance, in pixels, of an in-frame sampling coordinate of each bitmap's crop from an integer (the
    crop's gradient through the centre of mass jumps there).  In frame: a coordinate in [-1, n], whose two taps touch the
    bitmap.  The map is separable, so the first row's x and the first column's y are all there is."""
    flux, dims = _t(flux), _t(dims)
    B, Hh, W = flux.shape
    grid = crop_grid(flux, dims, crop_width, crop_height)
    out = torch.full((B,), float("inf"), dtype=F64)
    for coords, n in ((grid[:, 0, :, 0], W), (grid[:, :, 0, 1], Hh)):
        px = (coords + 1) / 2 * (n - 1)
        dist = (px - torch.round(px)).abs()
        dist = torch.where((px >= -1) & (px <= n), dist, torch.full_like(dist, float("inf")))
        out = torch.minimum(out, dist.min(dim=1).values)
    return out.numpy()


def reference(inp):
    """Everything the tests compare, from the inputs of ``make_inputs`` in fp64, gradients by autograd (numpy arrays):
    crop, crop_grad (of sum(crop * grad_out)), pixel / kl (per-sample loss of the crop against truth), pixel_grad / kl_grad (of
    sum(w * loss) w.r.t. the bitmaps, through the crop) and pixel_sum_grad / kl_sum_grad (of sum(loss)), com, com_grad (of
    sum(com * grad_com)), and for the two losses on a given prediction (flux + 0.05, no crop): direct_pixel / direct_kl with
    their _grad w.r.t. that prediction."""
    dims, truth, w = _t(inp["dims"]), _t(inp["truth"]), _t(inp["w"])
    out = {}
    flux = _t(inp["flux"]).requires_grad_(True)
    c = crop(flux, dims)
    out["crop"] = c.detach().numpy()
    out["crop_grad"] = torch.autograd.grad((c * _t(inp["grad_out"])).sum(), flux, retain_graph=True)[0].numpy()
    for name, fn in (("pixel", pixel_loss), ("kl", kl_loss)):
        loss = fn(c, truth)
        out[name] = loss.detach().numpy()
        out[name + "_grad"] = torch.autograd.grad((loss * w).sum(), flux, retain_graph=True)[0].numpy()
        out[name + "_sum_grad"] = torch.autograd.grad(loss.sum(), flux, retain_graph=True)[0].numpy()
    com = center_of_mass(flux)
    out["com"] = com.detach().numpy()
    out["com_grad"] = torch.autograd.grad((com * _t(inp["grad_com"])).sum(), flux)[0].numpy()
    for name, fn in (("direct_pixel", pixel_loss), ("direct_kl", kl_loss)):
        pred = (_t(inp["flux"]) + 0.05).requires_grad_(True)
        loss = fn(pred, truth)
        out[name] = loss.detach().numpy()
        out[name + "_grad"] = torch.autograd.grad((loss * w).sum(), pred)[0].numpy()
    return out


def oracle_chain(inp, dtype):
    """The same quantities as ``reference`` from the C oracle's chain flux_crop -> pixel_loss / kl_loss -> flux_crop(grad_out=...)
    and center_of_mass, run in ``dtype`` (np.float64: the yardstick; np.float32: the reference's own arithmetic)."""
    import oracle
    flux, dims, truth, w = (inp[k].astype(dtype) for k in ("flux", "dims", "truth", "w"))
    out = {}
    out["crop"], _ = oracle.flux_crop(flux, dims, CROP_W, CROP_H)
    out["crop_grad"] = oracle.flux_crop(flux, dims, CROP_W, CROP_H, grad_out=inp["grad_out"].astype(dtype))
    for name, fn in (("pixel", oracle.pixel_loss), ("kl", oracle.kl_loss)):
        out[name], g_crop = fn(out["crop"], truth, w)
        out[name + "_grad"] = oracle.flux_crop(flux, dims, CROP_W, CROP_H, grad_out=g_crop)
        out[name + "_sum_grad"] = oracle.flux_crop(flux, dims, CROP_W, CROP_H, grad_out=fn(out["crop"], truth, np.ones_like(w))[1])
        out["direct_" + name], out["direct_" + name + "_grad"] = fn(flux + dtype(0.05), truth, w)
    out["com"] = oracle.center_of_mass(flux)
    out["com_grad"] = oracle.center_of_mass(flux, grad_com=inp["grad_com"].astype(dtype))
    return out


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _integer_distance_np(bitmap, scale_x, scale_y):
    """``integer_distance`` of one bitmap in numpy fp64 (the generator's own check; the host test asserts the torch one)."""
    f = bitmap.astype(np.float64)
    Hh, W = f.shape
    nm = f / (f.sum() + 1e-8)
    best = np.inf
    for n, scale, centre in ((W, scale_x, (np.linspace(-1, 1, W)[None, :] * nm).sum()),
                             (Hh, scale_y, (np.linspace(-1, 1, Hh)[:, None] * nm).sum())):
        px = ((scale * np.linspace(-1, 1, n) + centre) + 1) / 2 * (n - 1)
        px = px[(px >= -1) & (px <= n)]
        if px.size:
            best = min(best, np.abs(px - np.round(px)).min())
    return best


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """Deterministic fp32 inputs of a case (read-only arrays): ``flux`` [B,Hh,W] = a Gaussian spot times noise, the spot's
    centre anywhere in the frame (near the border the spot is cut), bitmap 0 all zero; ``truth`` in [0.1, 1.1); ``dims`` [B,2];
    upstream gradients ``grad_out`` [B,Hh,W], ``w`` [B], ``grad_com`` [B,2].  A bitmap whose crop would sample within
    ``_KINK_MARGIN_PX`` of an integer coordinate is drawn again from the next seed: the kink condition is met by the choice of
    the inputs, on the CPU.

    The spot is broad (sigma 4 - 20 % of the longer side) so that every pixel of even the widest bitmap carries a value of its
    own, and the noise is +-10 %: the loss's gradient through the centre of mass is a sum over the lit pixels in which the terms
    cancel while its derivative w.r.t. the centre does not, so an error of the centre is amplified by about
    sqrt(lit pixels) x the pixel-to-pixel roughness.  With +-50 % noise on a broad spot at 128 x 512 that turns the 3e-14 by which
    the oracle's sequential fp64 sums miss the centre into 1e-10 of the gradient - the reference's own summation error, at the
    bound the host test asserts; at +-10 % it is 2e-11."""
    B, Hh, W = case.B, case.Hh, case.W
    dims = np.empty((B, 2), np.float32)
    dims[:, 0], dims[:, 1] = CROP_W / case.scale_x, CROP_H / case.scale_y
    scale_x, scale_y = CROP_W / np.float64(dims[0, 0]), CROP_H / np.float64(dims[0, 1])     # what the fp64 references see
    ys, xs = np.meshgrid(np.arange(Hh, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flux = np.zeros((B, Hh, W), np.float32)
    for b in range(1, B):
        for attempt in range(200):
            rng = np.random.default_rng([20240611, Hh, W, b, attempt])
            cx, cy = rng.uniform(0, W), rng.uniform(0, Hh)
            sigma = 2.0 + rng.uniform(0.04, 0.2) * max(Hh, W)
            spot = np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sigma ** 2))
            bitmap = (spot * rng.uniform(0.9, 1.1, size=(Hh, W))).astype(np.float32)
            if _integer_distance_np(bitmap, scale_x, scale_y) > _KINK_MARGIN_PX:
                break
        else:
            raise AssertionError(f"no admissible bitmap {b} for {case_id(case)}")
        flux[b] = bitmap
    rng = np.random.default_rng([20240612, B, Hh, W])
    inp = dict(flux=flux, dims=dims,
               truth=(rng.uniform(0.1, 1.1, size=(B, Hh, W))).astype(np.float32),
               grad_out=rng.standard_normal((B, Hh, W)).astype(np.float32),
               w=rng.uniform(0.5, 1.5, size=B).astype(np.float32),
               grad_com=rng.standard_normal((B, 2)).astype(np.float32))
    for a in inp.values():
        a.setflags(write=False)
    return inp


@functools.lru_cache(maxsize=None)
def oracle_f64(case):
    return oracle_chain(make_inputs(case), np.float64)


@functools.lru_cache(maxsize=None)
def oracle_f32(case):
    return oracle_chain(make_inputs(case), np.float32)


# ------------------------------------------------------------------------------------------------
# which path a case takes: the launch rules of artist_amd/csrc/flux_kernels.hip restated on the host, so that the host test can
# assert that the table reaches what its notes say (a shape that stops reaching its path after a change of a tile size or a
# threshold then fails there, instead of quietly testing something else).  Centres in fp64 rounded to fp32: a decision that hangs
# on the last bit of a coordinate may differ from the kernel's - the cases keep away from those.
# ------------------------------------------------------------------------------------------------
TILE_X, TILE_Y, TAPS, TILE_ROWS = 64, 32, 4, 64          # kTileX, kTileY, kTaps, kTileRows
BLOCK, PARTS, MAX_PART_BITMAPS, STAGE_LIMIT = 1024, 4, 512, 76 * 1024


def _centres(bitmap):
    f = bitmap.astype(np.float64)
    nm = f / (f.sum() + 1e-8)
    return (np.float32((np.linspace(-1, 1, f.shape[1])[None, :] * nm).sum()),
            np.float32((np.linspace(-1, 1, f.shape[0])[:, None] * nm).sum()))


def _tap_range(scale, centre, n, p):
    """tap_range(): the output indices [lo, hi] whose sampling coordinate can lie within a pixel of input index p (fp32)."""
    f = np.float32
    b = (centre + f(1)) * f(0.5) * f(n - 1) - scale * f(0.5) * f(n - 1)
    lo = (p.astype(f) - f(1.004) - b) / scale
    hi = (p.astype(f) + f(1.004) - b) / scale
    return np.maximum(0, np.ceil(lo)).astype(np.int64), np.minimum(n - 1, np.floor(hi)).astype(np.int64)


def backward_paths(case):
    """The set of paths the tiles of the case's non-empty bitmaps take in flux_crop_bwd_tiled_kernel: "tiled" (with "narrow" for
    W < 4), or the per-pixel form because a column or row has more than four taps ("wide") or because the tile's rows sample
    64 output rows or more ("rows64"), and there "gather4" / "gather8" / "general" by the taps of a pixel's columns; "taps3" /
    "taps4" when a tiled column or row has that many candidates; "unsampled" when an input pixel has none."""
    inp = make_inputs(case)
    Hh, W = case.Hh, case.W
    sx, sy = np.float32(CROP_W) / inp["dims"][0, 0], np.float32(CROP_H) / inp["dims"][0, 1]
    paths = set()
    for b in range(1, case.B):
        xc, yc = _centres(inp["flux"][b])
        jlo, jhi = _tap_range(sx, xc, W, np.arange(W))
        ilo, ihi = _tap_range(sy, yc, Hh, np.arange(Hh))
        if (jhi < jlo).any() or (ihi < ilo).any():
            paths.add("unsampled")
        for y0 in range(0, Hh, TILE_Y):
            for x0 in range(0, W, TILE_X):
                cols, rows = slice(x0, min(x0 + TILE_X, W)), slice(y0, min(y0 + TILE_Y, Hh))
                wide = ((jhi[cols] - jlo[cols]) >= TAPS).any() or ((ihi[rows] - ilo[rows]) >= TAPS).any()
                live = ihi[rows] >= ilo[rows]
                span = (ihi[rows][live].max() - ilo[rows][live].min()) if live.any() else -1
                if wide or span >= TILE_ROWS:
                    paths.add("wide" if wide else "rows64")
                    n = jhi[cols] - jlo[cols]
                    paths.update({"gather4"} if (n < 4).any() else set(), {"gather8"} if ((n >= 4) & (n < 8)).any() else set(),
                                 {"general"} if (n >= 8).any() else set())
                else:
                    paths.add("tiled")
                    if W < 4:
                        paths.add("narrow")
                    for n in (jhi[cols] - jlo[cols] + 1, ihi[rows] - ilo[rows] + 1):
                        paths.update({f"taps{k}" for k in (3, 4) if (n == k).any()})
    return paths


def fused_forward_plan(case, compute_units=256):
    """How art_flux_crop_pixel_loss_fwd launches the case when nothing forces the number of workgroups per bitmap: ``workgroups``
    per bitmap, ``column_owner``, ``stage_rows`` / ``stage_bytes`` (0: nothing staged), and over the non-empty bitmaps the number
    of ``staged`` parts, of parts ``refused`` because they sample more rows than were staged, and of ``empty`` parts."""
    inp = make_inputs(case)
    B, Hh, W = case.B, case.Hh, case.W
    column_owner = BLOCK % W == 0
    stage_rows = min(Hh, (Hh + PARTS - 1) // PARTS + 4)
    if W % 4 or not column_owner or stage_rows * W * 4 > STAGE_LIMIT:
        stage_rows = 0
    if B > MAX_PART_BITMAPS or Hh < PARTS:
        workgroups = 1
    else:
        workgroups = 4 if 4 * B <= compute_units else (2 if 2 * B <= compute_units else 1)
    plan = dict(workgroups=workgroups, column_owner=column_owner, stage_rows=stage_rows, stage_bytes=stage_rows * W * 4,
                staged=0, refused=0, empty=0)
    sy = CROP_H / np.float64(inp["dims"][0, 1])
    lin = np.linspace(-1, 1, Hh)
    for b in range(1, B):
        iy = ((sy * lin + np.float64(_centres(inp["flux"][b])[1])) + 1) / 2 * (Hh - 1)
        for v in range(PARTS):
            r0, r1 = Hh * v // PARTS, Hh * (v + 1) // PARTS
            if r0 == r1:
                plan["empty"] += 1
            elif stage_rows:
                ylo, yhi = max(0, int(np.floor(iy[r0]))), min(Hh - 1, int(np.floor(iy[r1 - 1])) + 1)
                plan["staged" if 0 < yhi - ylo + 1 <= stage_rows else "refused"] += 1
    return plan
