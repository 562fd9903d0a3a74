"""GPU tests (``-m gpu``) of the radial window of the convolved sun - ``artist_amd.flux.radial_blur_flux``, the radial window mode
of ``art_flux_crop_fwd`` - at the tables, metrics and shapes of ``radial_blur_ref.CASES``: every branch of
artist_amd/csrc/radial_blur_kernels.hip that the metric, the table, the shape or the batch selects (``radial_blur_ref.BRANCHES``:
the six tile shapes, stencil row 64 out of LDS, 64 columns of taps, a table counted in several chunks, a cut table, ragged last
tiles in both directions, tiles walked in turns, a grid that B cuts), against the fp64 restatement tests/radial_blur_ref.py.
tests/test_blur_shapes_host.py proves without a GPU that the table reaches every one of these branches.

Rule of every comparison (the one of tests/test_gpu_radial_blur.py, whose ``bound`` and ``check`` are used here): per bitmap,
max |gpu - fp64| <= max(4 x yardstick, 1e-6 x peak), the yardstick being the distance of the fp32 numpy evaluation from the fp64
one on the same input.  No case and no pixel is left out.  Every comparison prints error, bound and error / bound.

Measured on an MI355X, over the 41 cases (92 bitmaps): the largest error / bound is 0.340 (buie (33, 9) dense: error 7.83e-9, bound
2.31e-8).  Sums: at most 2.0e-6 relative (the 50 px pillbox).  Adjoint: at most 5.0e-4 of its tolerance.  The infinite pixel: the
kernel's zero taps spread it over 8, 67 and 27 columns for stencils of 5, 64 and 20 columns - at most seven more than the stencil, within
the 64 + 11 allowed - and the rest is within 0.28 of the bound.  No test here found a fault in the kernel.

What these tests see and tests/test_gpu_radial_blur.py does not - one value-only change at a time in a scratch copy of the kernel,
old and new file run once:
- stencil row 64 skipped: 12 value tests (the pillbox, uniform1024 and uniform4096 tables from 65 rows on), three sums and the
  infinite pixel fail, by up to 155 000 bounds (uniform4096 (65, 17) seams: error 7.44e-5, bound 4.79e-10); the old file passes.
- the weights of the RW = 32 tile shape scaled by 1.001: all 10 value tests of uniform4096 and its sum fail, by 1000 bounds; the old
  file passes.
"""
import functools

import numpy as np
import pytest
import torch

import radial_blur_ref as ref
from artist_amd import _lib
from artist_amd.flux import radial_blur_flux
from test_gpu_radial_blur import bound, check, gpu

pytestmark = pytest.mark.gpu

LARGEST = (130, 70)
TABLE_NAMES = ("pillbox", "uniform1024", "uniform4096", "buie")
ALL_METRICS = [("pillbox", i) for i in range(6)] + [("uniform1024", 0), ("uniform4096", 0), ("buie", 0)]
_worst = {"ratio": 0.0, "what": ""}


def input_of(shape, name):
    if name == "other":             # the adjoint's second operand
        return np.random.default_rng(77 + shape[0]).standard_normal(shape).astype(np.float32)
    return ref.case_input(shape, name)


@functools.lru_cache(maxsize=None)
def one(table_name, index, shape, name):
    """(fp64 reference [Hh,W], yardstick) of one bitmap: computed once, shared, never written."""
    table, metrics, _ = ref.tables()[table_name]
    want, yard = ref.yardstick(input_of(shape, name)[None], metrics[index:index + 1], table)
    want.setflags(write=False)
    return want[0], float(yard[0])


def case(table_name, shape, name, count=None):
    """(x [B,Hh,W] fp32, fp64 reference, per-bitmap yardstick) with the table's (first ``count``) metrics as the batch."""
    metrics = ref.tables()[table_name][1][:count]
    parts = [one(table_name, index, shape, name) for index in range(len(metrics))]
    x = np.repeat(input_of(shape, name)[None], len(metrics), axis=0)
    return x, np.stack([p[0] for p in parts]), np.array([p[1] for p in parts]), metrics


def compare(got, want, yard, what):
    err = np.abs(got.double().cpu().numpy() - want).reshape(want.shape[0], -1).max(axis=1)
    tol = bound(want, yard)
    for b in range(want.shape[0]):
        print(f"{what} bitmap {b}: error {err[b]:.3e} bound {tol[b]:.3e} ratio {err[b] / tol[b]:.3f}")
        if err[b] / tol[b] > _worst["ratio"]:
            _worst.update(ratio=err[b] / tol[b], what=f"{what} bitmap {b}: error {err[b]:.3e}, bound {tol[b]:.3e}")
    print("largest error / bound so far:", _worst)
    check(got, want, yard)


@pytest.mark.parametrize("table_name,shape,name", ref.CASES, ids=[f"{t}-{s[0]}x{s[1]}-{n}" for t, s, n in ref.CASES])
def test_operator_against_fp64(table_name, shape, name):
    x, want, yard, metrics = case(table_name, shape, name)
    assert not np.isnan(want).any()
    got = radial_blur_flux(gpu(x), gpu(metrics), gpu(ref.tables()[table_name][0]))
    compare(got, want, yard, f"{table_name} {shape} {name}")


def test_a_spot_among_zero_tiles():
    """(200, 150), zero but for six pixels, under the first two pillbox metrics: all-zero tiles, ragged ones among them, and under
    the second metric a workgroup that builds its stencil at its second tile."""
    x, want, yard, metrics = case("pillbox", ref.SPOT_SHAPE, "spot", count=2)
    compare(radial_blur_flux(gpu(x), gpu(metrics), gpu(ref.tables()["pillbox"][0])), want, yard, f"pillbox {ref.SPOT_SHAPE} spot")


@pytest.mark.parametrize("table_name", TABLE_NAMES)
def test_sums_at_the_largest_shape(table_name):
    x, want, _, metrics = case(table_name, LARGEST, "dense")
    got = radial_blur_flux(gpu(x), gpu(metrics), gpu(ref.tables()[table_name][0])).double().cpu().numpy()
    for b in range(len(metrics)):
        print("bitmap", b, "sum", got[b].sum(), "fp64", want[b].sum(), "relative", abs(got[b].sum() - want[b].sum()) / abs(want[b].sum()))
        assert abs(got[b].sum() - want[b].sum()) <= 1e-5 * abs(want[b].sum())


@pytest.mark.parametrize("table_name,index", ALL_METRICS, ids=[f"{t}-{i}" for t, i in ALL_METRICS])
def test_adjoint(table_name, index):
    """<F x, y> = <x, F y> within the yardstick (a wrong tile seam breaks this even where the values stay inside the bound), and
    autograd's gradient IS the forward call on the upstream gradient."""
    table, metrics, _ = ref.tables()[table_name]
    x, y = input_of(LARGEST, "dense")[None], input_of(LARGEST, "other")[None]
    (want_x, yard_x), (want_y, yard_y) = one(table_name, index, LARGEST, "dense"), one(table_name, index, LARGEST, "other")
    bound_x, bound_y = bound(want_x[None], np.array([yard_x]))[0], bound(want_y[None], np.array([yard_y]))[0]
    m, t = gpu(metrics[index:index + 1]), gpu(table)
    fx, fy = radial_blur_flux(gpu(x), m, t).double().cpu().numpy(), radial_blur_flux(gpu(y), m, t).double().cpu().numpy()
    left, right = (fx * y).sum(), (x.astype(np.float64) * fy).sum()
    # each side is off by at most (the bound of test 1 per pixel of its blurred operand) x (the other operand's absolute sum)
    tol = bound_x * np.abs(y).sum() + bound_y * np.abs(x).sum()
    print("<Fx,y> - <x,Fy>", left - right, "bound", tol, "ratio", abs(left - right) / tol)
    assert abs(left - right) <= tol
    xt = gpu(x).requires_grad_(True)
    (radial_blur_flux(xt, m, t) * gpu(y)).sum().backward()
    assert torch.equal(xt.grad, radial_blur_flux(gpu(y), m, t))


@pytest.mark.parametrize("table_name,shape,batches", ref.BATCH_CASES, ids=[f"{t}-{s[0]}x{s[1]}" for t, s, _ in ref.BATCH_CASES])
def test_same_bits_whatever_the_batch(table_name, shape, batches):
    """Alone, at places 0, 1024 and 2048 of a batch of 2049 (share = 1: one workgroup walks all of a bitmap's tiles with one
    stencil) and in a batch of 1025 (share = 2); the other bitmaps are seeded noise under the same metric."""
    table, metrics, _ = ref.tables()[table_name]
    t = gpu(table)
    bitmap = gpu(input_of(shape, "dense"))
    alone = radial_blur_flux(bitmap[None], gpu(metrics[:1]), t)
    assert torch.isfinite(alone).all() and alone.abs().max() > 0
    for B in batches[1:]:
        batch = torch.randn((B,) + shape, device="cuda", generator=torch.Generator("cuda").manual_seed(B))
        places = (0, B // 2, B - 1)
        for place in places:
            batch[place] = bitmap
        got = radial_blur_flux(batch, gpu(metrics[:1]).repeat(B, 1), t)
        for place in places:
            assert torch.equal(got[place], alone[0]), (B, place)
        del batch, got
    assert torch.equal(radial_blur_flux(bitmap[None], gpu(metrics[:1]), t), alone)


def test_a_nan_bitmap_keeps_to_itself():
    x, _, _, metrics = case("pillbox", LARGEST, "dense")
    x = x[:3].copy()
    m, t = gpu(metrics[[3, 1, 4]]), gpu(ref.tables()["pillbox"][0])
    clean = radial_blur_flux(gpu(x), m, t)
    x[1] = np.nan
    got = radial_blur_flux(gpu(x), m, t)
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_one_infinite_pixel_stays_inside_its_window():
    """x[2, 3] = inf at (140, 90): what the reference makes non-finite is non-finite, and every output more than 64 rows or more
    than 64 + 11 columns from the pixel is finite and within the bound (the kernel walks taps in blocks of 8 that may start up to
    three taps early: a zero tap on the pixel is 0 x inf)."""
    shape, r0, c0 = (140, 90), 2, 3
    table, metrics, _ = ref.tables()["pillbox"]
    metrics = metrics[[0, 3, 4]]
    x = np.repeat(input_of(shape, "dense")[None], len(metrics), axis=0)
    x[:, r0, c0] = np.inf
    with np.errstate(all="ignore"):
        want = ref.blur(x, metrics, table, np.float64)
        low = ref.blur(x, metrics, table, np.float32).astype(np.float64)
    got = radial_blur_flux(gpu(x), gpu(metrics), gpu(table)).double().cpu().numpy()
    rows, cols = np.mgrid[:shape[0], :shape[1]]
    far = (np.abs(rows - r0) > 64) | (np.abs(cols - c0) > 64 + 11)
    for b in range(len(metrics)):
        assert np.isfinite(want[b][far]).all() and not np.isfinite(want[b]).all(), b
        assert not np.isfinite(got[b][~np.isfinite(want[b])]).any(), b
        spread = ~np.isfinite(got[b])
        print("bitmap", b, "non-finite outputs: reference", int((~np.isfinite(want[b])).sum()), "gpu", int(spread.sum()), "rows",
              np.abs(rows - r0)[spread].max(), "columns", np.abs(cols - c0)[spread].max())
        assert np.isfinite(got[b][far]).all(), b
        yard = np.abs(low[b][far] - want[b][far]).max()
        tol = bound(np.where(far, want[b], 0.0)[None], np.array([yard]))[0]
        err = np.abs(got[b][far] - want[b][far]).max()
        print("bitmap", b, "far from the pixel: error", err, "bound", tol, "ratio", err / tol)
        assert err <= tol, b


def test_the_limits():
    """B = 65535 bitmaps of one pixel are served (a pillbox far below a pixel is the identity); B = 65536 is refused and nothing
    is written.  K = 4096 is served (the `uniform4096` cases above); K = 4097 is refused."""
    table, _, _ = ref.tables()["pillbox"]
    t = gpu(table)
    sub_pixel = torch.tensor([(1.0e2, 0.0, 1.0e2)], device="cuda")
    x = torch.randn(65535, 1, 1, device="cuda")
    assert torch.equal(radial_blur_flux(x, sub_pixel.repeat(65535, 1), t), x)
    x = torch.randn(65536, 1, 1, device="cuda")
    metric = sub_pixel.repeat(65536, 1)
    with pytest.raises(_lib.ArtistHipError, match="code"):
        radial_blur_flux(x, metric, t)
    out = torch.full_like(x, -7.0)
    with pytest.raises(_lib.ArtistHipError, match="code"):
        _lib.call("art_flux_crop_fwd", x.device, x.data_ptr(), t.data_ptr(), 65536, 1, 1, -2.0, -1.0, out.data_ptr(), metric.data_ptr())
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    x = torch.randn(2, 4, 5, device="cuda")
    with pytest.raises(ValueError, match="1 <= K <= 4096"):
        radial_blur_flux(x, sub_pixel.repeat(2, 1), torch.zeros(4098, device="cuda"))
    long_table, out = torch.zeros(4100, device="cuda"), torch.full_like(x, -7.0)
    with pytest.raises(_lib.ArtistHipError, match="code"):
        _lib.call("art_flux_crop_fwd", x.device, x.data_ptr(), long_table.data_ptr(), 2, 4, 5, -2.0, -4097.0, out.data_ptr(),
                  sub_pixel.repeat(2, 1).data_ptr())
    torch.cuda.synchronize()
    assert (out == -7.0).all()
