"""GPU tests (``-m gpu``) of the Gaussian window of the convolved sun - ``artist_amd.flux.blur_flux``, the blur mode of
``art_flux_crop_fwd`` - at the shapes and covariances of ``flux_blur_ref.CASES``: every branch of
artist_amd/csrc/flux_blur_kernels.hip that the shape or the covariance selects (``flux_blur_ref.BRANCHES``: tile rows, tiles lower
than the image or taller, one to three table segments per pass, the identity passes, the 16-bit and the 10-bit shear, skipped
corner tiles, tiles walked in turns, runs of more than 128 rows, the clamped wave alone and behind a full block, blocks of 8 taps),
against the fp64 restatement tests/flux_blur_ref.py.  tests/test_blur_shapes_host.py proves without a GPU that the table reaches
every one of these branches.

Rule of every comparison (the one of tests/test_gpu_flux_blur.py, whose ``bound`` and ``check`` are used here): per bitmap,
max |gpu - fp64| <= max(4 x yardstick, 1e-6 x peak), the yardstick being the distance of the fp32 numpy evaluation from the fp64
one on the same input.  No case and no pixel is left out.  Every comparison prints error, bound and error / bound.

Measured on an MI355X, over the 27 cases x 13 covariances (351 bitmaps): the largest error / bound is 0.285 ((129, 70) dense under
covariance 10, (256, 0, 1e-5): error 2.44e-7, bound 8.56e-7).  Sums: at most 7.7e-8 relative.  Adjoint: at most 0.0038 of its
tolerance.  The infinite pixel: for every covariance the non-finite outputs are exactly the reference's (up to 5250 of them) - the
kernel spreads it no further - and the rest is within 0.27 of the bound.  No test here found a fault in the kernel.

What these tests see and tests/test_gpu_flux_blur.py does not - one value-only change at a time in a scratch copy of the kernel, old
and new file run once:
- the third table segment of the row pass (the single tap k = +64) dropped: the 12 value tests of the shapes of 129 rows and more
  fail, by up to 316 bounds ((129, 70) bands, covariance 10: error 3.14e-5), and so does the infinite pixel; the old file passes.
- the row pass's fractions formed from the rounded shear instead of s: the old file's two value tests fail as well (the 16-bit
  rounding of s = 1/3); here 8 value tests and the infinite pixel, by 1.22 bounds (covariance 12, s = 0.3).  Under the 10-bit shear
  no comparison of values can see this change: |s| > 64 needs S_rr < 1/16, so Kr = 1 and the two off-centre taps weigh at most
  exp(-8) = 3.4e-4, while rounding s to 10 bits moves their fraction by at most 4.9e-4 - 2e-7 of a value, inside any fp32 bound.
"""
import functools

import numpy as np
import pytest
import torch

import flux_blur_ref as ref
from artist_amd import _lib
from artist_amd.flux import blur_flux
from test_gpu_flux_blur import bound, check, gpu

pytestmark = pytest.mark.gpu

COV = ref.COVARIANCES
LARGEST = (300, 130)
_worst = {"ratio": 0.0, "what": ""}


def input_of(shape, name):
    if name == "other":             # the adjoint's second operand
        return np.random.default_rng(77 + shape[0]).standard_normal(shape).astype(np.float32)
    return ref.case_input(shape, name)


@functools.lru_cache(maxsize=None)
def case(shape, name):
    """(x [B,Hh,W] fp32, fp64 reference, per-bitmap yardstick) with every covariance of the table as the batch: computed once,
    shared, never written."""
    x = np.repeat(input_of(shape, name)[None], len(COV), axis=0)
    want, yard = ref.yardstick(x, COV)
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


def compare(got, want, yard, what):
    err = np.abs(got.double().cpu().numpy() - want).reshape(want.shape[0], -1).max(axis=1)
    tol = bound(want, yard)
    for b in range(want.shape[0]):
        print(f"{what} bitmap {b}: error {err[b]:.3e} bound {tol[b]:.3e} ratio {err[b] / tol[b]:.3f}")
        if err[b] / tol[b] > _worst["ratio"]:
            _worst.update(ratio=err[b] / tol[b], what=f"{what} bitmap {b}: error {err[b]:.3e}, bound {tol[b]:.3e}")
    print("largest error / bound so far:", _worst)
    check(got, want, yard)


@pytest.mark.parametrize("shape,name", ref.CASES, ids=[f"{s[0]}x{s[1]}-{n}" for s, n in ref.CASES])
def test_operator_against_fp64(shape, name):
    x, want, yard = case(shape, name)
    assert not np.isnan(want).any()
    compare(blur_flux(gpu(x), gpu(COV)), want, yard, f"{shape} {name}")


def test_sums_at_the_largest_shape():
    x, want, _ = case(LARGEST, "dense")
    got = blur_flux(gpu(x), gpu(COV)).double().cpu().numpy()
    for b in range(len(COV)):
        print("bitmap", b, "sum", got[b].sum(), "fp64", want[b].sum(), "relative", abs(got[b].sum() - want[b].sum()) / abs(want[b].sum()))
        assert abs(got[b].sum() - want[b].sum()) <= 1e-5 * abs(want[b].sum())


@pytest.mark.parametrize("shape", [LARGEST, (9, 65)], ids=["300x130", "9x65"])
def test_adjoint(shape):
    """<F x, y> = <x, F y> within the yardstick (a wrong tile seam breaks this even where the values stay inside the bound), and
    autograd's gradient IS the forward call on the upstream gradient."""
    (x, want_x, yard_x), (y, want_y, yard_y) = case(shape, "dense"), case(shape, "other")
    cov = gpu(COV)
    bound_x, bound_y = bound(want_x, yard_x), bound(want_y, yard_y)
    fx, fy = blur_flux(gpu(x), cov).double().cpu().numpy(), blur_flux(gpu(y), cov).double().cpu().numpy()
    for b in range(len(COV)):
        left, right = (fx[b] * y[b]).sum(), (x[b].astype(np.float64) * fy[b]).sum()
        # each side is off by at most (the bound of test 1 per pixel of its blurred operand) x (the other operand's absolute sum)
        tol = bound_x[b] * np.abs(y[b]).sum() + bound_y[b] * np.abs(x[b]).sum()
        print("bitmap", b, "<Fx,y> - <x,Fy>", left - right, "bound", tol, "ratio", abs(left - right) / tol)
        assert abs(left - right) <= tol
    xt = gpu(x).requires_grad_(True)
    (blur_flux(xt, cov) * gpu(y)).sum().backward()
    assert torch.equal(xt.grad, blur_flux(gpu(y), cov))


def test_same_bits_alone_in_a_batch_and_again():
    """The sheared limit and the s = 90 bitmap at (257, 66): two tile rows, corner tiles, tiles walked in turns."""
    shape = (257, 66)
    bitmap = input_of(shape, "dense")
    for index in (2, 7):
        alone = blur_flux(gpu(bitmap[None]), gpu(COV[index][None]))
        batch = np.random.default_rng(3).standard_normal((5,) + shape).astype(np.float32)
        cov = np.repeat(np.array([(2.0, 0.5, 3.0)], np.float32), 5, axis=0)
        for place in (0, 2, 4):
            batch[place], cov[place] = bitmap, COV[index]
        got = blur_flux(gpu(batch), gpu(cov))
        for place in (0, 2, 4):
            assert torch.equal(got[place], alone[0]), (index, place)
        assert torch.equal(blur_flux(gpu(batch), gpu(cov)), got)               # two runs
        assert torch.equal(blur_flux(gpu(bitmap[None]), gpu(COV[index][None])), alone)


def test_a_nan_bitmap_keeps_to_itself():
    shape = (257, 66)
    x = np.repeat(input_of(shape, "dense")[None], 3, axis=0)
    cov = gpu(COV[[2, 1, 7]])
    clean = blur_flux(gpu(x), cov)
    x[1] = np.nan
    got = blur_flux(gpu(x), cov)
    assert torch.isnan(got[1]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[2], clean[2])


def test_one_infinite_pixel_stays_inside_its_window():
    """x[10, 5] = inf at (300, 130): what the reference makes non-finite is non-finite, and every output more than 64 rows or more
    than Ka + |s| Kr + 2 columns from the pixel is finite and within the bound."""
    r0, c0 = 10, 5
    x = np.repeat(input_of(LARGEST, "dense")[None], len(COV), axis=0)
    x[:, r0, c0] = np.inf
    with np.errstate(all="ignore"):
        want = ref.blur(x, COV, np.float64)
        low = ref.blur(x, COV, np.float32).astype(np.float64)
    got = blur_flux(gpu(x), gpu(COV)).double().cpu().numpy()
    rows, cols = np.mgrid[:LARGEST[0], :LARGEST[1]]
    for b, covariance in enumerate(COV):
        plan = ref.tiling(covariance, *LARGEST)
        reach = plan["Ka"] + abs(plan["s"]) * plan["Kr"] + 2
        far = (np.abs(rows - r0) > 64) | (np.abs(cols - c0) > reach)
        assert far.any() and np.isfinite(want[b][far]).all() and not np.isfinite(want[b]).all(), b
        assert not np.isfinite(got[b][~np.isfinite(want[b])]).any(), b
        spread = ~np.isfinite(got[b])
        print("bitmap", b, "non-finite outputs: reference", int((~np.isfinite(want[b])).sum()), "gpu", int(spread.sum()), "rows",
              np.abs(rows - r0)[spread].max(), "columns", np.abs(cols - c0)[spread].max(), "allowed columns", reach)
        assert np.isfinite(got[b][far]).all(), b
        yard = np.abs(low[b][far] - want[b][far]).max()
        tol = bound(np.where(far, want[b], 0.0)[None], np.array([yard]))[0]
        err = np.abs(got[b][far] - want[b][far]).max()
        print("bitmap", b, "far from the pixel: error", err, "bound", tol, "ratio", err / tol)
        assert err <= tol, b


def test_the_batch_limit():
    """B = 65535 bitmaps of one pixel are served (the identity under a sub-pixel covariance); B = 65536 is refused and nothing is
    written."""
    identity = np.array([(1e-5, 0.0, 1e-5)], np.float32)
    x = torch.randn(65535, 1, 1, device="cuda")
    assert torch.equal(blur_flux(x, gpu(identity).repeat(65535, 1)), x)
    x = torch.randn(65536, 1, 1, device="cuda")
    cov = gpu(identity).repeat(65536, 1)
    with pytest.raises(_lib.ArtistHipError, match="code"):
        blur_flux(x, cov)
    out = torch.full_like(x, -7.0)
    with pytest.raises(_lib.ArtistHipError, match="code"):
        _lib.call("art_flux_crop_fwd", x.device, x.data_ptr(), None, 65536, 1, 1, -1.0, -1.0, out.data_ptr(), cov.data_ptr())
    torch.cuda.synchronize()
    assert (out == -7.0).all()
