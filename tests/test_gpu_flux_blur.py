"""``artist_amd.flux.blur_flux`` (the blur mode of ``art_flux_crop_fwd``) on the GPU against its fp64 restatement
(tests/flux_blur_ref.py): values at every branch of the definition, the same bits whatever the batch, and the adjoint."""
import functools

import numpy as np
import pytest
import torch

import flux_blur_ref as ref
from artist_amd import _lib
from artist_amd.flux import blur_flux

pytestmark = pytest.mark.gpu

Hh, W = 48, 40                      # not square: a swap of rows and columns cannot pass
# isotropic below one pixel; sheared; |s| > 1; a ~ 0 (the column pass is the identity); S_rr ~ 0 (the row pass is); a window
# wider than the image
COVARIANCES = np.array([(0.64, 0.0, 0.64), (9.0, 3.0, 4.0), (4.0, -5.0, 9.0), (9.0, 6.0, 4.00001), (1e-5, 0.0, 6.0),
                        (30.0, 0.0, 30.0)], np.float32)
BIG = np.array([(118.86, 54.12, 178.89)], np.float32)


def inputs():
    rng = np.random.default_rng(11)
    deltas = np.zeros((Hh, W), np.float32)
    for r, c, v in ((0, 0, 1.0), (Hh - 1, W - 1, 2.0), (0, W // 2, 0.5), (Hh // 2, W // 2, 3.0)):     # corners, an edge, the centre
        deltas[r, c] = v
    dense = rng.random((Hh, W), dtype=np.float32) + 0.1
    return {"deltas": deltas, "dense": dense}


@functools.lru_cache(maxsize=None)
def small_case(name):
    """(x [6,Hh,W] fp32, fp64 reference, per-bitmap yardstick): computed once, shared, never written."""
    x = np.repeat(inputs()[name][None], len(COVARIANCES), axis=0)
    want, yard = ref.yardstick(x, COVARIANCES)
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(12)
    x = np.zeros((1, 256, 256), np.float32)
    x[0, 90:150, 100:170] = rng.random((60, 70), dtype=np.float32)         # a spot, and zero tiles around it
    x[0, 0, 0] = x[0, 255, 255] = 5.0
    want, yard = ref.yardstick(x, BIG)
    for a in (x, want, yard):
        a.setflags(write=False)
    return x, want, yard


def gpu(a):
    return torch.tensor(np.asarray(a)).cuda()


def bound(want, yard):
    """Per bitmap: 4 x the distance of the fp32 numpy evaluation from the fp64 one, at least 1e-6 of the largest value."""
    return np.maximum(4.0 * yard, 1e-6 * np.abs(want).reshape(want.shape[0], -1).max(axis=1))


def check(got, want, yard):
    err = np.abs(got.double().cpu().numpy() - want).reshape(want.shape[0], -1).max(axis=1)
    tol = bound(want, yard)
    print("max |gpu - fp64| per bitmap", err, "bound", tol)
    assert (err <= tol).all(), (err, tol)


@pytest.mark.parametrize("name", ["deltas", "dense"])
def test_operator_against_fp64(name):
    x, want, yard = small_case(name)
    check(blur_flux(gpu(x), gpu(COVARIANCES)), want, yard)


def test_operator_against_fp64_at_the_bench_size():
    x, want, yard = big_case()
    got = blur_flux(gpu(x), gpu(BIG))
    check(got, want, yard)
    assert abs(float(got.double().sum()) - want.sum()) <= 1e-5 * want.sum()


def test_same_bits_alone_in_a_batch_and_again():
    x, _, _ = small_case("dense")
    spot, _, _ = big_case()
    for bitmap, covariance in ((x[1], COVARIANCES[1]), (x[2], COVARIANCES[2]), (spot[0], BIG[0])):
        alone = blur_flux(gpu(bitmap[None]), gpu(covariance[None]))
        rng = np.random.default_rng(3)
        batch = rng.random((5,) + bitmap.shape, dtype=np.float32)
        cov = np.repeat(np.array([(2.0, 0.5, 3.0)], np.float32), 5, axis=0)
        for place in (0, 2, 4):
            batch[place], cov[place] = bitmap, covariance
        got = blur_flux(gpu(batch), gpu(cov))
        for place in (0, 2, 4):
            assert torch.equal(got[place], alone[0]), place
        assert torch.equal(blur_flux(gpu(batch), gpu(cov)), got)               # two runs


def test_bad_covariances_mark_their_own_bitmap():
    x, _, _ = small_case("dense")
    good = blur_flux(gpu(x[:5]), gpu(COVARIANCES[:5]))
    cov = COVARIANCES[:5].copy()
    cov[1] = (4.0, 5.0, 4.0)            # not positive semi-definite
    cov[3] = (300.0, 0.0, 9.0)          # beyond the limit: 4 sqrt(300) > 64
    got = blur_flux(gpu(x[:5]), gpu(cov))
    assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
    for keep in (0, 2, 4):
        assert torch.equal(got[keep], good[keep])
    for bad in ((float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, -2.0)):
        assert torch.isnan(blur_flux(gpu(x[:1]), torch.tensor([bad], device="cuda"))).all(), bad
    edge = blur_flux(gpu(x[:1]), torch.tensor([(256.0, 0.0, 256.0)], device="cuda"))       # the limit itself is served
    assert torch.isfinite(edge).all()


def test_adjoint():
    """<F x, y> = <x, F y> within the yardstick, and autograd's gradient IS the forward call on the upstream gradient."""
    rng = np.random.default_rng(21)
    x = rng.random((len(COVARIANCES), Hh, W), dtype=np.float32)
    y = rng.random((len(COVARIANCES), Hh, W), dtype=np.float32)
    cov = gpu(COVARIANCES)
    bound_x, bound_y = bound(*ref.yardstick(x, COVARIANCES)), bound(*ref.yardstick(y, COVARIANCES))
    fx, fy = blur_flux(gpu(x), cov).double().cpu().numpy(), blur_flux(gpu(y), cov).double().cpu().numpy()
    for b in range(len(COVARIANCES)):
        left, right = (fx[b] * y[b]).sum(), (x[b].astype(np.float64) * fy[b]).sum()
        # each side is off by at most (the bound of test 1 per pixel of its blurred operand) x (the other operand's absolute sum)
        tol = bound_x[b] * np.abs(y[b]).sum() + bound_y[b] * np.abs(x[b]).sum()
        print("bitmap", b, "<Fx,y> - <x,Fy>", left - right, "bound", tol)
        assert abs(left - right) <= tol
    xt = gpu(x).requires_grad_(True)
    (blur_flux(xt, cov) * gpu(y)).sum().backward()
    assert torch.equal(xt.grad, blur_flux(gpu(y), cov))


def test_refusals_and_empty_batches():
    x, cov = torch.zeros(2, 4, 5, device="cuda"), torch.ones(2, 3, device="cuda")
    assert blur_flux(x[:0], cov[:0]).shape == (0, 4, 5)
    assert blur_flux(x[:, :0], cov).shape == (2, 0, 5)
    with pytest.raises(ValueError, match="covariance of blur_flux is a constant"):
        blur_flux(x, cov.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"must be \[B,Hh,W\]"):
        blur_flux(x, cov[:1])
    with pytest.raises(ValueError, match="float32"):
        blur_flux(x.double(), cov)
    # the C ABI: blur mode refuses target dimensions, null pointers and an output that overlaps the input
    dims = torch.ones(2, 2, device="cuda")
    out = torch.empty_like(x)
    for args in ((x.data_ptr(), dims.data_ptr(), 2, 4, 5, -1.0, -1.0, out.data_ptr(), cov.data_ptr()),
                 (None, None, 2, 4, 5, -1.0, -1.0, out.data_ptr(), cov.data_ptr()),
                 (x.data_ptr(), None, 2, 4, 5, -1.0, -1.0, None, cov.data_ptr()),
                 (x.data_ptr(), None, 2, 4, 5, -1.0, -1.0, out.data_ptr(), None),
                 (x.data_ptr(), None, 2, 4, 5, -1.0, -1.0, x.data_ptr(), cov.data_ptr())):
        with pytest.raises(_lib.ArtistHipError, match="code"):
            _lib.call("art_flux_crop_fwd", x.device, *args)
    torch.cuda.synchronize()
