"""The gradient of the blur with respect to its covariance on the GPU: the blur mode of ``art_flux_crop_bwd``
against its fp64 restatement (tests/flux_blur_grad_ref.py) at every branch of the definition and of the kernel's tiling, the
same bits whatever the batch, ``artist_amd.flux.differentiable_blur_flux`` on top of it, and a sigma that learns."""
import functools

import numpy as np
import pytest
import torch

import flux_blur_grad_ref as gref
import flux_blur_ref as ref
import flux_ref
from artist_amd import EpochGraph, _lib, differentiable_blur_flux
from artist_amd.flux import FluxCrop, blur_flux

pytestmark = pytest.mark.gpu

Hh, W = gref.OPERATOR_SHAPE
COVARIANCES = np.array(gref.OPERATOR_COVARIANCES, np.float32)
BIG = np.array([gref.SPOT[0]], np.float32)
_worst = {"ratio": 0.0, "what": ""}


def gpu(a):
    return torch.tensor(np.asarray(a)).cuda()


def window_gradient(x, covariance, g):
    """The C ABI itself: ``art_flux_crop_bwd`` in its blur mode, no gradient of the flux asked for."""
    x, covariance, g = x.contiguous(), covariance.contiguous(), g.contiguous()
    B, rows, cols = x.shape
    out = torch.full((B, 3), 7.0, device="cuda")            # fully written: nothing of this survives
    _lib.call("art_flux_crop_bwd", x.device, x.data_ptr(), None, covariance.data_ptr(), B, rows, cols, -1.0, -1.0, g.data_ptr(), None,
              out.data_ptr())
    return out


def check(what, got, want, tol):
    err = np.abs(got.double().cpu().numpy() - want)
    ratio = float(np.divide(err, tol, out=np.zeros_like(err), where=tol > 0).max())         # (0 of 0: an identity pass)
    if ratio > _worst["ratio"]:
        _worst.update(ratio=ratio, what=what)
    print(f"{what}: largest |gpu - fp64| / bound {ratio:.3f}   [worst so far {_worst['ratio']:.3f}: {_worst['what']}]")
    assert (err <= tol).all(), (what, err, tol)


def small_inputs(name):
    rng = np.random.default_rng(11)
    x = rng.random((Hh, W), dtype=np.float32) + 0.1
    if name == "dense":
        g = np.random.default_rng(13).standard_normal((Hh, W)).astype(np.float32)           # signed: an upstream gradient
    else:
        g = np.zeros((Hh, W), np.float32)
        for r, c, v in ((0, 0, 1.0), (Hh - 1, W - 1, -2.0), (0, W // 2, 0.5), (Hh // 2, W // 2, 3.0)):
            g[r, c] = v
    return x, g


@functools.lru_cache(maxsize=None)
def small_case(name):
    """(x, g [6,Hh,W] fp32, fp64 gradients [6,3], bounds [6,3]): computed once, shared, never written."""
    x, g = (np.repeat(a[None], len(COVARIANCES), axis=0) for a in small_inputs(name))
    want, tol = gref.yardstick(x, g, COVARIANCES)
    for a in (x, g, want, tol):
        a.setflags(write=False)
    return x, g, want, tol


@functools.lru_cache(maxsize=None)
def big_case():
    rng = np.random.default_rng(12)
    x = np.zeros((1, 256, 256), np.float32)
    x[0, 90:150, 100:170] = rng.random((60, 70), dtype=np.float32)         # a spot, and zero tiles around it
    x[0, 0, 0] = x[0, 255, 255] = 5.0
    g = rng.standard_normal((1, 256, 256)).astype(np.float32)
    want, tol = gref.yardstick(x, g, BIG)
    for a in (x, g, want, tol):
        a.setflags(write=False)
    return x, g, want, tol


@pytest.mark.parametrize("name", ["dense", "deltas"])
def test_kernel_against_fp64(name):
    x, g, want, tol = small_case(name)
    check(f"48 x 40, g {name}", window_gradient(gpu(x), gpu(COVARIANCES), gpu(g)), want, tol)


@pytest.mark.parametrize("shape", gref.BATCH_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_against_fp64_at_every_tiling_branch(shape):
    """``flux_blur_ref.COVARIANCES`` as the batch: dense bitmaps and bitmaps with rounds of zeros in turn, a signed dense g."""
    B = len(ref.COVARIANCES)
    x = np.stack([ref.case_input(shape, "dense" if b % 2 == 0 else "bands") for b in range(B)])
    g = np.random.default_rng(7000 + shape[0]).standard_normal((B,) + tuple(shape)).astype(np.float32)
    want, tol = gref.yardstick(x, g, ref.COVARIANCES)
    check(f"{shape}", window_gradient(gpu(x), gpu(ref.COVARIANCES), gpu(g)), want, tol)


def test_kernel_against_fp64_at_the_bench_size():
    x, g, want, tol = big_case()
    check("256 x 256 spot", window_gradient(gpu(x), gpu(BIG), gpu(g)), want, tol)


def test_same_bits_alone_in_a_batch_and_again():
    x, g, _, _ = small_case("dense")
    spot, spot_g, _, _ = big_case()
    for bitmap, upstream, covariance in ((x[1], g[1], COVARIANCES[1]), (x[2], g[2], COVARIANCES[2]), (spot[0], spot_g[0], BIG[0])):
        alone = window_gradient(gpu(bitmap[None]), gpu(covariance[None]), gpu(upstream[None]))
        rng = np.random.default_rng(3)
        batch = rng.random((5,) + bitmap.shape, dtype=np.float32)
        batch_g = rng.standard_normal((5,) + bitmap.shape).astype(np.float32)
        cov = np.repeat(np.array([(2.0, 0.5, 3.0)], np.float32), 5, axis=0)
        for place in (0, 2, 4):
            batch[place], batch_g[place], cov[place] = bitmap, upstream, covariance
        got = window_gradient(gpu(batch), gpu(cov), gpu(batch_g))
        for place in (0, 2, 4):
            assert torch.equal(got[place], alone[0]), place
        assert torch.equal(window_gradient(gpu(batch), gpu(cov), gpu(batch_g)), got)               # two runs


def test_invalid_covariances_mark_their_own_gradient():
    x, g, _, _ = small_case("dense")
    good = window_gradient(gpu(x[:5]), gpu(COVARIANCES[:5]), gpu(g[:5]))
    assert torch.isfinite(good).all()
    cov = COVARIANCES[:5].copy()
    cov[1] = (4.0, 5.0, 4.0)            # not positive semi-definite
    cov[3] = (300.0, 0.0, 9.0)          # beyond the limit: 4 sqrt(300) > 64
    got = window_gradient(gpu(x[:5]), gpu(cov), gpu(g[:5]))
    assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
    for keep in (0, 2, 4):
        assert torch.equal(got[keep], good[keep])
    for bad in ((float("nan"), 0.0, 1.0), (1.0, float("inf"), 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, -2.0)):
        assert torch.isnan(window_gradient(gpu(x[:1]), torch.tensor([bad], device="cuda"), gpu(g[:1]))).all(), bad
    edge = window_gradient(gpu(x[:1]), torch.tensor([(256.0, 0.0, 256.0)], device="cuda"), gpu(g[:1]))      # the limit is served
    assert torch.isfinite(edge).all()
    # the identity passes: a row pass that is the identity leaves (0, 0, D_a), two of them (0, 0, 0)
    row_identity = window_gradient(gpu(x[:1]), torch.tensor([(1e-5, 0.0, 6.0)], device="cuda"), gpu(g[:1]))[0]
    assert row_identity[0] == 0 and row_identity[1] == 0 and row_identity[2] != 0
    assert not window_gradient(gpu(x[:1]), torch.tensor([(1e-5, 0.0, 1e-5)], device="cuda"), gpu(g[:1])).any()


def test_differentiable_blur_flux():
    x, g, _, _ = small_case("dense")
    cov = gpu(COVARIANCES)
    xt, ct = gpu(x).requires_grad_(True), cov.clone().requires_grad_(True)
    z = differentiable_blur_flux(xt, ct)
    assert torch.equal(z, blur_flux(gpu(x), cov))
    (z * gpu(g)).sum().backward()
    assert torch.equal(xt.grad, blur_flux(gpu(g), cov))
    assert torch.equal(ct.grad, window_gradient(gpu(x), cov, gpu(g)))
    # a constant window: blur_flux's values and gradient, and no gradient for the covariance
    xt = gpu(x).requires_grad_(True)
    z = differentiable_blur_flux(xt, cov)
    assert torch.equal(z, blur_flux(gpu(x), cov))
    (z * gpu(g)).sum().backward()
    assert torch.equal(xt.grad, blur_flux(gpu(g), cov))
    # the window alone learns
    ct = cov.clone().requires_grad_(True)
    (differentiable_blur_flux(gpu(x), ct) * gpu(g)).sum().backward()
    assert torch.equal(ct.grad, window_gradient(gpu(x), cov, gpu(g)))
    with pytest.raises(ValueError, match=r"must be \[B,Hh,W\]"):
        differentiable_blur_flux(gpu(x), cov[:1])
    with pytest.raises(ValueError, match="float32"):
        differentiable_blur_flux(gpu(x).double(), cov)
    with pytest.raises(_lib.ArtistHipError, match="no CPU fallback"):
        differentiable_blur_flux(torch.zeros(2, 4, 5), torch.ones(2, 3))
    with pytest.raises(ValueError, match="covariance of blur_flux is a constant"):          # the old name keeps its refusal
        blur_flux(gpu(x), cov.clone().requires_grad_(True))


def test_abi_refusals_and_empty_batches():
    x, cov, g = torch.zeros(2, 4, 5, device="cuda"), torch.ones(2, 3, device="cuda"), torch.ones(2, 4, 5, device="cuda")
    out = torch.full((2, 3), 7.0, device="cuda")
    blur = (-1.0, -1.0)
    for B, rows, cols in ((0, 4, 5), (2, 0, 5), (2, 4, 0)):           # nothing to launch, nothing written
        _lib.call("art_flux_crop_bwd", x.device, x.data_ptr(), None, cov.data_ptr(), B, rows, cols, *blur, g.data_ptr(), None, out.data_ptr())
        _lib.call("art_flux_crop_bwd", x.device, None, None, None, B, rows, cols, *blur, None, None, None)
    assert (out == 7.0).all()
    wide = 65535 * 64 + 1
    for args in ((None, None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), None, out.data_ptr()),
                 (x.data_ptr(), None, None, 2, 4, 5, *blur, g.data_ptr(), None, out.data_ptr()),
                 (x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, None, None, out.data_ptr()),
                 (x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), None, None),
                 (x.data_ptr(), None, cov.data_ptr(), 2, 65536, 5, *blur, g.data_ptr(), None, out.data_ptr()),      # the forward's limits
                 (x.data_ptr(), None, cov.data_ptr(), 2, 1, wide, *blur, g.data_ptr(), None, out.data_ptr()),
                 (x.data_ptr(), None, cov.data_ptr(), 65536, 4, 5, *blur, g.data_ptr(), None, out.data_ptr()),
                 (x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), None, x.data_ptr()),             # overlaps
                 (x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), None, g.data_ptr()),
                 (x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), None, cov.data_ptr())):
        with pytest.raises(_lib.ArtistHipError, match="code"):
            _lib.call("art_flux_crop_bwd", x.device, *args)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # a gradient of the flux that is asked for is not touched either
    grad_flux = torch.full_like(x, 5.0)
    _lib.call("art_flux_crop_bwd", x.device, x.data_ptr(), None, cov.data_ptr(), 2, 4, 5, *blur, g.data_ptr(), grad_flux.data_ptr(),
              out.data_ptr())
    assert (grad_flux == 5.0).all() and torch.isfinite(out).all() and not (out == 7.0).any()


def test_the_crop_backward_is_unchanged():
    """The crop itself (target dimensions given): ``FluxCrop``'s gradient against the fp64 chain by the rule of
    tests/test_gpu_flux_fuzz.py - 3 x the fp32 oracle's distance, at least 2e-5, relative to the largest value."""
    case = next(c for c in flux_ref.CASES if (c.B, c.Hh, c.W) == (3, 33, 65))
    inp = flux_ref.make_inputs(case)
    a = gpu(inp["flux"]).requires_grad_(True)
    (FluxCrop.apply(a, gpu(inp["dims"]), flux_ref.CROP_W, flux_ref.CROP_H) * gpu(inp["grad_out"])).sum().backward()
    want, low = flux_ref.oracle_f64(case)["crop_grad"], flux_ref.oracle_f32(case)["crop_grad"]
    scale = np.abs(want).max()
    err, yard = np.abs(a.grad.double().cpu().numpy() - want).max() / scale, np.abs(low - want).max() / scale
    print("crop gradient: error", err, "yardstick", yard)
    assert err <= max(3.0 * yard, 2e-5)


def test_replay_gives_the_eager_bits():
    x, g, _, _ = small_case("dense")
    xs, gs = gpu(x), gpu(g)

    def step_on(leaf):
        def step():
            loss = (differentiable_blur_flux(xs, leaf) * gs).sum()
            loss.backward()
            return loss
        return step

    eager_leaf = gpu(COVARIANCES).requires_grad_(True)
    eager_loss = step_on(eager_leaf)().detach().clone()
    leaf = gpu(COVARIANCES).requires_grad_(True)                # a fresh leaf: the captured step's own
    graph = EpochGraph(step_on(leaf), warmup=2)
    for _ in range(3):
        loss = graph.replay()
        assert torch.equal(loss, eager_loss) and torch.equal(leaf.grad, eager_leaf.grad)


def test_sigma_recovery():
    """The optical error of one bitmap learns from its blurred image, on the operator alone: ``S = M sigma^2``, the target made
    with 1.5 mrad, Adam from 0.8 mrad.  The fp64 reference ends at 1.4929e-3 (tests/test_flux_blur_grad_host.py)."""
    setup = gref.RECOVERY
    x = gpu(gref.sparse_spot(np.random.default_rng(0))[None])
    metric = gpu(gref.RECOVERY_METRIC.astype(np.float32)[None])
    target = blur_flux(x, metric * setup["truth"] ** 2)
    sigma = torch.tensor(setup["start"], device="cuda", requires_grad=True)
    optimiser = torch.optim.Adam([sigma], lr=setup["lr"])
    for _ in range(setup["steps"]):
        optimiser.zero_grad()
        loss = 0.5 * ((differentiable_blur_flux(x, metric * sigma * sigma) - target) ** 2).sum()
        loss.backward()
        optimiser.step()
    print("sigma after", setup["steps"], "steps:", float(sigma.detach()))
    assert abs(float(sigma.detach()) - setup["truth"]) <= setup["bound"] * setup["truth"]
