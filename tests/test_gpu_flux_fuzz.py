"""GPU fuzz (``-m gpu``) of the flux epilogue - ``art_flux_crop_fwd/bwd``, ``art_flux_loss``, the fused
``art_flux_crop_pixel_loss_*`` and ``art_flux_crop_kl_loss_*`` and ``art_flux_center_of_mass*`` - against the C oracle's fp64 chain
(pinned to a torch fp64 autograd restatement by tests/test_flux_reference_host.py) at the shapes of ``flux_ref.CASES``: every branch
of artist_amd/csrc/flux_kernels.hip that depends on the shape, the crop scale or the batch size.  Everything goes through the
Python classes, which go through the C ABI.

Rule of every comparison: the yardstick of a case and quantity is the distance between the oracle's fp32 run (the reference's own
arithmetic) and its fp64 run on that case, computed here; the HIP result must be within ``max(3 x yardstick, floor)`` of the fp64
run, in relative L2 AND in the largest single entry (max |error| / max |reference|: one wrong column cannot hide in a norm).  The
floors are the ones the suite already asserts for these ops - 2e-5 for crops and gradients
(test_gpu_parity.py::test_flux_crop_known_answers_and_autograd), 1e-5 for losses (test_flux_losses) - and the factor 3 is the
margin test_fused_crop_kl_loss grants for kink flips between two fp32 evaluations.  Every test prints error, yardstick and
error / bound per quantity.

Measured on an MI355X, over the 29 cases and every quantity (2 030 comparisons): the largest error / bound is 0.341 (3x64x64 at
scale 2, largest entry of the KL gradient: error 1.57e-5, yardstick 1.53e-5), i.e. wherever the yardstick and not the floor sets
the bound the HIP result is at most 1.02 yardsticks from the fp64 run; under the floors the largest error / yardstick is 3.9 (KL
loss of the 2 x 2 bitmaps: error 9.7e-8 against the floor of 1e-5).
"""
import numpy as np
import pytest
import torch

import flux_ref
from conftest import rel_l2
from flux_ref import CROP_H, CROP_W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MARGIN = 3.0
FLOOR_FIELD, FLOOR_LOSS = 2e-5, 1e-5
CASE_IDS = [flux_ref.case_id(c) for c in flux_ref.CASES]

_worst = {"ratio": 0.0, "what": ""}


def t(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(case, what, got, key, floor, rows=slice(None)):
    """``got`` against the oracle's fp64 ``key`` of the case (optionally some bitmaps only) by the rule of the module docstring."""
    ref64, ref32 = flux_ref.oracle_f64(case)[key][rows], flux_ref.oracle_f32(case)[key][rows]
    got = np.asarray(got)[rows]
    assert got.shape == ref64.shape and np.isfinite(got).all(), what
    failures = []
    for norm, fn in (("L2", rel_l2), ("max", max_rel)):
        err, yard = fn(got, ref64), fn(ref32, ref64)
        bound = max(MARGIN * yard, floor)
        ratio = err / bound
        if ratio > _worst["ratio"]:
            _worst.update(ratio=ratio, what=f"{flux_ref.case_id(case)} {what} {norm}")
        print(f"{flux_ref.case_id(case)} {what:46s} {norm:3s} error {err:.2e} yardstick {yard:.2e} error/yardstick "
              f"{err / max(yard, 1e-300):9.2e} error/bound {ratio:.3f}   [worst so far {_worst['ratio']:.3f}: {_worst['what']}]")
        if not err <= bound:
            failures.append((what, norm, err, yard, bound))
    return failures


def check_gradient(case, what, got, key):
    """A gradient w.r.t. the bitmaps: the whole batch, the lit bitmaps and the empty bitmap 0 each by the rule (the empty bitmap's
    KL gradient is all -P / 1e-12 terms and would drown the others in a norm over the batch)."""
    return (check(case, what, got, key, FLOOR_FIELD) + check(case, what + ", lit bitmaps", got, key, FLOOR_FIELD, rows=slice(1, None))
            + check(case, what + ", empty bitmap", got, key, FLOOR_FIELD, rows=slice(0, 1)))


def inputs(case):
    inp = flux_ref.make_inputs(case)
    return {k: t(v) for k, v in inp.items()}


@pytest.mark.parametrize("case", flux_ref.CASES, ids=CASE_IDS)
def test_unfused_ops_vs_fp64_chain(case):
    """FluxCrop forward and backward (random upstream gradient), PixelLoss and KLDivergenceLoss on the crop with the gradient
    taken back to the bitmaps, the two losses on a prediction of their own, and get_center_of_mass forward and backward."""
    from artist_amd import KLDivergenceLoss, PixelLoss, get_center_of_mass
    from artist_amd.flux import FluxCrop
    d = inputs(case)
    bad = []
    a = d["flux"].clone().requires_grad_(True)
    crop = FluxCrop.apply(a, d["dims"], CROP_W, CROP_H)
    (crop * d["grad_out"]).sum().backward()
    bad += check(case, "crop", n(crop), "crop", FLOOR_FIELD)
    bad += check_gradient(case, "crop gradient", n(a.grad), "crop_grad")
    assert not n(crop)[0].any()
    for name, cls in (("pixel", PixelLoss), ("kl", KLDivergenceLoss)):
        a = d["flux"].clone().requires_grad_(True)
        loss = cls()(FluxCrop.apply(a, d["dims"], CROP_W, CROP_H), d["truth"], reduction_dimensions=(1, 2))
        (loss * d["w"]).sum().backward()
        bad += check(case, f"{name} loss of the crop", n(loss), name, FLOOR_LOSS)
        bad += check_gradient(case, f"{name} gradient", n(a.grad), name + "_grad")
        p = (d["flux"] + 0.05).requires_grad_(True)
        loss = cls()(p, d["truth"], reduction_dimensions=(1, 2))
        (loss * d["w"]).sum().backward()
        bad += check(case, f"{name} loss (art_flux_loss)", n(loss), "direct_" + name, FLOOR_LOSS)
        bad += check(case, f"{name} loss gradient (art_flux_loss)", n(p.grad), "direct_" + name + "_grad", FLOOR_FIELD)
    a = d["flux"].clone().requires_grad_(True)
    com = get_center_of_mass(a)
    (com * d["grad_com"]).sum().backward()
    bad += check(case, "centre of mass", n(com), "com", FLOOR_FIELD)
    # (the empty bitmap's gradient is (index - 0) / 1e-8: checked on its own, it would drown the others)
    bad += check(case, "centre of mass gradient", n(a.grad), "com_grad", FLOOR_FIELD, rows=slice(1, None))
    bad += check(case, "centre of mass gradient, empty bitmap", n(a.grad), "com_grad", FLOOR_FIELD, rows=slice(0, 1))
    assert not n(com)[0].any()                                             # the empty bitmap -> (0, 0)
    assert not bad, bad


def _fused(cls, d, weighted):
    a = d["flux"].clone().requires_grad_(True)
    loss = cls.apply(a, d["dims"], d["truth"], CROP_W, CROP_H)
    ((loss * d["w"]).sum() if weighted else loss.sum()).backward()
    return n(loss), n(a.grad)


@pytest.mark.parametrize("case", flux_ref.CASES, ids=CASE_IDS)
def test_fused_crop_pixel_loss_vs_fp64_chain(case, monkeypatch):
    """FluxCropPixelLoss against the fp64 chain (not against the unfused HIP ops), with the gradient of ``loss.sum()`` (an
    expanded scalar, stride 0) and of a weighted sum (stride 1); and the same loss bits and gradient bits with the number of
    workgroups per bitmap left to the library and forced to 1, 2 and 4, from run to run, and from a forward-only call."""
    from artist_amd.flux import FluxCropPixelLoss
    monkeypatch.setenv("ARTIST_HIP_DEBUG", "1")
    monkeypatch.delenv("ARTIST_HIP_LOSS_PARTS", raising=False)
    d = inputs(case)
    bad = []
    first = {}
    for parts in (None, "1", "2", "4", None):
        if parts is None:
            monkeypatch.delenv("ARTIST_HIP_LOSS_PARTS", raising=False)
        else:
            monkeypatch.setenv("ARTIST_HIP_LOSS_PARTS", parts)
        for weighted in (False, True):
            loss, grad = _fused(FluxCropPixelLoss, d, weighted)
            if weighted not in first:
                first[weighted] = (loss, grad)
                tag = "weighted sum" if weighted else "loss.sum()"
                bad += check(case, f"fused pixel loss ({tag})", loss, "pixel", FLOOR_LOSS)
                key = "pixel_grad" if weighted else "pixel_sum_grad"
                bad += check_gradient(case, f"fused pixel gradient ({tag})", grad, key)
            np.testing.assert_array_equal(loss, first[weighted][0], err_msg=f"loss bits, parts {parts}")
            np.testing.assert_array_equal(grad, first[weighted][1], err_msg=f"gradient bits, parts {parts}")
        with torch.no_grad():                                    # forward only (no residual kept)
            only = n(FluxCropPixelLoss.apply(d["flux"], d["dims"], d["truth"], CROP_W, CROP_H))
        np.testing.assert_array_equal(only, first[True][0], err_msg=f"forward-only loss bits, parts {parts}")
    np.testing.assert_array_equal(first[False][0], first[True][0])
    assert not bad, bad


@pytest.mark.parametrize("case", flux_ref.CASES, ids=CASE_IDS)
def test_fused_crop_kl_loss_vs_fp64_chain(case):
    """FluxCropKLLoss against the fp64 chain; crops with exact zeros (spots cut by the border, zoom-out) bring log(0 + 1e-12)
    terms.  Deterministic: the same bits on a second run."""
    from artist_amd.flux import FluxCropKLLoss
    d = inputs(case)
    bad = []
    for weighted in (False, True):
        loss, grad = _fused(FluxCropKLLoss, d, weighted)
        tag = "weighted sum" if weighted else "loss.sum()"
        key = "kl_grad" if weighted else "kl_sum_grad"
        bad += check(case, f"fused KL loss ({tag})", loss, "kl", FLOOR_LOSS)
        bad += check_gradient(case, f"fused KL gradient ({tag})", grad, key)
        again = _fused(FluxCropKLLoss, d, weighted)
        np.testing.assert_array_equal(again[0], loss)
        np.testing.assert_array_equal(again[1], grad)
    assert not bad, bad


# the centre-of-mass loops and the two shapes at which the scalar loop runs in more than one trip (33 x 65 and 33 x 17 pixels on
# 1024 threads): the scalar loop, the float4 loop with W / 4 above and below the block size, and the remainder case
ONE_ROUTINE = flux_ref.CENTRE_LOOPS + [c for c in flux_ref.CASES if (c.B, c.Hh, c.W) in ((3, 33, 65), (2, 33, 17))]


@pytest.mark.parametrize("case", ONE_ROUTINE, ids=[flux_ref.case_id(c) for c in ONE_ROUTINE])
def test_crop_and_fused_kl_form_the_same_centre_bits(case):
    """The unfused crop and the fused crop + KL loss form a bitmap's centre of mass with one routine: ``centers`` of
    ``art_flux_crop_fwd`` and the first three floats of each ``record8`` row of ``art_flux_crop_kl_loss_fwd`` are the same bits."""
    from artist_amd import _lib
    assert len(ONE_ROUTINE) == 5
    d = inputs(case)
    B, Hh, W = d["flux"].shape
    crop, centers = torch.empty_like(d["flux"]), torch.empty((B, 3), device=DEV)
    loss, record8 = torch.empty(B, device=DEV), torch.empty((B, 8), device=DEV)
    p = lambda x: x.data_ptr()
    _lib.call("art_flux_crop_fwd", DEV, p(d["flux"]), p(d["dims"]), B, Hh, W, CROP_W, CROP_H, p(crop), p(centers))
    _lib.call("art_flux_crop_kl_loss_fwd", DEV, p(d["flux"]), p(d["dims"]), p(d["truth"]), B, Hh, W, CROP_W, CROP_H, p(loss), p(record8))
    np.testing.assert_array_equal(n(centers).view(np.uint32), np.ascontiguousarray(n(record8)[:, :3]).view(np.uint32))


def test_empty_batch_returns_cleanly():
    """B = 0 (a rank without an active heliostat): every entry point returns ART_OK without a launch, given valid pointers or
    the null pointers of empty tensors; the Python classes return empty results and empty gradients."""
    from artist_amd import KLDivergenceLoss, PixelLoss, _lib, get_center_of_mass
    from artist_amd.flux import FluxCrop, FluxCropKLLoss, FluxCropPixelLoss
    buf = torch.zeros(64, device=DEV)
    p, z = buf.data_ptr(), None
    for q in (p, z):
        _lib.call("art_flux_crop_fwd", DEV, q, q, 0, 8, 8, 6.0, 5.0, q, q)
        _lib.call("art_flux_crop_bwd", DEV, q, q, q, 0, 8, 8, 6.0, 5.0, q, q, q)
        for kind in (0, 1):
            _lib.call("art_flux_loss", DEV, q, q, 0, 64, kind, q, q, q)
        _lib.call("art_flux_crop_pixel_loss_fwd", DEV, q, q, q, 0, 8, 8, 6.0, 5.0, q, q, q, q, None)
        _lib.call("art_flux_crop_pixel_loss_fwd", DEV, q, q, q, 0, 8, 8, 6.0, 5.0, q, q, None, None, None)
        _lib.call("art_flux_crop_pixel_loss_bwd", DEV, q, q, q, 0, q, q, 0, 8, 8, 6.0, 5.0, q)
        _lib.call("art_flux_crop_kl_loss_fwd", DEV, q, q, q, 0, 8, 8, 6.0, 5.0, q, q)
        _lib.call("art_flux_crop_kl_loss_bwd", DEV, q, q, q, q, q, 0, 8, 8, 6.0, 5.0, q, q)
        _lib.call("art_flux_center_of_mass", DEV, q, 0, 8, 8, q)
        _lib.call("art_flux_center_of_mass_bwd", DEV, q, q, 0, 8, 8, q)
    torch.cuda.synchronize()
    assert not n(buf).any()
    empty = torch.zeros((0, 8, 8), device=DEV)
    dims = torch.zeros((0, 2), device=DEV)
    for fn in (lambda a: FluxCrop.apply(a, dims, CROP_W, CROP_H),
               lambda a: PixelLoss()(a, empty, reduction_dimensions=(1, 2)),
               lambda a: KLDivergenceLoss()(a, empty, reduction_dimensions=(1, 2)),
               lambda a: FluxCropPixelLoss.apply(a, dims, empty, CROP_W, CROP_H),
               lambda a: FluxCropKLLoss.apply(a, dims, empty, CROP_W, CROP_H),
               get_center_of_mass):
        a = empty.clone().requires_grad_(True)
        out = fn(a)
        assert out.shape[0] == 0
        out.sum().backward()
        assert a.grad.shape == (0, 8, 8)
    torch.cuda.synchronize()
