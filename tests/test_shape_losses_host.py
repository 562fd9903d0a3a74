"""The gain-invariant flux losses without a GPU: the torch restatement (tests/shape_loss_ref.py) that the GPU test measures the
kernels by is pinned to the reference's own loss classes and to known answers, the input generator keeps its promises, and the
Python classes refuse what they document.

Restatement against ``tests/golden/shape_losses.npz`` (the reference's ``KLDivergenceLoss``, ``PixelLoss`` and
``CosineSimilarityLoss`` in fp64, tests/golden/generate_shape_losses_golden.py), both in fp64 on the same fp32 inputs; observed
largest |difference|, over all pairs:
    kind 2   3.6e-16 at values up to 0.51.  The classes normalise ``m``, ``p`` and ``g`` once more (a factor 1 + O(1e-16)) and form
             ``exp(log(g^ + eps))`` where the restatement has ``g^ + eps``.
    kind 3   4.4e-16 at values up to 3.2.  ``PixelLoss`` divides by ``sum(K g^) = K (1 + O(1e-16))`` and squares ``K p^ - K g^``.
    kind 5   0: the same torch call.
The bound is 1e-14 + 1e-13 |value|: a hundred roundings of the values' size, and ten orders below anything a wrong formula
gives."""
import math

import numpy as np
import pytest
import torch

import shape_loss_ref as ref

F64 = torch.float64


def test_restatement_matches_the_reference_classes(golden):
    d = golden("shape_losses")
    worst = {}
    for k, (B, Hh, W) in enumerate(d["shapes"]):
        p, g = torch.from_numpy(d[f"p_{k}"]).to(F64), torch.from_numpy(d[f"g_{k}"]).to(F64)
        assert p.shape == (B, Hh, W) and (p >= 0).all() and (g >= 0).all() and (p.sum((1, 2)) > 0).all() and (g.sum((1, 2)) > 0).all()
        for kind in (2, 3, 5):
            got, want = ref.loss(kind, p, g).numpy(), d[f"kind{kind}_{k}"]
            assert want.dtype == np.float64 and np.isfinite(want).all()
            err = np.abs(got - want)
            worst[kind] = max(worst.get(kind, 0.0), float(err.max()))
            print(f"{B}x{Hh}x{W} kind {kind}: largest |restatement - reference| {err.max():.2e}, values up to {np.abs(want).max():.3g}")
            assert (err <= 1e-14 + 1e-13 * np.abs(want)).all(), (kind, k, err.max())
        # the last pair is one shape at two gains: every loss is 0 up to rounding - and not by an empty comparison
        for kind in ref.KINDS:
            values = ref.loss(kind, p, g).numpy()
            assert abs(values[-1]) < 1e-12 and (Hh * W == 1 or values[:-1].min() > 1e-4), (kind, values)
    print("largest difference per kind:", worst)


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
@pytest.mark.parametrize("shape", sorted({(c.Hh, c.W) for c in ref.CASES}))
def test_known_answers(shape, dtype):
    """Disjoint one-hot bitmaps: JS = ln 2 within 1e-6, TV = 1, shape = 2 K, cosine = 1.  Equal bitmaps: JS = TV = shape = 0
    exactly.  In fp64 and in fp32, at every case's bitmap shape."""
    p, g = (torch.from_numpy(x).to(dtype) for x in ref.known_answer_inputs(*shape))
    K = shape[0] * shape[1]
    assert torch.equal(p[0], g[0]) and p.shape[0] == (2 if K > 1 else 1)
    for kind in ref.KINDS:
        values = ref.loss(kind, p, g).double().numpy()
        equal, one_hot = ref.known_answers(kind, K)
        if equal is None:
            assert abs(values[0]) < 1e-6
        else:
            assert values[0] == equal, (kind, values)
        if K > 1:
            if kind == 2:
                assert abs(values[1] - math.log(2.0)) < 1e-6
            else:
                assert values[1] == one_hot, (kind, values)


def test_bounds_and_the_empty_prediction():
    """An empty prediction costs about ln(2) / 2 under Jensen-Shannon where the KL divergence costs about 27.6; TV gives 1/2,
    the cosine loss 1; the gradient is finite."""
    g = torch.rand((1, 6, 5), dtype=F64, generator=torch.Generator().manual_seed(3)) + 0.1
    p = torch.zeros_like(g).requires_grad_(True)
    values = {kind: ref.loss(kind, p, g) for kind in ref.KINDS}
    at = {kind: float(value.detach()) for kind, value in values.items()}
    assert abs(at[2] - 0.5 * math.log(2.0)) < 1e-9 and at[4] == 0.5 and at[5] == 1.0
    gh = ref.unit_l1(g)
    kl = float(((gh + 1e-12) * (torch.log(gh + 1e-12) - math.log(1e-12))).sum())
    assert 20.0 < kl < 27.7
    for kind, value in values.items():
        (grad,) = torch.autograd.grad(value.sum(), p, retain_graph=True)
        assert torch.isfinite(grad).all(), kind


@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_generator_conditions(case):
    """Every non-zero pixel is positive; row 0 is empty, one row equals its truth (from three rows on), the one-hot pair lies on
    different pixels; and |p^ - g^| >= 1e-3 max g^ at every pixel of the random pairs, so that the kink of kind 4 cannot flip
    between fp32 and fp64.  The same arrays come back on every call."""
    margin = ref.check_generator_conditions(case)
    print(f"{ref.case_id(case)}: rows {ref.roles(case)[:5]}, smallest |p^ - g^| / max g^ over the random pairs {margin:.3g}")
    assert margin >= ref.KINK
    d = ref.make_inputs(case)
    assert d["prediction"].shape == (case.B, case.Hh, case.W) and d["prediction"].dtype == np.float32 and d["w"].shape == (case.B,)
    assert ref.make_inputs(case)["prediction"] is d["prediction"] and not d["prediction"].flags.writeable
    if case.B <= 5:                   # the fp32 run of kind 4 takes every pixel's sign as the fp64 run does
        p32, p64 = (ref.unit_l1(torch.tensor(d["prediction"]).to(t)) for t in (torch.float32, F64))
        g32, g64 = (ref.unit_l1(torch.tensor(d["truth"]).to(t)) for t in (torch.float32, F64))
        assert torch.equal(torch.sign(p32 - g32).double(), torch.sign(p64 - g64))


def test_case_table_is_the_documented_one():
    assert [(c.B, c.Hh, c.W, c.misaligned) for c in ref.CASES] == [
        (3, 1, 1, False), (3, 1, 3, False), (3, 2, 2, False), (2, 33, 17, False), (2, 3, 1366, False), (2, 4, 1028, False),
        (5, 8, 8, True), (65537, 1, 4, False)]


def test_gain_invariance_of_the_restatement():
    d = ref.make_inputs(ref.CASES[6])
    p, g = torch.tensor(d["prediction"]).to(F64), torch.tensor(d["truth"]).to(F64)
    for kind in ref.KINDS:
        a, b = ref.loss(kind, p, g), ref.loss(kind, 0.37 * p, 11.0 * g)
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-14), kind


CLASSES = {"JensenShannonLoss": ("Jensen-Shannon", 2), "ShapePixelLoss": ("shape pixel", 3), "TotalVariationLoss": ("total variation", 4),
           "CosineFluxLoss": ("cosine flux", 5)}


def test_classes_are_exported_and_refuse_what_they_document():
    import artist_amd
    from artist_amd import ArtistHipError, flux, losses, optim
    x = torch.rand(2, 4, 4)
    for name, (what, _) in CLASSES.items():
        cls = getattr(flux, name)
        for module in (artist_amd, optim, losses):
            assert getattr(module, name) is cls, (module.__name__, name)
        assert name in optim.__all__ and name in losses.__all__
        with pytest.raises(ValueError, match=f"The {what} loss expects 'reduction_dimensions' as keyword argument. Please add this argument."):
            cls()(x, x)
        with pytest.raises(NotImplementedError, match="reduce over the two bitmap dimensions"):
            cls()(x, x, reduction_dimensions=(1,))
        with pytest.raises(ArtistHipError, match="no CPU fallback"):
            cls()(x, x, reduction_dimensions=(1, 2))
        with pytest.raises(ArtistHipError, match="no CPU fallback"):
            cls()(prediction=x, ground_truth=x, target_area_indices=None, reduction_dimensions=(-2, -1), device=None)
    # the two losses the reference has keep their messages
    with pytest.raises(ValueError, match=r"The vector loss expects \['reduction_dimensions'\] as keyword arguments"):
        flux.PixelLoss()(x, x)
    with pytest.raises(ValueError, match="The KL-divergence loss expects 'reduction_dimensions' as keyword argument"):
        flux.KLDivergenceLoss()(x, x)


def test_the_aim_point_optimiser_takes_kl_and_jensen_shannon_only():
    from artist_amd import (CosineFluxLoss, JensenShannonLoss, KLDivergenceLoss, PixelLoss, ShapePixelLoss, TotalVariationLoss)
    from artist_amd.aim_point_optimizer import _require_kl
    _require_kl(KLDivergenceLoss())
    _require_kl(JensenShannonLoss())
    for cls in (PixelLoss, ShapePixelLoss, TotalVariationLoss, CosineFluxLoss):
        with pytest.raises(TypeError) as info:
            _require_kl(cls())
        assert str(info.value) == ("AimPointOptimizer defines its total loss (flux loss + flux-integral, intercept and local-flux "
                                   f"constraints) for artist_amd.KLDivergenceLoss only, got {cls.__name__}: with any "
                                   "other loss definition there is no loss to differentiate")
