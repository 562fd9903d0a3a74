"""The gain-invariant flux losses on the GPU (``-m gpu``): ``art_flux_loss`` kinds 2 to 5 through ``JensenShannonLoss``,
``ShapePixelLoss``, ``TotalVariationLoss`` and ``CosineFluxLoss`` against the torch restatement of tests/shape_loss_ref.py (pinned
to the reference's own classes by tests/test_shape_losses_host.py) at the shapes of ``shape_loss_ref.CASES`` - every branch of
``for_each_pair`` - and up through ``EpochGraph``, ``AimPointOptimizer`` and ``SurfaceReconstructor``.

Rule of every comparison with the restatement (the rule of tests/test_gpu_flux_fuzz.py, restated): the yardstick of a case and
quantity is the distance between the restatement's fp32 run and its fp64 run on that case, computed here; the HIP result must be
within ``max(3 x yardstick, floor)`` of the fp64 run, in relative L2 AND in the largest single entry (max |error| / max |reference|).
Floors: 1e-5 for losses, 2e-5 for gradients.  A gradient is checked over the whole batch, over the lit bitmaps and over the empty
bitmap 0 on its own (its entries are direct terms over a norm clamped at 1e-12, or at 1e-8 for the cosine: they would drown the
others in a norm).  Where the fp64 gradient of a set of rows is identically zero - a bitmap of ONE lit pixel has p^ = 1 whatever p
is, so the pixel's own part and the part through the norm cancel altogether - there is nothing to be relative to: the HIP result
must then be within the gradient floor of zero in units of the largest own part (``shape_loss_ref.own_part``), the size of the two
numbers whose roundings are left over.  Every comparison prints error, yardstick and error / bound.

What is exact is asserted exactly: gain by powers of two, rows of a batch against single calls, run to run, replay against eager,
``epoch_graph=True`` against the eager loop.
"""
import json
import math

import numpy as np
import pytest
import torch

import shape_loss_ref as ref
import test_gpu_aim_point as aim_point_suite
import test_gpu_surface_reconstructor as surface_suite
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MARGIN = 3.0
FLOOR_FIELD, FLOOR_LOSS = 2e-5, 1e-5
CASE_IDS = [ref.case_id(c) for c in ref.CASES]
KIND_IDS = [ref.KINDS[k] for k in ref.KINDS]
BOTH = dict(reduction_dimensions=(1, 2))


def classes():
    from artist_amd import CosineFluxLoss, JensenShannonLoss, ShapePixelLoss, TotalVariationLoss
    return {2: JensenShannonLoss, 3: ShapePixelLoss, 4: TotalVariationLoss, 5: CosineFluxLoss}


def t(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def bits(x):
    return n(x).view(np.uint32)


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def check(tag, what, got, ref64, ref32, floor, own=None):
    """``got`` against the restatement's fp64 result by the rule of the module docstring; the list of what failed."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape and np.isfinite(got).all(), (tag, what)
    failures = []
    if not ref64.any():
        assert own is not None and own.any(), (tag, what)
        err, bound = float(np.abs(got).max()), floor * float(np.abs(own).max())
        print(f"{tag} {what:34s} zero reference: largest |entry| {err:.2e}, largest own part {np.abs(own).max():.2e}, bound {bound:.2e}")
        return [] if err <= bound else [(what, "zero", err, bound)]
    for norm, fn in (("L2", rel_l2), ("max", max_rel)):
        err, yard = fn(got, ref64), fn(ref32, ref64)
        bound = max(MARGIN * yard, floor)
        print(f"{tag} {what:34s} {norm:3s} error {err:.2e} yardstick {yard:.2e} error/bound {err / bound:.3f}")
        if not err <= bound:
            failures.append((what, norm, err, yard, bound))
    return failures


def device_inputs(case):
    """The case's tensors on the device.  The prediction is a leaf; what the loss is handed is the leaf itself, or - a misaligned
    case - a contiguous view that starts 4 bytes into a buffer of its own."""
    d = ref.make_inputs(case)
    leaf = t(d["prediction"]).requires_grad_(True)
    handed = leaf
    if case.misaligned:
        handed = torch.cat((torch.zeros(1, device=DEV), leaf.reshape(-1)))[1:].view(leaf.shape)
        assert handed.is_contiguous() and handed.data_ptr() % 16 == 4
    else:
        assert leaf.data_ptr() % 16 == 0
    truth = t(d["truth"])
    assert truth.data_ptr() % 16 == 0
    return leaf, handed, truth, t(d["w"])


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=KIND_IDS)
@pytest.mark.parametrize("case", ref.CASES, ids=CASE_IDS)
def test_loss_and_gradient_vs_restatement(case, kind):
    """Loss and gradient (upstream weights ``w[B]``) of every case and kind through the Python classes.  Measured on an MI355X:
    the largest error / bound is 0.14 (1 x 3 pixels, cosine gradient of the lit bitmaps: 2.7e-6 against the floor); every
    other error is below 3e-7."""
    leaf, handed, truth, w = device_inputs(case)
    loss = classes()[kind]()(handed, truth, **BOTH)
    (loss * w).sum().backward()
    (l64, g64), (l32, g32) = ref.reference(case, kind, 64), ref.reference(case, kind, 32)
    own = ref.own_part(case, kind)
    tag = f"{ref.case_id(case)} {ref.KINDS[kind]}"
    grad = n(leaf.grad)
    bad = check(tag, "loss", n(loss), l64, l32, FLOOR_LOSS)
    bad += check(tag, "gradient", grad, g64, g32, FLOOR_FIELD)
    bad += check(tag, "gradient, lit bitmaps", grad[1:], g64[1:], g32[1:], FLOOR_FIELD, own[1:])
    bad += check(tag, "gradient, empty bitmap", grad[:1], g64[:1], g32[:1], FLOOR_FIELD, own[:1])
    assert not bad, bad
    roles = ref.roles(case)
    if ref.EQUAL in roles and kind != 5:              # an equal pair costs nothing and pulls nowhere, exactly
        row = roles.index(ref.EQUAL)
        assert n(loss)[row] == 0.0 and not grad[row].any()


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=KIND_IDS)
def test_known_answers_at_every_shape(kind):
    """An equal pair and a pair of one-hot bitmaps on different pixels at every case's bitmap shape: JS = TV = shape = 0 exactly
    and the cosine loss 0 within 1e-6 for the first; JS = ln 2 within 1e-6, TV = 1, shape = 2 K, cosine = 1 for the second."""
    for Hh, W in sorted({(c.Hh, c.W) for c in ref.CASES}):
        p, g = (t(x) for x in ref.known_answer_inputs(Hh, W))
        values = n(classes()[kind]()(p, g, **BOTH)).astype(np.float64)
        equal, one_hot = ref.known_answers(kind, Hh * W)
        print(f"{Hh}x{W} {ref.KINDS[kind]}: {values}")
        assert abs(values[0]) < 1e-6 if equal is None else values[0] == equal
        if Hh * W > 1:
            assert abs(values[1] - math.log(2.0)) < 1e-6 if kind == 2 else values[1] == one_hot


def _run(kind, p, g, w):
    leaf = p.detach().clone().requires_grad_(True)
    loss = classes()[kind]()(leaf, g, **BOTH)
    (loss * w).sum().backward()
    return loss.detach(), leaf.grad


GAIN_CASES = [ref.CASES[5], ref.CASES[3], ref.CASES[2]]          # the float4 loop, the scalar loop, one float4 with its equal pair


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=KIND_IDS)
@pytest.mark.parametrize("case", GAIN_CASES, ids=[ref.case_id(c) for c in GAIN_CASES])
def test_gain_invariance(case, kind):
    """``L(4 p, g / 2)`` has the bits of ``L(p, g)`` and its gradient is exactly a quarter of the original in every lit bitmap
    (powers of two commute with every rounding of the kernel); ``L(0.37 p, g)`` agrees with the restatement of ``L(p, g)`` within
    the loss bound."""
    d = ref.make_inputs(case)
    p, g, w = t(d["prediction"]), t(d["truth"]), t(d["w"])
    loss, grad = _run(kind, p, g, w)
    scaled_loss, scaled_grad = _run(kind, 4.0 * p, 0.5 * g, w)
    np.testing.assert_array_equal(bits(scaled_loss), bits(loss))
    np.testing.assert_array_equal(bits(scaled_grad[1:]), bits(0.25 * grad[1:]))
    # (the empty prediction is the same input at every gain, its norm the same clamp: the same gradient)
    np.testing.assert_array_equal(bits(scaled_grad[:1]), bits(grad[:1]))
    assert float(grad[1:].abs().max()) > 0
    other, _ = _run(kind, (0.37 * p), g, w)
    l64, l32 = ref.reference(case, kind, 64)[0], ref.reference(case, kind, 32)[0]
    bad = check(f"{ref.case_id(case)} {ref.KINDS[kind]}", "loss at gain 0.37", n(other), l64, l32, FLOOR_LOSS)
    assert not bad, bad


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=KIND_IDS)
def test_batch_independence_and_determinism(kind):
    """Row ``i`` of a ``B = 5`` call has the bits of a ``B = 1`` call on that bitmap (a view of the same memory: the same
    alignment, hence the same loop), loss and gradient; a second run gives the same bits."""
    case = ref.CASES[6]
    assert case.B == 5
    d = ref.make_inputs(case)
    p, g, w = t(d["prediction"]), t(d["truth"]), t(d["w"])
    loss, grad = _run(kind, p, g, w)
    again = _run(kind, p, g, w)
    np.testing.assert_array_equal(bits(again[0]), bits(loss))
    np.testing.assert_array_equal(bits(again[1]), bits(grad))
    for i in range(case.B):
        cls = classes()[kind]()
        leaf = p.detach().clone().requires_grad_(True)
        one = cls(leaf[i:i + 1], g[i:i + 1], **BOTH)
        (one * w[i:i + 1]).sum().backward()
        np.testing.assert_array_equal(bits(one), bits(loss[i:i + 1]), err_msg=f"loss of row {i}")
        np.testing.assert_array_equal(bits(leaf.grad[i]), bits(grad[i]), err_msg=f"gradient of row {i}")
        assert not leaf.grad[:i].any() and not leaf.grad[i + 1:].any()


def test_invalid_kinds_and_the_empty_batch():
    """``kind = 6`` and ``kind = -1`` are ART_EINVAL and write nothing; ``B = 0`` is ART_OK for kinds 2 to 5 with null pointers;
    forward-only and backward-only calls follow the rule of kinds 0 and 1; the classes return empty results on an empty batch."""
    from artist_amd import _lib
    handle = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    p, g = torch.rand((2, 4, 4), device=DEV) + 0.1, torch.rand((2, 4, 4), device=DEV) + 0.1
    loss, grad, gl = torch.full((2,), -7.0, device=DEV), torch.full((2, 4, 4), -7.0, device=DEV), torch.ones(2, device=DEV)
    q = lambda x: x.data_ptr()  # noqa: E731
    for kind in (6, -1):
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, q(loss), q(gl), q(grad), stream) == _lib.ART_EINVAL
        assert handle.art_flux_loss(None, None, 0, 16, kind, None, None, None, stream) == _lib.ART_EINVAL
    torch.cuda.synchronize()
    assert (loss == -7.0).all() and (grad == -7.0).all()
    for kind in ref.KINDS:
        assert handle.art_flux_loss(None, None, 0, 16, kind, None, None, None, stream) == _lib.ART_OK
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, None, None, None, stream) == _lib.ART_EINVAL       # nothing asked for
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, q(loss), None, q(grad), stream) == _lib.ART_EINVAL  # no upstream gradient
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, q(loss), None, None, stream) == _lib.ART_OK
        torch.cuda.synchronize()
        assert (grad == -7.0).all() and (loss != -7.0).all()
        forward = loss.clone()
        loss.fill_(-7.0)
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, None, q(gl), q(grad), stream) == _lib.ART_OK
        torch.cuda.synchronize()
        assert (loss == -7.0).all() and (grad != -7.0).all()
        assert handle.art_flux_loss(q(p), q(g), 2, 16, kind, q(loss), q(gl), q(grad), stream) == _lib.ART_OK     # both at once
        torch.cuda.synchronize()
        np.testing.assert_array_equal(bits(loss), bits(forward))
        loss.fill_(-7.0)
        grad.fill_(-7.0)
        empty = torch.zeros((0, 4, 4), device=DEV, requires_grad=True)
        out = classes()[kind]()(empty, torch.zeros((0, 4, 4), device=DEV), **BOTH)
        out.sum().backward()
        assert out.shape == (0,) and empty.grad.shape == (0, 4, 4)


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=KIND_IDS)
def test_epoch_graph_replay_gives_the_eager_bits(kind):
    """One step - loss plus backward - per class, captured into an ``EpochGraph`` and replayed twice, against the eager step."""
    from artist_amd import EpochGraph, ops
    d = ref.make_inputs(ref.CASES[3])
    g, w = t(d["truth"]), t(d["w"])
    cls = classes()[kind]()
    leaf = t(d["prediction"]).requires_grad_(True)

    def step():
        loss = cls(leaf, g, **BOTH)
        (loss * w).sum().backward()
        return loss

    graph = EpochGraph(step, warmup=2)
    for _ in range(2):
        replayed = graph.replay()
        replayed_loss, replayed_grad = replayed.detach().clone(), leaf.grad.detach().clone()
    torch.cuda.synchronize()
    graph.close()
    loss, grad = _run(kind, t(d["prediction"]), g, w)
    ops.check_async_errors(DEV)
    np.testing.assert_array_equal(bits(replayed_loss), bits(loss))
    np.testing.assert_array_equal(bits(replayed_grad), bits(grad))
    assert float(grad.abs().max()) > 0


def test_aim_point_optimizer_with_jensen_shannon(golden):
    """The scenario of tests/test_gpu_aim_point.py with ``JensenShannonLoss``: the flux-loss term of an epoch is the restatement's
    on that epoch's total flux, within the loss bound; the gradient reaches the motor parameters; ``optimize()`` for three epochs
    returns finite histories; any other new class is still refused."""
    from artist_amd import JensenShannonLoss, TotalVariationLoss
    d = golden("aim_point_optimizer_epochs")
    optimizer, _ = aim_point_suite._optimizer(d)
    optimizer.prepare(DEV)
    total, flux_loss, _, total_flux, _ = optimizer.epoch_loss(JensenShannonLoss(), DEV)
    total.backward()
    flux, truth = n(total_flux)[None], np.asarray(d["ground_truth"], np.float32)[None]
    one = np.ones(1, np.float32)
    l64 = ref.loss_and_gradient(2, flux, truth, one, torch.float64)[0]
    l32 = ref.loss_and_gradient(2, flux, truth, one, torch.float32)[0]
    bad = check("aim point", "flux loss (Jensen-Shannon)", n(flux_loss), l64, l32, FLOOR_LOSS)
    assert not bad, bad
    assert 0.0 < float(flux_loss.detach()) < math.log(2.0)
    grad = optimizer.groups[0]["parameter"].grad
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    with pytest.raises(TypeError, match="for artist_amd.KLDivergenceLoss only, got TotalVariationLoss"):
        optimizer.epoch_loss(TotalVariationLoss(), DEV)
    optimizer, _ = aim_point_suite._optimizer(d, max_epoch=2)
    final_loss, history, *_ = optimizer.optimize(loss_definition=JensenShannonLoss(), device=DEV)
    print("total loss per epoch:", history["total_loss"], " flux loss:", history["flux_loss"])
    assert all(len(v) == 3 and all(math.isfinite(x) for x in v) for v in history.values())
    assert all(0.0 < x < math.log(2.0) for x in history["flux_loss"]) and math.isfinite(float(final_loss))


def test_surface_reconstructor_with_shape_pixel_loss(golden):
    """Two epochs of ``SurfaceReconstructor`` with ``ShapePixelLoss`` on the scenario of tests/test_gpu_surface_reconstructor.py,
    eagerly and with ``epoch_graph=True``: the same histories, final losses and control points, bit for bit."""
    from artist_amd import ShapePixelLoss
    d = golden(surface_suite.NAME)
    runs = []
    for epoch_graph in (False, True):
        configuration = json.loads(str(d["configuration"]))
        configuration["optimization"].update(max_epoch=1)
        reconstructor, scenario = surface_suite._reconstructor(d, configuration)
        reconstructor.epoch_graph = epoch_graph
        start = scenario.heliostat_field.heliostat_groups[0].nurbs_control_points.detach().clone()
        final_loss, histories = reconstructor.reconstruct_surfaces(loss_definition=ShapePixelLoss(), device=DEV)
        torch.cuda.synchronize()
        runs.append((final_loss, histories[0][0], scenario.heliostat_field.heliostat_groups[0].nurbs_control_points.detach().clone(), start))
    (loss_e, history_e, points_e, start), (loss_r, history_r, points_r, _) = runs
    print("total loss per epoch:", history_e["total_loss"], " flux loss:", history_e["flux_loss"])
    assert set(history_e) == set(history_r) == surface_suite.HISTORY_KEYS
    for key in sorted(surface_suite.HISTORY_KEYS - {"test_loss"}):
        assert len(history_e[key]) == 2 and all(math.isfinite(x) for x in history_e[key]), key
        assert history_e[key] == history_r[key], (key, history_e[key], history_r[key])
    for key in history_e["test_loss"]:
        assert torch.equal(history_e["test_loss"][key], history_r["test_loss"][key]), key
    assert torch.equal(loss_e, loss_r) and torch.equal(points_e, points_r)
    sampled = torch.as_tensor(d["parser_mask"]) > 0
    assert torch.isfinite(loss_e[sampled]).all() and not torch.equal(points_e, start)
    assert all(x > 0 for x in history_e["flux_loss"])
