"""torch (CPU) restatement of the four gain-invariant flux losses - ``art_flux_loss`` kinds 2 to 5, the classes
``JensenShannonLoss``, ``ShapePixelLoss``, ``TotalVariationLoss`` and ``CosineFluxLoss`` of artist_amd/flux.py - written from the
formulas of include/artist_hip.h and differentiated by autograd, in fp64 and in fp32, plus the case table and the seeded input
generator that tests/test_shape_losses_host.py and tests/test_gpu_shape_losses.py share.

Per bitmap of ``K`` pixels, prediction ``p``, truth ``g``, ``eps = 1e-12``; ``p^ = p / max(sum |p|, eps)`` and ``g^`` likewise, formed
with ``torch.nn.functional.normalize(p=1, eps=eps)`` as the reference's KLDivergenceLoss forms them (artist/optim/loss.py:391-403):

    kind 2  Jensen-Shannon   m = (p^ + g^) / 2;  1/2 sum (g^ + eps)(log(g^ + eps) - log(m + eps)) + 1/2 sum (p^ + eps)(log(p^ + eps) - log(m + eps))
    kind 3  shape pixel      K sum (p^ - g^)^2            (the reference's PixelLoss of both bitmaps scaled to unit mean)
    kind 4  total variation  1/2 sum |p^ - g^|            (no reference counterpart: this restatement is its definition)
    kind 5  cosine           1 - torch.nn.functional.cosine_similarity(p, g, eps=1e-8) over the flattened bitmaps, no L1 normalisation

The host test pins kinds 2, 3 and 5 to values the reference's own classes gave (tests/golden/shape_losses.npz); the GPU test then
measures the HIP kernel against the fp64 run of this restatement, with the distance between its fp32 and fp64 runs as the yardstick.

A case's rows, as far as its ``B`` goes: row 0 has an EMPTY prediction, row 1 is a random pair (positive pixels, exact zeros at
different pixels of the two bitmaps), row 2 a prediction EQUAL to its truth, row 3 a pair of ONE-HOT bitmaps on different pixels, the
rest random pairs.  The random pair comes before the two known answers because a case of two or three bitmaps is in the table for the
loop its shape reaches, and an equal pair (every term 0) would not show a pixel the loop skipped; ``known_answer_inputs`` gives the
equal and the one-hot pair at every case's bitmap shape, so that each shape meets all four.  A bitmap of one pixel has no two
different pixels: its random pair is a lit prediction against a dark truth, and it has no one-hot pair.
"""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12
COSINE_EPS = 1e-8
KINDS = {2: "jensen_shannon", 3: "shape_pixel", 4: "total_variation", 5: "cosine"}
KINK = 1e-3                 # kind 4: |p^ - g^| >= KINK * max g^ at every pixel of a random pair
_KINK_MARGIN = 2e-3         # what the generator asks of the pairs it accepts

Case = collections.namedtuple("Case", "B Hh W misaligned note")

# for_each_pair of artist_amd/csrc/flux_kernels.hip: 1024 lanes; four pixels per load when npix % 4 == 0 and both bitmaps are
# 16-byte aligned
CASES = [
    Case(3, 1, 1, False, "a single pixel"),
    Case(3, 1, 3, False, "scalar path, fewer pixels than a wave"),
    Case(3, 2, 2, False, "one float4"),
    Case(2, 33, 17, False, "scalar path, npix % 4 != 0"),
    Case(2, 3, 1366, False, "the scalar loop wraps"),
    Case(2, 4, 1028, False, "the float4 loop wraps"),
    Case(5, 8, 8, True, "npix % 4 == 0, but the prediction starts 4 bytes into its buffer: scalar path"),
    Case(65537, 1, 4, False, "more than 2^16 bitmaps"),
]
EMPTY, RANDOM, EQUAL, ONE_HOT = "empty", "random", "equal", "one-hot"


def case_id(case):
    return f"{case.B}x{case.Hh}x{case.W}" + ("-misaligned" if case.misaligned else "")


def roles(case):
    """What each row of the case is (module docstring)."""
    first = [EMPTY, RANDOM, EQUAL] + ([ONE_HOT] if case.Hh * case.W > 1 else [RANDOM])
    return (first + [RANDOM] * max(case.B - 4, 0))[:case.B]


# ------------------------------------------------------------------------------------------------
# the four losses
# ------------------------------------------------------------------------------------------------
def unit_l1(x):
    return F.normalize(x, p=1, dim=(1, 2), eps=EPS)


def loss(kind, prediction, ground_truth, norm_path=True):
    """``[B,Hh,W]`` x 2 -> ``[B]`` in the dtype of the arguments.  ``norm_path=False``: the same values with the prediction's norm
    held constant under autograd - the gradient is then each pixel's own part, without the part through the norm."""
    if kind == 5:
        if norm_path:
            return 1.0 - F.cosine_similarity(prediction.flatten(1), ground_truth.flatten(1), dim=1, eps=COSINE_EPS)
        p, g = prediction.flatten(1), ground_truth.flatten(1)
        return 1.0 - ((p / p.norm(dim=1, keepdim=True).clamp(min=COSINE_EPS).detach())
                      * (g / g.norm(dim=1, keepdim=True).clamp(min=COSINE_EPS))).sum(dim=1)
    p = unit_l1(prediction) if norm_path else prediction / prediction.abs().sum(dim=(1, 2), keepdim=True).clamp(min=EPS).detach()
    g = unit_l1(ground_truth)
    if kind == 2:
        log_m = torch.log(0.5 * (p + g) + EPS)
        return 0.5 * ((g + EPS) * (torch.log(g + EPS) - log_m)).sum(dim=(1, 2)) \
            + 0.5 * ((p + EPS) * (torch.log(p + EPS) - log_m)).sum(dim=(1, 2))
    if kind == 3:
        return (p.shape[1] * p.shape[2]) * ((p - g) ** 2).sum(dim=(1, 2))
    if kind == 4:
        return 0.5 * (p - g).abs().sum(dim=(1, 2))
    raise ValueError(kind)


def loss_and_gradient(kind, prediction, ground_truth, w, dtype, norm_path=True):
    """numpy ``[B,Hh,W]`` x 2, upstream weights ``[B]`` -> the losses ``[B]`` and the gradient of ``sum(w * loss)`` w.r.t. the
    prediction, computed in ``dtype`` from the same fp32 inputs, as fp64 numpy."""
    p = torch.tensor(prediction).to(dtype).requires_grad_(True)
    g = torch.tensor(ground_truth).to(dtype)
    value = loss(kind, p, g, norm_path)
    (value * torch.tensor(w).to(dtype)).sum().backward()
    return value.detach().double().numpy(), p.grad.double().numpy()


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def _normalised64(x):
    x = x.astype(np.float64)
    return x / np.maximum(np.abs(x).sum(axis=1, keepdims=True), EPS)


def _random_pairs(rng, n, K):
    """``n`` pairs ``[n,K]`` of positive pixels with exact zeros at different pixels of the two bitmaps (from three pixels on),
    the prediction at a gain of its own, and every |p^ - g^| at least _KINK_MARGIN * max g^."""
    g = rng.uniform(0.2, 1.0, size=(n, K)).astype(np.float32)
    if K == 1:
        return rng.uniform(0.5, 40.0, size=(n, 1)).astype(np.float32), np.zeros((n, 1), np.float32)
    ratio = np.where(rng.random((n, K)) < 0.5, rng.uniform(0.45, 0.8, size=(n, K)), rng.uniform(1.25, 1.9, size=(n, K)))
    p = (g * ratio * rng.uniform(0.5, 40.0, size=(n, 1))).astype(np.float32)
    if K >= 3:                                                  # about a tenth of each bitmap's pixels, never the same in both
        stride = min(K, 10)
        first = rng.integers(0, stride, size=(n, 1))
        gap = rng.integers(1, stride, size=(n, 1))
        residue = np.arange(K)[None, :] % stride
        p[residue == first] = 0.0
        g[residue == (first + gap) % stride] = 0.0
    for _ in range(50):
        ph, gh = _normalised64(p), _normalised64(g)
        close = np.abs(ph - gh) < _KINK_MARGIN * gh.max(axis=1, keepdims=True)
        if not close.any():
            return p, g
        p = np.where(close, p * np.float32(1.5), p)             # (close pixels are lit in both: dark ones differ by a whole pixel)
    raise AssertionError("no pair without a pixel at the kink of |p^ - g^|")


@functools.lru_cache(maxsize=None)
def _inputs(case):
    B, K = case.B, case.Hh * case.W
    rng = np.random.default_rng(1000 * case.B + 10 * K + int(case.misaligned))
    what = np.array(roles(case))
    p, g = _random_pairs(rng, B, K)
    rows = np.nonzero(what == EMPTY)[0]
    p[rows] = 0.0
    g[rows] = rng.uniform(0.2, 1.0, size=(len(rows), K)).astype(np.float32)
    rows = np.nonzero(what == EQUAL)[0]
    g[rows] = rng.uniform(0.2, 1.0, size=(len(rows), K)).astype(np.float32)
    if K >= 3:
        g[rows, 0] = 0.0
    p[rows] = g[rows]
    for row in np.nonzero(what == ONE_HOT)[0]:
        p[row], g[row] = one_hot_pair(K)
    w = rng.uniform(0.5, 1.5, size=B).astype(np.float32)
    out = dict(prediction=p.reshape(B, case.Hh, case.W), truth=g.reshape(B, case.Hh, case.W), w=w)
    for v in out.values():
        v.setflags(write=False)
    return out


def one_hot_pair(K):
    p, g = np.zeros(K, np.float32), np.zeros(K, np.float32)
    p[K // 3], g[(K // 3 + 1 + K // 2) % K] = 3.0, 0.5
    assert K // 3 != (K // 3 + 1 + K // 2) % K
    return p, g


def make_inputs(case):
    """``prediction``, ``truth`` ``[B,Hh,W]`` and the upstream weights ``w`` ``[B]`` of a case, fp32 numpy, read-only and the same
    arrays on every call."""
    return _inputs(case)


def known_answer_inputs(Hh, W):
    """An equal pair and (from two pixels on) a pair of one-hot bitmaps on different pixels at a case's bitmap shape:
    ``(prediction, truth)`` ``[1 or 2,Hh,W]``."""
    K = Hh * W
    rng = np.random.default_rng(77 + K)
    g = rng.uniform(0.2, 1.0, size=(1, K)).astype(np.float32)
    p = g.copy()
    if K > 1:
        hot = one_hot_pair(K)
        p, g = np.concatenate((p, hot[0][None])), np.concatenate((g, hot[1][None]))
    return p.reshape(-1, Hh, W), g.reshape(-1, Hh, W)


def known_answers(kind, K):
    """``(loss of the equal pair, loss of the disjoint one-hot pair)``; None where the value is only known to rounding."""
    return {2: (0.0, math.log(2.0)), 3: (0.0, 2.0 * K), 4: (0.0, 1.0), 5: (None, 1.0)}[kind]


def check_generator_conditions(case):
    """What the comparisons of fp32 against fp64 rest on: every non-zero pixel is positive (no sign(p) flips), and no pixel of a
    random pair is near the kink of kind 4.  Returns the smallest |p^ - g^| / max g^ over the random pairs."""
    d = make_inputs(case)
    B, K = case.B, case.Hh * case.W
    p, g = d["prediction"].reshape(B, K), d["truth"].reshape(B, K)
    what = np.array(roles(case))
    assert (p >= 0).all() and (g >= 0).all() and (d["w"] > 0).all()
    assert not p[what == EMPTY].any() and (what == EMPTY).sum() == 1 and what[0] == EMPTY
    assert (what == RANDOM).any()
    assert (what == EQUAL).sum() == (1 if B >= 3 else 0) and np.array_equal(p[what == EQUAL], g[what == EQUAL])
    for row in np.nonzero(what == ONE_HOT)[0]:
        assert (p[row] > 0).sum() == 1 and (g[row] > 0).sum() == 1 and not ((p[row] > 0) & (g[row] > 0)).any()
    lit = what != EMPTY
    assert (p[lit].sum(axis=1) > 0).all() and (g[what != RANDOM].sum(axis=1) > 0).all()
    rows = what == RANDOM
    ph, gh = _normalised64(p[rows]), _normalised64(g[rows])
    if K >= 3:
        assert ((p[rows] == 0).sum(axis=1) >= 1).all() and ((g[rows] == 0).sum(axis=1) >= 1).all()
    assert not ((p[rows] == 0) & (g[rows] == 0)).any()
    scale = np.maximum(gh.max(axis=1, keepdims=True), 1e-300)
    margin = float((np.abs(ph - gh) / scale).min()) if gh.max() > 0 else float("inf")
    assert (np.abs(ph - gh) >= KINK * gh.max(axis=1, keepdims=True)).all(), margin
    return margin


@functools.lru_cache(maxsize=None)
def reference(case, kind, precision):
    """``(losses [B], gradient [B,Hh,W])`` of the restatement on a case's inputs in fp64 (``precision=64``) or fp32 (``32``),
    computed once and shared."""
    d = make_inputs(case)
    value, grad = loss_and_gradient(kind, d["prediction"], d["truth"], d["w"], torch.float64 if precision == 64 else torch.float32)
    value.setflags(write=False)
    grad.setflags(write=False)
    return value, grad


@functools.lru_cache(maxsize=None)
def own_part(case, kind):
    """The fp64 gradient ``[B,Hh,W]`` without the part through the prediction's norm.  A gradient is the difference of the two
    parts; where they cancel altogether (a single lit pixel: p^ = 1 whatever p is) this is the size an fp32 result's rounding
    is measured by."""
    d = make_inputs(case)
    grad = loss_and_gradient(kind, d["prediction"], d["truth"], d["w"], torch.float64, norm_path=False)[1]
    grad.setflags(write=False)
    return grad
