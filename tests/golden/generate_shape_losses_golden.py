#!/usr/bin/env python3
"""Fixture of the gain-invariant flux losses (runs ONLY in the build container, like generate_golden.py, whose reference import
recipe and ``save`` it uses).

TEST INFRASTRUCTURE - not part of the product.  Writes ``shape_losses.npz`` next to this script: small non-negative bitmap pairs
and what the reference's OWN loss classes (artist/optim/loss.py) give on them in fp64, arranged so that each value is one of the
losses of ``art_flux_loss`` kinds 2, 3 and 5 (tests/shape_loss_ref.py restates the formulas; tests/test_shape_losses_host.py compares):

    kind 2  1/2 KLDivergenceLoss()(m, g) + 1/2 KLDivergenceLoss()(m, p),  m = (p^ + g^) / 2 of the L1-normalised bitmaps
            (called as (prediction, ground_truth): D_KL(g^ || m) and D_KL(p^ || m); the class normalises its arguments once
            more, which leaves m - of sum 1 - and p, g what they are up to rounding)
    kind 3  PixelLoss()(K p^, K g^)                (K pixels: both bitmaps scaled to unit mean)
    kind 5  CosineSimilarityLoss()(p.flatten(1), g.flatten(1))

Kind 4 (total variation) has no counterpart in the reference.  Every pair is lit in both bitmaps (the reference's classes divide
by the sums); some pixels are exact zeros, in one bitmap or in both.

Keys: ``shapes`` [n,3]; per shape k ``p_<k>``, ``g_<k>`` (fp32 [B,Hh,W]), ``kind2_<k>``, ``kind3_<k>``, ``kind5_<k>`` (fp64 [B]).

Usage:  PYTHONPATH=<repo root> python tests/golden/generate_shape_losses_golden.py
"""
from __future__ import annotations

import generate_golden as gg  # noqa: E402  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(4, 1, 1), (4, 1, 3), (4, 2, 2), (3, 5, 7), (3, 8, 8), (2, 33, 17)]
EPS = 1e-12


def shape_losses_fixture():
    from artist.optim.loss import CosineSimilarityLoss, KLDivergenceLoss, PixelLoss

    rng = np.random.default_rng(5)
    out = dict(shapes=np.asarray(SHAPES, dtype=np.int64))
    for k, (B, Hh, W) in enumerate(SHAPES):
        K = Hh * W
        g = rng.uniform(0.05, 1.0, size=(B, K)).astype(np.float32)
        p = (g * rng.uniform(0.4, 2.5, size=(B, K)) * rng.uniform(0.5, 40.0, size=(B, 1))).astype(np.float32)
        if K >= 3:                                  # exact zeros: one pixel dark in the prediction, one in the truth, one in both
            p[:, 0] = 0.0
            g[:, 1] = 0.0
        if K >= 8:
            p[:, 5] = g[:, 5] = 0.0
        p[B - 1] = g[B - 1] * np.float32(4.0)       # the same shape at another gain (exact in fp32): every loss about 0
        p, g = p.reshape(B, Hh, W), g.reshape(B, Hh, W)
        p64, g64 = torch.from_numpy(p).double(), torch.from_numpy(g).double()
        ph = torch.nn.functional.normalize(p64, p=1, dim=(1, 2), eps=EPS)
        gh = torch.nn.functional.normalize(g64, p=1, dim=(1, 2), eps=EPS)
        m = 0.5 * (ph + gh)
        kl = KLDivergenceLoss()
        out[f"p_{k}"], out[f"g_{k}"] = p, g
        out[f"kind2_{k}"] = gg.npy(0.5 * kl(m, g64, reduction_dimensions=(1, 2)) + 0.5 * kl(m, p64, reduction_dimensions=(1, 2)))
        out[f"kind3_{k}"] = gg.npy(PixelLoss()(K * ph, K * gh, reduction_dimensions=(1, 2)))
        out[f"kind5_{k}"] = gg.npy(CosineSimilarityLoss()(p64.flatten(1), g64.flatten(1)))
        for kind in (2, 3, 5):
            assert out[f"kind{kind}_{k}"].dtype == np.float64 and out[f"kind{kind}_{k}"].shape == (B,)
    return out


if __name__ == "__main__":
    gg.save("shape_losses", shape_losses_fixture())
