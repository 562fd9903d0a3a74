#!/usr/bin/env python3
"""Fixtures of the surface regularisers (runs ONLY in the build container, like generate_golden.py, whose reference import
recipe and helpers it uses).

TEST INFRASTRUCTURE - not part of the product.  Writes two files next to this script:

  regularizers.npz
      The reference's own ``SmoothnessRegularizer`` / ``IdealSurfaceRegularizer`` (artist/optim/regularizers.py:60-186) on
      control nets of size O(1), shapes (H, F, U, V) in SHAPES, displaced by about 2e-5 (an Adam step at lr 2e-5) and 1e-2, for
      each of the ``reduction_dimensions`` in REDUCTIONS: both terms in fp32 and in fp64 (the same fp32 inputs, upcast), and the
      autograd gradient w.r.t. ``current`` of a randomly weighted sum of each term - for one reduction per (shape, scale), in
      turn - in fp32, and in fp64 at the small displacement (the fp64 gradients of the large one would double the file; the
      tests restate them in numpy, a restatement checked against the stored ones).
      Keys: ``org_<k>``, ``cur_<k>_<j>`` (shape k, scale j), ``S_<k>_<j>_<r>``, ``I_<k>_<j>_<r>`` (+ ``S64_`` / ``I64_``),
      ``grad_red_<k>_<j>`` (index r of the gradients' reduction), ``wS_<k>_<j>``, ``wI_<k>_<j>``, ``gS_<k>_<j>``,
      ``gI_<k>_<j>`` (+ ``gS64_<k>_0`` / ``gI64_<k>_0``).

  surface_reconstructor_regularized_epochs.npz
      generate_golden.py::surface_reconstructor_epochs - the reference's own SurfaceReconstructor, three epochs - with both
      regulariser weights at 0.005 (ARTIST's tutorial and its own reconstructor test), the same keys as
      surface_reconstructor_epochs.npz, plus per epoch, recorded by wrapping the instance's ``_compute_regularization_terms``
      (surface_reconstructor.py:656-749): ``smoothness_per_heliostat``, ``ideal_per_heliostat``, ``alpha``, ``beta``, the
      gradients w.r.t. the control points of ``mean(S)`` alone (``grad_smoothness_mean``), of ``mean(I)`` alone
      (``grad_ideal_mean``) and of the regulariser part ``mean(alpha S + beta I)`` (``grad_regularizer_part``); and the first
      epoch of the fp64 run (``<key>_f64_epoch0``).

Usage:  PYTHONPATH=<repo root> python tests/golden/generate_regularizers.py
"""
from __future__ import annotations

import generate_golden as gg  # noqa: E402  (imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = [(3, 4, 6, 6), (2, 4, 10, 10), (2, 4, 7, 4), (1, 3, 2, 2), (2, 1, 1, 5), (2, 2, 5, 1), (1, 1, 1, 1)]
SCALES = [2e-5, 1e-2]
REDUCTIONS = [(1,), (0,), (0, 1)]
WEIGHT = 0.005


def regularizers_fixture():
    from artist.optim.regularizers import IdealSurfaceRegularizer, SmoothnessRegularizer

    gen = torch.Generator().manual_seed(11)
    out = dict(shapes=np.asarray(SHAPES, dtype=np.int64), scales=np.asarray(SCALES, dtype=np.float64),
               reductions=np.asarray([list(r) + [-1] * (2 - len(r)) for r in REDUCTIONS], dtype=np.int64))
    for k, (H, F, U, V) in enumerate(SHAPES):
        # O(1) nets: a planar grid over [-1, 1]^2 per facet, bent into a saddle of its own (no noise: it compresses)
        gu = torch.linspace(-1.0, 1.0, U, dtype=torch.float64) if U > 1 else torch.zeros(1, dtype=torch.float64)
        gv = torch.linspace(-1.0, 1.0, V, dtype=torch.float64) if V > 1 else torch.zeros(1, dtype=torch.float64)
        x, y = gu.view(1, 1, U, 1).expand(H, F, U, V), gv.view(1, 1, 1, V).expand(H, F, U, V)
        bend = torch.arange(1, H * F + 1, dtype=torch.float64).view(H, F, 1, 1) / (H * F)
        org = torch.stack([x + 0.5 * bend, y - 0.25 * bend, 0.3 * bend * (x ** 2 - 0.5 * y ** 2) + 0.1], dim=-1).float()
        out[f"org_{k}"] = gg.npy(org)
        for j, scale in enumerate(SCALES):
            cur = (org + scale * torch.randn(H, F, U, V, 3, generator=gen)).float()
            out[f"cur_{k}_{j}"] = gg.npy(cur)
            for r, red in enumerate(REDUCTIONS):
                for dtype, tag in ((torch.float32, ""), (torch.float64, "64")):
                    c, o = cur.to(dtype), org.to(dtype)
                    out[f"S{tag}_{k}_{j}_{r}"] = gg.npy(SmoothnessRegularizer(red)(c, o))
                    out[f"I{tag}_{k}_{j}_{r}"] = gg.npy(IdealSurfaceRegularizer(red)(c, o))
            r = (k + j) % len(REDUCTIONS)
            red = REDUCTIONS[r]
            out[f"grad_red_{k}_{j}"] = np.int64(r)
            shape_red = SmoothnessRegularizer(red)(cur, org).shape
            w_s = torch.rand(shape_red, generator=gen) + 0.5
            w_i = torch.rand(shape_red, generator=gen) + 0.5
            out[f"wS_{k}_{j}"], out[f"wI_{k}_{j}"] = gg.npy(w_s), gg.npy(w_i)
            for dtype, tag in ((torch.float32, ""), (torch.float64, "64"))[:2 if j == 0 else 1]:
                for cls, w, key in ((SmoothnessRegularizer, w_s, "gS"), (IdealSurfaceRegularizer, w_i, "gI")):
                    c = cur.detach().to(dtype).clone().requires_grad_(True)
                    (cls(red)(c, org.to(dtype)) * w.to(dtype)).sum().backward()
                    out[f"{key}{tag}_{k}_{j}"] = gg.npy(c.grad)
    return out


def regularized_epochs(dtype):
    """surface_reconstructor_epochs with both weights at WEIGHT; returns its dict plus the regulariser records."""
    import artist.optim
    from artist.util import constants

    log = dict(smoothness_per_heliostat=[], ideal_per_heliostat=[], alpha=[], beta=[], grad_smoothness_mean=[],
               grad_ideal_mean=[], grad_regularizer_part=[])
    base = artist.optim.SurfaceReconstructor

    class RegularizedReconstructor(base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.constraint_dict[constants.weight_smoothness] = WEIGHT
            self.constraint_dict[constants.weight_ideal_surface] = WEIGHT
            terms = self._compute_regularization_terms

            def terms_wrapped(**kw):
                alpha, s, beta, i = terms(**kw)
                prm = kw["heliostat_group"].nurbs_control_points
                log["smoothness_per_heliostat"].append(gg.npy(s).copy())
                log["ideal_per_heliostat"].append(gg.npy(i).copy())
                log["alpha"].append(gg.npy(alpha).copy())
                log["beta"].append(gg.npy(beta).copy())
                for key, value in (("grad_smoothness_mean", s.mean()), ("grad_ideal_mean", i.mean()),
                                   ("grad_regularizer_part", (alpha * s + beta * i).mean())):
                    (g,) = torch.autograd.grad(value, prm, retain_graph=True)
                    log[key].append(gg.npy(g).copy())
                return alpha, s, beta, i

            self._compute_regularization_terms = terms_wrapped

    artist.optim.SurfaceReconstructor = RegularizedReconstructor
    try:
        out = gg.surface_reconstructor_epochs(dtype=dtype)
    finally:
        artist.optim.SurfaceReconstructor = base
    E = out["cp_start"].shape[0]
    assert all(len(v) == E for v in log.values()), {k: len(v) for k, v in log.items()}
    out.update({k: np.stack(v) for k, v in log.items()})
    out["weight_smoothness"] = out["weight_ideal_surface"] = np.float64(WEIGHT)
    return out


def main():
    gg.save("regularizers", regularizers_fixture())
    a32 = regularized_epochs(torch.float32)
    a64 = regularized_epochs(torch.float64)
    for key in ("cropped_flux", "flux_loss_per_sample", "grad_locked", "cp_after", "total_loss", "smoothness_per_heliostat",
                "ideal_per_heliostat", "alpha", "beta", "grad_smoothness_mean", "grad_ideal_mean", "grad_regularizer_part"):
        a32[key + "_f64_epoch0"] = a64[key][0]
    torch.set_default_dtype(torch.float32)
    gg.save("surface_reconstructor_regularized_epochs", a32)


if __name__ == "__main__":
    main()
