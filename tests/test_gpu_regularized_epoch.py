"""The reference's optimiser run with its regularisers switched on, reproduced on the GPU (``-m gpu``).

``tests/golden/surface_reconstructor_regularized_epochs.npz`` (generate_regularizers.py) is the run of
test_gpu_optimizer_epoch.py - ARTIST's own ``SurfaceReconstructor``, three epochs - with both regulariser weights at 0.005, as
ARTIST's tutorial and its own reconstructor test set them.  Here the epoch is assembled as there (``_Epoch``) and
``surface_regularization_terms`` adds ``alpha * S + beta * I`` to the loss (surface_reconstructor.py:1023-1066).

The balancing factors are not detached, and their gradient cancels the terms' own down to a factor eps / (mean(S) + eps): the
regularisers' own per-control-point gradient is ~1e-4 of the locked gradient, far inside the locked gradient's
tolerance.  So the gradients of mean(S) and mean(I) alone - the kernel's backward without the cancellation - get legs of their
own at 1e-5."""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from test_gpu_optimizer_epoch import _Epoch, _lock, n, t

pytestmark = pytest.mark.gpu


def _regularized_loss(ep, cp, original, orientation):
    """The epoch's total loss with the regulariser terms, and its parts."""
    from artist_amd import surface_regularization_terms
    d = ep.d
    total_flux, cropped, per_sample, violation = ep.loss(cp, orientation)
    per_heliostat = per_sample.view(ep.H, int(d["number_of_train_samples"])).mean(dim=-1)
    alpha, s, beta, i = surface_regularization_terms(cp, original, per_heliostat, float(d["weight_smoothness"]),
                                                     float(d["weight_ideal_surface"]), epsilon=float(d["epsilon"]))
    regularizer_part = torch.mean(alpha * s + beta * i)
    return total_flux + regularizer_part, regularizer_part, (alpha, s, beta, i), per_heliostat, violation


def test_each_regularized_epoch_of_the_reference_run_is_reproduced(golden):
    d = golden("surface_reconstructor_regularized_epochs")
    ep = _Epoch(d)
    original = t(d["cp_start"][0])                     # the frozen copy of the surfaces (surface_reconstructor.py:421-425)
    grad_yard = rel_l2(d["grad_locked"][0], d["grad_locked_f64_epoch0"])
    flux_loss_yard = 2e-5                              # test_gpu_optimizer_epoch.py's per-sample flux-loss tolerance
    for e in range(d["cp_start"].shape[0]):
        cp = t(d["cp_start"][e]).requires_grad_(True)
        total, reg, (alpha, s, beta, i), per_heliostat, violation = _regularized_loss(ep, cp, original, t(d["orientation"][e]))
        g_s, = torch.autograd.grad(s.mean(), cp, retain_graph=True)
        g_i, = torch.autograd.grad(i.mean(), cp, retain_graph=True)
        g_reg, = torch.autograd.grad(reg, cp, retain_graph=True)
        total.backward()
        ep.after_backward(violation)
        errs = dict(S=rel_l2(n(s), d["smoothness_per_heliostat"][e]) if e else float(np.abs(n(s)).max()),
                    I=rel_l2(n(i), d["ideal_per_heliostat"][e]) if e else float(np.abs(n(i)).max()),
                    grad_S=rel_l2(n(g_s), d["grad_smoothness_mean"][e]), grad_I=rel_l2(n(g_i), d["grad_ideal_mean"][e]),
                    grad_reg=rel_l2(n(g_reg), d["grad_regularizer_part"][e]), grad_locked=rel_l2(n(_lock(cp.grad)), d["grad_locked"][e]))
        print(f"epoch {e}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
              + f"; alpha {float(alpha):.6e} (reference {float(d['alpha'][e]):.6e}), total loss {float(total):.7f} "
                f"(reference {d['total_loss'][e]:.7f})")
        if e == 0:                                     # the start is the original surface: both terms are exactly zero
            assert errs["S"] == 0.0 and errs["I"] == 0.0
            assert not d["smoothness_per_heliostat"][0].any() and not d["ideal_per_heliostat"][0].any()
        np.testing.assert_allclose(n(s), d["smoothness_per_heliostat"][e], rtol=1e-5, atol=0)
        np.testing.assert_allclose(n(i), d["ideal_per_heliostat"][e], rtol=1e-5, atol=0)
        # alpha = w mean(flux loss) / (mean(S) + eps): what the regulariser decides of it to 1e-5, the flux loss at its own tolerance
        mean_flux, mean_flux_ref = float(per_heliostat.mean()), float(d["flux_loss_per_sample"][e].mean())
        for got, key in ((alpha, "alpha"), (beta, "beta")):
            np.testing.assert_allclose(float(got) / mean_flux, float(d[key][e]) / mean_flux_ref, rtol=1e-5)
            np.testing.assert_allclose(float(got), float(d[key][e]), rtol=max(1e-5, flux_loss_yard))
        assert errs["grad_S"] < 1e-5 and errs["grad_I"] < 1e-5, errs      # the kernel's own backward, uncancelled
        assert errs["grad_reg"] < max(3 * grad_yard, 5e-4), (errs, grad_yard)
        np.testing.assert_allclose(float(total.detach()), d["total_loss"][e], rtol=2e-5)
        assert errs["grad_locked"] < max(3 * grad_yard, 5e-4), (errs, grad_yard)
        if e > 0:       # the terms are live from the second epoch on
            assert float(s.detach().min()) > 0 and float(i.detach().min()) > 0 and np.abs(d["grad_smoothness_mean"][e]).max() > 0


def test_the_whole_regularized_run_lands_on_the_reference_control_points(golden):
    """The three epochs chained with artist_amd.optim.Adam (edge lock in the kernel) at the recorded learning rates, against
    the control points after every step of the reference's run, by the rule of test_gpu_optimizer_epoch.py."""
    from artist_amd.optim import Adam
    d = golden("surface_reconstructor_regularized_epochs")
    ep = _Epoch(d)
    original = t(d["cp_start"][0])
    cp = t(d["cp_start"][0]).requires_grad_(True)
    optimizer = Adam([cp], lr=float(d["lr"][0]), lock_outer_edges=True)
    for e in range(d["cp_start"].shape[0]):
        for group in optimizer.param_groups:
            group["lr"] = float(d["lr"][e])
        optimizer.zero_grad()
        total, _, _, _, violation = _regularized_loss(ep, cp, original, t(d["orientation"][e]))
        total.backward()
        ep.after_backward(violation)
        optimizer.step()
        moved = (n(cp) - d["cp_after"][e]) / float(d["lr"][e])
        np.testing.assert_allclose(float(total.detach()), d["total_loss"][e], rtol=1e-4)
        frac_close = float((np.abs(moved) < 0.05).mean())
        print(f"epoch {e}: total loss {float(total):.7f} (reference {d['total_loss'][e]:.7f}); control points within 0.05 lr of the "
              f"reference's: {100 * frac_close:.2f} %, largest difference {np.abs(moved).max():.3f} lr")
        assert frac_close > 0.97 and np.abs(moved).max() < 2.0 * (e + 1) + 0.1, (e, frac_close, np.abs(moved).max())
