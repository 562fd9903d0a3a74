"""The surface regularisers on the GPU (``-m gpu``): artist_amd's SmoothnessRegularizer / IdealSurfaceRegularizer against the
reference's own outputs (tests/golden/regularizers.npz, generate_regularizers.py), the fp64 restatement at the metric size,
reproducibility, sharding, and the graph that surface_regularization_terms builds."""
import numpy as np
import pytest
import torch

import regularizer_ref as ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_SHAPES = 7


def t(x, dtype=torch.float32):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


@pytest.mark.parametrize("k", range(N_SHAPES))
def test_forward_matches_the_reference_for_every_case_and_reduction(golden, k):
    """The Laplacian is torch's fp32 value bit for bit; only the order of the final sum differs: 2e-6 relative."""
    from artist_amd import IdealSurfaceRegularizer, SmoothnessRegularizer
    d = golden("regularizers")
    org = t(d[f"org_{k}"])
    for j in range(len(d["scales"])):
        cur = t(d[f"cur_{k}_{j}"])
        for r, red in enumerate(ref.REDUCTIONS):
            s, i = SmoothnessRegularizer(red)(cur, org), IdealSurfaceRegularizer(red)(cur, org)
            assert s.dtype == torch.float32 and s.shape == d[f"S_{k}_{j}_{r}"].shape and i.shape == d[f"I_{k}_{j}_{r}"].shape
            np.testing.assert_allclose(n(s), d[f"S_{k}_{j}_{r}"], rtol=2e-6, atol=0)
            np.testing.assert_allclose(n(i), d[f"I_{k}_{j}_{r}"], rtol=2e-6, atol=0)


@pytest.mark.parametrize("k", range(N_SHAPES))
def test_backward_matches_the_reference(golden, k):
    """Gradient of the weighted sums w.r.t. current within max(3 x the reference's fp32-vs-fp64 distance, 1e-5); the fp64 side is
    the fixture's where it has one, the restatement (checked against the fixture on the host) otherwise."""
    from artist_amd import IdealSurfaceRegularizer, SmoothnessRegularizer
    d = golden("regularizers")
    org_np = d[f"org_{k}"]
    org = t(org_np)
    for j in range(len(d["scales"])):
        cur_np = d[f"cur_{k}_{j}"]
        red = ref.REDUCTIONS[int(d[f"grad_red_{k}_{j}"])]
        hf = d[f"org_{k}"].shape[:2]
        gs64, gi64 = ref.gradients(cur_np, org_np, ref.upstream(d[f"wS_{k}_{j}"], red, hf), ref.upstream(d[f"wI_{k}_{j}"], red, hf))
        if f"gS64_{k}_{j}" in d:
            gs64, gi64 = d[f"gS64_{k}_{j}"], d[f"gI64_{k}_{j}"]
        for cls, w, key, g64 in ((SmoothnessRegularizer, "wS", "gS", gs64), (IdealSurfaceRegularizer, "wI", "gI", gi64)):
            cur = t(cur_np).requires_grad_(True)
            (cls(red)(cur, org) * t(d[f"{w}_{k}_{j}"])).sum().backward()
            yard = rel_l2(d[f"{key}_{k}_{j}"], g64)
            err = rel_l2(n(cur.grad), d[f"{key}_{k}_{j}"])
            assert err < max(3 * yard, 1e-5), (key, j, err, yard)


def _metric_nets(H=1000, F=4, U=10, V=10, scale=2e-5, seed=5):
    g = torch.Generator().manual_seed(seed)
    org = torch.randn(H, F, U, V, 3, generator=g)
    cur = (org + scale * torch.randn(H, F, U, V, 3, generator=g)).float()
    return cur.to(DEV), org.to(DEV)


@pytest.mark.parametrize("scale", [2e-5, 1e-2])
def test_metric_size_against_the_restatement(scale):
    """1000 heliostats x 4 facets x 10 x 10 control points: both terms and both gradients against the fp64 restatement."""
    from artist_amd.regularizers import surface_regularizers
    cur, org = _metric_nets(scale=scale)
    cur.requires_grad_(True)
    s, i = surface_regularizers(cur, org)
    s64, i64 = ref.terms(n(cur), n(org))
    assert rel_l2(n(s), s64) < 1e-6 and rel_l2(n(i), i64) < 1e-6
    ws, wi = torch.rand(s.shape, device=DEV), torch.rand(i.shape, device=DEV)
    gs, = torch.autograd.grad((s * ws).sum(), cur, retain_graph=True)
    gi, = torch.autograd.grad((i * wi).sum(), cur)
    gs64, gi64 = ref.gradients(n(cur), n(org), n(ws), n(wi))
    err_s, err_i = rel_l2(n(gs), gs64), rel_l2(n(gi), gi64)
    print(f"metric size, scale {scale:g}: smoothness {rel_l2(n(s), s64):.1e}, ideal {rel_l2(n(i), i64):.1e}, "
          f"gradients {err_s:.1e} / {err_i:.1e}")
    assert err_s < 1e-5 and err_i < 1e-5


def test_two_calls_give_the_same_bits_and_a_rank_slice_its_rows():
    """No atomics, fixed-order sums, a net's bits depend on that net alone: 125 heliostats (one rank's share) called alone give
    the rows of the full call, forward and backward."""
    from artist_amd.regularizers import surface_regularizers
    cur, org = _metric_nets()
    outs = []
    for rows in (slice(None), slice(None), slice(375, 500)):
        c = cur[rows].clone().requires_grad_(True)
        s, i = surface_regularizers(c, org[rows])
        (s * 3.0 + i * 5.0).sum().backward()
        outs.append((s.detach(), i.detach(), c.grad))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for a, b in zip(outs[0], outs[2]):
        assert torch.equal(a[375:500], b)


class _Spy:
    """Records the calls into the library (name, arguments)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*args):
            self.calls.append((name, args))
            return fn(*args)
        return call


def test_one_launch_each_way_and_a_zero_weight_does_no_work(monkeypatch):
    from artist_amd import _lib, surface_regularization_terms
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    cur, org = _metric_nets(H=8)
    cur.requires_grad_(True)
    flux = torch.rand(8, device=DEV, requires_grad=True)

    alpha, s, beta, i = surface_regularization_terms(cur, org, flux, 0.005, 0.005)
    assert [c[0] for c in spy.calls] == ["art_surface_regularizers_fwd"]
    (alpha * s + beta * i).mean().backward()
    assert [c[0] for c in spy.calls] == ["art_surface_regularizers_fwd", "art_surface_regularizers_bwd"]
    assert all(a is not None for a in spy.calls[1][1][5:7])           # both upstream gradients passed on

    for w_s, w_i in ((0.0, 0.005), (0.005, 0.0)):
        spy.calls.clear()
        cur.grad = None
        alpha, s, beta, i = surface_regularization_terms(cur, org, flux, w_s, w_i)
        zero, live = (s, i) if w_s == 0 else (i, s)
        assert not zero.requires_grad and float(zero.abs().max()) == 0.0 and zero.shape == flux.shape and live.requires_grad
        assert float((alpha if w_s == 0 else beta).detach()) == 0.0
        (name, args), = spy.calls
        assert name == "art_surface_regularizers_fwd" and (args[5] is None) == (w_s == 0) and (args[6] is None) == (w_i == 0)
        (alpha * s + beta * i).mean().backward()
        assert spy.calls[1][0] == "art_surface_regularizers_bwd"
        assert (spy.calls[1][1][5] is None) == (w_s == 0) and (spy.calls[1][1][6] is None) == (w_i == 0)

    spy.calls.clear()
    alpha, s, beta, i = surface_regularization_terms(cur, org, flux, 0.0, 0.0)
    assert spy.calls == [] and float(alpha) == 0.0 and float(beta) == 0.0 and not s.requires_grad and not i.requires_grad


def test_the_unselected_output_gets_no_gradient_pass(monkeypatch):
    """A term whose output is not in the loss gets a null upstream gradient (no zeros tensor is made and read)."""
    from artist_amd import _lib
    from artist_amd.regularizers import surface_regularizers
    spy = _Spy(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: spy)
    cur, org = _metric_nets(H=4)
    cur.requires_grad_(True)
    s, i = surface_regularizers(cur, org)
    s.sum().backward()
    args = spy.calls[-1][1]
    assert spy.calls[-1][0] == "art_surface_regularizers_bwd" and args[5] is not None and args[6] is None


def test_original_gets_the_negative_gradient_when_it_asks_for_one():
    from artist_amd.regularizers import surface_regularizers
    cur, org = _metric_nets(H=6)
    cur, org = cur.clone().requires_grad_(True), org.clone().requires_grad_(True)
    s, i = surface_regularizers(cur, org)
    (s * 2.0 + i).sum().backward()
    assert torch.equal(org.grad, -cur.grad) and float(cur.grad.abs().max()) > 0
    frozen = org.detach()
    c2 = cur.detach().clone().requires_grad_(True)
    s, i = surface_regularizers(c2, frozen)
    (s * 2.0 + i).sum().backward()
    assert torch.equal(c2.grad, cur.grad) and frozen.grad is None


def test_empty_and_odd_inputs():
    """No nets: nothing launched, empty results; fp64 / non-contiguous inputs are converted as every op does."""
    from artist_amd import IdealSurfaceRegularizer, SmoothnessRegularizer
    z = torch.zeros(0, 4, 6, 6, 3, device=DEV)
    assert SmoothnessRegularizer((1,))(z, z).shape == (0,) and IdealSurfaceRegularizer((0,))(z, z).shape == (4,)
    cur, org = _metric_nets(H=3)
    base = SmoothnessRegularizer((1,))(cur, org)
    odd = SmoothnessRegularizer((1,))(cur.double().transpose(2, 3).contiguous().transpose(2, 3), org.double())
    assert torch.equal(base, odd)
    with pytest.raises(ValueError, match="must be on"):
        SmoothnessRegularizer((1,))(cur, org.cpu())
