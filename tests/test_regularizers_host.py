"""Host side of the surface regularisers: the numpy fp64 restatement (tests/regularizer_ref.py) against the reference's fp64 outputs
in tests/golden/regularizers.npz, and the argument checks of artist_amd.regularizers and of the entry points of
include/artist_hip_regularizers.h."""
import ctypes

import numpy as np
import pytest
import torch

import regularizer_ref as ref

N_SHAPES = 7


def _max_close(got, want, rel):
    scale = max(float(np.abs(want).max()), 1e-300)
    return float(np.abs(np.asarray(got) - want).max()) <= rel * scale


@pytest.mark.parametrize("k", range(N_SHAPES))
def test_restatement_equals_the_reference_in_fp64(golden, k):
    """Both terms for every scale and reduction, and both gradients (clamped adjoint included), to 1e-12."""
    d = golden("regularizers")
    assert [tuple(r[r >= 0]) for r in d["reductions"]] == ref.REDUCTIONS
    org = d[f"org_{k}"]
    for j in range(len(d["scales"])):
        cur = d[f"cur_{k}_{j}"]
        s, i = ref.terms(cur, org)
        for r, red in enumerate(ref.REDUCTIONS):
            np.testing.assert_allclose(ref.reduce(s, red), d[f"S64_{k}_{j}_{r}"], rtol=1e-12, atol=0)
            np.testing.assert_allclose(ref.reduce(i, red), d[f"I64_{k}_{j}_{r}"], rtol=1e-12, atol=0)
        if f"gS64_{k}_{j}" in d:
            red = ref.REDUCTIONS[int(d[f"grad_red_{k}_{j}"])]
            gs, gi = ref.gradients(cur, org, ref.upstream(d[f"wS_{k}_{j}"], red, s.shape), ref.upstream(d[f"wI_{k}_{j}"], red, s.shape))
            assert _max_close(gs, d[f"gS64_{k}_{j}"], 1e-12) and _max_close(gi, d[f"gI64_{k}_{j}"], 1e-12)
    assert f"gS64_{k}_0" in d


def test_the_clamped_laplacian_is_its_own_adjoint():
    """<L x, y> == <x, L y> for the nets of every edge case (U or V equal to 1 or 2): why one stencil serves both passes."""
    rng = np.random.default_rng(3)
    for U, V in ((1, 1), (1, 2), (2, 1), (2, 2), (1, 5), (5, 1), (2, 7), (6, 6)):
        x, y = rng.standard_normal((2, 1, U, V, 3)), rng.standard_normal((2, 1, U, V, 3))
        assert abs(np.sum(ref.laplacian(x) * y) - np.sum(x * ref.laplacian(y))) < 1e-12
        np.testing.assert_allclose(ref.laplacian_adjoint(y), ref.laplacian(y), rtol=0, atol=1e-12)


def test_shapes_and_dtypes_are_validated():
    from artist_amd import IdealSurfaceRegularizer, SmoothnessRegularizer
    z = torch.zeros
    for reg in (SmoothnessRegularizer((1,)), IdealSurfaceRegularizer((1,))):
        with pytest.raises(ValueError, match=r"\[H, F, U, V, 3\]"):
            reg(z(2, 4, 6, 3), z(2, 4, 6, 3))
        with pytest.raises(ValueError, match=r"\[H, F, U, V, 3\]"):
            reg(z(2, 4, 6, 6, 4), z(2, 4, 6, 6, 4))
        with pytest.raises(ValueError, match=r"U, V >= 1"):
            reg(z(2, 4, 0, 6, 3), z(2, 4, 0, 6, 3))
        with pytest.raises(ValueError, match="differ in shape"):
            reg(z(2, 4, 6, 6, 3), z(2, 4, 6, 5, 3))
        with pytest.raises(TypeError, match="floating point"):
            reg(z(2, 4, 6, 6, 3, dtype=torch.int32), z(2, 4, 6, 6, 3))


def test_no_cpu_fallback():
    from artist_amd import ArtistHipError, IdealSurfaceRegularizer, SmoothnessRegularizer, surface_regularization_terms
    cur, org = torch.rand(2, 4, 6, 6, 3), torch.rand(2, 4, 6, 6, 3)
    for reg in (SmoothnessRegularizer((1,)), IdealSurfaceRegularizer((0, 1))):
        with pytest.raises(ArtistHipError, match="no CPU fallback"):
            reg(cur, org)
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        surface_regularization_terms(cur, org, torch.rand(2), 0.005, 0.005)


def test_exported_where_the_reference_has_them():
    import artist_amd
    import artist_amd.optim
    assert artist_amd.optim.SmoothnessRegularizer is artist_amd.SmoothnessRegularizer
    assert artist_amd.optim.IdealSurfaceRegularizer is artist_amd.IdealSurfaceRegularizer
    assert artist_amd.SmoothnessRegularizer((0, 1)).reduction_dimensions == (0, 1)


def test_regularizer_argument_checks_need_no_device():
    from artist_amd import _lib
    fwd, bwd = _lib.lib().art_surface_regularizers_fwd, _lib.lib().art_surface_regularizers_bwd
    assert fwd(None, None, 0, 6, 6, None, None, None) == 0          # no nets: no launch, no pointer needed
    assert bwd(None, None, 0, 6, 6, None, None, None, None) == 0
    for N, U, V in ((-1, 6, 6), (0, 0, 6), (4, 6, 0), (4, 53, 53), (1, 1, 2731)):   # bad sizes; nets larger than the LDS staging
        assert fwd(None, None, N, U, V, None, None, None) == _lib.ART_EINVAL, (N, U, V)
        assert bwd(None, None, N, U, V, None, None, None, None) == _lib.ART_EINVAL, (N, U, V)
    p = ctypes.c_void_p(16)                                          # (never dereferenced: every call below fails its checks)
    assert fwd(p, p, 4, 6, 6, None, None, None) == _lib.ART_EINVAL      # neither output
    assert fwd(None, p, 4, 6, 6, p, p, None) == _lib.ART_EINVAL
    assert bwd(p, p, 4, 6, 6, p, p, None, None) == _lib.ART_EINVAL     # no gradient buffer
    assert bwd(p, None, 4, 6, 6, None, None, p, None) == _lib.ART_EINVAL
