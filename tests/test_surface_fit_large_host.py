"""Surface fitting up to 2^20 rows per facet, the part that needs no GPU: the size limits of the three entry points
(include/artist_hip_surface_fit.h).  Every call below returns before the library makes a HIP call."""
import ctypes

import pytest

MAX_N = 1 << 20


def _calls(lib, p, B, N, nu, nv, deg):
    """The three entry points with the same sizes; ``p`` stands for every data pointer."""
    return {
        "prepare": lib.art_surface_fit_prepare(p, None, p, p, B, N, nu, nv, deg, deg, p, p, p, p, p, None),
        "loss_grad": lib.art_surface_fit_loss_grad(p, p, None, p, p, p, B, N, nu, nv, deg, deg, 1, p, p, None, None, None),
        "run": lib.art_surface_fit_run(p, p, p, p, p, p, p, None, p, p, p, B, N, nu, nv, deg, deg, 1, 401, 1e-10, 400, 0.9, 0.999, 1e-8,
                                       0.0, 0, 1, 0, 0.2, 5, 1e-7, 1, 0, 0.0, 1e-8, None),
    }


@pytest.mark.parametrize("net,deg", [(10, 3), (5, 2), (12, 4)])
def test_row_limit_is_two_to_the_twentieth(net, deg):
    """With no facets and null data pointers the sizes alone decide: 2^20 rows are admitted, one more is ART_EINVAL (never
    narrowed), and so is no row at all."""
    from artist_amd import _lib
    lib = _lib.lib()
    assert _calls(lib, None, 0, MAX_N, net, net, deg) == dict(prepare=_lib.ART_OK, loss_grad=_lib.ART_OK, run=_lib.ART_OK)
    for rows in (MAX_N + 1, 1 << 31, (1 << 32) + 800, 0):
        assert _calls(lib, None, 0, rows, net, net, deg) == dict(prepare=_lib.ART_EINVAL, loss_grad=_lib.ART_EINVAL, run=_lib.ART_EINVAL), rows
    # the old limits are no limits any more: one row past the former cap, and a count no CU's LDS holds
    for rows in (16385, 80000):
        assert set(_calls(lib, None, 0, rows, net, net, deg).values()) == {_lib.ART_OK}


def test_a_net_too_large_for_lds_is_still_unsupported():
    """ART_EUNSUPPORTED remains where the net's own block - net, two moments, cell partial sums, bias tables - exceeds 160 KiB,
    whatever N: loss_grad and run decide that from the sizes before their first HIP call, so it shows without a device (the
    pointers are never dereferenced).  prepare keeps only offsets and knots in LDS beside a tile of rows, which always fit: it
    has no such case left, and with work to do it would launch - it is not called here."""
    from artist_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(16)
    for rows in (37, 800, 80000, MAX_N):
        assert lib.art_surface_fit_loss_grad(p, p, None, p, p, p, 1, rows, 64, 64, 3, 3, 1, p, p, None, None, None) == _lib.ART_EUNSUPPORTED
        assert lib.art_surface_fit_run(p, p, p, p, p, p, p, None, p, p, p, 1, rows, 64, 64, 3, 3, 1, 401, 1e-10, 400, 0.9, 0.999, 1e-8,
                                       0.0, 0, 1, 0, 0.2, 5, 1e-7, 1, 0, 0.0, 1e-8, None) == _lib.ART_EUNSUPPORTED
    # a size error wins over it, and null data with facets to fit is ART_EINVAL
    assert lib.art_surface_fit_loss_grad(p, p, None, p, p, p, 1, MAX_N + 1, 64, 64, 3, 3, 1, p, p, None, None, None) == _lib.ART_EINVAL
    assert lib.art_surface_fit_loss_grad(p, None, None, p, p, p, 1, 80000, 10, 10, 3, 3, 1, p, p, None, None, None) == _lib.ART_EINVAL
    assert lib.art_surface_fit_prepare(None, None, p, p, 1, 80000, 10, 10, 3, 3, p, p, p, p, p, None) == _lib.ART_EINVAL
