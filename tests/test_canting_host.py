"""Host side of the facet canting: the numpy restatement (tests/canting_ref.py) against the reference's outputs in
tests/golden/canting.npz (generate_canting_golden.py), and the argument checks of art_cant_facets_fwd / _bwd
(include/artist_hip_canting.h)."""
import ctypes

import numpy as np
import pytest
import torch

import canting_ref as ref
from conftest import rel_l2


def _max_close(got, want, rel):
    scale = max(float(np.abs(want).max()), 1e-300)
    return float(np.abs(np.asarray(got) - want).max()) <= rel * scale


def _restated(c, dtype, sfx):
    """The restatement's counterparts of the fixture's results for one case, from the fixture's un-canted surfaces."""
    mask = c["mask"]
    cant, tr = ref.activate(c["canting"], mask), ref.activate(c["translations"], mask)
    p0, n0 = c["points0" + sfx], c["normals0" + sfx]
    out = dict(points=ref.rotate(cant, p0, translations=tr, dtype=dtype), normals=ref.rotate(cant, n0, dtype=dtype))
    g_c, g_t, _ = ref.gradients(cant, [(p0, c["wp"], True), (n0, c["wn"], False)], with_translations=True, dtype=dtype)
    out.update(grad_canting=ref.to_base(g_c, mask), grad_translations=ref.to_base(g_t, mask))
    out["pc_fwd"] = ref.rotate(c["canting"], c["pc_data"], dtype=dtype)
    out["pc_inv"] = ref.rotate(c["canting"], c["pc_data"], inverse=True, dtype=dtype)
    g_c, _, (g_d,) = ref.gradients(c["canting"], [(c["pc_data"], c["pc_w"], False)], inverse=True, dtype=dtype)
    out.update(pc_inv_grad_canting=g_c, pc_inv_grad_data=g_d)
    return out


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_equals_the_reference_in_fp64(golden, name):
    """Rotation, translation and every gradient to 1e-12 of the tensor's largest value; the w components of the canting
    gradient are 0, the translation's is not (points.w = 1 + translation.w)."""
    c = ref.fixture_case(golden("canting"), name)
    got = _restated(c, np.float64, "_f64")
    for key, value in got.items():
        assert value.dtype == np.float64 and value.shape == c[key + "_f64"].shape, key
        if "grad" in key and not int(c["grads_finite"]):
            continue
        assert _max_close(value, c[key + "_f64"], 1e-12), (key, float(np.abs(value - c[key + "_f64"]).max()))
    if int(c["grads_finite"]):
        assert not c["grad_canting_f64"][..., 3].any() and c["grad_translations_f64"][..., 3].all()


@pytest.mark.parametrize("name", ref.CASES)
def test_restatement_in_fp32_stays_within_the_reference_own_distance(golden, name):
    """max(3 x rel-L2(fixture fp32, fixture fp64), 1e-5) per tensor: the bound the GPU tests use."""
    c = ref.fixture_case(golden("canting"), name)
    got = _restated(c, np.float32, "")
    for key, value in got.items():
        if "grad" in key and not int(c["grads_finite"]):
            continue
        yard = rel_l2(c[key], c[key + "_f64"])
        err = rel_l2(value, c[key])
        assert value.dtype == np.float32 and err < max(3 * yard, 1e-5), (key, err, yard)


def test_the_fixture_holds_what_the_tests_need(golden):
    d = golden("canting")
    assert all(v.dtype != object for v in d.values())
    finite = {name: int(d[f"{name}_grads_finite"]) for name in ref.CASES}
    print("gradients finite per case:", finite, "descent: fraction", float(d["descent_fraction"]), "reference ratio",
          float(d["descent_ref_ratio"]))
    assert all(finite[name] for name in "abcd")                    # (e), the degenerate facet, may be forward-only
    assert d["d_mask"].tolist() == [1, 2] and d["d_points"].shape[0] == 3
    assert 0.8 <= float(d["descent_ref_ratio"]) <= 1.2 and 0 < float(d["descent_fraction"]) <= 0.01
    e, n = d["e_canting"][0, 1, 0, :3], d["e_canting"][0, 1, 1, :3]
    assert not np.cross(e, n).any()                                # n parallel to e
    b = d["b_canting"][1, :, :, :3]
    assert (np.abs((b[:, 0] * b[:, 1]).sum(-1)) > 0.05).all()      # n not orthogonal to e


def test_canting_argument_checks_need_no_device():
    from artist_amd import _lib
    fwd, bwd = _lib.lib().art_cant_facets_fwd, _lib.lib().art_cant_facets_bwd
    p = ctypes.c_void_p(16)                                          # (never dereferenced: every call below returns first)
    # nothing to do: no launch, no pointer needed
    for HF, M in ((0, 0), (0, 35), (4, 0)):
        assert fwd(None, None, None, None, 0, HF, M, None, None, None) == 0
    assert fwd(p, p, None, None, 0, 4, 0, None, None, None) == 0                           # (an empty array has no pointer)
    assert bwd(None, None, None, None, None, 0, 0, 35, p, None, None, None, None) == 0
    assert bwd(None, None, None, None, None, 0, 4, 0, p, None, None, None, None) == 0     # (no sum requested: nothing to zero)
    # negative or oversized sizes, whatever the pointers
    for HF, M in ((-1, 35), (4, -1), (1 << 31, 1), (1, 1 << 31)):
        assert fwd(p, None, p, p, 0, HF, M, p, p, None) == _lib.ART_EINVAL, (HF, M)
        assert bwd(p, p, p, p, p, 0, HF, M, p, p, p, None, None) == _lib.ART_EINVAL, (HF, M)
    # forward: null pointers with work to do
    assert fwd(None, None, p, p, 0, 4, 35, p, p, None) == _lib.ART_EINVAL         # no canting
    assert fwd(p, None, None, None, 0, 4, 35, p, p, None) == _lib.ART_EINVAL      # no data at all
    assert fwd(p, None, p, None, 0, 4, 35, None, p, None) == _lib.ART_EINVAL      # points without their output
    assert fwd(p, None, None, p, 0, 4, 35, p, None, None) == _lib.ART_EINVAL      # normals without their output
    assert fwd(p, p, None, p, 0, 4, 35, None, p, None) == _lib.ART_EINVAL         # translations without points
    assert fwd(p, p, p, None, 1, 4, 35, p, None, None) == _lib.ART_EINVAL         # translations with the inverse
    # backward
    assert bwd(p, p, p, p, p, 0, 4, 35, None, None, None, None, None) == _lib.ART_EINVAL      # no output requested
    assert bwd(p, p, p, p, p, 0, 0, 35, None, None, None, None, None) == _lib.ART_EINVAL      # ... whatever the sizes
    assert bwd(None, p, p, p, p, 0, 4, 35, p, p, p, p, None) == _lib.ART_EINVAL               # no canting
    assert bwd(p, p, p, None, p, 0, 4, 35, p, None, None, None, None) == _lib.ART_EINVAL      # grad_data_points without grad_out_points
    assert bwd(p, p, p, p, None, 0, 4, 35, None, p, None, None, None) == _lib.ART_EINVAL      # grad_data_normals without grad_out_normals
    assert bwd(p, None, p, p, p, 0, 4, 35, None, None, p, None, None) == _lib.ART_EINVAL      # grad_canting without the points
    assert bwd(p, p, None, p, p, 0, 4, 35, None, None, p, None, None) == _lib.ART_EINVAL      # grad_canting without the normals
    assert bwd(p, p, p, p, p, 1, 4, 35, None, None, None, p, None) == _lib.ART_EINVAL         # grad_translations with the inverse


def test_perform_canting_is_exported_and_has_no_cpu_fallback():
    import artist_amd
    from artist_amd import ArtistHipError, NURBSSurfaces, ops, perform_canting
    assert perform_canting is ops.perform_canting and artist_amd.perform_canting is perform_canting
    canting = torch.tensor(ref.activate(np.float32([[[0.8025, 0, 0, 0], [0, 0.6375, 0, 0]]]), [2])[None])    # [1,2,2,4]
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        perform_canting(canting, torch.rand(1, 2, 5, 4))
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        perform_canting(canting, torch.rand(1, 2, 5, 4), inverse=True, device=torch.device("cpu"))
    # a canting that learns takes the two-stage route, which has no CPU path either
    surf = NURBSSurfaces(torch.tensor([3, 3]), torch.rand(1, 2, 6, 6, 3), device=torch.device("cpu"))
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        surf(torch.rand(1, 2, 5, 2), canting.clone().requires_grad_(True), torch.zeros(1, 2, 4))
