"""GPU tests (``-m gpu``) of the NURBS evaluation and its adjoint - ``art_nurbs_fwd`` / ``art_nurbs_bwd`` through ``NURBSSurfaces`` -
at the shapes of ``nurbs_ref.CASES``: every branch of artist_amd/csrc/nurbs_kernels.hip that the shape of the call selects (scheme,
row groups, stage-1 passes, rows longer than a wave, strips of one or several lane-steps, the two stage-A paths, four or eight
waves, the generic-degree kernel), against ``nurbs_ref.reference`` - a torch fp64 restatement from the definitions that
tests/test_nurbs_reference_host.py pins to the oracle's fp64 run and to the reference project's fixtures.

Rule of every comparison with the reference (the one of tests/test_gpu_flux_fuzz.py): the yardstick of a case and quantity is the
distance between the oracle's fp32 run (the reference project's own arithmetic, bit-pinned to its fixtures) and the fp64 reference
on that case, computed here and never taken from HIP output; the HIP result must be within ``max(3 x yardstick, floor)`` of the
reference, in relative L2 AND in the largest single entry (max |error| / max |reference|).  Floors: the ones the suite already
asserts for these quantities against the fp32 oracle (test_gpu_parity.py::test_nurbs_forward_backward) - 1e-6 for points, 2e-6
for normals, 2e-5 for the control-point gradient; the factor 3 is the margin the project grants elsewhere for a differently
ordered fp32 sum.  No point is left out of any comparison (the host test asserts that every normal of every case is well defined).
Every test prints error, yardstick and error / bound.

The kernels cannot be asked which scheme they ran, so ``nurbs_ref.plan`` restates the launch decisions, and the engagement check
holds the restatement to what the kernels show: where the plan says the backward is the tensor-product adjoint, two backward passes
give identical bits AND the gradient differs in at least one bit from the scattered scheme's (``ARTIST_HIP_NURBS_GRID=0``) - a case
that silently fell back would have equal bits there and pass everything else.

Measured on an MI355X, over the 29 case variants and three quantities (174 comparisons): the largest error / bound is 0.314
(largest entry of the points of the 50 x 50 grid: error 3.14e-7, yardstick 3.14e-7 - the points are the oracle's bits, so error and
yardstick coincide wherever rule 2 applies); normals: at most 1.87e-7 in the largest entry (0.094 of the bound); control-point
gradient: at most 1.17 yardsticks from the reference (case 17, largest entry: error 3.05e-7, yardstick 2.60e-7) and at most 0.023 of
the bound (case 1 canted: 4.62e-7).  Engagement: on every case whose plan says tensor-product adjoint, between a third (the single point of case 13: 4 of 12) and 97 % (case 3) of the gradient
entries differ in their bits from the scattered scheme's - nothing is exempt.  A row index off
by one in the multi-step strip (the gradient of the next grid row) puts case 1's gradient error at 0.34 (17 000 bounds).
"""
import numpy as np
import pytest
import torch

import nurbs_ref
from conftest import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MARGIN = 3.0
FLOORS = dict(points=1e-6, normals=2e-6, grad=2e-5)
SCHEME_GRADIENT_TOLERANCE = 2e-6          # tensor-product against scattered adjoint (fp64 LDS sums): the existing tolerance
CASE_IDS = [nurbs_ref.case_id(c) for c in nurbs_ref.CASES]
KNOBS = ("ARTIST_HIP_NURBS_GRID", "ARTIST_HIP_NURBS_GROUPS", "ARTIST_HIP_NURBS_BWD_BLOCK")
# Grid cases whose tensor-product gradient may equal the scattered scheme's bit for bit by chance (so few terms per sum that both
# orders round alike); every other case whose plan says `grid` is held to the engagement check.
ENGAGEMENT_EXEMPT = ()

_worst = {"ratio": 0.0, "what": "", "count": 0}


def t(x):
    return torch.from_numpy(np.array(x)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


def max_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("ARTIST_HIP_DEBUG", "1")
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)


def run(case, variant="plain", alone=False, contiguous_uv=False, staged_alignment=False):
    """The case through ``NURBSSurfaces`` on the GPU: points, normals, the control-point gradient for the case's ``g_points`` and
    ``g_normals`` from two backward passes, and the fp32 knot vectors the module evaluated with.  ``alone``: facet (0, 0) only.
    ``staged_alignment``: the ``oriented`` variant as evaluation followed by ``align_surfaces``."""
    from artist_amd import NURBSSurfaces, align_surfaces
    inp = nurbs_ref.make_inputs(case)
    cut = (lambda a: a[:1, :1]) if alone else (lambda a: a)
    cp = t(cut(inp["control_points"])).requires_grad_(True)
    H, F = cp.shape[:2]
    surf = NURBSSurfaces(torch.tensor(case.degrees), cp, uniform=case.uniform, device=DEV)
    if not case.uniform:
        surf.knot_vectors_u = t(inp["knots_u"])[None, None].expand(H, F, -1)
        surf.knot_vectors_v = t(inp["knots_v"])[None, None].expand(H, F, -1)
    uv = t(inp["uv"] if inp["expanded"] else cut(inp["uv"]))
    if inp["expanded"]:
        uv = uv.expand(H, F, -1, -1)
        assert (H == 1 or uv.stride(0) == 0) and (F == 1 or uv.stride(1) == 0)
        if contiguous_uv:
            uv = uv.contiguous()
    canted = variant in ("canted", "oriented")
    cant, tr = (t(cut(inp["canting"])), t(cut(inp["translations"]))) if canted else (None, None)
    ori = t(inp["orientation"][:H]) if variant == "oriented" else None
    if staged_alignment:
        pts, nrm = surf.calculate_surface_points_and_normals(uv, cant, tr)
        pts, nrm = align_surfaces(pts.reshape(H, -1, 4), nrm.reshape(H, -1, 4), ori)
        pts, nrm = pts.reshape(H, F, -1, 4), nrm.reshape(H, F, -1, 4)
    else:
        pts, nrm = surf.calculate_surface_points_and_normals(uv, cant, tr, orientations=ori)
    gp, gn = t(cut(inp["g_points"])), t(cut(inp["g_normals"]))
    (g1,) = torch.autograd.grad([pts, nrm], [cp], [gp, gn], retain_graph=True)
    (g2,) = torch.autograd.grad([pts, nrm], [cp], [gp, gn])
    out = dict(points=n(pts), normals=n(nrm), grad=n(g1), grad_again=n(g2),
               knots=(n(surf.knot_vectors_u[0, 0]).copy(), n(surf.knot_vectors_v[0, 0]).copy()))
    assert all(np.isfinite(out[k]).all() for k in ("points", "normals", "grad", "grad_again"))
    return out


def check(case, variant, got, key, knots):
    """``got[key]`` against the fp64 reference of the case by the rule of the module docstring; returns the failures."""
    ref = nurbs_ref.reference(case, variant, knots)[key]
    orc = nurbs_ref.oracle_run(case, variant, np.float32, knots)[key]
    assert got[key].shape == ref.shape == orc.shape and got[key].dtype == orc.dtype == np.float32
    failures = []
    for norm, fn in (("L2", rel_l2), ("max", max_rel)):
        err, yard = fn(got[key], ref), fn(orc, ref)
        bound = max(MARGIN * yard, FLOORS[key])
        ratio = err / bound
        _worst["count"] += 1
        if ratio > _worst["ratio"]:
            _worst.update(ratio=ratio, what=f"{nurbs_ref.case_id(case)} {variant} {key} {norm}: error {err:.2e}, yardstick {yard:.2e}")
        print(f"{nurbs_ref.case_id(case)} {variant:8s} {key:8s} {norm:3s} error {err:.2e} yardstick {yard:.2e} error/yardstick "
              f"{err / max(yard, 1e-300):9.2e} error/bound {ratio:.3f}   [worst so far {_worst['ratio']:.3f}: {_worst['what']}]")
        if not err <= bound:
            failures.append((variant, key, norm, err, yard, bound))
    return failures


def facets_of(case, plans, want):
    """Index arrays (h, f) of the facets whose plan satisfies ``want`` (all facets share the plan of an expanded point list)."""
    if len(plans) == 1:
        return [(h, f) for h in range(case.H) for f in range(case.F)] if want(plans[0]) else []
    return [(i // case.F, i % case.F) for i, pl in enumerate(plans) if want(pl)]


VARIANT_RUNS = [(c, v) for c in nurbs_ref.CASES
                for v in ["plain"] + (["canted"] if c.name in nurbs_ref.CANTED else []) + (["oriented"] if c.name in nurbs_ref.ORIENTED else [])]


@pytest.mark.parametrize("case,variant", VARIANT_RUNS, ids=[f"{nurbs_ref.case_id(c)}-{v}" for c, v in VARIANT_RUNS])
def test_against_the_fp64_reference(case, variant):
    """Rule 1: points, normals and the control-point gradient against the reference.  Rule 2: where the compile-time-degree
    kernels run on uniform knots (p == q <= 4), the points are the oracle's fp32 bits (the alignment is not part of the oracle:
    not for the ``oriented`` variant)."""
    got = run(case, variant)
    bad = []
    for key in ("points", "normals", "grad"):
        bad += check(case, variant, got, key, got["knots"])
    assert not bad, bad
    p, q = case.degrees
    if p == q and p <= 4 and case.uniform and variant != "oriented":
        np.testing.assert_array_equal(got["points"], nurbs_ref.oracle_run(case, variant, np.float32, got["knots"])["points"])


@pytest.mark.parametrize("case", nurbs_ref.CASES, ids=CASE_IDS)
def test_schemes_agree_and_the_planned_one_ran(case, monkeypatch):
    """Rule 3: with ``ARTIST_HIP_NURBS_GRID=1`` and ``=0`` the points and normals are the same bits and the gradients agree to 2e-6.
    Rule 4 (engagement): on the facets whose plan says the backward is the tensor-product adjoint, two backward passes give
    identical bits and the gradient differs from the scattered scheme's in at least one bit."""
    monkeypatch.setenv("ARTIST_HIP_NURBS_GRID", "1")
    grid = run(case)
    monkeypatch.setenv("ARTIST_HIP_NURBS_GRID", "0")
    scattered = run(case)
    np.testing.assert_array_equal(bits(grid["points"]), bits(scattered["points"]))
    np.testing.assert_array_equal(bits(grid["normals"]), bits(scattered["normals"]))
    err = rel_l2(grid["grad"], scattered["grad"])
    print(f"{nurbs_ref.case_id(case)} gradient, grid scheme on vs off: relative L2 {err:.2e}")
    assert err < SCHEME_GRADIENT_TOLERANCE, err
    planned = facets_of(case, nurbs_ref.plan(case), lambda pl: pl["bwd"]["scheme"] == "grid")
    assert planned or case.name not in nurbs_ref.ENGAGEMENT_AT_LEAST
    assert not set(ENGAGEMENT_EXEMPT) & set(nurbs_ref.ENGAGEMENT_AT_LEAST)
    for h, f in planned:
        np.testing.assert_array_equal(bits(grid["grad"][h, f]), bits(grid["grad_again"][h, f]), err_msg=f"facet {h},{f}: not reproducible")
    if planned and case.name not in ENGAGEMENT_EXEMPT:
        differing = [int((bits(grid["grad"][h, f]) != bits(scattered["grad"][h, f])).sum()) for h, f in planned]
        print(f"{nurbs_ref.case_id(case)} gradient entries whose bits differ between the schemes, per planned facet: "
              f"{differing[:8]}{' ...' if len(differing) > 8 else ''} of {grid['grad'][0, 0].size}")
        assert sum(differing) > 0, "the plan says tensor-product adjoint, the bits say the scattered scheme ran"


@pytest.mark.parametrize("name", nurbs_ref.KNOB_SWEEPS)
def test_launch_geometry_changes_speed_only(name, monkeypatch):
    """Rule 5: the forward's bits do not depend on the number of row groups, nor the gradient's on the number of waves per
    workgroup wherever the plan says the tensor-product adjoint runs at every block size compared (2e-6 otherwise)."""
    case = nurbs_ref.BY_NAME[name]
    base = run(case)
    for groups in ("1", "2", "5", "64"):
        monkeypatch.setenv("ARTIST_HIP_NURBS_GROUPS", groups)
        got = run(case)
        np.testing.assert_array_equal(bits(got["points"]), bits(base["points"]), err_msg=f"points, groups {groups}")
        np.testing.assert_array_equal(bits(got["normals"]), bits(base["normals"]), err_msg=f"normals, groups {groups}")
    monkeypatch.delenv("ARTIST_HIP_NURBS_GROUPS")
    blocks = (64, 128, 256, 512)
    all_grid = all(pl["bwd"]["scheme"] == "grid" for b in (0,) + blocks for pl in nurbs_ref.plan(case, bwd_block_env=b))
    for block in blocks:
        monkeypatch.setenv("ARTIST_HIP_NURBS_BWD_BLOCK", str(block))
        got = run(case)
        if all_grid:
            np.testing.assert_array_equal(bits(got["grad"]), bits(base["grad"]), err_msg=f"gradient, block {block}")
            np.testing.assert_array_equal(bits(got["grad_again"]), bits(base["grad"]), err_msg=f"gradient again, block {block}")
        else:
            assert rel_l2(got["grad"], base["grad"]) < SCHEME_GRADIENT_TOLERANCE, block
    print(f"{nurbs_ref.case_id(case)}: gradient bits compared across blocks {blocks}: {all_grid}")


@pytest.mark.parametrize("name", nurbs_ref.BATCH_INDEPENDENCE)
def test_a_facet_alone_has_the_bits_it_has_in_the_batch(name):
    """Rule 6: facet (0, 0) evaluated alone (H = F = 1: other row groups, and past 1024 facets another block size) - points and
    normals always, the gradient where both plans say tensor-product adjoint."""
    case = nurbs_ref.BY_NAME[name]
    batch, alone = run(case), run(case, alone=True)
    np.testing.assert_array_equal(bits(alone["points"][0, 0]), bits(batch["points"][0, 0]))
    np.testing.assert_array_equal(bits(alone["normals"][0, 0]), bits(batch["normals"][0, 0]))
    both_grid = nurbs_ref.plan(case)[0]["bwd"]["scheme"] == nurbs_ref.plan(case, alone=True)[0]["bwd"]["scheme"] == "grid"
    assert both_grid                                         # (so the host test says of all four cases)
    np.testing.assert_array_equal(bits(alone["grad"][0, 0]), bits(batch["grad"][0, 0]))
    print(f"{nurbs_ref.case_id(case)}: fwd {nurbs_ref.fwd_label(nurbs_ref.plan(case)[0])} | alone {nurbs_ref.fwd_label(nurbs_ref.plan(case, alone=True)[0])}; "
          f"gradient bits compared: {both_grid}")


@pytest.mark.parametrize("name", nurbs_ref.ORIENTED)
def test_layout_of_the_point_list_and_fused_alignment(name):
    """Rule 7: the expanded (stride-0) ``uv`` and a contiguous per-facet copy give identical bits; the fused ``orientations=``
    call equals evaluation followed by ``align_surfaces`` bit for bit forward and within 1e-6 in the gradient."""
    case = nurbs_ref.BY_NAME[name]
    assert nurbs_ref.make_inputs(case)["expanded"] and nurbs_ref.plan(case)[0]["bwd"]["scheme"] == "grid"
    expanded, copied = run(case), run(case, contiguous_uv=True)
    for key in ("points", "normals", "grad"):
        np.testing.assert_array_equal(bits(expanded[key]), bits(copied[key]), err_msg=key)
    fused, staged = run(case, "oriented"), run(case, "oriented", staged_alignment=True)
    np.testing.assert_array_equal(bits(fused["points"]), bits(staged["points"]))
    np.testing.assert_array_equal(bits(fused["normals"]), bits(staged["normals"]))
    err = rel_l2(fused["grad"], staged["grad"])
    print(f"{nurbs_ref.case_id(case)} gradient, fused alignment vs align_surfaces: relative L2 {err:.2e}")
    assert err < 1e-6, err


def test_report_the_largest_error_over_the_module():
    """Runs last: the largest error / bound over every comparison with the reference made above (the number of the module
    docstring and of DESIGN.md 4.3)."""
    print(f"largest error / bound over {_worst['count']} comparisons: {_worst['ratio']:.3f} ({_worst['what']})")
    assert _worst["ratio"] <= 1.0
