"""torch fp64 (CPU) restatement of ``NURBSSurfaces.calculate_surface_points_and_normals`` (artist/nurbs/surfaces.py:475-689) written
from the definitions, not from the kernels' or the oracle's algorithm: dense basis matrices by the Cox-de Boor recursion over the
whole knot vector (no span search, no A2.3), the first derivative as the difference of the degree p-1 bases, S = sum_ab Bu[a] Bv[b]
CP[a][b], the normal as normalize(Su x Sv), canting and translation from ``canting_ref``, the optional alignment ``x @ M^T``, and the
control-point gradient by ``torch.autograd``.  Plus the case table and the input generator that tests/test_nurbs_reference_host.py
and tests/test_gpu_nurbs_shapes.py share, and :func:`plan`, a pure-Python restatement of the launch decisions of
artist_amd/csrc/nurbs_kernels.hip (which scheme, how many passes, strips and waves a shape gets).

TEST INFRASTRUCTURE - not part of the product.  The host test pins this reference to the oracle's fp64 run and to the fixtures
generated from the reference project, and asserts the plan of every case against the labels of the table; the GPU test measures the
HIP kernels against the reference and checks the plan's scheme against what the kernels show (bit-reproducible or not)."""
import collections
import functools
import math

import numpy as np
import torch

import canting_ref

F64 = torch.float64
KNOT_MARGIN = 1e-4        # degree-1 directions (and degree 2 with a repeated knot): no coordinate this close to an interior knot

# The canting of tests/test_gpu_parity.py::test_nurbs_tensor_product_scheme_equals_the_scattered_scheme, w = 0
CANTING = np.array([[0.8, 0.05, 0.0, 0.0], [0.02, 0.6, 0.1, 0.0]], dtype=np.float32)

Case = collections.namedtuple("Case", "name degrees net points H F uniform fwd bwd note")
Case.__new__.__defaults__ = (2, 2, True, None, None, "")

# ``points``: ("grid", Mu, Mv) a cartesian grid (u outer, v inner, vs unsorted), shared by all facets (expanded, stride 0);
#             ("us", (u, ...), Mv) the same with the given u rows;  ("lists", ...) a list per facet, not expanded.
# ``fwd`` / ``bwd``: what :func:`fwd_label` / :func:`bwd_label` must say about the case's :func:`plan` (one entry per point list).
CASES = [
    Case("1", [3, 3], (10, 10), ("grid", 3, 70),
         fwd=["grid, 1 pass, no empty group, long rows"], bwd=["grid, block 512, multi-step, 3 strips, two-lane"],
         note="fwd rows longer than a wave; bwd grid scheme, multi-step strip, two-lane stage A (rows nv 3 = 30 <= 32)"),
    Case("2", [3, 3], (12, 12), ("grid", 2, 65), H=1, F=2,
         fwd=["grid, 1 pass, no empty group, long rows"], bwd=["grid, block 512, multi-step, 2 strips, loop"],
         note="the same, stage A through the loop (36 > 32)"),
    Case("3", [2, 2], (5, 5), ("grid", 70, 70), H=1, F=2,
         fwd=["grid, 1 pass, 3 empty groups of 38, long rows"], bwd=["grid, block 512, multi-step, 70 strips, two-lane"],
         note="fwd 38 row groups, 3 of them empty; bwd 70 strips over 8 waves, multi-step"),
    Case("4", [3, 3], (10, 10), ("grid", 100, 100), H=1, F=1,
         fwd=["grid, 1 pass, 28 empty groups of 78, long rows"], bwd=["grid, block 512, multi-step, 100 strips, two-lane"],
         note="the largest square grid the bwd LDS budget still takes as a grid (65 304 B of 65 536)"),
    Case("5", [3, 3], (10, 10), ("grid", 128, 128), H=1, F=1,
         fwd=["grid, 1 pass, no empty group, long rows"], bwd=["scattered (no room), block 512"],
         note="fwd grid with 128 one-row groups; bwd falls to scattered because the grid does not fit"),
    Case("6", [3, 3], (4, 4), ("grid", 2, 2), H=256, F=4,
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 256, one-step, 1 strip, two-lane"],
         note="four-wave backward (block 256)"),
    Case("7", [3, 3], (4, 4), ("grid", 2, 2), H=255, F=4,
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 1 strip, two-lane"],
         note="the other side of that threshold"),
    Case("8", [6, 6], (8, 9), ("grid", 9, 10),
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 2 strips, loop"],
         note="generic-degree kernel"),
    Case("9", [7, 7], (8, 8), ("grid", 5, 6),
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 1 strip, loop"],
         note="generic-degree kernel, no interior knot at all"),
    Case("10", [7, 1], (9, 3), ("grid", 6, 7),
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 1 strip, loop"],
         note="generic-degree kernel, mixed degrees"),
    Case("11", [3, 3], (6, 6), ("grid", 1, 700),
         fwd=["scattered (no room), 5 groups"], bwd=["scattered (no room), block 512"],
         note="thin list: scattered in both passes, fwd in 5 groups of points"),
    Case("12", [3, 3], (6, 6), ("grid", 700, 1),
         fwd=["scattered (no room), 5 groups"], bwd=["scattered (no room), block 512"],
         note="thin list: scattered in both passes"),
    Case("13", [1, 1], (2, 2), ("grid", 1, 1), H=1, F=1,
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 1 strip, two-lane"],
         note="the smallest legal call"),
    Case("14", [2, 2], (3, 3), ("grid", 5, 16), H=1, F=1,
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 2 strips, both"],
         note="bwd grid, a full strip through the loop, the last strip through the two-lane path"),
    Case("15", [3, 3], (10, 10), ("grid", 14, 15),
         fwd=["grid, 2 passes, no empty group, short rows"], bwd=["grid, block 512, one-step, 4 strips, loop"],
         note="fwd two stage-1 passes (rows_pass 12 < 14 rows); bwd grid"),
    Case("16", [3, 3], (10, 10), ("grid", 70, 3),
         fwd=["grid, 7 passes, no empty group, short rows"], bwd=["scattered (no room), block 512"],
         note="fwd several stage-1 passes; bwd scattered"),
    Case("17", [3, 3], (10, 10), ("lists", ("grid", 3, 70), ("grid", 70, 3), ("grid", 14, 15), ("random", 210)),
         fwd=["grid, 1 pass, no empty group, long rows", "grid, 7 passes, no empty group, short rows",
              "grid, 2 passes, no empty group, short rows", "scattered (no room), 1 group"],
         bwd=["grid, block 512, multi-step, 3 strips, two-lane", "scattered (no room), block 512",
              "grid, block 512, one-step, 4 strips, loop", "scattered (no room), block 512"],
         note="per-facet lists; each facet picks its own scheme; uv not expanded"),
    Case("18", [3, 3], (10, 10), ("us", ("knot", 0.0, 1.0), 70), uniform=False,
         fwd=["grid, 1 pass, no empty group, long rows"], bwd=["grid, block 512, multi-step, 3 strips, two-lane"],
         note="case 1 with non-uniform clamped knots, one interior knot of multiplicity 2 in u; rows on that knot, on 0 and on 1"),
    Case("18b", [3, 3], (10, 10), ("us", (1.0 - 1e-6, "knot", 0.0), 70), uniform=False,
         fwd=["grid, 1 pass, no empty group, long rows"], bwd=["grid, block 512, multi-step, 3 strips, two-lane"],
         note="the same with the first row on 1 - 1e-6 (a fourth row would not fit the backward's LDS budget as a grid)"),
    Case("19", [3, 3], (6, 6), ("us", (0.2, 0.2, 0.5, 0.5), 9),
         fwd=["grid, 1 pass, no empty group, short rows"], bwd=["grid, block 512, one-step, 1 strip, loop"],
         note="row length found as 2 Mv and still a grid"),
    Case("20", [3, 3], (6, 6), ("us", (0.2, 0.2, 0.5, 0.7), 9),
         fwd=["scattered (off grid after a pass), 1 group"], bwd=["scattered (off grid after a pass), block 512"],
         note="row length found as 2 Mv; the off-grid check sends it to the scattered scheme after a wasted pass"),
    Case("21", [3, 3], (10, 10), ("grid", 50, 50), H=3, F=2,
         fwd=["grid, 1 pass, 2 empty groups of 19, short rows"], bwd=["grid, block 512, one-step, 50 strips, two-lane"],
         note="the metric shape, as the anchor"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
CANTED = ["1", "3", "8", "15", "18"]          # also run with canting and translations
ORIENTED = ["1", "15"]                        # also run with fused orientations=
KNOB_SWEEPS = ["1", "3", "6", "15", "21"]
BATCH_INDEPENDENCE = ["1", "3", "14", "21"]
ENGAGEMENT_AT_LEAST = ["1", "2", "3", "4", "14", "15", "21"]


def case_id(case):
    kind = case.points[0]
    shape = f"{case.points[1]}x{case.points[2]}" if kind == "grid" else kind
    return f"case{case.name}-deg{case.degrees[0]}{case.degrees[1]}-net{case.net[0]}x{case.net[1]}-{shape}-H{case.H}F{case.F}"


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def module_knots(case):
    """The knot vectors the product evaluates with, fp32: those ``NURBSSurfaces`` builds for a uniform case, the ones the test
    swaps in for a non-uniform one (cases 18: one interior knot of multiplicity 2 in u)."""
    if case.uniform:
        from artist_amd import NURBSSurfaces
        surf = NURBSSurfaces(torch.tensor(case.degrees), torch.zeros(1, 1, case.net[0], case.net[1], 3), device=torch.device("cpu"))
        return surf.knot_vectors_u[0, 0].numpy().copy(), surf.knot_vectors_v[0, 0].numpy().copy()
    assert case.degrees == [3, 3] and case.net == (10, 10)
    ku = np.array([0, 0, 0, 0, 0.15, 0.3, 0.3, 0.55, 0.7, 0.85, 1, 1, 1, 1], dtype=np.float32)
    kv = np.array([0, 0, 0, 0, 0.1, 0.25, 0.45, 0.6, 0.8, 0.9, 1, 1, 1, 1], dtype=np.float32)
    return ku, kv


def _interior(knots, degree):
    return np.unique(knots[degree + 1:len(knots) - degree - 1])


def needs_knot_margin(knots, degree):
    """Only here is the first derivative discontinuous across an interior knot, so that the side the span rule picks matters."""
    inner = knots[degree + 1:len(knots) - degree - 1]
    return degree == 1 or (degree == 2 and len(np.unique(inner)) < len(inner))


def _coordinates(count, knots, degree, gen, sort):
    """``count`` distinct fp32 coordinates in [0.01, 0.99], away from the interior knots where that matters."""
    x = torch.rand(count, generator=gen) * 0.98 + 0.01
    inner = torch.from_numpy(_interior(knots, degree).astype(np.float32))
    for _ in range(100):
        bad = torch.zeros(count, dtype=torch.bool)
        if needs_knot_margin(knots, degree) and len(inner):
            bad |= ((x[:, None] - inner[None, :]).abs() < 2 * KNOT_MARGIN).any(dim=1)
        bad |= torch.tensor([bool((x[:i] == x[i]).any()) for i in range(count)])
        if not bad.any():
            break
        x[bad] = torch.rand(int(bad.sum()), generator=gen) * 0.98 + 0.01
    assert not bad.any()
    return torch.sort(x).values if sort else x


def _point_list(spec, ku, kv, degrees, gen):
    kind = spec[0]
    if kind == "random":
        return torch.stack([_coordinates(spec[1], ku, degrees[0], gen, False), _coordinates(spec[1], kv, degrees[1], gen, False)], dim=1)
    if kind == "grid":
        us = _coordinates(spec[1], ku, degrees[0], gen, True)
        if spec[1] > 2:                    # both ends of the parameter range, as ARTIST's evaluation grid has them
            us[0], us[-1] = 1e-7, 1.0 - 1e-7
    else:
        knot = float(ku[degrees[0] + 2])
        us = torch.tensor([knot if u == "knot" else u for u in spec[1]], dtype=torch.float32)
    vs = _coordinates(spec[2], kv, degrees[1], gen, False)            # columns in no particular order
    return torch.cartesian_prod(us, vs).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _inputs(name, H, F):
    case = BY_NAME[name]
    gen = torch.Generator().manual_seed(1000 + CASES.index(case))
    ku, kv = module_knots(case)
    nu, nv = case.net
    # a regular x/y lattice with 2 % jitter (of the lattice spacing) and z in [0, 0.05]: every normal is well defined
    x = torch.linspace(-1, 1, nu)[:, None].expand(nu, nv)
    y = torch.linspace(-1, 1, nv)[None, :].expand(nu, nv)
    cp = torch.stack([x, y, torch.zeros(nu, nv)], dim=-1)[None, None].repeat(case.H, case.F, 1, 1, 1)
    jitter = (torch.rand(case.H, case.F, nu, nv, 3, generator=gen) - 0.5) * 2
    cp[..., 0] += jitter[..., 0] * 0.02 * (2.0 / (nu - 1))
    cp[..., 1] += jitter[..., 1] * 0.02 * (2.0 / (nv - 1))
    cp[..., 2] = torch.rand(case.H, case.F, nu, nv, generator=gen) * 0.05
    if case.points[0] == "lists":
        assert len(case.points) - 1 == case.H * case.F
        lists = [_point_list(spec, ku, kv, case.degrees, gen) for spec in case.points[1:]]
        uv = torch.stack(lists).reshape(case.H, case.F, -1, 2).contiguous()
        expanded = False
    else:
        uv = _point_list(case.points, ku, kv, case.degrees, gen)[None, None]
        expanded = True
    M = uv.shape[2]
    g_points = torch.rand(case.H, case.F, M, 4, generator=gen) * 2 - 1
    g_normals = torch.rand(case.H, case.F, M, 4, generator=gen) * 2 - 1
    translations = torch.rand(case.H, case.F, 4, generator=gen)
    translations[..., 3] = 0.0
    # a random rotation with a translation of about 100 m per heliostat
    q = torch.randn(case.H, 4, generator=gen, dtype=F64)
    q = q / q.norm(dim=1, keepdim=True)
    w, a, b, c = q.unbind(1)
    R = torch.stack([1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w),
                     2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w),
                     2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)], dim=1).reshape(case.H, 3, 3)
    ori = torch.zeros(case.H, 4, 4, dtype=F64)
    ori[:, :3, :3] = R
    ori[:, :3, 3] = (torch.rand(case.H, 3, generator=gen, dtype=F64) * 2 - 1) * 100.0
    ori[:, 3, 3] = 1.0
    out = dict(control_points=cp.numpy(), uv=uv.numpy(), expanded=expanded, knots_u=ku, knots_v=kv,
               g_points=g_points.numpy(), g_normals=g_normals.numpy(),
               canting=np.broadcast_to(CANTING, (case.H, case.F, 2, 4)).copy(), translations=translations.numpy(),
               orientation=ori.float().numpy())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def make_inputs(case):
    """fp32 numpy inputs of a case (read-only, shared): ``control_points`` [H,F,nu,nv,3], ``uv`` [1,1,M,2] (to be expanded) or
    [H,F,M,2], ``knots_u/v``, ``g_points``, ``g_normals`` [H,F,M,4], ``canting`` [H,F,2,4], ``translations`` [H,F,4],
    ``orientation`` [H,4,4]."""
    return _inputs(case.name, case.H, case.F)


def full_uv(inp):
    H, F = inp["control_points"].shape[:2]
    return np.broadcast_to(inp["uv"], (H, F) + inp["uv"].shape[2:])


def point_lists(inp):
    """The distinct point lists of a case, [(h, f, uv [M,2])]: one for an expanded ``uv``, one per facet otherwise."""
    if inp["expanded"]:
        return [(0, 0, inp["uv"][0, 0])]
    H, F = inp["uv"].shape[:2]
    return [(h, f, inp["uv"][h, f]) for h in range(H) for f in range(F)]


# ------------------------------------------------------------------------------------------------
# the operation, torch fp64
# ------------------------------------------------------------------------------------------------
def basis_matrices(x, knots, degree):
    """Dense ``(B, dB)`` [M, n_ctrl] of the B-spline basis of ``degree`` on ``knots`` and its first derivative at ``x`` [M], by
    the Cox-de Boor recursion over the whole knot vector.  Degree 0 is the indicator of knot[i] <= x < knot[i+1], with
    x >= last knot in the last non-empty span; a zero-length knot interval contributes zero."""
    x = torch.as_tensor(x, dtype=F64)
    k = torch.from_numpy(np.array(knots, dtype=np.float64))
    K = len(k)
    N = ((k[None, :-1] <= x[:, None]) & (x[:, None] < k[None, 1:])).to(F64)                     # [M, K-1]
    last = max(i for i in range(K - 1) if k[i] < k[i + 1])
    at_end = x >= k[-1]
    N[at_end] = 0.0
    N[at_end, last] = 1.0
    assert bool((N.sum(dim=1) == 1).all()), "a coordinate outside the knot range"

    def ratio(num, den):
        return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)), torch.zeros_like(num))

    lower = N
    for d in range(1, degree + 1):
        lower = N                                                                               # degree d - 1, [M, K-d]
        n = K - d - 1
        left = ratio(x[:, None] - k[None, :n], (k[d:d + n] - k[:n])[None, :].expand(len(x), n))
        right = ratio(k[None, d + 1:d + 1 + n] - x[:, None], (k[d + 1:d + 1 + n] - k[1:1 + n])[None, :].expand(len(x), n))
        N = left * lower[:, :n] + right * lower[:, 1:1 + n]
    n = K - degree - 1
    one = torch.ones(len(x), n, dtype=F64)
    dN = degree * (ratio(one, (k[degree:degree + n] - k[:n])[None, :].expand(len(x), n)) * lower[:, :n]
                   - ratio(one, (k[degree + 1:degree + 1 + n] - k[1:1 + n])[None, :].expand(len(x), n)) * lower[:, 1:1 + n])
    return N, dN


def evaluate(cp, uv, knots_u, knots_v, degrees, canting=None, translations=None, orientation=None):
    """Points and normals [H,F,M,4] (torch fp64, differentiable w.r.t. ``cp``) plus the raw tangents ``Su``, ``Sv`` [H,F,M,3].
    ``uv`` [1,1,M,2] or [H,F,M,2]."""
    H, F = cp.shape[:2]
    uv = torch.from_numpy(np.array(uv, dtype=np.float64))
    Bu, dBu, Bv, dBv = [], [], [], []
    for h in range(uv.shape[0]):
        for f in range(uv.shape[1]):
            a, da = basis_matrices(uv[h, f, :, 0], knots_u, degrees[0])
            b, db = basis_matrices(uv[h, f, :, 1], knots_v, degrees[1])
            Bu.append(a), dBu.append(da), Bv.append(b), dBv.append(db)
    stack = lambda parts: torch.stack(parts).reshape(uv.shape[0], uv.shape[1], *parts[0].shape).expand(H, F, -1, -1)  # noqa: E731
    Bu, dBu, Bv, dBv = stack(Bu), stack(dBu), stack(Bv), stack(dBv)
    S = torch.einsum("hfma,hfmb,hfabk->hfmk", Bu, Bv, cp)
    Su = torch.einsum("hfma,hfmb,hfabk->hfmk", dBu, Bv, cp)
    Sv = torch.einsum("hfma,hfmb,hfabk->hfmk", Bu, dBv, cp)
    cross = torch.linalg.cross(Su, Sv, dim=-1)
    normal = cross / cross.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    points = torch.cat([S, torch.ones_like(S[..., :1])], dim=-1)
    normals = torch.cat([normal, torch.zeros_like(normal[..., :1])], dim=-1)
    if canting is not None:
        # canting_ref.rotate is numpy (no autograd): the rotation is linear in the data, so its matrix comes from rotating the
        # unit vectors, and the translation from rotating the origin
        eye = np.broadcast_to(np.eye(4)[:3], (H, F, 3, 4))
        B = torch.from_numpy(canting_ref.rotate(canting, eye)[..., :3])                       # [H,F,3(k),3(j)]: out_j = sum_k x_k B[k][j]
        tr = torch.from_numpy(canting_ref.rotate(canting, np.zeros((H, F, 1, 4)), translations=translations)[..., 0, :])
        points = torch.cat([torch.einsum("hfmk,hfkj->hfmj", points[..., :3], B), points[..., 3:]], dim=-1) + tr[:, :, None, :]
        normals = torch.cat([torch.einsum("hfmk,hfkj->hfmj", normals[..., :3], B), normals[..., 3:]], dim=-1)
    if orientation is not None:
        Mo = torch.from_numpy(np.array(orientation, dtype=np.float64))
        points = torch.einsum("hfmj,hij->hfmi", points, Mo)
        normals = torch.einsum("hfmj,hij->hfmi", normals, Mo)
    return points, normals, Su, Sv


VARIANTS = ("plain", "canted", "oriented")


def reference_on(inp, degrees, variant="plain", knots=None):
    """``dict(points, normals, grad, su, sv)`` (numpy fp64) of the inputs ``inp`` (the fp32 values the GPU gets, cast to double)."""
    ku, kv = knots if knots is not None else (inp["knots_u"], inp["knots_v"])
    cp = torch.from_numpy(np.array(inp["control_points"], dtype=np.float64)).requires_grad_(True)
    canted = variant in ("canted", "oriented")
    points, normals, Su, Sv = evaluate(cp, inp["uv"], ku, kv, degrees,
                                       inp["canting"] if canted else None, inp["translations"] if canted else None,
                                       inp["orientation"] if variant == "oriented" else None)
    (grad,) = torch.autograd.grad([points, normals], [cp], [torch.from_numpy(np.array(inp["g_points"], dtype=np.float64)),
                                                            torch.from_numpy(np.array(inp["g_normals"], dtype=np.float64))])
    out = dict(points=points.detach().numpy(), normals=normals.detach().numpy(), grad=grad.numpy(),
               su=Su.detach().numpy(), sv=Sv.detach().numpy())
    for v in out.values():
        v.setflags(write=False)
    return out


_REFERENCES = {}


def reference(case, variant="plain", knots=None):
    """The fp64 reference of a case (computed once per case, variant and knot bits; read-only).  ``knots``: the fp32 knot
    vectors the module under test actually holds, when they were built elsewhere than :func:`module_knots` builds them."""
    inp = make_inputs(case)
    ku, kv = knots if knots is not None else (inp["knots_u"], inp["knots_v"])
    key = (case.name, variant, np.asarray(ku, np.float32).tobytes(), np.asarray(kv, np.float32).tobytes())
    if key not in _REFERENCES:
        _REFERENCES[key] = reference_on(inp, case.degrees, variant, (ku, kv))
    return _REFERENCES[key]


def oracle_run(case, variant="plain", dtype=np.float32, knots=None):
    """The C oracle (the reference project's algorithm and operation order) on a case in ``dtype``: ``dict(points, normals,
    grad)``.  The alignment of the ``oriented`` variant is not part of the oracle's NURBS entry points: it is applied here in
    ``dtype`` around them (points @ M^T after, gradients @ M before)."""
    import oracle
    inp = make_inputs(case)
    ku, kv = knots if knots is not None else (inp["knots_u"], inp["knots_v"])
    c = lambda a: np.ascontiguousarray(a, dtype=dtype)  # noqa: E731
    canted = variant in ("canted", "oriented")
    cant, tr = (c(inp["canting"]), c(inp["translations"])) if canted else (None, None)
    kw = dict(knots_u=c(ku), knots_v=c(kv), uniform=case.uniform)
    uv = c(full_uv(inp))
    pts, nrm = oracle.nurbs_fwd(c(inp["control_points"]), uv, case.degrees, cant, tr, **kw)
    gp, gn = c(inp["g_points"]), c(inp["g_normals"])
    if variant == "oriented":
        Mo = c(inp["orientation"])
        pts, nrm = np.einsum("hfmj,hij->hfmi", pts, Mo), np.einsum("hfmj,hij->hfmi", nrm, Mo)
        gp, gn = np.einsum("hfmi,hij->hfmj", gp, Mo), np.einsum("hfmi,hij->hfmj", gn, Mo)
    grad = oracle.nurbs_bwd(c(inp["control_points"]), uv, case.degrees, c(gp), c(gn), cant, **kw)
    return dict(points=pts, normals=nrm, grad=grad)


# ------------------------------------------------------------------------------------------------
# the launch decisions of artist_amd/csrc/nurbs_kernels.hip, restated
# ------------------------------------------------------------------------------------------------
K_MAX_DEG, K_SCATTER_THREADS, K_FWD_BLOCK = 7, 256, 64      # nurbs_basis.hpp:10, nurbs_kernels.hip:303, :46


def _ceil_div(a, b):
    return (a + b - 1) // b


def _row_length(uv):
    """find_row_length (nurbs_kernels.hip:185-196): the index of the first point whose u differs from point 0's, else M."""
    differs = np.nonzero(uv[:, 0] != uv[0, 0])[0]
    return int(differs[0]) if len(differs) else len(uv)


def _on_grid(uv, Mv):
    """The check of nurbs_kernels.hip:361 / :542: every point against (u of its row's first point, v of its column's first)."""
    g = uv.reshape(-1, Mv, 2)
    return bool((g[:, :, 0] == g[:, :1, 0]).all() and (g[:, :, 1] == g[:1, :, 1]).all())


def plan_list(uv, degrees, net, HF, groups_env=0, bwd_block_env=0, grid_mode=1):
    """``dict(fwd=..., bwd=...)`` for one facet's point list ``uv`` [M,2] (fp32) in a launch of ``HF`` facets."""
    p, q = degrees
    nu, nv = net
    M = len(uv)
    ncp = nu * nv * 3
    n0 = (ncp + (nu + p + 1) + (nv + q + 1) + 12 + 1) & ~1                                   # nurbs_f64_offset, :68-72
    deg = p if (p == q and p <= 4) else 0                                                    # :648, :675
    W = 2 * ((deg if deg > 0 else K_MAX_DEG) + 1) + 3                                        # BasisRec, :200 / :649
    side = math.isqrt(M - 1) + 1 if M > 1 else 1                                             # :653-654: smallest side^2 >= M
    Mv = _row_length(uv) if grid_mode else 0                                                 # :329, :473
    divides = Mv > 0 and M % Mv == 0                                                         # :330, :474
    Mu = M // Mv if divides else 0
    on_grid = divides and _on_grid(uv, Mv)

    # ---- forward: art_nurbs_fwd :701-712, nurbs_lds_bytes :650-666, nurbs_fwd_kernel :327-369
    groups = groups_env
    if groups <= 0:
        groups = 1
        while HF * groups < 4096 and M // (groups + 1) >= 128:                               # :705
            groups += 1
    groups = min(groups, M)                                                                  # :707
    lds = n0 + K_FWD_BLOCK * 2 * W                                                           # :650 (scattered)
    if grid_mode:
        rows = _ceil_div(side, groups)                                                       # :657
        grid = n0 + (rows + side) * W + min(rows, max(1, 128 // nv)) * nv * 6 + 64           # :658, :663
        if grid * 4 <= 64 * 1024:                                                            # :664
            lds = max(lds, grid)
    fwd = dict(groups=groups, Mv=Mv, Mu=Mu, lds_bytes=lds * 4, scheme="scattered", why="ragged", rows_per_group=0, rows_pass=0,
               passes=0, empty_groups=0, long_rows=False)
    if not grid_mode:
        fwd["why"] = "grid scheme off"
    elif divides:
        rpg = _ceil_div(Mu, groups)                                                          # :332
        room = lds - (n0 + Mv * W + rpg * W)                                                 # :335-338
        rows_pass = min(rpg, room // (nv * 6)) if room > 0 else 0                            # :339
        rows_pass = min(rows_pass, max(1, 128 // nv))                                        # :340
        fwd.update(rows_per_group=rpg, rows_pass=rows_pass, why="no room")
        if rows_pass >= 1:                                                                   # :341
            fwd.update(scheme="grid" if on_grid else "scattered", why="" if on_grid else "off grid after a pass",
                       passes=_ceil_div(min(rpg, Mu), rows_pass),                            # :351 (the fullest group)
                       empty_groups=groups - _ceil_div(Mu, rpg),                             # :333, :343
                       long_rows=Mv > K_FWD_BLOCK)                                           # :344, :355: more than one lane-step

    # ---- backward: art_nurbs_bwd :737-741, nurbs_lds_bytes :650-666, nurbs_bwd_kernel :473-598
    block = bwd_block_env if bwd_block_env in (64, 128, 256, 512) else (512 if HF < 1024 else 256)   # :738
    waves = block // 64
    lds = n0 + 2 * ncp + K_SCATTER_THREADS * 2 * W                                           # :650 (scattered)
    if grid_mode:
        rs = max(1, 64 // side)                                                              # :660
        grid = n0 + 2 + 2 * (nu + nv) + 2 * side * W + side * nv * 6 + waves * rs * (nv * 6 + side * 9) + 64   # :661, :663
        if grid * 4 <= 64 * 1024:
            lds = max(lds, grid)
    bwd = dict(block=block, Mv=Mv, Mu=Mu, lds_bytes=lds * 4, scheme="scattered", why="ragged", rows_per_strip=0, one_step=None,
               n_strips=0, stage_a=None)
    if not grid_mode:
        bwd["why"] = "grid scheme off"
    elif divides:
        s_wave = n0 + 2 + 2 * nv + 2 * nu + Mu * W + Mv * W + Mu * nv * 6                    # :478-484
        rs = max(1, 64 // Mv)                                                                # :485
        per_wave = rs * (nv * 6 + Mv * 9)                                                    # :486
        bwd.update(rows_per_strip=rs, why="no room", needed_bytes=(s_wave + waves * per_wave) * 4)
        if s_wave + waves * per_wave <= lds:                                                 # :487
            n_strips = _ceil_div(Mu, rs)                                                     # :512
            paths = {"two-lane" if min(rs, Mu - s * rs) * nv * 3 <= 32 else "loop" for s in range(n_strips)}   # :526, :551-552
            bwd.update(scheme="grid" if on_grid else "scattered", why="" if on_grid else "off grid after a pass",
                       n_strips=n_strips, one_step=rs * Mv <= 64,                            # :516
                       stage_a="both" if len(paths) == 2 else paths.pop())
    return dict(fwd=fwd, bwd=bwd)


def plan(case, groups_env=0, bwd_block_env=0, grid_mode=1, alone=False):
    """The launch plan of a case, one ``dict(fwd, bwd)`` per distinct point list (:func:`point_lists`).  ``alone``: facet (0, 0)
    evaluated on its own (H = F = 1)."""
    inp = make_inputs(case)
    lists = point_lists(inp)[:1] if alone else point_lists(inp)
    HF = 1 if alone else case.H * case.F
    return [plan_list(uv, case.degrees, case.net, HF, groups_env, bwd_block_env, grid_mode) for _, _, uv in lists]


def _count(n, word):
    return f"{n} {word}" + ("" if n == 1 else ("es" if word.endswith("s") else "s"))


def fwd_label(pl):
    f = pl["fwd"]
    if f["scheme"] != "grid":
        return f"scattered ({f['why']}), {_count(f['groups'], 'group')}"
    empty = f"{_count(f['empty_groups'], 'empty group')} of {f['groups']}" if f["empty_groups"] else "no empty group"
    return f"grid, {_count(f['passes'], 'pass')}, {empty}, {'long' if f['long_rows'] else 'short'} rows"


def bwd_label(pl):
    b = pl["bwd"]
    if b["scheme"] != "grid":
        return f"scattered ({b['why']}), block {b['block']}"
    return (f"grid, block {b['block']}, {'one-step' if b['one_step'] else 'multi-step'}, {_count(b['n_strips'], 'strip')}, "
            f"{b['stage_a']}")


def features(pl):
    """The ``(pass, label)`` pairs a plan shows - what the coverage check of the host test counts."""
    f, b = pl["fwd"], pl["bwd"]
    out = {("fwd", f["scheme"]), ("bwd", b["scheme"]), ("bwd", f"block {b['block']}")}
    if f["scheme"] == "grid":
        out |= {("fwd", "one pass" if f["passes"] == 1 else "several passes"), ("fwd", "long rows" if f["long_rows"] else "short rows")}
        if f["empty_groups"]:
            out.add(("fwd", "empty group"))
    if b["scheme"] == "grid":
        out |= {("bwd", "one-step" if b["one_step"] else "multi-step"), ("bwd", "stage A " + b["stage_a"])}
    return out


ALL_FEATURES = ({("fwd", x) for x in ("grid", "scattered", "one pass", "several passes", "empty group", "long rows", "short rows")}
                | {("bwd", x) for x in ("grid", "scattered", "one-step", "multi-step", "stage A two-lane", "stage A loop",
                                        "stage A both", "block 512", "block 256")})
