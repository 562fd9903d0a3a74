"""The reference the GPU fuzz of the flux epilogue leans on (tests/test_gpu_flux_fuzz.py), pinned on the CPU and independently of any
HIP code: for every case of ``flux_ref.CASES`` the C oracle's fp64 chain (``oracle.flux_crop`` -> ``oracle.pixel_loss`` /
``oracle.kl_loss`` -> ``oracle.flux_crop(grad_out=...)``, ``oracle.center_of_mass``) against the torch fp64 autograd restatement of
tests/flux_ref.py.  Both sides are fp64 and differ in the order of their sums only: 1e-10 relative L2 (measured: 3e-12 at most).

No bitmap of the table is one pixel wide or high, so ``affine_grid``'s own ``linspace(-1, 1, 1)`` never enters; such a shape
would have to be checked against the oracle alone.

The inputs also have to keep away from the crop's kinks: its gradient through the centre of mass jumps where a sampling
coordinate is an integer, and two correct evaluations in different precisions may then land on different sides.  That is a
condition on the inputs (the generator draws a bitmap again until it holds), asserted here for every non-empty bitmap of every
case."""
import numpy as np
import pytest

import flux_ref
from conftest import rel_l2

BOUND = 1e-10
_worst = {}


@pytest.mark.parametrize("case", flux_ref.CASES, ids=flux_ref.case_id)
def test_oracle_chain_matches_torch_fp64(case):
    inp = flux_ref.make_inputs(case)
    ref, orc = flux_ref.reference(inp), flux_ref.oracle_f64(case)
    assert set(ref) == set(orc)
    errs = {k: rel_l2(orc[k], ref[k]) for k in sorted(ref)}
    _worst[case] = max(errs.values())
    print(f"{flux_ref.case_id(case)}: oracle fp64 vs torch fp64, rel L2: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    print(f"maximum so far over {len(_worst)} cases: {max(_worst.values()):.2e}")
    for k, v in errs.items():
        assert orc[k].shape == ref[k].shape and np.isfinite(orc[k]).all(), k
        assert v <= BOUND, (k, v)
    # the empty bitmap: a crop of zeros, and finite gradients
    assert not inp["flux"][0].any() and not ref["crop"][0].any()
    assert all(np.isfinite(ref[k][0]).all() for k in ref)


@pytest.mark.parametrize("case", flux_ref.CASES, ids=flux_ref.case_id)
def test_sampling_coordinates_keep_away_from_integers(case):
    inp = flux_ref.make_inputs(case)
    dist = flux_ref.integer_distance(inp["flux"], inp["dims"])
    live = inp["flux"].reshape(case.B, -1).any(axis=1)
    assert live[1:].all() and not live[0]
    print(f"{flux_ref.case_id(case)}: smallest distance of an in-frame sampling coordinate from an integer {dist[live].min():.2e} px")
    assert (dist[live] > flux_ref.KINK_PX).all(), np.nonzero(live & ~(dist > flux_ref.KINK_PX))[0]


def _case(Hh, W, scale_x=None, scale_y=None, B=None):
    found = [c for c in flux_ref.CASES if (c.Hh, c.W) == (Hh, W) and scale_x in (None, c.scale_x) and scale_y in (None, c.scale_y)
             and B in (None, c.B)]
    assert len(found) == 1, found
    return found[0]


def test_table_reaches_the_backward_paths_it_names():
    """flux_crop_bwd_tiled_kernel's choice of path, restated on the host (flux_ref.backward_paths), for the inputs of the table."""
    paths = {c: flux_ref.backward_paths(c) for c in flux_ref.CASES}
    for c, p in paths.items():
        print(flux_ref.case_id(c), sorted(p))
    assert {"tiled", "taps3", "taps4"} <= paths[_case(33, 65)] and not paths[_case(33, 65)] & {"wide", "rows64"}
    assert {"wide", "gather4", "gather8"} <= paths[_case(40, 70, 0.45)] and "general" not in paths[_case(40, 70, 0.45)]
    assert "rows64" in paths[_case(70, 40, scale_y=0.505)] and "wide" not in paths[_case(70, 40, scale_y=0.505)]
    assert {"wide", "gather8"} <= paths[_case(36, 68)]
    assert {"wide", "general"} <= paths[_case(20, 24)]
    assert paths[_case(48, 64)] == {"tiled"}                                   # zoom-out: every input pixel has a candidate
    for c in (_case(40, 70, 0.55), _case(70, 40, scale_y=0.52), _case(9, 300)):
        assert "tiled" in paths[c] and not paths[c] & {"wide", "rows64"}, c
    for c in (_case(5, 3), _case(2, 2), _case(4, 2)):
        assert {"tiled", "narrow"} <= paths[c] and not paths[c] & {"wide", "rows64"}, c
    assert any("unsampled" in p for p in paths.values())                       # zoom-in: input pixels outside the crop window


def test_table_reaches_the_fused_forward_paths_it_names():
    """art_flux_crop_pixel_loss_fwd's launch rules, restated on the host (flux_ref.fused_forward_plan)."""
    plan = {c: flux_ref.fused_forward_plan(c) for c in flux_ref.CASES}
    for c, p in plan.items():
        print(flux_ref.case_id(c), p)
    for c in (_case(5, 4), _case(16, 64), _case(56, 1024)):                    # staged, every part
        assert plan[c]["stage_rows"] > 0 and plan[c]["staged"] == 4 * (c.B - 1) and plan[c]["refused"] == 0, c
    assert plan[_case(64, 64)]["refused"] > 0 and plan[_case(64, 64)]["stage_rows"] > 0
    assert plan[_case(128, 512)]["stage_bytes"] == 73728 and plan[_case(128, 512)]["staged"] == 4
    assert plan[_case(56, 1024)]["stage_bytes"] == 73728
    for c in (_case(160, 512), _case(64, 1024)):                               # too large to stage, yet column owners
        assert plan[c]["column_owner"] and plan[c]["stage_rows"] == 0, c
    for c in (_case(33, 17), _case(60, 100)):
        assert not plan[c]["column_owner"], c
    assert plan[_case(2, 8)]["empty"] == 2 * 2 and plan[_case(2, 8)]["staged"] == 2 * 2
    assert plan[_case(3, 6)]["empty"] == 2 * 1 and not plan[_case(3, 6)]["column_owner"]
    assert plan[_case(8, 8, B=129)]["workgroups"] == 1 and plan[_case(8, 8, B=129)]["staged"] == 4 * 128
    assert plan[_case(8, 8, B=512)]["stage_rows"] > 0                          # (four workgroups per bitmap are forced by the test)
    assert plan[_case(8, 8, B=513)]["workgroups"] == 1
    assert all(p["workgroups"] == 4 for c, p in plan.items() if c.B <= 3 and c.Hh >= 4)       # small batches: the knob matters


def test_table_reaches_what_it_names():
    """Properties of the inputs that the notes of the table promise, checked where they can be without a kernel."""
    zero_in_crop = [c for c in flux_ref.CASES if (flux_ref.oracle_f64(c)["crop"][1:] == 0).any()]
    assert any(c.W % 4 == 0 for c in zero_in_crop) and any(c.W % 4 != 0 for c in zero_in_crop)     # log(0 + 1e-12) terms, both loops
    assert {(c.Hh * c.W) % 4 == 0 for c in flux_ref.CASES} == {True, False}
    one = [c for c in flux_ref.CASES if c.scale_x == 1.0][0]
    inp = flux_ref.make_inputs(one)
    assert float(6.0 / inp["dims"][0, 0]) == 1.0
    com = flux_ref.oracle_f64(one)["com"]
    assert (np.abs(com[1:, 0] - (one.W - 1) / 2) > 1.0).all()                  # off centre
