#!/usr/bin/env python3
"""Branch fields for the rigid-body kinematics: the reference's ``RigidBody`` (artist/field/kinematics_rigid_body.py) with
its linear and ideal actuators on SYNTHETIC parameter tables in which every data-dependent branch of the iteration is taken
by a designed class of heliostats (runs ONLY in the build container, like generate_golden.py).

TEST INFRASTRUCTURE - not part of the product.  ``RigidBody`` objects are built directly from tables (no scenario file) and
run on the CPU, once in fp32 and once in fp64 ON THE SAME INPUT VALUES: every table is drawn in fp64, rounded to fp32 and
stored once as fp32; the fp64 runs read those values cast up.  The methods of the instances are wrapped to record what
passes through them; nothing of the reference is changed or copied.

Linear field, H = 203 (not a multiple of 64; 19 * 203 not a multiple of 256); ideal field, H = 65 (four-row actuator
tables).  Positions over +-80 m x 20..150 m, all four rotation deviations (sigma 0.03 rad, every seventh heliostat up to
0.2 rad), all nine translation deviations (sigma 0.15 m), incident directions, aim points and actuator tables of each
heliostat's own.  Classes (index arrays ``lin_cls_*`` / ``ideal_cls_*``, all taken FROM THE CENSUS of the reference's own
intermediate tensors, the designed blocks below are only the means to fill them):

 1. clockwise flags: ``cw00 cw01 cw10 cw11`` (actuator 1, actuator 2), heliostat h has combination h % 4; the initial
    angle of a flipped actuator is moved to the other end of its travel so that it covers the same joint angles.
 2. inverse solution: ``sol1`` (solution 1 valid at every iteration), ``sol2`` (1 invalid, 2 valid, at every iteration),
    ``neither`` (both invalid at every iteration: the reference falls to solution 2), ``choice_changes`` (the choice is
    not the same at all ten iterations).  Designed by a first pass with wide motor ranges that records both candidates
    and a second pass with the ranges put around / between them.
 3. stroke clamp in motor->angle, given-motor mode: ``given_lo1 given_hi1 given_lo2 given_hi2 given_both``.
 4. stroke clamp in angle->motor, iterative mode: ``a2m_stroke_hi`` / ``a2m_stroke_lo``.  The stroke there is
    sqrt(o^2 + p^2 - 2 o p c) with |c| <= 1 - 1e-6, which stays inside [|o-p|, o+p] whatever the joint angle is: the clamp
    only cuts the last 1e-6 m, so it is active over a joint-angle window of width ~ sqrt(1e-6 (o+p) / (o p)).  With
    ordinary geometry (o, p ~ 0.3 m) that window is 3.5e-3 rad and no margin fits; with o = p ~ 1e-4 m (high end) and
    ~ 1e-5 m (low end) it is 0.18 / 0.1 rad wide and starts outside the cos clamp's own window, so those heliostats carry
    such (unphysical, but valid) actuators and an initial angle placed from the first pass's joint angles.
 5. ``acos`` clamp in motor->angle: ``acos_clamp``, o = p = 30 m (1/o + 1/p < 1), reached at the stroke limit in the
    given-motor mode.  Its band is 1e-6 wide, see Margins.
 6. ``cos`` clamp in angle->motor: LEFT OUT.  It is active only where |cos| > 1 - 1e-6, a band narrower than any margin of
    1e-3 of the operand's scale (1): not reachable with a margin.  The census asserts that it is never active.
 7. softplus: ``softplus_log_offset`` / ``softplus_log_pivot`` / ``softplus_log_stroke`` and ``softplus_pass_*`` (raw
    value below / above 0.2 = 20 / beta).
 8. saturated ``asin`` ratio: ``asin_saturated`` (8 heliostats, members of no other class, fourth rotation deviation 1.2 rad so that den = 0.36 and
    the desired normal's east component lies beyond it).  Forward only; ``lin_asin_grad_finite_f32`` records whether the
    reference's own fp32 gradients are finite there.

Margins.  Every branch predicate is recomputed from the reference's own tensors (the recorded inputs of
``angles_to_motor_positions``, ``_motor_positions_to_absolute_angles``, ``_compute_motor_positions_from_normal`` and
``_physics_informed_parameters``, pushed through the same expressions in the run's dtype), for every heliostat and every one
of the ten iterations.  Asserted: (a) the fp32 and the fp64 run are on the same side of every predicate; (b) the fp64
operand is at least 1e-3 of its scale away from the threshold - scale = o + p for strokes, 1 for cosines and the asin
ratio, 20 for the softplus argument, max(|motor position|, |bound|) for each bound of the motor range (validity).  Three places
where (b) cannot hold by construction are treated as follows and nowhere else:
  - the acos argument of a stroke that sits ON its clamp is -1 + (o+p) 1e-6 / (o p) (or 1 - |o-p| 1e-6 / (o p)), a
    constant of the geometry within 1e-5 of the clamp whichever side it is on: asserted to be at least half the band
    (5e-7) from the threshold, which is eight fp32 ulps of the operand;
  - the motor->angle stroke of a motor position that angle->motor has just produced FROM a clamped stroke equals the clamp
    value up to rounding: both sides give the same value and the same (zero) derivative; excluded from (a) and (b);
  - the stopping rule compares max_h |loss_k - loss_k-1| with min_eps: at least 5 % of min_eps away, for min_eps >= 1e-4.
    With min_eps = 1e-30 the loop stops only at an exact fixed point of the arithmetic, which depends on the dtype: the
    evaluation counts are stored per dtype and results do not depend on them.

Stored per field: the inputs; orientations, final motor positions and the number of forward evaluations (counted by
wrapping ``_compute_orientations_from_motor_positions``) for (max_num_iterations, min_eps) in PAIRS on the whole field and
on the prefixes 1, 63, 65; the given-motor mode; gradients of (W * orientation).sum() for three weightings W w.r.t. the
rotation deviations, the translation deviations and the optimisable actuator parameters at max_num_iterations 1, 2, 4, and
the same plus the motor positions in the given-motor mode (the fp64 run's gradients are stored rounded to fp32 to keep the
file under 1 MB: every comparison made with them has a floor of 1e-5 of their scale or more).  ``lin_stop_pair`` = (pair, prefix, evaluations on the prefix,
evaluations on the whole field, heliostat): the prefix stops earlier than the field and that heliostat's orientation
differs between the two by more than 1e-3 (10 x the comparison bound) - heliostat 0 is tuned (one initial angle, by
bisection) so that its loss after the first update equals its loss at zero motors to within 5e-4.

Usage:  python tests/golden/generate_kinematics_branches_golden.py        (writes tests/golden/kinematics_branches.npz)
"""
from __future__ import annotations

import os
import pathlib
import sys
import tempfile
import types

REFERENCE = os.environ.get("ARTIST_REFERENCE", "/root/reference")
OUT_DIR = pathlib.Path(__file__).resolve().parent


def _import_reference():
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    class _Fmt:  # colorlog.ColoredFormatter stand-in (logging colours only)
        def __init__(self, *a, **k):
            pass

    stub("colorlog", ColoredFormatter=_Fmt)
    sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
    from artist_amd import h5lite
    stub("h5py", File=h5lite.File, Group=h5lite.Group, Dataset=h5lite.Dataset)
    stub("torchvision")
    stub("torchvision.transforms")
    stub("paint")
    stub("paint.util")
    pm = stub("paint.util.paint_mappings")
    pm.__getattr__ = lambda n: n
    sys.path.insert(0, REFERENCE)
    os.chdir(tempfile.mkdtemp(prefix="artist_ref_cwd_"))
    import artist.field  # noqa: F401  (must come first)


_import_reference()

import logging  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
from artist.field.kinematics_rigid_body import RigidBody  # noqa: E402
from artist.geometry import transforms  # noqa: E402

logging.disable(logging.WARNING)          # "No valid motor position combination ..." is what the neither class is for
CPU = torch.device("cpu")
SEED = 20260519
H_LINEAR, H_IDEAL = 203, 65
PAIRS = [(1, 1e-4), (2, 1e-4), (4, 1e-4), (10, 1e-3), (10, 1e-30)]
PREFIXES = [1, 63, 65]
GRAD_ITERATIONS = [1, 2, 4]
N_CENSUS = 10
WIDE = 3.0e5                              # motor range that never binds (linear); the ideal field uses 10 rad
MARGIN = 1e-3
BAND = 1e-6
DTYPES = ((torch.float32, "f32"), (torch.float64, "f64"))

# designed blocks of the linear field (the classes themselves come from the census)
B_STOP = [0]
B_ASIN = list(range(8, 16))
B_SOL2 = list(range(16, 24)) + list(range(140, 144))
B_NEITHER = list(range(24, 32)) + list(range(144, 148))
B_CHANGE = list(range(32, 40)) + list(range(148, 160))
B_A2M_HI = list(range(40, 48))
B_A2M_LO = list(range(48, 56))
B_ACOS = list(range(56, 64)) + [64, 65]
B_SP_GEOM = list(range(66, 74))
B_SP_STROKE = list(range(74, 82))
B_GIVEN = {"lo1": list(range(90, 98)), "hi1": list(range(98, 106)), "lo2": list(range(106, 114)),
           "hi2": list(range(114, 122)), "both": list(range(122, 130))}


def npy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def softplus100(x):
    x = np.asarray(x, np.float64)
    return np.where(100.0 * x > 20.0, x, np.log1p(np.exp(np.minimum(100.0 * x, 20.0))) / 100.0)


def inverse_softplus100(y):
    """raw value whose softplus(beta=100) is y, for y below the pass-through threshold."""
    return np.log(np.expm1(100.0 * np.asarray(y, np.float64))) / 100.0


# -------------------------------------------------------------------------------------- the tables
def linear_tables(rng):
    H = H_LINEAR
    pos = np.concatenate([rng.uniform(-80, 80, (H, 1)), rng.uniform(20, 150, (H, 1)), rng.uniform(0, 3, (H, 1)),
                          np.ones((H, 1))], 1)
    rot = rng.normal(0, 0.03, (H, 4))
    seventh = np.arange(H) % 7 == 3
    rot[seventh] = rng.uniform(-0.2, 0.2, (int(seventh.sum()), 4))
    trans = rng.normal(0, 0.15, (H, 9))
    sun = np.concatenate([rng.uniform(-0.35, 0.35, (H, 1)), rng.uniform(0.8, 1.0, (H, 1)), rng.uniform(-0.6, -0.25, (H, 1))], 1)
    incident = np.concatenate([sun / np.linalg.norm(sun, axis=1, keepdims=True), np.zeros((H, 1))], 1)
    aim = np.concatenate([rng.uniform(-5, 5, (H, 1)), rng.uniform(-4, 0, (H, 1)), rng.uniform(25, 50, (H, 1)), np.ones((H, 1))], 1)

    # geometry in metres (after softplus), drawn around the reference's fitted actuators
    off = rng.uniform(0.30, 0.36, (H, 2))
    piv = off + rng.uniform(-0.04, 0.04, (H, 2))
    s0 = rng.uniform(0.06, 0.09, (H, 2))
    off[B_SP_GEOM], s0[B_SP_GEOM] = rng.uniform(0.13, 0.17, (8, 2)), rng.uniform(0.03, 0.04, (8, 2))
    piv[B_SP_GEOM] = off[B_SP_GEOM] + rng.uniform(-0.015, 0.015, (8, 2))
    off[B_SP_STROKE], piv[B_SP_STROKE], s0[B_SP_STROKE] = rng.uniform(0.6, 0.7, (8, 2)), rng.uniform(0.6, 0.7, (8, 2)), rng.uniform(0.22, 0.27, (8, 2))
    off[B_ACOS], piv[B_ACOS], s0[B_ACOS] = 30.0, 30.0, rng.uniform(6.0, 7.0, (len(B_ACOS), 2))
    off[B_A2M_HI, 0] = piv[B_A2M_HI, 0] = 1.0e-4
    s0[B_A2M_HI, 0] = rng.uniform(2.0e-5, 3.0e-5, len(B_A2M_HI))
    off[B_A2M_LO, 1] = piv[B_A2M_LO, 1] = 1.0e-5
    s0[B_A2M_LO, 1] = rng.uniform(4.0e-6, 6.0e-6, len(B_A2M_LO))
    low_rows = B_GIVEN["lo1"] + B_GIVEN["lo2"] + B_GIVEN["both"]      # |o - p| / (o p) < 0.3: see Margins, the acos argument on a clamp
    piv[low_rows] = off[low_rows] + rng.uniform(-0.03, 0.03, (len(low_rows), 2))
    travel = rng.uniform(1.7, 1.85, (H, 2))
    abs0 = np.arccos((off**2 + piv**2 - s0**2) / (2 * off * piv))
    s_max = np.sqrt(off**2 + piv**2 - 2 * off * piv * np.cos(np.minimum(abs0 + travel, 3.0)))
    max_pos = rng.uniform(65000.0, 76000.0, (H, 2))
    inc = max_pos / (s_max - s0)
    assert (100.0 * inc > 21.0).all()

    cw = np.stack([(np.arange(H) % 4) // 2, np.arange(H) % 2], 1).astype(np.float64)
    # the joint angles the field needs: axis 1 from "up" (-pi/2) towards south (0), axis 2 around 0
    init_angle = np.empty((H, 2))
    start = np.stack([rng.uniform(-1.62, -1.52, H), rng.uniform(-0.95, -0.80, H)], 1)   # joint angle at the low end of the travel
    init_angle[:] = np.where(cw == 0, start, start + travel)
    min_pos = np.zeros((H, 2))
    narrowed = (np.arange(H) >= 160) & (np.arange(H) % 3 == 0)
    min_pos[narrowed] = max_pos[narrowed] * rng.uniform(0.15, 0.45, (int(narrowed.sum()), 2))
    max_pos[narrowed] = max_pos[narrowed] * rng.uniform(0.55, 0.85, (int(narrowed.sum()), 2))
    designed = B_STOP + B_SOL2 + B_NEITHER + B_CHANGE + B_A2M_HI + B_A2M_LO + B_ACOS + B_ASIN
    min_pos[designed], max_pos[designed] = -WIDE, WIDE

    # class 8: den = cos(1.2) = 0.36, desired normal's east component ~ 0.55 .. 0.7
    rot[B_ASIN, 3] = 1.2 * np.where(np.arange(8) % 2 == 0, 1.0, -1.0)
    rot[B_ASIN, :3] = rng.normal(0, 0.03, (8, 3))
    pos[B_ASIN, 0], pos[B_ASIN, 1] = rng.uniform(60, 80, 8) * np.where(np.arange(8) < 4, 1, -1), rng.uniform(20, 30, 8)
    incident[B_ASIN, :3] = np.array([0.0, 0.9, -0.436]) / np.linalg.norm([0.0, 0.9, -0.436])
    # the heliostats whose choice is to change sit close to the tower with long levers: candidates move between iterations
    pos[B_CHANGE, 1] = rng.uniform(20, 28, len(B_CHANGE))
    trans[B_CHANGE] = rng.normal(0, 0.8, (len(B_CHANGE), 9))

    raw = lambda y: np.where(y > 0.2, y, inverse_softplus100(np.minimum(y, 0.2)))
    nonopt = np.zeros((H, 7, 2))
    nonopt[:, 1], nonopt[:, 2], nonopt[:, 3] = cw, min_pos, max_pos
    nonopt[:, 4], nonopt[:, 5], nonopt[:, 6] = inc - 1e-6, raw(off - 1e-6), raw(piv - 1e-6)
    opt = np.stack([init_angle, raw(s0 - 1e-6)], 1)
    return dict(positions=pos, rot_dev=rot, trans_dev=trans, act_nonopt=nonopt, act_opt=opt, incident=incident, aim=aim)


def ideal_tables(rng):
    H = H_IDEAL
    pos = np.concatenate([rng.uniform(-80, 80, (H, 1)), rng.uniform(20, 150, (H, 1)), rng.uniform(0, 3, (H, 1)),
                          np.ones((H, 1))], 1)
    rot = rng.normal(0, 0.03, (H, 4))
    seventh = np.arange(H) % 7 == 3
    rot[seventh] = rng.uniform(-0.2, 0.2, (int(seventh.sum()), 4))
    trans = rng.normal(0, 0.15, (H, 9))
    sun = np.concatenate([rng.uniform(-0.35, 0.35, (H, 1)), rng.uniform(0.8, 1.0, (H, 1)), rng.uniform(-0.6, -0.25, (H, 1))], 1)
    incident = np.concatenate([sun / np.linalg.norm(sun, axis=1, keepdims=True), np.zeros((H, 1))], 1)
    aim = np.concatenate([rng.uniform(-5, 5, (H, 1)), rng.uniform(-4, 0, (H, 1)), rng.uniform(25, 50, (H, 1)), np.ones((H, 1))], 1)
    nonopt = np.zeros((H, 4, 2))
    nonopt[:, 0] = 1.0
    nonopt[:, 1] = np.stack([(np.arange(H) % 4) // 2, np.arange(H) % 2], 1)
    nonopt[:, 2], nonopt[:, 3] = -10.0, 10.0
    pos[32:48, 1] = rng.uniform(20, 28, 16)
    trans[32:48] = rng.normal(0, 0.8, (16, 9))
    return dict(positions=pos, rot_dev=rot, trans_dev=trans, act_nonopt=nonopt, act_opt=np.zeros((0,)), incident=incident, aim=aim)


def rounded(tables):
    return {k: np.asarray(v, np.float32) for k, v in tables.items()}


# -------------------------------------------------------------------------------------- the reference, instrumented
def rigid_body(tab, dtype, n=None, leaves=False):
    """The reference's RigidBody on the first ``n`` rows of the tables, every heliostat active, every tensor in ``dtype``."""
    torch.set_default_dtype(dtype)
    T = lambda a: torch.tensor(np.asarray(a[:n], np.float64), dtype=dtype)
    H = T(tab["positions"]).shape[0]
    opt = T(tab["act_opt"]) if tab["act_opt"].size else torch.tensor([])
    kin = RigidBody(number_of_heliostats=H, heliostat_positions=T(tab["positions"]), initial_orientations=torch.zeros((H, 4)),
                    translation_deviation_parameters=T(tab["trans_dev"]), rotation_deviation_parameters=T(tab["rot_dev"]),
                    actuator_parameters_non_optimizable=T(tab["act_nonopt"]), actuator_parameters_optimizable=opt, device=CPU)
    kin.number_of_active_heliostats = H
    kin.active_heliostat_positions = kin.heliostat_positions
    kin.active_initial_orientations = kin.initial_orientations
    kin.active_rotation_deviation_parameters = kin.rotation_deviation_parameters.clone().requires_grad_(leaves)
    kin.active_translation_deviation_parameters = kin.translation_deviation_parameters.clone().requires_grad_(leaves)
    kin.active_motor_positions = kin.motor_positions
    kin.actuators.active_non_optimizable_parameters = kin.actuators.non_optimizable_parameters
    kin.actuators.active_optimizable_parameters = kin.actuators.optimizable_parameters.clone()
    if opt.numel():
        kin.actuators.active_optimizable_parameters.requires_grad_(leaves)
    for a_ in ("initial_orientation_offsets", "kinematics_standard_orientation", "homogeneous_origin"):
        setattr(kin, a_, getattr(kin, a_).detach().to(dtype))
    evaluations = [0]
    inner = kin._compute_orientations_from_motor_positions

    def counted(*a, **k):
        evaluations[0] += 1
        return inner(*a, **k)

    kin._compute_orientations_from_motor_positions = counted
    kin.evaluations = evaluations
    return kin, T


def side(x, lo, hi):
    return (x > hi).to(torch.int8) - (x < lo).to(torch.int8)


def distance(x, lo, hi):
    return torch.minimum((x - lo).abs(), (x - hi).abs())


def census(tab, dtype, motor_given):
    """Ten iterations of the reference with every branch predicate of every iteration recomputed from what passed through
    its methods.  Returns {name: (side int8 [...], distance to the nearer threshold [...], scale [...])} and the recorded
    candidates; arrays are [iteration, H, ...]."""
    kin, T = rigid_body(tab, dtype)
    act = kin.actuators
    linear = tab["act_nonopt"].shape[1] == 7
    rec = {"a2m_in": [], "normals": [], "m2a_in": []}
    a2m, inverse = act.angles_to_motor_positions, kin._compute_motor_positions_from_normal

    def a2m_wrapped(angles, device=None):
        rec["a2m_in"].append(angles.detach().clone())
        return a2m(angles=angles, device=device)

    def inverse_wrapped(normals, epsilon=1e-8, device=None):
        rec["normals"].append(normals.detach().clone())
        return inverse(normals=normals, epsilon=epsilon, device=device)

    act.angles_to_motor_positions = a2m_wrapped
    kin._compute_motor_positions_from_normal = inverse_wrapped
    forward = kin._compute_orientations_from_motor_positions

    def forward_wrapped(motor_positions, device=None):
        rec["m2a_in"].append(motor_positions.detach().clone())
        return forward(motor_positions=motor_positions, device=device)

    kin._compute_orientations_from_motor_positions = forward_wrapped
    with torch.no_grad():
        kin.incident_ray_directions_to_orientations(incident_ray_directions=T(tab["incident"]), aim_points=T(tab["aim"]),
                                                    device=CPU, max_num_iterations=N_CENSUS, min_eps=-1.0)
    assert len(rec["normals"]) == N_CENSUS and len(rec["a2m_in"]) == 2 * N_CENSUS and len(rec["m2a_in"]) == N_CENSUS
    act.angles_to_motor_positions = a2m
    out = {}
    no = act.active_non_optimizable_parameters
    lo_m, hi_m = no[:, 2], no[:, 3]
    with torch.no_grad():
        if linear:
            pn, po = act._physics_informed_parameters(device=CPU)
            inc, off, piv, ia, s0 = pn[:, 4], pn[:, 5], pn[:, 6], po[:, 0], po[:, 1]
            s_lo, s_hi, s_scale = (off - piv).abs() + 1e-6, off + piv - 1e-6, off + piv
            one = torch.ones_like(off)
            raw = torch.stack([no[:, 4], no[:, 5], no[:, 6], act.active_optimizable_parameters[:, 1]], 1) * 100.0   # [H,4,2]
            out["softplus"] = ((raw > 20.0).to(torch.int8)[None], (raw - 20.0).abs()[None], torch.full_like(raw, 20.0)[None])

            def m2a(motor):
                stroke = motor / inc + s0
                div = (off**2 + piv**2 - torch.clamp(stroke, min=s_lo, max=s_hi) ** 2) / (2.0 * off * piv)
                return stroke, div

            def angle_to_motor(angles):
                delta = torch.where(no[:, 1] == 1, angles - ia, ia - angles)
                initial = act._motor_positions_to_absolute_angles(motor_positions=torch.zeros_like(angles), device=CPU) - delta
                c = torch.cos(initial)
                stroke = torch.sqrt(off**2 + piv**2 - 2.0 * off * piv * torch.clamp(c, -1.0 + 1e-6, 1.0 - 1e-6))
                return c, stroke

            def add_m2a(name, motors):
                st, dv = zip(*(m2a(m) for m in motors))
                st, dv = torch.stack(st), torch.stack(dv)
                out[name + "_stroke"] = (side(st, s_lo, s_hi), distance(st, s_lo, s_hi), s_scale.expand_as(st))
                out[name + "_acos"] = (side(dv, -1.0 + 1e-6, 1.0 - 1e-6), distance(dv, -one + 1e-6, one - 1e-6), torch.ones_like(dv))

            add_m2a("m2a", rec["m2a_in"])
            add_m2a("m2a_zero", [torch.zeros_like(rec["m2a_in"][0])])
            add_m2a("m2a_given", [T(motor_given)])
            cs, st = zip(*(angle_to_motor(a_) for a_ in rec["a2m_in"]))
            cs, st = torch.stack(cs).reshape(N_CENSUS, 2, -1, 2), torch.stack(st).reshape(N_CENSUS, 2, -1, 2)
            out["a2m_cos"] = (side(cs, -1.0 + 1e-6, 1.0 - 1e-6), distance(cs, -one + 1e-6, one - 1e-6), torch.ones_like(cs))
            out["a2m_stroke"] = (side(st, s_lo, s_hi), distance(st, s_lo, s_hi), s_scale.expand_as(st))
        # the two candidates of every iteration and their validity
        cand = torch.stack([a2m(angles=a_, device=CPU) for a_ in rec["a2m_in"]]).reshape(N_CENSUS, 2, -1, 2)
        relative = torch.minimum((cand - lo_m).abs() / torch.maximum(cand.abs(), lo_m.abs()),
                                 (cand - hi_m).abs() / torch.maximum(cand.abs(), hi_m.abs()))
        out["valid"] = (side(cand, lo_m, hi_m), relative, torch.ones_like(cand))
        # the asin ratio
        rot = kin.active_rotation_deviation_parameters
        f1 = transforms.rotate_n(n=rot[:, 0], device=CPU) @ transforms.rotate_u(u=rot[:, 1], device=CPU)
        f2 = transforms.rotate_e(e=rot[:, 2], device=CPU) @ transforms.rotate_n(n=rot[:, 3], device=CPU)
        den = torch.sqrt(f2[:, 0, 0] ** 2 + f2[:, 0, 1] ** 2)
        ratio = torch.stack([(f1.transpose(-1, -2) @ nrm[:, :, None])[:, 0, 0] / (den + 1e-8) for nrm in rec["normals"]])
        out["asin"] = (side(ratio, -1.0 + 1e-8, 1.0 - 1e-8), distance(ratio, -torch.ones_like(ratio) + 1e-8, torch.ones_like(ratio) - 1e-8),
                       torch.ones_like(ratio))
    torch.set_default_dtype(torch.float32)
    return {k: tuple(npy(x) for x in v) for k, v in out.items()}, npy(cand), [npy(a_) for a_ in rec["a2m_in"]]


def choice_of(valid_side):
    """[iteration, H]: 1 = solution 1, 2 = solution 2 valid, 0 = neither (the reference takes solution 2)."""
    ok = (valid_side == 0).all(-1)                       # [it, 2, H]
    return np.where(ok[:, 0], 1, np.where(ok[:, 1], 2, 0))


def run_iterative(tab, dtype, n, max_iter, eps):
    kin, T = rigid_body(tab, dtype, n)
    with torch.no_grad():
        ori = kin.incident_ray_directions_to_orientations(incident_ray_directions=T(tab["incident"]), aim_points=T(tab["aim"]),
                                                          device=CPU, max_num_iterations=max_iter, min_eps=eps)
    torch.set_default_dtype(torch.float32)
    return npy(ori), npy(kin.active_motor_positions), kin.evaluations[0]


def losses(tab, dtype, n, max_iter):
    """max_h |loss_k - loss_k-1| of the evaluations k = 2 .. max_iter (the operand of the stopping rule)."""
    kin, T = rigid_body(tab, dtype, n)
    seen = []
    inner = kin._compute_motor_positions_from_normal
    oris = []
    forward = kin._compute_orientations_from_motor_positions

    def forward_wrapped(motor_positions, device=None):
        oris.append(forward(motor_positions=motor_positions, device=device))
        return oris[-1]

    def inverse_wrapped(normals, epsilon=1e-8, device=None):
        seen.append((normals - oris[-1] @ kin.kinematics_standard_orientation).abs().mean(dim=-1))
        return inner(normals=normals, epsilon=epsilon, device=device)

    kin._compute_orientations_from_motor_positions = forward_wrapped
    kin._compute_motor_positions_from_normal = inverse_wrapped
    with torch.no_grad():
        kin.incident_ray_directions_to_orientations(incident_ray_directions=T(tab["incident"]), aim_points=T(tab["aim"]),
                                                    device=CPU, max_num_iterations=max_iter, min_eps=-1.0)
    torch.set_default_dtype(torch.float32)
    return np.array([float((seen[k] - seen[k - 1]).abs().max()) for k in range(1, len(seen))])


def run_given(tab, dtype, motor_given):
    kin, T = rigid_body(tab, dtype)
    with torch.no_grad():
        ori = kin.motor_positions_to_orientations(motor_positions=T(motor_given), device=CPU)
    torch.set_default_dtype(torch.float32)
    return npy(ori)


def gradients(tab, dtype, weights, max_iter=None, motor_given=None):
    """d((W * orientation).sum()) / d(rot, trans, opt[, motor]) for every W."""
    out = {}
    for w in weights:
        kin, T = rigid_body(tab, dtype, leaves=True)
        leaves = {"rot": kin.active_rotation_deviation_parameters, "trans": kin.active_translation_deviation_parameters}
        if tab["act_opt"].size:
            leaves["opt"] = kin.actuators.active_optimizable_parameters
        if motor_given is None:
            ori = kin.incident_ray_directions_to_orientations(incident_ray_directions=T(tab["incident"]), aim_points=T(tab["aim"]),
                                                              device=CPU, max_num_iterations=max_iter, min_eps=1e-4)
        else:
            leaves["motor"] = T(motor_given).requires_grad_(True)
            ori = kin.motor_positions_to_orientations(motor_positions=leaves["motor"], device=CPU)
        grads = torch.autograd.grad((ori * T(w)).sum(), list(leaves.values()), allow_unused=True)
        for k, p, g in zip(leaves, leaves.values(), grads):
            out.setdefault(k, []).append(npy(g if g is not None else torch.zeros_like(p)))
        torch.set_default_dtype(torch.float32)
    return {k: np.stack(v) for k, v in out.items()}


# -------------------------------------------------------------------------------------- the design passes
def design_ranges(tab, blocks, wide):
    """Second pass of class 2: motor ranges around / between the candidates that the first pass (wide ranges) recorded."""
    _, cand, _ = census(rounded(tab), torch.float64, np.zeros((tab["positions"].shape[0], 2)))
    no = tab["act_nonopt"]
    for h in blocks["sol2"] + blocks["neither"]:
        m1, m2 = cand[0, 0, h], cand[0, 1, h]
        ax = int(np.argmax(np.abs(m1 - m2)))
        d = abs(m1[ax] - m2[ax])
        centre = m2[ax] if h in blocks["sol2"] else 0.5 * (m1[ax] + m2[ax])
        width = 0.3 * d if h in blocks["sol2"] else 0.2 * d
        no[h, 2, ax], no[h, 3, ax] = centre - width, centre + width
    for h in blocks["change"]:
        first, second = cand[0, 0, h], cand[1, 0, h]          # solution 1 at iterations 1 and 2
        ax = int(np.argmax(np.abs(first - second) / np.maximum(np.abs(first), 1e-3)))
        mid = 0.5 * (first[ax] + second[ax])
        if abs(first[ax] - second[ax]) < 8 * MARGIN * abs(mid):
            continue                      # its candidates move too little for a margin: it keeps its wide range (class sol1)
        if first[ax] < second[ax]:
            no[h, 3, ax], no[h, 2, ax] = mid, min(-wide, mid - wide)
        else:
            no[h, 2, ax], no[h, 3, ax] = mid, max(wide, mid + wide)
    return tab


def settle_ranges(tab, designed):
    """A heliostat outside the designed blocks whose candidate comes within 3e-3 (relative) of a bound of its motor range at
    some iteration gets that bound moved 2 % outwards, until none does."""
    for _ in range(8):
        c, cand, _ = census(rounded(tab), torch.float64, np.zeros((tab["positions"].shape[0], 2)))
        no = tab["act_nonopt"]
        lo, hi = np.float32(no[:, 2]).astype(np.float64), np.float32(no[:, 3]).astype(np.float64)
        near_lo = (np.abs(cand - lo) / np.maximum(np.abs(cand), np.abs(lo)) < 3 * MARGIN).any((0, 1))
        near_hi = (np.abs(cand - hi) / np.maximum(np.abs(cand), np.abs(hi)) < 3 * MARGIN).any((0, 1))
        near_lo[designed], near_hi[designed] = False, False
        if not (near_lo.any() or near_hi.any()):
            return tab
        no[:, 2][near_lo] -= 0.02 * np.maximum(np.abs(no[:, 2][near_lo]), np.abs(cand).max((0, 1))[near_lo])
        no[:, 3][near_hi] += 0.02 * np.maximum(np.abs(no[:, 3][near_hi]), np.abs(cand).max((0, 1))[near_hi])
    raise AssertionError("motor ranges do not settle")


def design_a2m_windows(tab):
    """Class 4: the initial angle that puts the law-of-cosines angle of the needed joint angle into the clamp's window."""
    _, _, a2m_in = census(rounded(tab), torch.float64, np.zeros((H_LINEAR, 2)))
    need = a2m_in[2 * (N_CENSUS - 1)]                                      # solution 1's joint angles at the last iteration
    no, opt = tab["act_nonopt"], tab["act_opt"]
    r = rounded(tab)
    off, piv = softplus100(r["act_nonopt"][:, 5]) + 1e-6, softplus100(r["act_nonopt"][:, 6]) + 1e-6
    s0 = softplus100(r["act_opt"][:, 1]) + 1e-6
    abs0 = np.arccos((off**2 + piv**2 - s0**2) / (2 * off * piv))
    for block, ax, target in ((B_A2M_HI, 0, np.pi - 0.10), (B_A2M_LO, 1, 0.07)):
        for h in block:
            # angle->motor: initial = abs0 - delta, delta = angle - init_angle (clockwise) or init_angle - angle
            opt[h, 0, ax] = target - abs0[h, ax] + need[h, ax] if no[h, 1, ax] == 1 else abs0[h, ax] + need[h, ax] - target
    return tab


def given_motors(tab, rng, final_motor):
    """The given-motor mode's input: the iterative mode's final motor positions, shifted; class 3 beyond the stroke ends."""
    r = rounded(tab)
    H = final_motor.shape[0]
    if r["act_nonopt"].shape[1] == 4:
        return final_motor + rng.uniform(-0.05, 0.05, (H, 2))
    inc = softplus100(r["act_nonopt"][:, 4]) + 1e-6
    off, piv = softplus100(r["act_nonopt"][:, 5]) + 1e-6, softplus100(r["act_nonopt"][:, 6]) + 1e-6
    s0 = softplus100(r["act_opt"][:, 1]) + 1e-6
    low, high = (np.abs(off - piv) + 1e-6 - s0) * inc, (off + piv - 1e-6 - s0) * inc       # motor positions of the stroke ends
    span = high - low
    given = np.clip(final_motor + rng.uniform(-1500.0, 1500.0, (H, 2)), low + 0.05 * span, high - 0.05 * span)
    beyond_low, beyond_high = low - rng.uniform(0.1, 0.3, (H, 2)) * span, high + rng.uniform(0.1, 0.3, (H, 2)) * span
    for key, rows in B_GIVEN.items():
        if key in ("lo1", "both"):
            given[rows, 0] = beyond_low[rows, 0]
        if key == "hi1":
            given[rows, 0] = beyond_high[rows, 0]
        if key == "lo2":
            given[rows, 1] = beyond_low[rows, 1]
        if key in ("hi2", "both"):
            given[rows, 1] = beyond_high[rows, 1]
    given[B_ACOS] = beyond_high[B_ACOS]
    return given


def tune_stopping_heliostat(tab):
    """Heliostat 0 of the linear field: neither solution valid, and one initial angle found by bisection such that its loss
    after the first motor update equals its loss at zero motors - alone it stops after two evaluations."""
    no, opt = tab["act_nonopt"], tab["act_opt"]
    one = {k: (v[:1].copy() if v.size else v) for k, v in tab.items()}

    def gap(x):
        one["act_opt"][0, 0, 0] = x
        r = rounded(one)
        kin, T = rigid_body(r, torch.float64)
        seen, oris = [], []
        forward, inner = kin._compute_orientations_from_motor_positions, kin._compute_motor_positions_from_normal

        def forward_wrapped(motor_positions, device=None):
            oris.append(forward(motor_positions=motor_positions, device=device))
            return oris[-1]

        def inverse_wrapped(normals, epsilon=1e-8, device=None):
            seen.append(float((normals - oris[-1] @ kin.kinematics_standard_orientation).abs().mean(dim=-1)[0]))
            return inner(normals=normals, epsilon=epsilon, device=device)

        kin._compute_orientations_from_motor_positions, kin._compute_motor_positions_from_normal = forward_wrapped, inverse_wrapped
        with torch.no_grad():
            kin.incident_ray_directions_to_orientations(incident_ray_directions=T(r["incident"]), aim_points=T(r["aim"]),
                                                        device=CPU, max_num_iterations=2, min_eps=-1.0)
        torch.set_default_dtype(torch.float32)
        return seen[1] - seen[0]

    # a range that makes both solutions invalid whatever the angle is: the motor positions of the law of cosines are >= the
    # low stroke end's, far above this range
    no[0, 2], no[0, 3] = -2.0 * WIDE, -WIDE
    one["act_nonopt"][0] = no[0]
    x0 = float(opt[0, 0, 0])
    grid = x0 + np.linspace(-1.2, 1.2, 97)
    vals = np.array([gap(x) for x in grid])
    flips = np.nonzero(np.sign(vals[1:]) != np.sign(vals[:-1]))[0]
    assert flips.size, "no initial angle equalises the two losses of heliostat 0"
    k = flips[np.argmin(np.abs(grid[flips] - x0))]
    a, b, fa = grid[k], grid[k + 1], vals[k]
    for _ in range(40):
        mid = 0.5 * (a + b)
        fm = gap(mid)
        if np.sign(fm) == np.sign(fa):
            a, fa = mid, fm
        else:
            b = mid
    opt[0, 0, 0] = float(np.float32(0.5 * (a + b)))
    assert abs(gap(opt[0, 0, 0])) < 5e-4, gap(opt[0, 0, 0])
    return tab


def design_ideal(tab):
    blocks = {"sol2": list(range(8, 20)), "neither": list(range(20, 32)), "change": list(range(32, 48))}
    return design_ranges(tab, blocks, 10.0)


# -------------------------------------------------------------------------------------- margins and classes
def produced_from_clamp(c64):
    """[iteration, H, 2]: iteration k's motor positions were produced by iteration k-1's angle->motor from a clamped stroke."""
    choice = choice_of(c64["valid"][0])                                      # [it, H]
    a2m = c64["a2m_stroke"][0]                                               # [it, 2, H, 2]
    chosen = np.where((choice == 1)[:, :, None], a2m[:, 0], a2m[:, 1]) != 0  # [it, H, 2]
    return np.concatenate([np.zeros_like(chosen[:1]), chosen[:-1]])


def check_margins(c32, c64, linear):
    """(a) same side in fp32 and fp64, (b) fp64 operand >= 1e-3 of its scale from the threshold; see the module docstring
    for the three documented exceptions."""
    for name in c64:
        s32, s64, dist, scale = c32[name][0], c64[name][0], c64[name][1], c64[name][2]
        ok_a, ok_b = s32 == s64, dist >= MARGIN * scale
        if linear and name.endswith("_acos"):
            on_clamp = c64[name[:-5] + "_stroke"][0] != 0
            ok_b = np.where(on_clamp, dist >= 0.5 * BAND, ok_b)
        if linear and name == "m2a_stroke":
            produced = produced_from_clamp(c64)
            ok_a, ok_b = ok_a | produced, ok_b | produced
        bad = np.argwhere(~(ok_a & ok_b))
        if bad.size and os.environ.get("BRANCHES_DEBUG"):
            for b in bad[:60]:
                print(name, b.tolist(), dist[tuple(b)], scale[tuple(b)], s32[tuple(b)], s64[tuple(b)])
            continue
        assert bad.size == 0, (name, bad[:10].tolist(), dist[tuple(bad[0])], scale[tuple(bad[0])], s32[tuple(bad[0])], s64[tuple(bad[0])])
    if linear:
        assert (c64["a2m_cos"][0] == 0).all()          # class 6 is left out: never active


def classes(c64, tab, linear):
    idx = lambda mask: np.nonzero(mask)[0].astype(np.int32)
    choice = choice_of(c64["valid"][0])
    out = {"sol1": idx((choice == 1).all(0)), "sol2": idx((choice == 2).all(0)), "neither": idx((choice == 0).all(0)),
           "choice_changes": idx((choice != choice[:1]).any(0))}
    cw = tab["act_nonopt"][:, 1]
    for a in (0, 1):
        for b in (0, 1):
            out[f"cw{a}{b}"] = idx((cw[:, 0] == a) & (cw[:, 1] == b))
    sat = (c64["asin"][0] != 0).any(0)
    out["asin_saturated"] = idx(sat)
    if linear:
        g = c64["m2a_given_stroke"][0][0]                                            # [H,2]
        out.update(given_lo1=idx((g[:, 0] < 0) & (g[:, 1] == 0)), given_hi1=idx((g[:, 0] > 0) & (g[:, 1] == 0)),
                   given_lo2=idx((g[:, 0] == 0) & (g[:, 1] < 0)), given_hi2=idx((g[:, 0] == 0) & (g[:, 1] > 0)),
                   given_both=idx((g[:, 0] != 0) & (g[:, 1] != 0)),
                   acos_clamp=idx((c64["m2a_given_acos"][0][0] != 0).any(-1)))
        a2m = c64["a2m_stroke"][0]                                                   # [it, 2, H, 2]
        chosen = np.where((choice == 1)[:, :, None], a2m[:, 0], a2m[:, 1])            # the stroke of the solution that was taken
        out.update(a2m_stroke_hi=idx((chosen > 0).any((0, 2))), a2m_stroke_lo=idx((chosen < 0).any((0, 2))))
        sp = c64["softplus"][0][0]                                                   # [H,4,2]: increment, offset, pivot, stroke
        for row, key in ((1, "offset"), (2, "pivot"), (3, "stroke")):
            out[f"softplus_pass_{key}"] = idx((sp[:, row] == 1).any(-1))
            out[f"softplus_log_{key}"] = idx((sp[:, row] == 0).any(-1))
        assert (sp[:, 0] == 1).all()
    # the saturated heliostats are a class of their own: asin(1 - 1e-8) is asin(1) in fp32, 1.4e-4 away from fp64, which
    # would be the yardstick of every class they were counted in
    out = {k: (v if k == "asin_saturated" else np.setdiff1d(v, out["asin_saturated"]).astype(np.int32)) for k, v in out.items()}
    out["plain"] = idx(~sat)                                                          # every heliostat a gradient test may look at
    return out


MINIMUM = {"asin_saturated": 1}


def check_census(cls, linear):
    names = ["sol1", "sol2", "neither", "choice_changes", "cw00", "cw01", "cw10", "cw11"]
    if linear:
        names += ["given_lo1", "given_hi1", "given_lo2", "given_hi2", "given_both", "a2m_stroke_hi", "a2m_stroke_lo", "acos_clamp",
                  "softplus_pass_offset", "softplus_log_offset", "softplus_pass_pivot", "softplus_log_pivot", "softplus_pass_stroke",
                  "softplus_log_stroke", "asin_saturated"]
    for k in names:
        assert len(cls[k]) >= MINIMUM.get(k, 8), (k, len(cls[k]))
    if linear:
        assert 1 <= len(cls["asin_saturated"]) <= 8


# -------------------------------------------------------------------------------------- one field
def field(name, tab64, rng, linear):
    tab = rounded(tab64)
    H = tab["positions"].shape[0]
    out = {f"{name}_{k}": v for k, v in tab.items()}
    for dtype, sfx in DTYPES:          # the one input that each run computes itself (cos(pi/2) is -4.4e-8 in fp32)
        kin, _ = rigid_body(tab, dtype, 1)
        torch.set_default_dtype(torch.float32)
        out[f"{name}_{sfx}_offsets"] = npy(kin.initial_orientation_offsets[0])
    _, final_motor, _ = run_iterative(tab, torch.float64, None, 4, 1e-4)
    given = np.asarray(given_motors(tab64, rng, final_motor), np.float32)
    out[f"{name}_motor_given"] = given
    weights = rng.standard_normal((3, H, 4, 4)).astype(np.float32)
    out[f"{name}_W"] = weights

    cens = {sfx: census(tab, dtype, given)[0] for dtype, sfx in DTYPES}
    check_margins(cens["f32"], cens["f64"], linear)
    cls = classes(cens["f64"], tab, linear)
    check_census(cls, linear)
    out.update({f"{name}_cls_{k}": v for k, v in cls.items()})
    if linear:       # the one predicate that sits on its threshold by construction (see the module docstring) is no branch
        excluded = produced_from_clamp(cens["f64"])
        for sfx in ("f32", "f64"):
            cens[sfx]["m2a_stroke"] = (np.where(excluded, 0, cens[sfx]["m2a_stroke"][0]),) + cens[sfx]["m2a_stroke"][1:]
    for sfx in ("f32", "f64"):
        out[f"{name}_{sfx}_signature"] = np.concatenate(
            [np.broadcast_to(v[0], (N_CENSUS,) + v[0].shape[1:]).reshape(N_CENSUS, -1) if v[0].shape[0] == 1
             else v[0].reshape(N_CENSUS, -1) for k, v in sorted(cens[sfx].items())], 1).astype(np.int8)

    sizes = [H] + [n for n in PREFIXES if n < H]
    out[f"{name}_sizes"] = np.array(sizes, np.int32)
    out[f"{name}_pairs"] = np.array(PAIRS, np.float64)
    results = {}
    for dtype, sfx in DTYPES:
        evals = np.zeros((len(PAIRS), len(sizes)), np.int32)
        for p, (max_iter, eps) in enumerate(PAIRS):
            for s, n in enumerate(sizes):
                ori, motor, evals[p, s] = run_iterative(tab, dtype, n, max_iter, eps)
                results[sfx, p, n] = ori
                out[f"{name}_{sfx}_ori_p{p}_n{n}"], out[f"{name}_{sfx}_motor_p{p}_n{n}"] = ori, motor
        out[f"{name}_{sfx}_evals"] = evals
        out[f"{name}_{sfx}_ori_given"] = run_given(tab, dtype, given)
        for it in GRAD_ITERATIONS:
            for k, g in gradients(tab, dtype, weights, max_iter=it).items():
                out[f"{name}_{sfx}_grad_{k}_it{it}"] = g.astype(np.float32)
        for k, g in gradients(tab, dtype, weights, motor_given=given).items():
            out[f"{name}_{sfx}_grad_{k}_given"] = g.astype(np.float32)
    # the stopping rule: same counts in both dtypes and a margin, wherever min_eps is a real threshold
    for p, (max_iter, eps) in enumerate(PAIRS):
        if eps < 1e-4:
            continue
        for s, n in enumerate(sizes):
            assert out[f"{name}_f32_evals"][p, s] == out[f"{name}_f64_evals"][p, s], (p, n)
            moved = losses(tab, torch.float64, n, max_iter)[:max(out[f"{name}_f64_evals"][p, s] - 1, 0)]   # the comparisons made
            assert (np.abs(moved - eps) >= 0.05 * eps).all(), (p, n, moved)
    if linear:
        sat = cls["asin_saturated"]
        finite = all(np.isfinite(out[f"{name}_f32_grad_{k}_it{it}"][:, sat]).all() for it in GRAD_ITERATIONS for k in ("rot", "trans", "opt"))
        out[f"{name}_asin_grad_finite_f32"] = np.array(finite)
        # a prefix that stops before the field does, visibly
        found = None
        e64 = out[f"{name}_f64_evals"]
        for p in range(len(PAIRS)):
            for s, n in enumerate(sizes[1:], start=1):
                if PAIRS[p][1] >= 1e-4 and e64[p, s] != e64[p, 0]:
                    diff = np.abs(results["f64", p, n] - results["f64", p, H][:n]).max((1, 2))
                    if diff.max() > 10 * 1e-4 and found is None:
                        found = (p, n, e64[p, s], e64[p, 0], int(diff.argmax()))
        assert found is not None, e64
        out[f"{name}_stop_pair"] = np.array(found, np.int32)
    return out, cls


def main():
    rng = np.random.default_rng(SEED)
    lin = linear_tables(rng)
    lin = design_a2m_windows(lin)
    lin = design_ranges(lin, {"sol2": B_SOL2, "neither": B_NEITHER, "change": B_CHANGE}, WIDE)
    lin = tune_stopping_heliostat(lin)
    lin = settle_ranges(lin, B_STOP + B_SOL2 + B_NEITHER + B_CHANGE)
    ideal = settle_ranges(design_ideal(ideal_tables(rng)), list(range(8, 48)))
    out = {}
    for name, tab, linear in (("lin", lin, True), ("ideal", ideal, False)):
        o, cls = field(name, tab, rng, linear)
        out.update(o)
        print(name, {k: len(v) for k, v in cls.items()})
        print(name, "evaluations f64", o[f"{name}_f64_evals"].tolist(), "f32", o[f"{name}_f32_evals"].tolist())
    print("stop pair", out["lin_stop_pair"].tolist(), "fp32 asin gradients finite:", bool(out["lin_asin_grad_finite_f32"]))
    path = OUT_DIR / "kinematics_branches.npz"
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, "bytes")
    assert path.stat().st_size < 1_000_000


if __name__ == "__main__":
    main()
