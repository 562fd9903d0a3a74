"""The yardsticks of tests/test_gpu_kinematics_branches.py, pinned on the CPU: the branch fields of
tests/golden/kinematics_branches.npz (generate_kinematics_branches_golden.py: the reference's RigidBody on synthetic tables
in which every data-dependent branch of the iteration is taken by a class of heliostats) hold what they promise, the fp64
restatement equals the reference on every stored case, the fp32 restatement is as close to fp64 as the reference's fp32
run, and the stored gradients equal central differences of the restatement at a heliostat of every class."""
import numpy as np
import pytest

import oracle
from conftest import GOLDEN

FIELDS = ["lin", "ideal"]
MINIMUM = 8
LINEAR_CLASSES = ["cw00", "cw01", "cw10", "cw11", "sol1", "sol2", "neither", "choice_changes", "given_lo1", "given_hi1",
                  "given_lo2", "given_hi2", "given_both", "a2m_stroke_hi", "a2m_stroke_lo", "acos_clamp",
                  "softplus_pass_offset", "softplus_log_offset", "softplus_pass_pivot", "softplus_log_pivot",
                  "softplus_pass_stroke", "softplus_log_stroke"]
IDEAL_CLASSES = ["cw00", "cw01", "cw10", "cw11", "sol1", "sol2", "neither", "choice_changes"]
GRAD_ITERATIONS = [1, 2, 4]


def classes_of(d, field):
    """{class: indices}; ``asin_saturated`` (linear field only) is the one class gradients may leave out."""
    names = (LINEAR_CLASSES + ["asin_saturated"]) if field == "lin" else IDEAL_CLASSES
    return {k: d[f"{field}_cls_{k}"] for k in names}


def inputs(d, field, dtype, n=None):
    """The tables of a field in ``dtype`` (stored once, as the fp32 values both reference runs read), first ``n`` rows."""
    c = {k: d[f"{field}_{k}"][:n].astype(dtype) for k in ("positions", "rot_dev", "trans_dev", "act_nonopt", "incident", "aim",
                                                           "motor_given")}
    c["act_opt"] = d[f"{field}_act_opt"][:n].astype(dtype) if d[f"{field}_act_opt"].size else None
    c["offsets"] = d[f"{field}_{'f32' if dtype == np.float32 else 'f64'}_offsets"]
    return c


def restatement(c, **kw):
    return oracle.rigid_body_orientations(c["positions"], c["rot_dev"], c["trans_dev"], c["act_nonopt"], c["act_opt"], c["offsets"],
                                          **kw)


def cases(d, field):
    """(pair index, max_num_iterations, min_eps, column of the evaluation table, number of heliostats)."""
    return [(p, int(mi), float(eps), s, int(n)) for p, (mi, eps) in enumerate(d[f"{field}_pairs"])
            for s, n in enumerate(d[f"{field}_sizes"])]


def test_census(golden):
    """Every class has its heliostats, the fp32 and the fp64 reference run took the same branches, a prefix stops before the
    field does, and the file is small."""
    d = golden("kinematics_branches")
    assert (GOLDEN / "kinematics_branches.npz").stat().st_size < 1_000_000
    assert d["lin_positions"].shape[0] == 203 and d["ideal_positions"].shape[0] == 65
    assert d["lin_act_nonopt"].shape[1:] == (7, 2) and d["ideal_act_nonopt"].shape[1:] == (4, 2)
    for field in FIELDS:
        H = d[f"{field}_positions"].shape[0]
        for k, idx in classes_of(d, field).items():
            assert len(idx) >= (1 if k == "asin_saturated" else MINIMUM), (field, k, len(idx))
            assert len(np.unique(idx)) == len(idx) and idx.min() >= 0 and idx.max() < H
        np.testing.assert_array_equal(d[f"{field}_f32_signature"], d[f"{field}_f64_signature"])
        assert list(d[f"{field}_sizes"]) == [H] + [n for n in (1, 63, 65) if n < H]
        np.testing.assert_array_equal(d[f"{field}_pairs"], [(1, 1e-4), (2, 1e-4), (4, 1e-4), (10, 1e-3), (10, 1e-30)])
        real = d[f"{field}_pairs"][:, 1] >= 1e-4          # min_eps = 1e-30 stops at exact fixed points only, per dtype
        np.testing.assert_array_equal(d[f"{field}_f32_evals"][real], d[f"{field}_f64_evals"][real])
        for k in ("rot_dev", "trans_dev"):
            assert (d[f"{field}_{k}"] != 0).all()
    sat = d["lin_cls_asin_saturated"]
    assert len(sat) <= 8
    # everything outside the saturated class is in `plain`, which is what gradient tests iterate over
    np.testing.assert_array_equal(np.sort(np.concatenate([d["lin_cls_plain"], sat])), np.arange(203))
    np.testing.assert_array_equal(d["ideal_cls_plain"], np.arange(65))
    # the four inverse-solution classes and the saturated one (a class of its own) partition each field
    for field in FIELDS:
        parts = np.concatenate([d[f"{field}_cls_{k}"] for k in ("sol1", "sol2", "neither", "choice_changes")]
                               + ([sat] if field == "lin" else []))
        np.testing.assert_array_equal(np.sort(parts), np.arange(d[f"{field}_positions"].shape[0]))
    p, n, evals_prefix, evals_field, h = (int(x) for x in d["lin_stop_pair"])
    s = list(d["lin_sizes"]).index(n)
    assert d["lin_f64_evals"][p, s] == evals_prefix != evals_field == d["lin_f64_evals"][p, 0] and h < n
    moved = np.abs(d[f"lin_f64_ori_p{p}_n{n}"][h] - d[f"lin_f64_ori_p{p}_n203"][h]).max()
    assert moved > 10 * 1e-4, moved


@pytest.mark.parametrize("field", FIELDS)
def test_fp64_restatement_equals_reference(golden, field):
    """Every stored case - each (max_num_iterations, min_eps), the whole field and each prefix, and the given-motor mode:
    orientations, motor positions and the number of evaluations of the fp64 restatement are the reference's."""
    d = golden("kinematics_branches")
    for p, max_iter, eps, s, n in cases(d, field):
        c = inputs(d, field, np.float64, n)
        ori, motor, evals = restatement(c, incident=c["incident"], aim=c["aim"], max_iter=max_iter, min_eps=eps)
        assert evals == d[f"{field}_f64_evals"][p, s], (p, n, evals)
        np.testing.assert_allclose(ori, d[f"{field}_f64_ori_p{p}_n{n}"], rtol=0, atol=1e-12, err_msg=f"pair {p} n {n}")
        np.testing.assert_allclose(motor, d[f"{field}_f64_motor_p{p}_n{n}"], rtol=1e-12, atol=1e-9, err_msg=f"pair {p} n {n}")
    c = inputs(d, field, np.float64)
    ori, motor, evals = restatement(c, motor_positions=c["motor_given"])
    assert evals == 1
    np.testing.assert_allclose(ori, d[f"{field}_f64_ori_given"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(motor, c["motor_given"])


@pytest.mark.parametrize("field", FIELDS)
def test_fp32_restatement_no_further_from_fp64_than_the_reference(golden, field):
    """Per class, max-norm over the class's heliostats: |restatement32 - reference64| <= 4 |reference32 - reference64|, no
    floor, on the orientations of every (max_num_iterations, min_eps) and of the given-motor mode."""
    d = golden("kinematics_branches")
    c = inputs(d, field, np.float32)
    H = c["positions"].shape[0]
    runs = [("given", restatement(c, motor_positions=c["motor_given"])[0], d[f"{field}_f32_ori_given"], d[f"{field}_f64_ori_given"])]
    for p, (max_iter, eps) in enumerate(d[f"{field}_pairs"]):
        ori = restatement(c, incident=c["incident"], aim=c["aim"], max_iter=int(max_iter), min_eps=float(eps))[0]
        runs.append((f"pair {p}", ori, d[f"{field}_f32_ori_p{p}_n{H}"], d[f"{field}_f64_ori_p{p}_n{H}"]))
    failures = []
    for tag, ours, ref32, ref64 in runs:
        for k, idx in classes_of(d, field).items():
            mine, yard = np.abs(ours[idx] - ref64[idx]).max(), np.abs(ref32[idx] - ref64[idx]).max()
            print(f"{field} {tag:7s} {k:22s} restatement {mine:.3e} reference {yard:.3e} ratio {mine / yard:.2f}")
            if not mine <= 4 * yard:
                failures.append((tag, k, mine, yard))
    assert not failures, failures


def _scalar(c, w, max_iter, **over):
    a = dict(c, **over)
    if max_iter is None:
        ori = restatement(a, motor_positions=a["motor_given"])[0]
    else:       # min_eps < 0: exactly max_iter evaluations, which is what the whole field made when the gradients were stored
        ori = restatement(a, incident=a["incident"], aim=a["aim"], max_iter=max_iter, min_eps=-1.0)[0]
    return float((ori * w).sum())


@pytest.mark.parametrize("field", FIELDS)
def test_stored_gradients_equal_finite_differences(golden, field):
    """The reference's fp64 autograd gradients of (W * orientation).sum() against central differences of the fp64
    restatement, at the first heliostat (outside the saturated class) of every class, for every parameter, in both modes:
    the restatement depends on every parameter at every branch as the reference does.  Steps and tolerance of
    test_rigid_body_jacobians_by_finite_differences (1e-6, 1e-7 for the actuator parameters, 2e-5 of the scale)."""
    d = golden("kinematics_branches")
    plain = set(d[f"{field}_cls_plain"].tolist())
    chosen = sorted({next(int(h) for h in idx if int(h) in plain) for k, idx in classes_of(d, field).items() if k != "asin_saturated"})
    # the stored counts: the gradients were taken with min_eps = 1e-4 on the whole field
    assert [int(d[f"{field}_f64_evals"][p, 0]) for p in range(3)] == GRAD_ITERATIONS
    w_all = d[f"{field}_W"].astype(np.float64)
    groups = [("rot", "rot_dev", 1e-6), ("trans", "trans_dev", 1e-6)]
    if field == "lin":
        groups.append(("opt", "act_opt", 1e-7))
    for h in chosen:
        c = {k: (v[h:h + 1] if v is not None and k != "offsets" else v) for k, v in inputs(d, field, np.float64).items()}
        for mode in GRAD_ITERATIONS + [None]:
            tag = "given" if mode is None else f"it{mode}"
            w = w_all[0, h:h + 1]
            for name, key, rel in groups + ([("motor", "motor_given", 1e-6)] if mode is None else []):
                stored = d[f"{field}_f64_grad_{name}_{tag}"][0, h].reshape(-1).astype(np.float64)
                base = c[key].reshape(-1)
                fd = np.zeros_like(stored)
                for q in range(base.size):
                    step = rel * max(1.0, abs(float(base[q])))
                    plus, minus = base.copy(), base.copy()
                    plus[q] += step
                    minus[q] -= step
                    fd[q] = (_scalar(c, w, mode, **{key: plus.reshape(c[key].shape)})
                             - _scalar(c, w, mode, **{key: minus.reshape(c[key].shape)})) / (2 * step)
                scale = max(1.0, float(np.abs(stored).max()))
                np.testing.assert_allclose(fd, stored, rtol=0, atol=2e-5 * scale, err_msg=f"{field} heliostat {h} {name} {tag}")
