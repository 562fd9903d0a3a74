"""NURBS surface fitting, host side (no GPU): the numpy restatement of the fit (tests/surface_fit_ref.py) is pinned to the
reference's own runs (tests/golden/surface_fit_*.npz) - it is the yardstick the GPU tests carry -, and the argument handling of
``artist_amd.SurfaceGenerator`` is checked."""
import math

import numpy as np
import pytest
import torch

import surface_fit_ref as sfr

CASES = [(n, net, deg, method) for n in (37, 800) for net, deg in ((5, 2), (10, 3)) for method in (sfr.POINTS, sfr.NORMALS)]
PLATEAU = dict(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")
MARGIN = 3.0            # the margin of tests/test_gpu_optimizer_epoch.py over the reference's own fp32-vs-fp64 distance
K_GRAD, FLOOR_GRAD = 3.0, 2e-4      # tests/test_gpu_parity.py::test_trace_backward


def case_name(n, net, deg, method):
    return f"surface_fit_{n}_{net}x{net}_d{deg}_{method}"


def test_surface_generator_is_exported():
    import artist_amd
    from artist_amd.surface_generator import SurfaceGenerator
    assert artist_amd.SurfaceGenerator is SurfaceGenerator
    gen = artist_amd.SurfaceGenerator()
    assert gen._n_cp == (10, 10) and gen._deg == (3, 3)
    for name in ("fit_nurbs", "fit_nurbs_batch", "generate_fitted_surface_config", "generate_ideal_surface_config"):
        assert callable(getattr(gen, name))


@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_normalisation_and_initial_net_are_bit_equal(golden, case):
    n, net, deg, method = case
    d = golden(case_name(*case))
    pts, _ = sfr.synthetic_facet(n, {37: 5, 800: 9}[n])
    assert np.array_equal(pts, d["points"])                                        # the recipe travels with the helper
    assert np.array_equal(sfr.normalize_points(d["points"][:, :2]), d["eval_points"])
    assert np.array_equal(sfr.initial_net(d["points"], net, net), d["cp_initial"])
    assert 0.0 < d["eval_points"].min() and d["eval_points"].max() < 1.0


@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_helper_loss_and_gradient_match_the_reference(golden, case):
    n, net, deg, method = case
    d = golden(case_name(*case))
    targets = d["points"] if method == sfr.POINTS else d["normals"]
    for tag in ("none", "plateau"):
        for i, epoch in enumerate(d["record_epochs"]):
            if epoch not in (0, 10, d["record_epochs"][-1]):
                continue
            cp = d[f"cp_{tag}"][i]
            loss32, grad32, _, _ = sfr.loss_and_grad(cp, d["eval_points"], targets, d["degrees"], method)
            loss64, grad64, _, _ = sfr.loss_and_grad(cp.astype(np.float64), d["eval_points"].astype(np.float64),
                                                     targets.astype(np.float64), d["degrees"], method)
            yard = max(sfr.rel_l2(grad32, grad64), sfr.rel_l2(d[f"grad_{tag}"][i], grad64))
            assert sfr.rel_l2(grad32, d[f"grad_{tag}"][i]) < max(K_GRAD * yard, FLOOR_GRAD), (tag, epoch, yard)
            # the loss like the gradient: relative distance under the same rule, the fp32-vs-fp64 distance as yardstick
            loss_yard = max(abs(float(loss32) - float(loss64)), abs(d[f"loss_{tag}"][epoch] - float(loss64))) / float(loss64)
            loss_err = abs(float(loss32) - d[f"loss_{tag}"][epoch]) / float(loss64)
            assert loss_err < max(K_GRAD * loss_yard, FLOOR_GRAD), (tag, epoch, loss_err, loss_yard)


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == 37], ids=lambda c: case_name(*c))
@pytest.mark.parametrize("tag", ["none", "plateau"])
def test_helper_fit_follows_the_reference(golden, case, tag):
    """Control points at the recorded epochs within MARGIN x the reference's own fp32-vs-fp64 drift; lr schedule exact."""
    n, net, deg, method = case
    d = golden(case_name(*case))
    rec = [int(e) for e in d["record_epochs"]]
    r = sfr.fit(d["points"], d["normals"], net, net, d["degrees"], method, plateau=PLATEAU if tag == "plateau" else None,
                max_epoch=int(d["max_epoch"]), record=rec)
    assert r["epochs_run"] == int(d[f"epochs_run_{tag}"])
    assert np.array_equal(r["lr"], d[f"lr_{tag}"])
    if tag == "plateau":
        assert (np.diff(d["lr_plateau"]) < 0).sum() >= 2
    for i, e in enumerate(rec):
        drift = np.abs(d[f"cp_{tag}"][i].astype(np.float64) - d[f"cp64_{tag}"][i])
        err = np.abs(r["cp_at"][e].astype(np.float64) - d[f"cp_{tag}"][i])
        assert err.max() <= MARGIN * drift.max(), (e, err.max(), drift.max())
    drift = np.abs(d[f"cp_final_{tag}"].astype(np.float64) - d[f"cp64_final_{tag}"]).max()
    assert np.abs(r["cp"].astype(np.float64) - d[f"cp_final_{tag}"]).max() <= MARGIN * drift


def test_helper_stops_where_the_reference_stops(golden):
    d = golden("surface_fit_early_stop")
    r = sfr.fit(d["points"], d["normals"], int(d["net"][0]), int(d["net"][1]), d["degrees"], sfr.POINTS,
                tolerance=float(d["tolerance"]), max_epoch=int(d["max_epoch"]))
    assert r["epochs_run"] == int(d["epochs_run"]) < int(d["max_epoch"])
    drift = np.abs(d["cp_final"].astype(np.float64) - d["cp64_final"]).max()
    assert np.abs(r["cp"].astype(np.float64) - d["cp_final"]).max() <= MARGIN * drift


def test_plateau_matches_torch():
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1e-3)
    for kw in (PLATEAU, dict(mode="max", factor=0.5, patience=2, threshold=1e-2, cooldown=3, min_lr=1e-5),
               dict(factor=0.1, patience=0, threshold=0.1, threshold_mode="rel")):
        opt.param_groups[0]["lr"] = 1e-3
        theirs = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **kw)
        ours = sfr.Plateau(1e-3, **kw)
        rng = np.random.default_rng(3)
        for k in range(200):
            m = float(np.float32(1.0 / (1 + k) + 0.05 * rng.random()))
            theirs.step(m)
            ours.step(m)
            assert ours.lr == opt.param_groups[0]["lr"] and ours.best == theirs.best
            assert (ours.num_bad_epochs, ours.cooldown_counter) == (theirs.num_bad_epochs, theirs.cooldown_counter)


def test_optimizer_and_scheduler_arguments():
    from artist_amd import optim
    from artist_amd.surface_generator import adam_hyperparameters, plateau_hyperparameters
    prm = [torch.zeros(1, requires_grad=True)]
    h = adam_hyperparameters(torch.optim.Adam(prm, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01, maximize=True))
    assert h == dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01, maximize=True)
    assert adam_hyperparameters(optim.Adam(prm, lr=5e-4))["lr"] == 5e-4
    assert adam_hyperparameters(None)["lr"] == 1e-3
    assert adam_hyperparameters(torch.optim.SGD(prm, lr=0.1)) is None            # generic path
    with pytest.raises(ValueError, match="amsgrad"):
        adam_hyperparameters(torch.optim.Adam(prm, amsgrad=True))
    with pytest.raises(ValueError, match="float learning rate"):
        adam_hyperparameters(torch.optim.Adam(prm, lr=torch.tensor(1e-3)))
    opt = torch.optim.Adam(prm, lr=1e-3)
    assert plateau_hyperparameters(None)["use"] is False
    assert plateau_hyperparameters(torch.optim.lr_scheduler.StepLR(opt, 10)) is None
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
    sched.step(0.5)
    sched.step(0.7)
    s = plateau_hyperparameters(sched)
    assert s["use"] and not s["mode_max"] and s["threshold_abs"] and (s["factor"], s["patience"], s["threshold"]) == (0.2, 5, 1e-7)
    assert (s["best"], s["num_bad_epochs"], s["cooldown_counter"], s["min_lr"], s["eps"]) == (0.5, 1, 0, 0.0, 1e-8)
    assert plateau_hyperparameters(torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="max"))["mode_max"]
    assert math.isinf(plateau_hyperparameters(torch.optim.lr_scheduler.ReduceLROnPlateau(opt))["best"])


def test_errors_without_a_gpu_path():
    from artist_amd import ArtistHipError, SurfaceGenerator
    gen = SurfaceGenerator(torch.tensor([5, 5]), torch.tensor([2, 2]))
    pts, nrm = (torch.from_numpy(a) for a in sfr.synthetic_facet(37, 5))
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    with pytest.raises(NotImplementedError, match=r"The conversion method 'splines' is not yet supported in ARTIST\."):
        gen.fit_nurbs(pts, nrm, opt, fit_method="splines")
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        gen.fit_nurbs(pts, nrm, opt)
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        gen.fit_nurbs_batch(pts[None], nrm[None])
    with pytest.raises(ArtistHipError, match="no CPU fallback"):
        gen.generate_fitted_surface_config("h", torch.zeros(1, 4), torch.zeros(1, 2, 4), [pts[:, :3]], [nrm[:, :3]], opt,
                                           deflectometry_step_size=1)
    ideal = gen.generate_ideal_surface_config(torch.zeros(4, 4), torch.tensor([[[0.8, 0, 0, 0], [0, 0.65, 0, 0]]]).repeat(4, 1, 1))
    assert len(ideal) == 4 and ideal[0].control_points.shape == (5, 5, 3) and ideal[3].facet_key == "facet_4"
