"""NURBS surface fitting on the GPU: ``art_surface_fit_prepare / _loss_grad / _run`` through the C ABI wrappers and through
``artist_amd.SurfaceGenerator``, against the reference's own runs (tests/golden/surface_fit_*.npz) and the numpy restatement
(tests/surface_fit_ref.py).  Bounds: the reference's own fp32-vs-fp64 distance times the margins of the existing tests
(MARGIN: tests/test_gpu_optimizer_epoch.py; K_GRAD / FLOOR_GRAD: tests/test_gpu_parity.py::test_trace_backward)."""
import os
import pathlib
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import surface_fit_ref as sfr

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
DEV = torch.device("cuda:0")
CASES = [(n, net, deg, method) for n in (37, 800) for net, deg in ((5, 2), (10, 3)) for method in (sfr.POINTS, sfr.NORMALS)]
PLATEAU = dict(factor=0.2, patience=5, threshold=1e-7, threshold_mode="abs")
MARGIN = 3.0
K_GRAD, FLOOR_GRAD = 3.0, 2e-4
LOSS_WINDOW = 10        # epochs on either side of a recorded one over which the reference's fp32-vs-fp64 loss distance is taken


def loss_yardstick(d, tag, epoch):
    """The reference's own fp32-vs-fp64 loss distance around ``epoch``: the largest |loss32 - loss64| of the fixture over the
    epochs within LOSS_WINDOW of it.  One epoch's difference alone is a single draw of a signed rounding error - at some epochs
    it is, by chance, 1e-7 of the loss - so the scale of that error is read from the 21 draws around it."""
    diff = np.abs(d[f"loss_{tag}"] - d[f"loss64_{tag}"])
    return float(diff[max(0, epoch - LOSS_WINDOW): epoch + LOSS_WINDOW + 1].max())


def case_name(n, net, deg, method):
    return f"surface_fit_{n}_{net}x{net}_d{deg}_{method}"


def t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def n(x):
    return x.detach().cpu().numpy()


def generator(net, deg):
    from artist_amd import SurfaceGenerator
    return SurfaceGenerator(torch.tensor([net, net]), torch.tensor([deg, deg]))


def record(line):
    """Measured distances: printed, and appended to the file named by SURFACE_FIT_PARITY_OUT (profiles/surface_fit_parity.txt is
    such a file)."""
    print(line)
    out = os.environ.get("SURFACE_FIT_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def new_state(prep, lr=1e-3, plateau=False):
    from artist_amd.surface_generator import _FitState, plateau_hyperparameters
    sched = plateau_hyperparameters(None)
    if plateau:
        sched.update(use=True, factor=PLATEAU["factor"], patience=PLATEAU["patience"], threshold=PLATEAU["threshold"], threshold_abs=True)
    return _FitState(prep.initial_control_points.clone(), lr, sched), sched


ADAM = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, maximize=False)


@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_prepare_matches_the_reference_bit_for_bit(golden, case):
    npts, net, deg, method = case
    d = golden(case_name(*case))
    prep = generator(net, deg).prepare(t(d["points"])[None])
    assert np.array_equal(n(prep.eval_uv)[0], d["eval_points"])
    assert np.array_equal(n(prep.initial_control_points)[0], d["cp_initial"])
    perm, starts = n(prep.perm)[0], n(prep.cell_start)[0]
    assert sorted(perm.tolist()) == list(range(npts)) and starts[0] == 0 and starts[-1] == npts and np.all(np.diff(starts) >= 0)
    ncv = net - deg
    span = np.floor(d["eval_points"] * np.float32(ncv)).astype(np.int64)
    cell = span[:, 0] * ncv + span[:, 1]
    for c in range(ncv * ncv):
        members = perm[starts[c]:starts[c + 1]]
        assert np.all(cell[members] == c) and np.all(np.diff(members) > 0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_loss_and_gradient_against_the_helper(golden, case):
    from artist_amd import NURBSSurfaces
    npts, net, deg, method = case
    d = golden(case_name(*case))
    m = 0 if method == sfr.POINTS else 1
    targets_np = d["points"] if m == 0 else d["normals"]
    prep = generator(net, deg).prepare(t(d["points"])[None])
    targets = t(targets_np)[None]
    for i, epoch in enumerate(d["record_epochs"]):
        if epoch not in (0, 10, d["record_epochs"][-1]):
            continue
        cp = d["cp_none"][i]
        loss, grad, pts, nrm = prep.loss_grad(t(cp)[None], targets, m, with_points=True)
        loss32, grad32, _, _ = sfr.loss_and_grad(cp, d["eval_points"], targets_np, d["degrees"], method)
        loss64, grad64, _, _ = sfr.loss_and_grad(cp.astype(np.float64), d["eval_points"].astype(np.float64),
                                                 targets_np.astype(np.float64), d["degrees"], method)
        yard = sfr.rel_l2(grad32, grad64)
        err, err_ref = sfr.rel_l2(n(grad)[0], grad32), sfr.rel_l2(n(grad)[0], d["grad_none"][i])
        record(f"loss_grad {case_name(*case)} epoch {epoch}: grad rel-L2 vs helper {err:.3e}, vs reference {err_ref:.3e}, "
               f"yardstick (helper fp32 vs fp64) {yard:.3e}; loss {float(loss):.9e} helper {float(loss32):.9e} fp64 {float(loss64):.9e}")
        assert err < max(K_GRAD * yard, FLOOR_GRAD), (epoch, err, yard)
        assert err_ref < max(K_GRAD * yard, FLOOR_GRAD), (epoch, err_ref, yard)
        # the loss like the gradient: relative distance to the helper's fp32 value, the helper's fp32-vs-fp64 distance as yardstick
        loss_yard = abs(float(loss32) - float(loss64)) / float(loss64)
        loss_err = abs(float(loss) - float(loss32)) / float(loss64)
        assert loss_err < max(K_GRAD * loss_yard, FLOOR_GRAD), (epoch, float(loss), float(loss32), loss_yard)
        assert abs(float(loss) - d["loss_none"][epoch]) / float(loss64) < max(K_GRAD * loss_yard, FLOOR_GRAD), (epoch, float(loss))
        surf = NURBSSurfaces(torch.tensor([deg, deg]), t(cp)[None, None], device=DEV)
        want_pts, want_nrm = surf.calculate_surface_points_and_normals(prep.eval_uv[None], None, None)
        assert torch.equal(pts[0], want_pts[0, 0]) and torch.equal(nrm[0], want_nrm[0, 0])


@pytest.mark.parametrize("tag", ["none", "plateau"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: case_name(*c))
def test_run_follows_the_reference(golden, case, tag):
    from artist_amd.surface_generator import run_epochs
    npts, net, deg, method = case
    d = golden(case_name(*case))
    m = 0 if method == sfr.POINTS else 1
    prep = generator(net, deg).prepare(t(d["points"])[None])
    targets = t(d["points"] if m == 0 else d["normals"])[None]
    state, sched = new_state(prep, plateau=tag == "plateau")
    max_epoch, lr_ref, loss_ref = int(d["max_epoch"]), d[f"lr_{tag}"], d[f"loss_{tag}"]
    at, lrs = 0, []
    for i, epoch in enumerate([int(e) for e in d["record_epochs"]] + [max_epoch + 1]):
        for k in range(epoch - at):                    # epoch by epoch: the rate every single epoch stepped with is compared
            lrs.append(float(state.lr[0]))
            if k == epoch - at - 1:                    # the loss an epoch reports is the loss_grad kernel's at the net it started from
                before = prep.loss_grad(state.control_points, targets, m)[0].clone()
            run_epochs(prep, state, targets, m, 1, 1e-10, max_epoch, ADAM, sched)
        if epoch > at:
            assert torch.equal(before, state.last_loss)
        at = epoch
        want, want64 = (d[f"cp_{tag}"][i], d[f"cp64_{tag}"][i]) if epoch <= max_epoch else (d[f"cp_final_{tag}"], d[f"cp64_final_{tag}"])
        drift = np.abs(want.astype(np.float64) - want64).max()
        err = np.abs(n(state.control_points)[0].astype(np.float64) - want).max()
        record(f"run {case_name(*case)} {tag} after {epoch} epochs: max |cp - reference| {err:.3e}, reference fp32-vs-fp64 drift {drift:.3e}")
        assert err <= MARGIN * drift, (epoch, err, drift)
        if epoch > 0:
            allowed = MARGIN * loss_yardstick(d, tag, epoch - 1)
            loss_err = abs(float(state.last_loss[0]) - loss_ref[epoch - 1])
            record(f"run {case_name(*case)} {tag} epoch {epoch - 1}: |loss - reference| {loss_err:.3e} (loss {loss_ref[epoch - 1]:.6e}, "
                   f"allowed {allowed:.3e} = {MARGIN:g} x the reference's largest fp32-vs-fp64 distance within {LOSS_WINDOW} epochs)")
            assert loss_err <= allowed, (epoch, loss_err, allowed)
    assert np.array_equal(np.asarray(lrs), lr_ref), "the lr schedule differs from the reference's"
    assert int(state.epochs_run[0]) == int(d[f"epochs_run_{tag}"]) == max_epoch + 1 and int(state.step[0]) == max_epoch + 1
    run_epochs(prep, state, targets, m, 5, 1e-10, max_epoch, ADAM, sched)          # past max_epoch: frozen
    assert int(state.epochs_run[0]) == max_epoch + 1 and int(state.done[0]) == 1


def test_early_stop_matches_the_reference(golden):
    d = golden("surface_fit_early_stop")
    gen = generator(int(d["net"][0]), int(d["degrees"][0]))
    surf, epochs_run, final_loss = gen.fit_nurbs_batch(t(d["points"])[None], t(d["normals"])[None], fit_method=sfr.POINTS,
                                                       tolerance=float(d["tolerance"]), max_epoch=int(d["max_epoch"]))
    assert int(epochs_run[0]) == int(d["epochs_run"])
    assert float(final_loss[0]) <= float(d["tolerance"]) and int(surf.fit_state.done[0]) == 1
    drift = np.abs(d["cp_final"].astype(np.float64) - d["cp64_final"]).max()
    err = np.abs(n(surf.control_points)[0, 0].astype(np.float64) - d["cp_final"]).max()
    record(f"early stop: epochs_run {int(epochs_run[0])}, max |cp - reference| {err:.3e}, drift {drift:.3e}")
    assert err <= MARGIN * drift


def batch_of_64(golden, method):
    """64 facets padded to 800 rows: rows 0 and 40 are the 800-point fixture, row 7 the 37-point one, the rest other seeds with
    n_valid between 100 and 800."""
    d800, d37 = golden(case_name(800, 10, 3, method)), golden(case_name(37, 10, 3, method))
    pts, nrm = np.zeros((64, 800, 4), np.float32), np.zeros((64, 800, 4), np.float32)
    n_valid = np.zeros(64, np.int32)
    for b in range(64):
        if b in (0, 40):
            p, q = d800["points"], d800["normals"]
        elif b == 7:
            p, q = d37["points"], d37["normals"]
        else:
            p, q = sfr.synthetic_facet(100 + (b * 37) % 701, 1000 + b)
        n_valid[b] = p.shape[0]
        pts[b, :p.shape[0]], nrm[b, :p.shape[0]] = p, q
        pts[b, p.shape[0]:] = 7.0            # rows beyond n_valid must not matter
    return pts, nrm, n_valid


@pytest.mark.parametrize("method", [sfr.POINTS, sfr.NORMALS])
def test_fit_is_deterministic_and_independent_of_batch_and_chunking(golden, method, monkeypatch):
    gen = generator(10, 3)
    pts, nrm, n_valid = batch_of_64(golden, method)
    kw = dict(fit_method=method, scheduler=None, max_epoch=400)
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
    kw["optimizer"], kw["scheduler"] = opt, sch
    a, ea, la = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), **kw)
    b, eb, lb = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), **kw)
    assert torch.equal(a.control_points, b.control_points) and torch.equal(ea, eb) and torch.equal(la, lb)
    assert torch.equal(a.fit_state.f64, b.fit_state.f64) and torch.equal(a.fit_state.i32, b.fit_state.i32)
    assert torch.isfinite(a.control_points).all() and int(ea.min()) == 401
    assert float(a.fit_state.lr.max()) < 1e-3                                          # the plateau scheduler did reduce
    # 401 epochs in one launch == 4 launches (100 + 100 + 100 + 101)
    c, ec, lc = gen.fit_nurbs_batch(t(pts), t(nrm), t(n_valid, torch.int32), epochs_per_launch=100, **kw)
    assert torch.equal(a.control_points, c.control_points) and torch.equal(a.fit_state.f64, c.fit_state.f64)
    assert torch.equal(a.fit_state.exp_avg_sq, c.fit_state.exp_avg_sq) and torch.equal(la, lc)
    # a facet alone (B = 1, its own N) == its row in the batch of 64
    for row in (40, 7):
        k = int(n_valid[row])
        one, e1, l1 = gen.fit_nurbs_batch(t(pts[row:row + 1, :k]), t(nrm[row:row + 1, :k]), None, **kw)
        assert torch.equal(one.control_points[0], a.control_points[row]) and torch.equal(l1[0], la[row])
        assert torch.equal(one.fit_state.f64[0], a.fit_state.f64[row])
    assert torch.equal(a.control_points[0], a.control_points[40])
    # the per-point tables streamed from global memory instead of LDS: the same bits
    monkeypatch.setenv("ARTIST_HIP_FIT_STREAM", "1")
    s, es, ls = gen.fit_nurbs_batch(t(pts[:8]), t(nrm[:8]), t(n_valid[:8], torch.int32), **kw)
    assert torch.equal(s.control_points, a.control_points[:8]) and torch.equal(ls, la[:8])


def test_no_float_atomics_in_the_fit_kernels(tmp_path):
    """Determinism by construction: the device code of the surface-fit kernels holds no atomic instruction at all - float or
    integer, global or LDS (the scan of tests/test_boundary.py, for these kernels' names and every atomic mnemonic)."""
    llvm = pathlib.Path("/opt/rocm/lib/llvm/bin")
    assert (llvm / "llvm-objdump").exists() and (llvm / "clang-offload-bundler").exists(), "ROCm LLVM tools not installed"
    lib = ROOT / "artist_amd" / "libartist_hip.so"
    fat = tmp_path / "fat.bin"
    subprocess.run([str(llvm / "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", str(lib), str(tmp_path / "stripped.so")], check=True)
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
    seen, offenders = set(), {}
    for k, start in enumerate(starts):
        part = tmp_path / f"part{k}.bin"
        part.write_bytes(blob[start: starts[k + 1] if k + 1 < len(starts) else len(blob)])
        code = tmp_path / f"code{k}.co"
        subprocess.run([str(llvm / "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={part}", f"--output={code}"], check=True)
        if not code.exists() or code.stat().st_size == 0:
            continue
        text = subprocess.run([str(llvm / "llvm-objdump"), "-d", str(code)], check=True, capture_output=True, text=True).stdout
        current = None
        for line in text.splitlines():
            mm = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
            if mm:
                current = mm.group(1) if "surface_fit_" in mm.group(1) else None
                if current:
                    seen.add(re.sub(r"ILi\d+ELb\d+E.*", "", current))
            elif current and re.search(r"\b(global|flat|buffer|scratch)_atomic|\bs_atomic|\bds_(add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|"
                                       r"cmpst|cmpswap|wrxchg|wrap|pk_add|fadd|condxchg)\w*", line.split("//")[0]):    # any atomic, float or not
                offenders[current] = offenders.get(current, 0) + 1
    assert any("surface_fit_run_kernel" in s for s in seen) and any("surface_fit_loss_grad_kernel" in s for s in seen) and \
        any("surface_fit_prepare_kernel" in s for s in seen), seen
    assert not offenders, offenders


def test_four_facet_surface_config_matches_the_reference(golden):
    d = golden("surface_fit_four_facets")
    gen = generator(int(d["net"][0]), int(d["degrees"][0]))
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    facets = gen.generate_fitted_surface_config(
        "synthetic", t(d["translations"]), t(d["canting"]), [t(d[f"points_{i}"]) for i in range(4)],
        [t(d[f"normals_{i}"]) for i in range(4)], opt, None, deflectometry_step_size=int(d["step_size"]),
        fit_method=sfr.NORMALS, max_epoch=int(d["max_epoch"]))
    assert [f.facet_key for f in facets] == ["facet_1", "facet_2", "facet_3", "facet_4"]
    for i, f in enumerate(facets):
        drift = np.abs(d["control_points"][i].astype(np.float64) - d["control_points64"][i]).max()
        err = np.abs(n(f.control_points).astype(np.float64) - d["control_points"][i]).max()
        record(f"four facets, facet {i + 1}: max |cp - reference| {err:.3e}, reference fp32-vs-fp64 drift {drift:.3e}")
        assert err <= MARGIN * drift, (i, err, drift)
        assert torch.equal(f.translation_vector, t(d["translations"])[i]) and torch.equal(f.canting, t(d["canting"])[i])


def test_fit_nurbs_drop_in_and_generic_path(golden):
    from artist_amd import NURBSSurfaces, optim
    d = golden(case_name(37, 5, 2, sfr.NORMALS))
    gen = generator(5, 2)
    pts, nrm = t(d["points"]), t(d["normals"])
    results = []
    for cls in (torch.optim.Adam, optim.Adam):
        opt = cls([torch.zeros(1, requires_grad=True, device=DEV)], lr=1e-3)
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
        surf = gen.fit_nurbs(pts, nrm, opt, sch, fit_method=sfr.NORMALS, max_epoch=120)
        assert surf.control_points.shape == (1, 1, 5, 5, 3) and opt.param_groups[0]["params"][0] is surf.control_points
        assert opt.param_groups[0]["lr"] == d["lr_plateau"][121] and sch.last_epoch == 121
        results.append((surf.control_points.detach().clone(), sch.best, sch.num_bad_epochs))
    assert torch.equal(results[0][0], results[1][0]) and results[0][1:] == results[1][1:]
    # a second facet with the SAME scheduler starts from the carried state, as in the reference's loop
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True, device=DEV)], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
    gen.fit_nurbs(pts, nrm, opt, sch, fit_method=sfr.NORMALS, max_epoch=120)
    carried = gen.fit_nurbs(pts, nrm, opt, sch, fit_method=sfr.NORMALS, max_epoch=120)
    assert not torch.equal(carried.control_points, results[0][0]) and sch.last_epoch == 242
    # generic path: SGD through the fused loss-and-gradient kernel vs a host loop over NURBSSurfaces + MSELoss
    steps = 20
    sgd = torch.optim.SGD([torch.zeros(1, requires_grad=True, device=DEV)], lr=0.5)
    got = gen.fit_nurbs(pts, nrm, sgd, None, fit_method=sfr.NORMALS, max_epoch=steps - 1).control_points.detach()
    prep = gen.prepare(pts[None])
    cp = prep.initial_control_points.clone().reshape(1, 1, 5, 5, 3).requires_grad_(True)
    sgd2 = torch.optim.SGD([cp], lr=0.5)
    for _ in range(steps):
        sgd2.zero_grad()
        _, normals = NURBSSurfaces(torch.tensor([2, 2]), cp, device=DEV).calculate_surface_points_and_normals(prep.eval_uv[None], None, None)
        torch.nn.MSELoss()(normals, nrm[None, None]).backward()
        sgd2.step()
    start = n(prep.initial_control_points).reshape(1, 1, 5, 5, 3).astype(np.float64)
    moved = float(np.abs(n(cp) - start).max())
    err = sfr.rel_l2(n(got) - start, n(cp) - start)                 # of the displacement: the nets themselves are O(1)
    record(f"generic path (SGD, {steps} steps): displacement rel-L2 vs host loop {err:.3e} (largest displacement {moved:.3e})")
    assert moved > 0 and err < FLOOR_GRAD


def test_fitted_surface_traces_like_the_reference_fit(golden):
    """End to end: control points fitted here and the reference's fitted control points give the same flux.  Bound: 1e-5
    relative L2 (the contract's flux bound) when the reference's own fp32-vs-fp64 control-point drift, pushed through the same
    tracer, stays inside it; that drift otherwise."""
    from artist_amd import HeliostatRayTracer, NURBSSurfaces
    from artist_amd.scene import build_synthetic_scenario
    d = golden("surface_fit_four_facets")
    gen = generator(10, 3)
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    zero_tr = torch.zeros(4, 4, device=DEV)
    facets = gen.generate_fitted_surface_config(
        "synthetic", zero_tr, t(d["canting"]), [t(d[f"points_{i}"]) for i in range(4)], [t(d[f"normals_{i}"]) for i in range(4)],
        opt, None, deflectometry_step_size=int(d["step_size"]), fit_method=sfr.NORMALS, max_epoch=int(d["max_epoch"]))
    ours = torch.stack([f.control_points for f in facets])[None]
    tr = d["translations"][:, None, None, :3]
    ref32 = t(d["control_points"] - tr)[None]
    ref64 = t((d["control_points64"] - tr.astype(np.float64)).astype(np.float32))[None]
    scenario, uv = build_synthetic_scenario(1, n_rays=8, n_cp=(10, 10), n_eval=16, device=DEV)
    group = scenario.heliostat_field.heliostat_groups[0]
    mask = torch.ones(1, dtype=torch.int32, device=DEV)
    tix = torch.zeros(1, dtype=torch.long, device=DEV)
    inc = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device=DEV)
    rt = None
    fluxes = []
    for cp in (ours, ref32, ref64):
        group.activate_heliostats(mask)
        with torch.no_grad():
            pts, nrm = NURBSSurfaces(group.nurbs_degrees, cp, device=DEV).calculate_surface_points_and_normals(
                uv, group.active_canting, group.active_facet_translations)
        group.active_surface_points, group.active_surface_normals = pts.reshape(1, -1, 4), nrm.reshape(1, -1, 4)
        group.align_surfaces_with_incident_ray_directions(scenario.solar_tower.get_centers_of_target_areas(tix), inc, mask)
        if rt is None:
            rt = HeliostatRayTracer(scenario, group, blocking_active=False, bitmap_resolution=torch.tensor([64, 64]))
        fluxes.append(n(rt.trace_rays(inc, mask, tix)[0]))
    assert fluxes[1].sum() > 0
    yard, err = sfr.rel_l2(fluxes[2], fluxes[1]), sfr.rel_l2(fluxes[0], fluxes[1])
    bound = 1e-5 if yard <= 1e-5 else yard
    record(f"end to end: flux rel-L2 ours vs reference-fitted {err:.3e}; reference fp32- vs fp64-fitted {yard:.3e}; bound {bound:.3e}")
    assert err <= bound, (err, yard)


def test_fit_nurbs_batch_does_not_synchronise(golden):
    d = golden(case_name(800, 10, 3, sfr.NORMALS))
    gen = generator(10, 3)
    pts, nrm = t(d["points"])[None].repeat(8, 1, 1), t(d["normals"])[None].repeat(8, 1, 1)
    n_valid = torch.full((8,), 800, dtype=torch.int32, device=DEV)
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, **PLATEAU)
    gen.fit_nurbs_batch(pts, nrm, n_valid, opt, sch, max_epoch=20)      # (loads the library, builds the knot vectors of this size)
    for fresh in (False, True):                                         # ... a generator's very first call included
        if fresh:
            gen = generator(10, 3)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                surf, epochs_run, loss = gen.fit_nurbs_batch(pts, nrm, n_valid, opt, sch, max_epoch=20, epochs_per_launch=10)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert not caught, (fresh, [str(c.message)[:160] for c in caught])
        assert int(epochs_run.min()) == 21 and torch.isfinite(loss).all()


def test_facet_without_valid_rows_and_oversized_n_valid(golden):
    """What include/artist_hip_surface_fit.h says about n_valid: a facet without valid rows keeps a zero net, runs one epoch on
    a NaN loss and stops, without disturbing its neighbour; an n_valid larger than the one prepare was given is cut to the rows
    prepare sorted."""
    from artist_amd.surface_generator import run_epochs
    d = golden(case_name(37, 5, 2, sfr.NORMALS))
    gen = generator(5, 2)
    pts, nrm = t(d["points"])[None].repeat(2, 1, 1), t(d["normals"])[None].repeat(2, 1, 1)
    both, epochs_run, loss = gen.fit_nurbs_batch(pts, nrm, torch.tensor([0, 37], dtype=torch.int32, device=DEV), max_epoch=30)
    alone, _, loss_alone = gen.fit_nurbs_batch(pts[1:], nrm[1:], None, max_epoch=30)
    assert torch.equal(both.control_points[1], alone.control_points[0]) and torch.equal(loss[1], loss_alone[0])
    assert epochs_run.tolist() == [1, 31] and both.fit_state.done.tolist() == [1, 1]
    assert torch.isnan(loss[0]) and float(both.control_points[0].abs().max()) == 0.0
    prep = gen.prepare(pts[:1], torch.tensor([20], dtype=torch.int32, device=DEV))
    want = prep.loss_grad(prep.initial_control_points, nrm[:1], 1, with_points=True)
    prep.n_valid = torch.tensor([37], dtype=torch.int32, device=DEV)             # more than prepare sorted
    got = prep.loss_grad(prep.initial_control_points, nrm[:1], 1, with_points=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    monkey = os.environ.get("ARTIST_HIP_FIT_STREAM")
    os.environ["ARTIST_HIP_FIT_STREAM"] = "1"
    try:
        streamed = prep.loss_grad(prep.initial_control_points, nrm[:1], 1, with_points=True)
    finally:
        if monkey is None:
            del os.environ["ARTIST_HIP_FIT_STREAM"]
        else:
            os.environ["ARTIST_HIP_FIT_STREAM"] = monkey
    assert all(torch.equal(a, b) for a, b in zip(want, streamed))
